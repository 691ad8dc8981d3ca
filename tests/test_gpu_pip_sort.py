"""The sort contract of the batched Pippenger (csrc/msm.hip: count, scan,
scatter) for both digit sources: the SRS source of msm_batch_impl and the
point source of msm_points_impl.

After one call on the context's stream the workspace holds, per bucket set b,
offsets[b][0..NB] and the entries of bucket k in
entries[base_b + offsets[b][k] : base_b + offsets[b][k + 1]].  Both are
checked against the signed-digit recoding done here in Python: digit = raw
window + carry; a digit above 2^(c-1) becomes digit - 2^c with a carry of 1;
bucket = |digit| - 1; zero digits and infinite points emit nothing.  The
order inside a bucket comes from LDS atomics and is not defined, so buckets
are compared as sorted lists."""
import numpy as np
import pytest

import corc
import kzg_ref as K
from test_gpu_msm_points import max_digit_scalar

pytestmark = pytest.mark.gpu

CURVES = [("BN254", K.BN254), ("BLS12381", K.BLS12381)]
CB = 10
W = (257 + CB - 1) // CB
NB = 1 << (CB - 1)
SIGN = 0x80000000


def digits(s):
    """the W signed c-bit digits of s"""
    out, carry = [], 0
    for w in range(W):
        raw = ((s >> (CB * w)) & ((1 << CB) - 1)) + carry
        carry = 1 if raw > NB else 0
        out.append(raw - (carry << CB))
    return out


def sorted_sets(sets):
    """per bucket set a list of (bucket, entry word) -> per set the sorted (bucket, word) rows"""
    return [np.array(sorted(s), dtype=np.int64).reshape(-1, 2) for s in sets]


def check_sort(ctx, expected, stride):
    """offsets / entries of the context stream's workspace against expected[b] = sorted (bucket, word)
    rows; bucket set b's entries start at word b * stride"""
    nset = len(expected)
    off = ctx.debug_ws_read("offsets", nset * (NB + 1) * 4).view(np.uint32).reshape(nset, NB + 1).astype(np.int64)
    ent = ctx.debug_ws_read("entries", nset * stride * 4).view(np.uint32).reshape(nset, stride).astype(np.int64)
    for b, exp in enumerate(expected):
        assert off[b, 0] == 0 and (np.diff(off[b]) >= 0).all(), b
        assert off[b, NB] == len(exp), b  # the non-zero digits
        lens = np.diff(off[b])
        assert np.array_equal(lens, np.bincount(exp[:, 0], minlength=NB)), b
        # bucket k's slice as a sorted list, all buckets at once: rows (bucket, word) in order
        got = np.stack([np.repeat(np.arange(NB), lens), ent[b, :off[b, NB]]], axis=1)
        got = got[np.lexsort((got[:, 1], got[:, 0]))]
        assert np.array_equal(got, exp), b


@pytest.mark.parametrize("name,C", CURVES)
def test_srs_source(name, C):
    """msm_batch of 2 MSMs of 1100 scalars over a 1200-point SRS, c = 10, no table: two full
    512-scalar count blocks and one of 76; one SRS point is infinite"""
    import kzgx
    n_srs, n, batch, inf_at = 1200, 1100, 2, 7
    ctx = kzgx.Context(name)
    try:
        ctx.set_window_bits(CB)   # the main window table itself at c = 10: no small-batch table
        ctx.set_default_table(0)  # table-less: msm_batch_impl
        srs = corc.gen_srs(name, K.default_tau(C), n_srs)
        srs[inf_at] = 0
        ctx.load_srs(srs)
        sc = [K.random_scalars(C, n, seed=900 + b) for b in range(batch)]
        sc[0][:4] = [0, 1, C.r - 1, max_digit_scalar(CB) % C.r]
        sc[1][n - 4:] = [max_digit_scalar(CB) % C.r, C.r - 1, 1, 0]
        sc[1][600] = 0
        assert sc[0][inf_at] != 0 and sc[1][inf_at] != 0  # the infinite point's digits must not appear
        ctx.prof_enable()
        out, oi = ctx.msm_batch(np.concatenate([corc.ints_to_limbs(s, 4) for s in sc]), n, batch)
        for span in ("msm_count", "msm_scan", "msm_scatter", "msm_accum"):
            assert ctx.prof_read(span)[1] == 1, span  # one batched Pippenger, nothing else
        ctx.prof_enable(False)
        expected = []
        for b in range(batch):
            rows = []
            for i, s in enumerate(sc[b]):
                if i == inf_at:
                    continue
                # rows of the main table: n_rows = n_srs
                rows += [(abs(d) - 1, (w * n_srs + i) | (SIGN if d < 0 else 0)) for w, d in enumerate(digits(s)) if d]
            expected.append(rows)
        check_sort(ctx, sorted_sets(expected), n * W)
        for b in range(batch):
            got = None if oi[b] else corc.array_to_points(name, out[b][None, :])[0]
            assert got == corc.msm_naive(name, srs[:n], corc.ints_to_limbs(sc[b], 4)), b
    finally:
        ctx.close()


@pytest.mark.parametrize("name,C", CURVES)
def test_point_source(name, C):
    """msm_points of 4097 points: L = 4097, c = 10, one chunk of W = 26 bucket sets, a full
    4096-point count block and one of a single point; half the scalars are 128-bit, so the windows
    above bit 128 are at most half-full sets; one point is flagged infinite"""
    import kzgx
    n, inf_at = 4097, 4096
    ctx = kzgx.Context(name)
    try:
        tau = K.default_tau(C)
        P = corc.gen_srs(name, tau, 64)
        d = [pow(tau, k, C.r) for k in range(64)]
        pts = np.tile(P, ((n + 63) // 64, 1))[:n]
        sc = K.random_scalars(C, n, seed=4097)
        sc[1::2] = [s % (1 << 128) for s in sc[1::2]]
        sc[0], sc[2], sc[4], sc[6] = 0, 1, C.r - 1, max_digit_scalar(CB) % C.r
        assert sc[inf_at] != 0
        flags = np.zeros(n, dtype=np.int32)
        flags[inf_at] = 1
        ctx.prof_enable()
        out, oi = ctx.msm_points(pts, corc.ints_to_limbs(sc, 4), flags)
        assert ctx.prof_read("var_sort")[1] == 1
        ctx.prof_enable(False)
        expected = [[] for _ in range(W)]
        for i, s in enumerate(sc):
            if i == inf_at:
                continue
            for w, dg in enumerate(digits(s)):
                if dg:
                    expected[w].append((abs(dg) - 1, i | (SIGN if dg < 0 else 0)))
        assert all(len(expected[w]) <= n // 2 for w in range(13, W))  # windows above bit 128: the full scalars only
        check_sort(ctx, sorted_sets(expected), n)
        sums = [sum(s for i, s in enumerate(sc) if i % 64 == j and i != inf_at) for j in range(64)]
        e = sum(s * dk for s, dk in zip(sums, d)) % C.r
        got = None if oi else corc.array_to_points(name, out[None, :])[0]
        assert got == corc.scalar_mul(name, (C.gx, C.gy), e)
    finally:
        ctx.close()
