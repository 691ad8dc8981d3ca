"""GPU: the batched radix-2 Fr NTT (kzgx_ntt / _device, csrc/ntt.hip) and the
evaluation-form commits and openings built on it (kzgx_commit_evals_batch,
kzgx_prove_evals_batch and their device forms).

Checker: the recursive pure-Python integer FFT of tests/test_ntt_consts.py (itself
checked there against the O(n^2) definition) and the Python oracle's [P(tau)]G.
Vectors come from K.random_scalars with 0, 1, r - 1, an all-equal row and a unit
impulse forced in; every comparison is bit-exact on canonical limbs.  L, the
largest transform one workgroup runs out of LDS, is read from the one place that
defines it (KZGX_NTT_TILE_LOG2 of include/kzg_gpu.h, via kzgx.NTT_TILE_LOG2); the
kernel splits larger sizes n = 2^ceil(k/2) x 2^floor(k/2), so L + 1 and 15 are its
non-square splits and 16 the square one."""
import functools

import numpy as np
import pytest
import torch

import corc
import kzg_ref as K
import kzgx
from test_ntt_consts import bitrev, bls_root, dft_definition, fft, ifft

pytestmark = pytest.mark.gpu

BLS = K.BLS12381
L = kzgx.NTT_TILE_LOG2
ERR_ARG, ERR_NO_SRS, ERR_DEGREE = -1, -4, -5
POISON = 0x5A5A5A5AA5A5A5A5  # every word of the padding between transforms


def to_limbs(vals) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def to_ints(arr) -> list:
    raw = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


@functools.lru_cache(maxsize=None)
def perm(k):
    return np.array([bitrev(i, k) for i in range(1 << k)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def vectors(k, rows=3):
    """rows x n scalars: row 0 random with 0, 1, r - 1 forced in, row 1 all equal, row 2 a unit impulse;
    -> (limbs, forward transforms as limbs, inverse transforms as limbs), computed once per size"""
    n, r = 1 << k, BLS.r
    a = K.random_scalars(BLS, n, 0xE7A1 + k)
    for i, v in enumerate((0, 1, r - 1)):
        if i < n:
            a[i] = v
    c = K.random_scalars(BLS, 1, 0xC0 + k)[0]
    imp = [0] * n
    imp[n // 3] = 1
    data = [a, [c] * n, imp][:rows]
    if rows > 3:
        data += [K.random_scalars(BLS, n, 0xABC + j) for j in range(rows - 3)]
    w = bls_root(k)
    fwd = [fft(row, w) for row in data]
    inv = [ifft(row, w) for row in data]
    return (np.stack([to_limbs(x) for x in data]), np.stack([to_limbs(x) for x in fwd]),
            np.stack([to_limbs(x) for x in inv]))


@pytest.fixture(scope="module")
def ctx():
    c = kzgx.Context("BLS12381")
    c.set_default_table(0)  # small SRSs below: keep the setups quick (the MSM paths have their own tests)
    yield c
    c.close()


def dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def strided(rows: np.ndarray, stride: int) -> torch.Tensor:
    """batch x stride scalars on the device, the rows at the front of each, poison behind"""
    batch, n = rows.shape[0], rows.shape[1]
    buf = np.full((batch, stride, 4), POISON, dtype=np.int64)
    buf[:, :n] = rows.view(np.int64)
    return torch.from_numpy(buf).cuda()


def run_device(ctx, rows, k, inverse, bitrev_, inplace, stream=None):
    """-> transform of rows through kzgx_ntt_device, padding checked"""
    batch, n = rows.shape[0], 1 << k
    s_in, s_out = n + 3, (n + 3 if inplace else n + 5)
    d_in = strided(rows, s_in)
    d_out = d_in if inplace else torch.full((batch, s_out, 4), POISON, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.ntt_device(d_in.data_ptr(), s_in, d_out.data_ptr(), s_out, k, batch, inverse, bitrev_, stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[:, n:] == POISON).all(), "padding of the output written"
    if not inplace:
        src = d_in.cpu().numpy()
        assert (src[:, n:] == POISON).all() and (src[:, :n].view(np.uint64) == rows).all(), "input changed"
    return out[:, :n].view(np.uint64)


# ---- 1. forward and inverse against the Python FFT ---------------------------------------
SIZES = sorted({0, 1, 2, 5, 6, 7, 10, L - 1, L, L + 1, L + 2})


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("k", SIZES)
def test_ntt_matches_python_fft(ctx, k, batch, inplace):
    a, fwd, inv = vectors(k)
    a, fwd, inv = a[:batch], fwd[:batch], inv[:batch]
    p = perm(k)
    assert (run_device(ctx, a, k, False, False, inplace) == fwd).all()
    assert (run_device(ctx, a, k, False, True, inplace) == fwd[:, p]).all()  # out[brev(i)] = X[i]
    assert (run_device(ctx, a, k, True, False, inplace) == inv).all()
    assert (run_device(ctx, a[:, p], k, True, True, inplace) == inv).all()  # in[brev(i)] = value i
    if batch == 3 and not inplace:  # the host entry, one row and the batch
        assert (ctx.ntt(a) == fwd).all() and (ctx.ntt(a[0], inverse=True) == inv[0]).all()
        assert (ctx.ntt(fwd[:, p], inverse=True, bitrev=True) == a).all()


# ---- 2. two-pass sizes, batch 2, the full output -------------------------------------------
@pytest.mark.parametrize("k", [16 if L == 12 else 15, 15 if L == 12 else 14])
def test_two_pass_full_output(ctx, k):
    n, r = 1 << k, BLS.r
    rows = [K.random_scalars(BLS, n, 0x2FA5 + k + j) for j in range(2)]
    rows[0][0], rows[0][1], rows[0][n - 1] = 0, 1, r - 1
    rows[1][n // 2:] = [rows[1][n // 2]] * (n - n // 2)  # half a constant row
    a = np.stack([to_limbs(x) for x in rows])
    w = bls_root(k)
    fwd = np.stack([to_limbs(fft(x, w)) for x in rows])
    p = perm(k)
    got = run_device(ctx, a, k, False, False, False)
    assert (got == fwd).all()
    assert (run_device(ctx, a, k, False, True, True) == fwd[:, p]).all()
    assert (run_device(ctx, got, k, True, False, True) == a).all()  # inverse(forward(a)) == a
    assert (run_device(ctx, fwd[:, p], k, True, True, False) == a).all()


# ---- 3. BN254: the whole domain is n <= 4 -----------------------------------------------------
def test_bn254_domain():
    C = K.BN254
    c = kzgx.Context("BN254")
    try:
        w = kzgx.domain_root("BN254", 2)
        a = [0, 1, C.r - 1, K.random_scalars(C, 1, 77)[0]]
        X = dft_definition(a, w, C.r)
        assert to_ints(c.ntt(to_limbs(a))) == X
        assert to_ints(c.ntt(to_limbs(X), inverse=True)) == a
        assert to_ints(c.ntt(to_limbs(a), bitrev=True)) == [X[0], X[2], X[1], X[3]]
        assert to_ints(c.ntt(to_limbs(a[:2]))) == [(a[0] + a[1]) % C.r, (a[0] - a[1]) % C.r]
        with pytest.raises(kzgx.KzgxError) as e:
            c.ntt(to_limbs(list(range(8))))
        assert e.value.status == ERR_ARG
    finally:
        c.close()


# ---- argument checks ---------------------------------------------------------------------------
def test_ntt_statuses(ctx):
    d = torch.zeros((2, 8, 4), dtype=torch.int64, device="cuda")
    lib, p = kzgx.lib(), d.data_ptr()
    assert lib.kzgx_ntt_device(ctx.h, p, 8, p, 8, 3, 0, 0, None) == 0  # batch 0
    assert lib.kzgx_ntt_device(ctx.h, p, 7, p, 7, 3, 2, 0, None) == ERR_ARG  # stride < n
    assert lib.kzgx_ntt_device(ctx.h, p, 8, p, 8, 3, 2, 4, None) == ERR_ARG  # unknown flag
    assert lib.kzgx_ntt_device(ctx.h, p, 1 << 23, p, 1 << 23, 23, 1, 0, None) == ERR_ARG  # beyond 2^22
    assert lib.kzgx_ntt_device(ctx.h, None, 8, p, 8, 3, 2, 0, None) == ERR_ARG


# ---- 4. commit_evals -------------------------------------------------------------------------------
def point(out_row, inf):
    return None if inf else corc.array_to_points("BLS12381", out_row[None, :])[0]


@pytest.mark.parametrize("k", [5, 8])
def test_commit_evals(ctx, k):
    n, tau = 1 << k, K.default_tau(BLS)
    ctx.gen_srs(tau, n + 1)
    ev, _, inv = vectors(k)
    coeffs = [to_ints(inv[b]) for b in range(3)]  # the Python inverse FFT: P_k
    want = [K.commit_via_tau(BLS, tau, P) for P in coeffs]
    ref, ref_inf = ctx.msm_batch(inv, n, 3)  # the existing path on those coefficients
    for br in (False, True):
        e = ev[:, perm(k)] if br else ev
        out, inf = ctx.commit_evals(e, bitrev=br)
        assert [point(out[b], inf[b]) for b in range(3)] == want
        assert (out == ref).all() and (inf == ref_inf).all()
    z = np.stack([np.zeros((n, 4), dtype=np.uint64), ev[0]])
    out, inf = ctx.commit_evals(z)
    assert inf[0] and not out[0].any() and point(out[1], inf[1]) == want[0]
    big = np.zeros((1, 2 * n, 4), dtype=np.uint64)
    with pytest.raises(kzgx.KzgxError) as e:
        ctx.commit_evals(big)  # 2^(k+1) > the 2^k + 1 SRS points
    assert e.value.status == ERR_DEGREE
    with pytest.raises(kzgx.KzgxError) as e:
        kzgx._chk(kzgx.lib().kzgx_commit_evals_batch(ctx.h, kzgx._p(ev), k, 3, kzgx.NTT_INVERSE, kzgx._p(out),
                                                     None), "flags")
    assert e.value.status == ERR_ARG  # only KZGX_NTT_BITREV has a meaning here


def test_evals_without_srs():
    c = kzgx.Context("BLS12381")
    try:
        with pytest.raises(kzgx.KzgxError) as e:
            c.commit_evals(np.zeros((1, 4, 4), dtype=np.uint64))
        assert e.value.status == ERR_NO_SRS
        with pytest.raises(kzgx.KzgxError) as e:
            c.prove_evals(np.zeros((4, 4), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64))
        assert e.value.status == ERR_NO_SRS
    finally:
        c.close()


# ---- 5. prove_evals -----------------------------------------------------------------------------------
def test_prove_evals(ctx):
    k, r = 8, BLS.r
    n, tau = 1 << k, K.default_tau(BLS)
    ctx.gen_srs(tau, n + 1)
    ctx.gen_srs_g2(tau, 2)
    w = bls_root(k)
    zs = [3, K.random_scalars(BLS, 1, 0x51)[0], pow(w, 5, r), 1]  # small, full width, the domain point w^5, z = 1
    assert zs[1].bit_length() > 200
    ev, _, inv = vectors(k, rows=4)
    evals = [to_ints(ev[b]) for b in range(4)]
    coeffs = [to_ints(inv[b]) for b in range(4)]
    zl = to_limbs(zs)
    for shared in (True, False):
        for br in (False, True):
            polys = [coeffs[0]] * 4 if shared else coeffs
            e = ev[0] if shared else ev
            e = e[..., perm(k), :] if br else e
            out, inf, y = ctx.prove_evals(e, zl, shared=shared, bitrev=br)
            ys = to_ints(y)
            assert ys == [K.poly_eval(BLS, K.normalize(list(P)), z) for P, z in zip(polys, zs)]
            assert ys[2] == (evals[0] if shared else evals[2])[5]  # at w^5 the value is evals[5] itself
            want = [K.commit_via_tau(BLS, tau, K.proof_quotient(BLS, K.normalize(list(P)), z, 1))
                    for P, z in zip(polys, zs)]
            assert [point(out[j], inf[j]) for j in range(4)] == want
            c_out, c_inf = ctx.commit_evals(np.stack([e] * 4) if shared else e, bitrev=br)
            ok = ctx.verify_single_batch(c_out, out, zl, y, commit_inf=c_inf, proof_inf=inf)
            assert ok.all()
    out, inf, y = ctx.prove_evals(ev[1], zl)  # the constant polynomial: zero quotient
    assert inf.all() and to_ints(y) == [evals[1][0]] * 4


# ---- 6. device entry on a second stream, the context's first use -------------------------------------
def test_first_use_on_a_fresh_stream():
    k = L + 1
    a, fwd, _ = vectors(k)
    c = kzgx.Context("BLS12381")
    try:
        st = torch.cuda.Stream()
        got = run_device(c, a, k, False, False, False, stream=st.cuda_stream)  # builds the twiddles on st
        assert (got == fwd).all()
        assert (c.ntt(a) == got).all()  # the host entry, on the context's own stream
        st2 = torch.cuda.Stream()
        assert (run_device(c, a, k, False, True, True, stream=st2.cuda_stream) == fwd[:, perm(k)]).all()
    finally:
        c.close()


# ---- 7. the caller's evaluations are only read ---------------------------------------------------------
def test_device_entries_leave_the_evaluations_intact(ctx):
    k = 8
    n, tau = 1 << k, K.default_tau(BLS)
    ctx.gen_srs(tau, n + 1)
    ev, _, inv = vectors(k)
    stride = n + 7
    d_e = strided(ev, stride)
    before = d_e.clone()
    d_out = torch.zeros((3, 12), dtype=torch.int64, device="cuda")
    d_inf = torch.zeros((3,), dtype=torch.int32, device="cuda")
    d_y = torch.zeros((3, 4), dtype=torch.int64, device="cuda")
    d_z = dev(to_limbs([7, 8, 9]))
    ref, ref_inf = ctx.msm_batch(inv, n, 3)
    for br in (False, True):
        ctx.commit_evals_device(d_e.data_ptr(), k, 3, stride, d_out.data_ptr(), d_inf.data_ptr(), bitrev=br)
        torch.cuda.synchronize()
        assert torch.equal(d_e, before)
        ctx.prove_evals_device(d_e.data_ptr(), k, stride, d_z.data_ptr(), 3, d_out.data_ptr(), d_inf.data_ptr(),
                               d_y.data_ptr(), bitrev=br)
        ctx.prove_evals_device(d_e.data_ptr(), k, 0, d_z.data_ptr(), 3, d_out.data_ptr(), d_inf.data_ptr(), None,
                               bitrev=br)
        torch.cuda.synchronize()
        assert torch.equal(d_e, before)
    ctx.commit_evals_device(d_e.data_ptr(), k, 3, stride, d_out.data_ptr(), d_inf.data_ptr())
    torch.cuda.synchronize()
    assert (host(d_out) == ref).all() and (d_inf.cpu().numpy().astype(bool) == ref_inf).all()
    lib = kzgx.lib()
    assert lib.kzgx_commit_evals_batch_device(ctx.h, d_e.data_ptr(), k, 3, n - 1, 0, d_out.data_ptr(),
                                              d_inf.data_ptr(), None) == ERR_ARG  # stride < n
    assert lib.kzgx_commit_evals_batch_device(ctx.h, d_e.data_ptr(), k, 3, 0, 0, d_out.data_ptr(),
                                              d_inf.data_ptr(), None) == ERR_ARG  # 0 only for the openings
    assert lib.kzgx_commit_evals_batch_device(ctx.h, d_e.data_ptr(), k, 0, 0, 0, None, None, None) == 0  # batch 0
