"""GPU tests of the blob proofs (include/kzg_gpu.h "blob proofs"): the Fiat-Shamir challenge hashed on
the device, the barycentric value of an evaluation-form polynomial, and the blob-level prove / verify
entries built from them.

Expected values never come from the code under test: challenges come from hashlib on the stated byte
layout, values from the barycentric formula in Python, points from the oracle's curve arithmetic, and
verdicts from exponent arithmetic mod r with the golden tau (tests/blob_ref.py):
  ok_k = p_k (tau - z_k) == c_k - y_k,    aggregate = sum r_k (p_k (tau - z_k) - c_k + y_k) == 0.
Every parametrised verify case expects at least one True and at least one False among its verdicts."""
import ctypes
import hashlib

import numpy as np
import pytest

import blob_ref as B
import kzg_ref as K
import kzgx
from blob_ref import NAME, R, Blobs, make_blobs, tamper
from test_gpu_verify_aggregate import challenges128, scalars
from test_ntt_consts import bitrev as brev

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NO_SRS, ERR_DEGREE = -1, -4, -5
IDENTITY = bytes([0xC0]) + bytes(47)
SRS_POINTS = 8192  # kzgx_prove_evals_batch, the comparison of evals_at at log2n = 13, needs n points


@pytest.fixture(scope="module")
def env():
    tau = K.default_tau(B.C)
    ctx = kzgx.Context(NAME)
    ctx.set_default_table(0)  # keep the setup quick (the MSM paths have their own tests)
    ctx.gen_srs(tau, SRS_POINTS)
    ctx.gen_srs_g2(tau, 2)
    yield ctx, tau
    ctx.close()


def ints(a):
    return [B.to_int(row) for row in np.asarray(a).reshape(-1, 4)]


def some_records(count, seed):
    """48 arbitrary bytes each: the hash takes the record as it comes"""
    return b"".join(hashlib.sha512(b"rec %d %d" % (seed, j)).digest()[:48] for j in range(count))


def encode(vals_per_blob, as_bytes):
    flat = [v for b in vals_per_blob for v in b]
    return B.blob_bytes(flat) if as_bytes else B.blob_limbs(flat)


# ---- 1. challenges ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_bytes", [0, 1])
@pytest.mark.parametrize("k", [0, 1, 6, 12])
def test_challenges_shapes(env, k, as_bytes):
    """|M| = 112 (the padding inside the second block) up to 2050 compressions per lane"""
    ctx, _ = env
    vals = [tuple(K.random_scalars(B.C, 1 << k, seed=0xC4A1 + 16 * k + j)) for j in range(3)]
    recs = some_records(3, k)
    want = [B.challenge(v, recs[48 * j:48 * j + 48])[1] for j, v in enumerate(vals)]
    for bitrev in (False, True):  # the order hashed is the order given: the flag is accepted and changes nothing
        z, ok = ctx.blob_challenges(encode(vals, as_bytes), k, recs, bitrev=bitrev)
        assert ints(z) == want and ok.tolist() == [True] * 3
    for j, v in enumerate(vals):
        assert kzgx.blob_challenge(NAME, encode([v], as_bytes), recs[48 * j:48 * j + 48]) == (want[j], True)


@pytest.mark.parametrize("as_bytes", [0, 1])
@pytest.mark.parametrize("count", [1, 2, 3, 65, 300])
def test_challenges_counts(env, count, as_bytes):
    """across a wave and a workgroup; a non-canonical element at the first, a middle and the last position
    flags its own blob and no other, and the blob still hashes as given"""
    ctx, _ = env
    k, n = 4, 16
    vals = [list(K.random_scalars(B.C, n, seed=0xC0DE + j)) for j in range(count)]
    recs = some_records(count, 99)
    bad = {}
    if as_bytes:
        for j, pos in ((0, 0), (count // 2, n // 2), (count - 1, n - 1)):
            vals[j][pos] = R + (vals[j][pos] % 1000)
            bad[j] = pos
    want = [B.challenge(v, recs[48 * j:48 * j + 48])[1] for j, v in enumerate(vals)]
    z, ok = ctx.blob_challenges(encode(vals, as_bytes), k, recs)
    assert ints(z) == want
    assert ok.tolist() == [j not in bad for j in range(count)]


def test_challenge_reduction_cases(env):
    """digest div r = 0, 1 and 2 on the device (seeds searched with hashlib)"""
    ctx, _ = env
    picked, seed = {}, 0
    while len(picked) < 3:
        v = tuple(K.random_scalars(B.C, 4, seed=seed))
        rec = some_records(1, seed)
        picked.setdefault(B.challenge(v, rec)[0], (v, rec))
        seed += 1
    vals = [picked[q][0] for q in (0, 1, 2)]
    recs = b"".join(picked[q][1] for q in (0, 1, 2))
    z, ok = ctx.blob_challenges(encode(vals, True), 2, recs)
    assert ints(z) == [B.challenge(picked[q][0], picked[q][1])[1] for q in (0, 1, 2)] and ok.all()


# ---- 2. values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bitrev", [0, 1])
@pytest.mark.parametrize("k", [0, 1, 2, 6, 8, 12, 13])
def test_evals_at(env, k, bitrev):
    """n below, equal to and above a workgroup's lanes; a shared polynomial with many points: random ones, 0, 1,
    r - 1 and the domain points w^0, w^1, w^(n/2), w^(n-1), where y is the stored value"""
    ctx, _ = env
    n = 1 << k
    vals = tuple(K.random_scalars(B.C, n, seed=0xE7A1 + k))
    ws = B.domain(k, bool(bitrev))
    on_domain = sorted({0, 1 % n, n // 2, n - 1})
    pos = [brev(i, k) if bitrev else i for i in on_domain]  # where the value at w^i sits
    zs = K.random_scalars(B.C, 3, seed=k) + [0, 1, R - 1] + [ws[p] for p in pos]
    want = [B.bary(vals, k, bitrev, z) for z in zs]
    assert want[6:] == [vals[p] for p in pos]
    y = ctx.evals_at(B.blob_limbs(vals), k, scalars(zs), shared=True, bitrev=bool(bitrev))
    assert ints(y) == want
    y = ctx.evals_at(B.blob_bytes(vals), k, scalars(zs), shared=True, bitrev=bool(bitrev))
    assert ints(y) == want
    _, _, py = ctx.prove_evals(B.blob_limbs(vals), scalars(zs), shared=True, bitrev=bool(bitrev))
    assert np.array_equal(y, py)  # limb for limb


@pytest.mark.parametrize("bitrev", [0, 1])
def test_evals_at_one_polynomial_per_point(env, bitrev):
    """stride n: polynomial k at point k; an all-zero polynomial, a constant, z on the domain of one of them"""
    ctx, _ = env
    k, n = 6, 64
    polys = [tuple(K.random_scalars(B.C, n, seed=0xAB + j)) for j in range(5)] + [(0,) * n, (41,) * n]
    zs = K.random_scalars(B.C, 7, seed=3)
    zs[2] = B.domain(k, bool(bitrev))[17]
    want = [B.bary(p, k, bitrev, z) for p, z in zip(polys, zs)]
    assert want[2] == polys[2][17] and want[5] == 0 and want[6] == 41
    for as_bytes in (0, 1):
        y = ctx.evals_at(encode(polys, as_bytes), k, scalars(zs), bitrev=bool(bitrev))
        assert ints(y) == want
    _, _, py = ctx.prove_evals(np.stack([B.blob_limbs(p) for p in polys]), scalars(zs), shared=False,
                               bitrev=bool(bitrev))
    assert np.array_equal(y, py)


# ---- 3. prove ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_bytes,bitrev", [(1, 1), (1, 0), (0, 1)])
@pytest.mark.parametrize("k", [0, 2, 6])
def test_prove_blobs(env, k, as_bytes, bitrev):
    """records equal the compressed oracle points, z and y the independent values; the all-zero blob gives the
    identity record twice, a constant blob the identity proof"""
    ctx, tau = env
    n = 1 << k
    vals = [tuple(K.random_scalars(B.C, n, seed=0x9E0 + 8 * k + j)) for j in range(3)] + [(0,) * n, (5,) * n]
    hon = [B.honest(k, bitrev, tau, v) for v in vals]
    c, p, z, y = ctx.prove_blobs(encode(vals, as_bytes), k, bitrev=bool(bitrev))
    assert c == b"".join(B.record(h[0]) for h in hon)
    assert p == b"".join(B.record(h[1]) for h in hon)
    assert ints(z) == [h[2] for h in hon] and ints(y) == [h[3] for h in hon]
    assert c[48 * 3:48 * 4] == IDENTITY and p[48 * 3:48 * 4] == IDENTITY and p[48 * 4:] == IDENTITY
    assert c[48 * 4:] != IDENTITY


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint8): np.uint8}
    return torch.from_numpy(a.view(view[a.dtype]).copy()).to(torch.device("cuda", 0))


def test_prove_blobs_invalid_blob(env):
    """the device form flags the invalid blob, writes the identity twice and leaves its neighbours right; the
    host form refuses the call"""
    import torch
    ctx, tau = env
    k, n = 4, 16
    vals = [list(K.random_scalars(B.C, n, seed=0xBAD + j)) for j in range(5)]
    good = [tuple(v) for v in vals]
    vals[2][n - 1] += R
    assert vals[2][n - 1] < 1 << 256
    data = np.frombuffer(encode(vals, True), dtype=np.uint8)
    with pytest.raises(kzgx.KzgxError) as e:
        ctx.prove_blobs(data, k, bitrev=True)
    assert e.value.status == ERR_ARG
    d_b = dev(data)
    d_c, d_p = (torch.full((5 * 48 + 1,), 7, dtype=torch.uint8, device=d_b.device) for _ in range(2))
    d_z, d_y = (torch.zeros((5, 4), dtype=torch.int64, device=d_b.device) for _ in range(2))
    d_ok = torch.full((7,), 7, dtype=torch.int32, device=d_b.device)
    st = torch.cuda.Stream(device=d_b.device)
    torch.cuda.synchronize()
    ctx.prove_blobs_device(d_b.data_ptr(), k, 5, d_c.data_ptr(), d_p.data_ptr(), d_z.data_ptr(), d_y.data_ptr(),
                           d_ok[1:].data_ptr(), bytes_mode=True, bitrev=True, stream=st.cuda_stream)
    st.synchronize()
    assert d_ok.tolist() == [7, 1, 1, 0, 1, 1, 7]
    c, p = bytes(d_c.cpu().numpy()), bytes(d_p.cpu().numpy())
    assert c[-1] == 7 and p[-1] == 7
    z, y = ints(d_z.cpu().numpy().view(np.uint64)), ints(d_y.cpu().numpy().view(np.uint64))
    for j in range(5):
        cj, pj = c[48 * j:48 * j + 48], p[48 * j:48 * j + 48]
        if j == 2:
            assert cj == IDENTITY and pj == IDENTITY and y[j] == 0
            assert z[j] == B.challenge(vals[2], IDENTITY)[1]
            continue
        h = B.honest(k, 1, tau, good[j])
        assert (cj, pj, z[j], y[j]) == (B.record(h[0]), B.record(h[1]), h[2], h[3])
    assert bool((d_b.cpu() == torch.from_numpy(data.copy())).all())  # the blobs are only read


def test_prove_blobs_in_chunks(env):
    """more blobs than one internal chunk holds (KZGX_BLOB_CHUNK_SCALARS / n), the device form without z, y, ok"""
    import torch
    ctx, tau = env
    k = 12
    per = kzgx.BLOB_CHUNK_SCALARS >> k
    count = per + 2
    base = [tuple(K.random_scalars(B.C, 1 << k, seed=0xC4 + j)) for j in range(2)]
    hon = [B.honest(k, 1, tau, v) for v in base]
    one = [np.frombuffer(B.blob_bytes(v), dtype=np.uint8) for v in base]
    d_b = dev(np.concatenate([one[j & 1] for j in range(count)]))
    d_c, d_p = (torch.zeros(count * 48, dtype=torch.uint8, device=d_b.device) for _ in range(2))
    ctx.prove_blobs_device(d_b.data_ptr(), k, count, d_c.data_ptr(), d_p.data_ptr(), None, None, None,
                           bytes_mode=True, bitrev=True)
    ctx.sync()
    assert bytes(d_c.cpu().numpy()) == b"".join(B.record(hon[j & 1][0]) for j in range(count))
    assert bytes(d_p.cpu().numpy()) == b"".join(B.record(hon[j & 1][1]) for j in range(count))


# ---- 4. verify ---------------------------------------------------------------------------------------------------
def run_each(ctx, b, as_bytes, subgroup=False):
    blobs, c, p = b.data(as_bytes)
    got = ctx.verify_blobs_each(blobs, b.k, c, p, bitrev=bool(b.bitrev), subgroup=subgroup)
    assert got.dtype == np.bool_ and got.shape == (len(b),)
    return got.tolist()


def run_batch(ctx, b, as_bytes, ch, subgroup=False):
    blobs, c, p = b.data(as_bytes)
    return ctx.verify_blobs(blobs, b.k, c, p, challenges=None if ch is None else scalars(ch),
                            bitrev=bool(b.bitrev), subgroup=subgroup)


def check_verify(ctx, b, as_bytes, seed):
    """the valid batch is true; every tampering at the first, the middle and the last blob equals the exponent
    prediction, element for element and in the aggregate"""
    n = len(b)
    ch = challenges128(B.C, n, seed=seed)
    assert run_each(ctx, b, as_bytes) == [True] * n
    assert run_batch(ctx, b, as_bytes, ch) is True and run_batch(ctx, b, as_bytes, None) is True
    trues, falses = n, 0
    for pos in sorted({0, n // 2, n - 1}):
        for kind in B.KINDS:
            if kind == "noncanonical" and not as_bytes:
                continue  # limbs are taken as canonical
            t = tamper(b, pos, kind)
            if t is None:
                continue
            want = t.singles()
            if kind != "swap":
                assert want == [j != pos for j in range(n)], kind  # its own blob, and no other
            assert run_each(ctx, t, as_bytes, subgroup=(kind == "offcurve")) == want, (pos, kind)
            assert t.aggregate(ch) is False
            assert run_batch(ctx, t, as_bytes, ch) is False, (pos, kind)
            trues += want.count(True)
            falses += want.count(False)
    assert trues >= 1 and falses >= 1


@pytest.mark.parametrize("as_bytes,bitrev", [(1, 1), (1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("count", [1, 2, 3, 65, 300])
def test_verify_counts(env, count, as_bytes, bitrev):
    ctx, tau = env
    check_verify(ctx, make_blobs(4, bitrev, count, tau), as_bytes, seed=count)


def test_verify_empty_batch(env):
    ctx, _ = env
    assert ctx.verify_blobs(b"", 4, b"", b"", challenges=None) is True
    assert ctx.verify_blobs_each(b"", 4, b"", b"").tolist() == []


def test_verify_the_real_shape(env):
    """a few blobs of 4096 bit-reversed big-endian elements; the records are the prove entry's own"""
    ctx, tau = env
    b = make_blobs(12, 1, 3, tau)
    blobs, c, p = b.data(True)
    assert ctx.prove_blobs(blobs, 12, bitrev=True)[:2] == (c, p)
    check_verify(ctx, b, True, seed=12)


@pytest.mark.parametrize("as_bytes", [0, 1])
def test_cancelling_errors(env, as_bytes):
    """make_blobs makes the last blob repeat the first (equal commitments, so equal z): +1 and -1 on their
    proof exponents cancel under equal challenges -- the aggregate is TRUE, both blobs are false"""
    ctx, tau = env
    b = make_blobs(4, 1, 7, tau)
    n = len(b)
    assert b.vals[0] == b.vals[n - 1] and b.crec[0] == b.crec[n - 1]
    t = b.copy()
    t.set_p(0, b.p[0] + 1)
    t.set_p(n - 1, b.p[n - 1] - 1)
    assert t.aggregate([1] * n) is True
    want = [j not in (0, n - 1) for j in range(n)]
    assert t.singles() == want
    assert run_batch(ctx, t, as_bytes, [1] * n) is True
    assert run_each(ctx, t, as_bytes) == want


def test_subgroup_check(env):
    """a commitment record of a curve point outside the order-r subgroup: refused only with subgroup set"""
    import point_codec_ref as PC
    ctx, tau = env
    b = make_blobs(4, 1, 3, tau)
    from test_subgroup_consts import g1_curve_point, g1_member
    P = g1_curve_point(B.C, 424242)  # a raw curve point: the cofactor is large, [r]P != O
    assert not g1_member(B.C, P)
    t = b.copy()
    t.c[1], t.crec[1] = None, PC.g1_compress(B.C, P, PC.ZCASH)
    assert run_each(ctx, t, True, subgroup=True) == [True, False, True]
    assert run_batch(ctx, t, True, [1, 2, 3], subgroup=True) is False
    assert run_each(ctx, b, True, subgroup=True) == [True, True, True]
    assert run_batch(ctx, b, True, [1, 2, 3], subgroup=True) is True


def test_device_entries_on_a_caller_stream():
    """a fresh context (G1[0] and G2[0..1] only) and a fresh stream: the same answers as the host forms, the
    inputs only read, nothing written beside the outputs"""
    import torch
    tau = K.default_tau(B.C)
    good = make_blobs(4, 1, 65, tau)
    ch = challenges128(B.C, 65, seed=5)
    cases = [good, tamper(good, 40, "value"), tamper(good, 0, "noncanonical"), tamper(good, 64, "offcurve"),
             tamper(good, 33, "proof")]
    ctx = kzgx.Context(NAME)
    try:
        ctx.set_default_table(0)
        ctx.gen_srs(tau, 1)
        ctx.gen_srs_g2(tau, 2)
        d_r = dev(scalars(ch))
        st = torch.cuda.Stream(device=d_r.device)
        keep = []
        for t in cases:
            blobs, c, p = t.data(True)
            ins = [dev(np.frombuffer(x, dtype=np.uint8)) for x in (blobs, c, p)]
            before = [x.clone() for x in ins]
            one = torch.full((3,), 7, dtype=torch.int32, device=d_r.device)
            each = torch.full((67,), 7, dtype=torch.int32, device=d_r.device)
            torch.cuda.synchronize()
            ctx.verify_blobs_device(ins[0].data_ptr(), 4, 65, ins[1].data_ptr(), ins[2].data_ptr(), d_r.data_ptr(),
                                    True, one[1:].data_ptr(), bytes_mode=True, bitrev=True, stream=st.cuda_stream)
            ctx.verify_blobs_each_device(ins[0].data_ptr(), 4, 65, ins[1].data_ptr(), ins[2].data_ptr(), True,
                                         each[1:].data_ptr(), bytes_mode=True, bitrev=True, stream=st.cuda_stream)
            keep.append((ins, before, one, each))
        st.synchronize()
        for t, (ins, before, one, each) in zip(cases, keep):
            want = t.singles()
            assert one.tolist() == [7, int(t.aggregate(ch)), 7]
            assert each.tolist() == [7] + [int(v) for v in want] + [7]
            assert all(bool((x == x0).all()) for x, x0 in zip(ins, before))
            assert run_each(ctx, t, True, subgroup=True) == want
            assert run_batch(ctx, t, True, ch, subgroup=True) is t.aggregate(ch)
        assert cases[0].aggregate(ch) and not any(t.aggregate(ch) for t in cases[1:])
        # z and y of the device challenge / value entries on the same stream
        blobs, c, _ = good.data(False)
        d_b, d_c = dev(blobs), dev(np.frombuffer(c, dtype=np.uint8))
        d_z, d_y = (torch.zeros((65, 4), dtype=torch.int64, device=d_r.device) for _ in range(2))
        d_ok = torch.full((65,), 7, dtype=torch.int32, device=d_r.device)
        torch.cuda.synchronize()
        ctx.blob_challenges_device(d_b.data_ptr(), 4, 65, d_c.data_ptr(), d_z.data_ptr(), d_ok.data_ptr(),
                                   bitrev=True, stream=st.cuda_stream)
        ctx.evals_at_device(d_b.data_ptr(), 4, 16, d_z.data_ptr(), 65, d_y.data_ptr(), bitrev=True,
                            stream=st.cuda_stream)
        st.synchronize()
        zy = [good.zy(j) for j in range(65)]
        assert ints(d_z.cpu().numpy().view(np.uint64)) == [v[0] for v in zy]
        assert ints(d_y.cpu().numpy().view(np.uint64)) == [v[1] for v in zy]
        assert d_ok.tolist() == [1] * 65
    finally:
        ctx.close()


# ---- 5. statuses -------------------------------------------------------------------------------------------------
def test_statuses(env):
    import torch
    ctx, tau = env
    L = kzgx.lib()
    b = make_blobs(4, 1, 2, tau)
    blobs, c, p = b.data(True)
    hb, hc, hp = (np.frombuffer(x, dtype=np.uint8).copy() for x in (blobs, c, p))
    ch = scalars([1, 2])
    z, y = np.zeros((2, 4), dtype=np.uint64), np.zeros((2, 4), dtype=np.uint64)
    oc, op = np.zeros(96, dtype=np.uint8), np.zeros(96, dtype=np.uint8)
    ok = (ctypes.c_int * 2)(7, 7)
    u8 = lambda a: None if a is None else a.ctypes.data_as(kzgx.u8p)
    vp = lambda a: None if a is None else a.ctypes.data
    FL = kzgx.BLOB_BYTES | kzgx.NTT_BITREV

    def host(h=ctx.h, k=4, count=2, flags=FL, blobs=hb, c=hc, p=hp, okp=ok, zp=z):
        return {
            "challenges": L.kzgx_blob_challenges(h, vp(blobs), k, count, flags, u8(c), kzgx._p(zp), okp),
            "evals_at": L.kzgx_evals_at_batch(h, vp(blobs), k, 1 << min(k, 30), kzgx._p(zp), count, flags, kzgx._p(y)),
            "prove": L.kzgx_prove_blobs_batch(h, vp(blobs), k, count, flags, u8(None if c is None else oc),
                                              u8(None if p is None else op), None, None),
            "batch": L.kzgx_verify_blobs_batch(h, vp(blobs), k, count, flags, u8(c), u8(p), kzgx._p(ch), 1, okp),
            "each": L.kzgx_verify_blobs_each(h, vp(blobs), k, count, flags, u8(c), u8(p), 1, okp),
        }

    assert set(host().values()) == {0}
    assert op.tobytes() == p and oc.tobytes() == c
    every = {"challenges", "evals_at", "prove", "batch", "each"}
    refused = lambda res: {n for n, rc in res.items() if rc == ERR_ARG}
    assert refused(host(flags=FL | 1)) == every and refused(host(flags=FL | 64)) == every
    assert refused(host(k=kzgx.ntt_max_log2(NAME) + 1)) == every
    assert refused(host(blobs=None)) == every
    assert refused(host(c=None)) == every - {"evals_at"}
    assert refused(host(p=None)) == {"prove", "batch", "each"}
    assert refused(host(okp=None)) == {"batch", "each"}
    assert refused(host(zp=None)) == {"challenges", "evals_at"}
    assert L.kzgx_prove_blobs_batch(ctx.h, vp(hb), 4, 65536, FL, u8(oc), u8(op), None, None) == ERR_ARG
    # limits, before anything is read
    assert L.kzgx_verify_blobs_batch(ctx.h, vp(hb), 4, 1 << 21, FL, u8(hc), u8(hp), kzgx._p(ch), 1, ok) == ERR_ARG
    assert L.kzgx_verify_blobs_each(ctx.h, vp(hb), 4, 1 << 21, FL, u8(hc), u8(hp), 1, ok) == ERR_ARG
    # prove needs 2^log2n SRS points; evals_at and the verifies do not
    big = np.zeros(32 << 14, dtype=np.uint8)
    assert L.kzgx_prove_blobs_batch(ctx.h, vp(big), 14, 1, FL, u8(oc), u8(op), None, None) == ERR_DEGREE
    # BN254: every entry, whatever else is passed
    bn = kzgx.Context("BN254")
    try:
        assert refused(host(h=bn.h, k=1)) == every
    finally:
        bn.close()
    # no setup at all
    bare = kzgx.Context(NAME)
    try:
        res = host(h=bare.h)
        assert (res["challenges"], res["evals_at"]) == (0, 0)
        assert (res["prove"], res["batch"], res["each"]) == (ERR_NO_SRS,) * 3
    finally:
        bare.close()
    # device entries: NULL challenges, NULL and misaligned pointers, before any device work
    buf = torch.zeros(4096, dtype=torch.uint8, device=torch.device("cuda", 0))
    d = buf.data_ptr()
    assert L.kzgx_verify_blobs_batch_device(ctx.h, d, 4, 2, FL, d, d, None, 1, d, None) == ERR_ARG
    assert L.kzgx_verify_blobs_batch_device(ctx.h, d, 4, 2, FL, d, d, d, 1, None, None) == ERR_ARG
    assert L.kzgx_verify_blobs_each_device(ctx.h, d + 8, 4, 2, FL, d, d, 1, d, None) == ERR_ARG
    assert L.kzgx_blob_challenges_device(ctx.h, d, 4, 2, FL, d, None, d, None) == ERR_ARG
    assert L.kzgx_evals_at_batch_device(ctx.h, d, 4, 8, d, 2, FL, d, None) == ERR_ARG  # a stride below n
    assert L.kzgx_prove_blobs_batch_device(ctx.h, d, 4, 2, FL, None, d, None, None, None, None) == ERR_ARG
    assert L.kzgx_prove_blobs_batch_device(ctx.h, d, 4, 65536, FL, d, d, None, None, None, None) == ERR_ARG
    ctx.sync()
