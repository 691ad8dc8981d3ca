"""GPU: the batched radix-2 NTT over G1 points (kzgx_g1_ntt / _device, csrc/g1_ntt.hip).

Checker: inputs are P_j = [a_j]G from known scalars a_j (K.scalar_mul, the Python
oracle's double-and-add); the expected output i is [DFT(a)_i]G, with the integer
fft / ifft of tests/test_ntt_consts.py and one K.scalar_mul per output.  Every
comparison is bit-exact on canonical limbs and infinity flags.  The one
size-dependent path of the implementation is the chunking of a call's transforms
(KZGX_G1_NTT_CHUNK_POINTS of include/kzg_gpu.h, via kzgx.G1_NTT_CHUNK_POINTS): one
case on each side of it."""
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
ERR_ARG = -1
POISON = 0x5A5A5A5AA5A5A5A5


@functools.lru_cache(maxsize=None)
def mulG(curve, a):
    C = K.CURVES[curve]
    return K.scalar_mul(C, (C.gx, C.gy), a)


def points_of(scalars, curve="BLS12381"):
    """[a]G for every a -> (limbs (len, 2 w64), flags (len,))"""
    pts = [mulG(curve, int(a) % K.CURVES[curve].r) for a in scalars]
    return corc.points_to_array(curve, pts), np.array([p is None for p in pts])


@functools.lru_cache(maxsize=None)
def perm(k):
    return np.array([bitrev(i, k) for i in range(1 << k)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def vectors(k):
    """3 x n scalars: row 0 random with 0, 1, r - 1 forced in (an infinite input, G and -G), row 1 all
    equal (every first butterfly subtracts equal points; the transform is infinite off index 0), row 2 a
    unit impulse -> the points of the rows, of their forward and of their inverse transforms, once per size"""
    n, r = 1 << k, BLS.r
    a = K.random_scalars(BLS, n, 0x61A7 + k)
    for i, v in enumerate((0, 1, r - 1)):
        if i < n:
            a[(i + 1) % n] = v
    c = K.random_scalars(BLS, 1, 0xC1 + k)[0]
    imp = [0] * n
    imp[n // 3] = 1
    data = [a, [c] * n, imp]
    w = bls_root(k)
    res = []
    for rows in (data, [fft(x, w) for x in data], [ifft(x, w) for x in data]):
        pf = [points_of(x) for x in rows]
        res.append((np.stack([p for p, _ in pf]), np.stack([f for _, f in pf])))
    return res


@pytest.fixture(scope="module")
def ctx():
    c = kzgx.Context("BLS12381")
    yield c
    c.close()


def run_device(ctx, pts, inf, k, inverse, bitrev_, stream=None, flags_in=True):
    """the transform through kzgx_g1_ntt_device; the input must come back byte-identical and the
    poisoned words around both outputs untouched"""
    batch, n, w = pts.shape[0], 1 << k, pts.shape[2]
    d_in = torch.from_numpy(np.ascontiguousarray(pts).view(np.int64).copy()).cuda()  # (fancy indexing reorders memory)
    d_inf = torch.from_numpy(np.ascontiguousarray(inf, dtype=np.int32)).cuda() if flags_in else None
    pad = 5
    d_out = torch.full((batch * n + 2 * pad, w), POISON, dtype=torch.int64, device="cuda")
    d_oi = torch.full((batch * n + 2 * pad,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    before, before_f = d_in.clone(), None if d_inf is None else d_inf.clone()
    torch.cuda.synchronize()
    ctx.g1_ntt_device(d_in.data_ptr(), None if d_inf is None else d_inf.data_ptr(), d_out[pad:].data_ptr(),
                      d_oi[pad:].data_ptr(), k, batch, inverse, bitrev_, stream)
    torch.cuda.synchronize()
    assert torch.equal(d_in, before) and (d_inf is None or torch.equal(d_inf, before_f)), "input changed"
    out, oi = d_out.cpu().numpy(), d_oi.cpu().numpy()
    for edge in (slice(0, pad), slice(pad + batch * n, None)):
        assert (out[edge] == POISON).all() and (oi[edge] == 0x5A5A5A5A).all(), "padding of the output written"
    return (out[pad:pad + batch * n].view(np.uint64).reshape(batch, n, w),
            oi[pad:pad + batch * n].reshape(batch, n).astype(bool))


def same(got, want):
    return (got[0] == want[0]).all() and (got[1] == want[1]).all()


# ---- 1. forward and inverse, natural and bit-reversed, against [DFT(a)]G -----------------------
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("k", [0, 1, 2, 3, 6])
def test_g1_ntt_matches_the_scalar_fft(ctx, k, batch):
    (a, af), (fwd, ff), (inv, vf) = vectors(k)
    if k >= 2:
        assert af[0].any() and ff[1, 1:].all() and not ff[1, 0]  # an infinite input; the all-equal row's output
    a, af, fwd, ff, inv, vf = a[:batch], af[:batch], fwd[:batch], ff[:batch], inv[:batch], vf[:batch]
    p = perm(k)
    assert same(run_device(ctx, a, af, k, False, False), (fwd, ff))
    assert same(run_device(ctx, a, af, k, False, True), (fwd[:, p], ff[:, p]))  # out[brev(i)] = X[i]
    assert same(run_device(ctx, a, af, k, True, False), (inv, vf))
    assert same(run_device(ctx, a[:, p], af[:, p], k, True, True), (inv, vf))  # in[brev(i)] = value i
    if batch == 3:  # the host entry: the batch, one transform, and infinity by all-zero words alone
        assert same(ctx.g1_ntt(a, af), (fwd, ff))
        assert same(ctx.g1_ntt(a[0], inverse=True), (inv[0], vf[0]))
        assert same(ctx.g1_ntt(fwd[:, p], None, inverse=True, bitrev=True), (a, af))
        assert same(run_device(ctx, a, af, k, False, False, flags_in=False), (fwd, ff))


def test_flag_alone_marks_infinity(ctx):
    """a set flag is infinity whatever the coordinates say"""
    k = 2
    (a, af), (fwd, ff), _ = vectors(k)
    g = points_of([1])[0][0]
    x = a[:1].copy()
    x[0, af[0]] = g  # the infinite entry now carries G's coordinates, the flag stays
    assert same(ctx.g1_ntt(x, af[:1]), (fwd[:1], ff[:1]))


# ---- 2. round trip at 2^8 ---------------------------------------------------------------------------
def test_round_trip(ctx):
    k = 8
    n = 1 << k
    sc = [(j * j + 1) % 17 for j in range(n)]  # few distinct scalars: the Python oracle multiplies 17 times
    pts, inf = points_of(sc)
    pts, inf = pts[None], inf[None]
    assert inf.any()
    f, ffl = run_device(ctx, pts, inf, k, False, True)
    assert same(run_device(ctx, f, ffl, k, True, True), (pts, inf))
    f, ffl = run_device(ctx, pts, inf, k, True, False)
    assert same(run_device(ctx, f, ffl, k, False, False), (pts, inf))


# ---- 3. the conventions are the Fr NTT's -----------------------------------------------------------
def test_agrees_with_the_fr_ntt(ctx):
    k = 4
    (a, af), _, _ = vectors(k)
    n = 1 << k
    sc = K.random_scalars(BLS, n, 0x61A7 + k)
    for i, v in enumerate((0, 1, BLS.r - 1)):
        sc[(i + 1) % n] = v
    limbs = np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in sc], dtype=np.uint64)
    assert same(points_of(sc), (a[0], af[0]))
    for inverse in (False, True):
        for br in (False, True):
            sel = perm(k) if inverse and br else np.arange(n)  # a bit-reversed evaluation side, scalars and points alike
            t = ctx.ntt(limbs[sel], inverse=inverse, bitrev=br)
            ints = [sum(int(t[j, i]) << (64 * i) for i in range(4)) for j in range(n)]
            assert same(ctx.g1_ntt(a[0][sel], af[0][sel], inverse=inverse, bitrev=br), points_of(ints))


# ---- 4. one chunk of transforms, and one transform more ---------------------------------------------
@pytest.mark.parametrize("extra", [0, 1])
def test_chunk_threshold(ctx, extra):
    k = 3
    batch = (kzgx.G1_NTT_CHUNK_POINTS >> k) + extra
    (a, af), (fwd, ff), _ = vectors(k)
    idx = np.arange(batch) % 3
    idx[-1] = 0  # the transform past the threshold is the random row
    got, gf = ctx.g1_ntt(a[idx], af[idx], bitrev=True)
    p = perm(k)
    assert (got == fwd[idx][:, p]).all() and (gf == ff[idx][:, p]).all()


# ---- 5. BN254: the whole domain is n <= 4 ------------------------------------------------------------
def test_bn254():
    C = K.BN254
    c = kzgx.Context("BN254")
    try:
        w = kzgx.domain_root("BN254", 2)
        a = [0, 1, C.r - 1, K.random_scalars(C, 1, 78)[0]]
        X = dft_definition(a, w, C.r)
        pa, fa = points_of(a, "BN254")
        assert same(c.g1_ntt(pa, fa), points_of(X, "BN254"))
        assert same(c.g1_ntt(*points_of(X, "BN254"), inverse=True), (pa, fa))
        assert same(c.g1_ntt(pa, fa, bitrev=True), points_of([X[0], X[2], X[1], X[3]], "BN254"))
        with pytest.raises(kzgx.KzgxError) as e:
            c.g1_ntt(np.zeros((8, 8), dtype=np.uint64))
        assert e.value.status == ERR_ARG
    finally:
        c.close()


# ---- argument checks -------------------------------------------------------------------------------
def test_statuses(ctx):
    d = torch.zeros((16, 12), dtype=torch.int64, device="cuda")
    o = torch.zeros((16, 12), dtype=torch.int64, device="cuda")
    f = torch.zeros((16,), dtype=torch.int32, device="cuda")
    lib, p, q, fl = kzgx.lib(), d.data_ptr(), o.data_ptr(), f.data_ptr()
    assert lib.kzgx_g1_ntt_device(ctx.h, p, None, q, fl, 3, 0, 0, None) == 0  # batch 0
    assert lib.kzgx_g1_ntt_device(ctx.h, p, None, q, fl, 3, 2, 4, None) == ERR_ARG  # unknown flag
    assert lib.kzgx_g1_ntt_device(ctx.h, p, None, q, fl, kzgx.ntt_max_log2("BLS12381") + 1, 1, 0, None) == ERR_ARG
    assert lib.kzgx_g1_ntt_device(ctx.h, None, None, q, fl, 3, 2, 0, None) == ERR_ARG
    assert lib.kzgx_g1_ntt(ctx.h, None, None, 3, 0, 0, None, None) == 0  # batch 0, host entry
    assert lib.kzgx_g1_ntt(ctx.h, kzgx._p(np.zeros((8, 12), dtype=np.uint64)), None, 3, 1, 8,
                           kzgx._p(np.zeros((8, 12), dtype=np.uint64)),
                           np.zeros(8, dtype=np.int32).ctypes.data_as(kzgx.intp)) == ERR_ARG


# ---- the context's first use, on a fresh stream -----------------------------------------------------
def test_first_use_on_a_fresh_stream():
    k = 3
    (a, af), (fwd, ff), _ = vectors(k)
    c = kzgx.Context("BLS12381")
    try:
        st = torch.cuda.Stream()
        assert same(run_device(c, a, af, k, False, False, stream=st.cuda_stream), (fwd, ff))  # twiddles built on st
        assert same(c.g1_ntt(a, af), (fwd, ff))  # the context's own stream, ordered behind the build
    finally:
        c.close()
