"""GPU: all-domain openings (kzgx_prove_all_batch / _device / _prepare, csrc/g1_ntt.hip): the n proofs
of a polynomial at every point of its size-n domain by Feist-Khovratovich.

Checker: with a known tau the proof of P at z is [(P(tau) - P(z)) / (tau - z)]G, one K.scalar_mul of
the Python oracle per proof, and y = P(z) by the oracle's Horner; bit-exact on canonical limbs and
infinity flags.  Larger sizes are compared limb for limb with the existing one-opening-at-a-time path
(prove_evals / prove_single_batch over the domain) and run through the verifier."""
import functools

import numpy as np
import pytest
import torch

import corc
import kzg_ref as K
import kzgx
from test_ntt_consts import bitrev

pytestmark = pytest.mark.gpu

BLS = K.BLS12381
ERR_ARG, ERR_NO_SRS, ERR_DEGREE = -1, -4, -5
POISON = 0x5A5A5A5AA5A5A5A5


def to_limbs(vals) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


@functools.lru_cache(maxsize=None)
def perm(k):
    return np.array([bitrev(i, k) for i in range(1 << k)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def mulG(curve, a):
    C = K.CURVES[curve]
    return K.scalar_mul(C, (C.gx, C.gy), a)


def oracle(curve, tau, coeffs, k):
    """-> (proof limbs (n, 2 w64), flags (n,), y limbs (n, 4), evaluations as ints), natural order"""
    C = K.CURVES[curve]
    r, w = C.r, kzgx.domain_root(curve, k)
    ptau = K.poly_eval(C, list(coeffs), tau)
    zs = [pow(w, i, r) for i in range(1 << k)]
    ys = [K.poly_eval(C, list(coeffs), z) for z in zs]
    pts = [mulG(curve, (ptau - y) * pow(tau - z, -1, r) % r) for y, z in zip(ys, zs)]
    return corc.points_to_array(curve, pts), np.array([p is None for p in pts]), to_limbs(ys), ys


@functools.lru_cache(maxsize=None)
def case(k, tau):
    """three polynomials of 2^k coefficients (the third with 0, 1, r - 1 forced in) and their expected openings"""
    n = 1 << k
    polys = [K.random_scalars(BLS, n, 0xF20 + 16 * k + j) for j in range(3)]
    for i, v in enumerate((0, 1, BLS.r - 1)):
        if i < n:
            polys[2][(i + 1) % n] = v
    exp = [oracle("BLS12381", tau, P, k) for P in polys]
    return (np.stack([to_limbs(P) for P in polys]), np.stack([e[0] for e in exp]), np.stack([e[1] for e in exp]),
            np.stack([e[2] for e in exp]))


@pytest.fixture(scope="module")
def ctx():
    c = kzgx.Context("BLS12381")
    c.set_default_table(0)  # small SRSs below: keep the setups quick (the MSM paths have their own tests)
    yield c
    c.close()


def same(got, want_xy, want_inf, want_y=None):
    ok = (got[0] == want_xy).all() and (got[1] == want_inf).all()
    return ok and (want_y is None or (got[2] == want_y).all())


# ---- 1. against the oracle: both orders, coefficient and evaluation input -----------------------------
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("k", [0, 1, 2, 3, 5])
def test_against_the_oracle(ctx, k, batch):
    n, tau = 1 << k, K.default_tau(BLS)
    ctx.gen_srs(tau, n)  # exactly n points
    coeffs, xy, inf, y = (x[:batch] for x in case(k, tau))
    p = perm(k)
    assert same(ctx.prove_all(coeffs), xy, inf, y)
    assert same(ctx.prove_all(coeffs, bitrev=True), xy[:, p], inf[:, p], y[:, p])  # proof i at brev(i)
    assert same(ctx.prove_all(y, evals=True), xy, inf, y)
    assert same(ctx.prove_all(y[:, p], evals=True, bitrev=True), xy[:, p], inf[:, p], y[:, p])
    got = ctx.prove_all(coeffs[0], want_y=False)  # one polynomial, no y
    assert same(got, xy[0], inf[0]) and got[2] is None
    if k == 0:
        assert inf.all()  # a constant's single proof


# ---- 2. against the existing path, and through the verifier ------------------------------------------------
@pytest.mark.parametrize("k", [8, 10])
def test_against_single_openings(ctx, k):
    n, tau, r = 1 << k, K.default_tau(BLS), BLS.r
    ctx.gen_srs(tau, n + 37)
    ctx.gen_srs_g2(tau, 2)
    coeffs = to_limbs(K.random_scalars(BLS, n, 0xA11 + k))
    w = kzgx.domain_root("BLS12381", k)
    dom, z = [], 1
    for _ in range(n):
        dom.append(z)
        z = z * w % r
    zs = to_limbs(dom)
    xy, inf, y = ctx.prove_all(coeffs)
    ref, ref_inf, ref_y = ctx.prove_single_batch(coeffs, zs)
    assert (xy == ref).all() and (inf == ref_inf.astype(bool)).all() and (y == ref_y).all()
    ev, ev_inf, ev_y = ctx.prove_evals(y, zs)  # y: the polynomial's values on the domain
    assert (xy == ev).all() and (inf == np.asarray(ev_inf, dtype=bool)).all() and (y == ev_y).all()
    p = perm(k)
    assert same(ctx.prove_all(y[p], evals=True, bitrev=True), xy[p], inf[p], y[p])
    c_out, c_inf = ctx.commit_evals(y)
    ok = ctx.verify_single_batch(np.repeat(c_out, n, axis=0), xy, zs, y, commit_inf=np.repeat(c_inf, n),
                                 proof_inf=inf)
    assert ok.all()
    bad = y.copy()
    bad[3] = y[4]
    assert not ctx.verify_single_batch(np.repeat(c_out, n, axis=0), xy, zs, bad, commit_inf=np.repeat(c_inf, n),
                                       proof_inf=inf)[3]


# ---- 3. degenerate polynomials ------------------------------------------------------------------------------
def test_degenerate_polynomials(ctx):
    k = 3
    n, tau = 1 << k, K.default_tau(BLS)
    ctx.gen_srs(tau, n)
    c = K.random_scalars(BLS, n, 0xDE6)
    rows = [[c[0]] + [0] * (n - 1), c[:n - 2] + [0, 0], [0] * n]  # a constant, degree n - 3, zero
    exp = [oracle("BLS12381", tau, P, k) for P in rows]
    xy, inf, y = ctx.prove_all(np.stack([to_limbs(P) for P in rows]))
    for b in range(3):
        assert same((xy[b], inf[b], y[b]), exp[b][0], exp[b][1], exp[b][2])
    assert inf[0].all() and inf[2].all() and not inf[1].any()
    assert not y[2].any() and (y[0] == to_limbs([c[0]] * n)).all()
    xy2, inf2, _ = ctx.prove_all(y, evals=True)  # the same three from their values
    assert (xy2 == xy).all() and (inf2 == inf).all()


# ---- 4. a new SRS drops the cached setup -------------------------------------------------------------------
def test_srs_change(ctx):
    k = 3
    n, tau = 1 << k, K.default_tau(BLS)
    tau2 = (tau * 3 + 11) % BLS.r
    coeffs = case(k, tau)[0]
    for t in (tau, tau2, tau):
        ctx.gen_srs(t, n + 5)
        _, xy, inf, y = case(k, t)
        assert same(ctx.prove_all(coeffs), xy, inf, y)
    assert not (case(k, tau)[1] == case(k, tau2)[1]).all()
    srs = ctx.get_srs()
    ctx.gen_srs(tau2, n)
    ctx.load_srs(srs)  # tau's points again, through the loader
    assert same(ctx.prove_all(coeffs), *case(k, tau)[1:])


# ---- 5. prepare ---------------------------------------------------------------------------------------------
def test_prepare():
    c = kzgx.Context("BLS12381")
    try:
        c.set_default_table(0)
        with pytest.raises(kzgx.KzgxError) as e:
            c.prove_all_prepare(3)
        assert e.value.status == ERR_NO_SRS
        tau = K.default_tau(BLS)
        c.gen_srs(tau, 8)
        c.prove_all_prepare(3)
        c.prove_all_prepare(3)
        c.prove_all_prepare(0)  # nothing to build
        coeffs, xy, inf, y = case(3, tau)
        assert same(c.prove_all(coeffs), xy, inf, y)
        with pytest.raises(kzgx.KzgxError) as e:
            c.prove_all_prepare(4)  # 16 > the 8 SRS points
        assert e.value.status == ERR_DEGREE
        with pytest.raises(kzgx.KzgxError) as e:
            c.prove_all_prepare(22)
        assert e.value.status == ERR_ARG
    finally:
        c.close()


# ---- 6. device entry: the first call on a fresh stream, strided input, poisoned padding --------------------
def run_device(c, rows, k, evals=False, bitrev_=False, stream=None, with_y=True):
    batch, n, w = rows.shape[0], 1 << k, 2 * c.w64
    stride, pad = n + 3, 4
    buf = np.full((batch, stride, 4), POISON, dtype=np.int64)
    buf[:, :n] = rows.view(np.int64)
    d_in = torch.from_numpy(buf).cuda()
    before = d_in.clone()
    d_out = torch.full((batch * n + 2 * pad, w), POISON, dtype=torch.int64, device="cuda")
    d_inf = torch.full((batch * n + 2 * pad,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_y = torch.full((batch * n + 2 * pad, 4), POISON, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    c.prove_all_device(d_in.data_ptr(), k, batch, stride, d_out[pad:].data_ptr(), d_inf[pad:].data_ptr(),
                       d_y[pad:].data_ptr() if with_y else None, evals=evals, bitrev=bitrev_, stream=stream)
    torch.cuda.synchronize()
    assert torch.equal(d_in, before), "input changed"
    out, oi, oy = d_out.cpu().numpy(), d_inf.cpu().numpy(), d_y.cpu().numpy()
    for edge in (slice(0, pad), slice(pad + batch * n, None)):
        assert (out[edge] == POISON).all() and (oi[edge] == 0x5A5A5A5A).all() and (oy[edge] == POISON).all()
    if not with_y:
        assert (oy == POISON).all()
    body = slice(pad, pad + batch * n)
    return (out[body].view(np.uint64).reshape(batch, n, w), oi[body].reshape(batch, n).astype(bool),
            oy[body].view(np.uint64).reshape(batch, n, 4))


def test_first_call_on_a_fresh_stream():
    k = 5
    n, tau = 1 << k, K.default_tau(BLS)
    coeffs, xy, inf, y = case(k, tau)
    c = kzgx.Context("BLS12381")
    try:
        c.set_default_table(0)
        c.gen_srs(tau, n)
        st = torch.cuda.Stream()
        assert same(run_device(c, coeffs, k, stream=st.cuda_stream), xy, inf, y)  # twiddles and setup built on st
        assert same(c.prove_all(coeffs), xy, inf, y)  # the context's stream, ordered behind both builds
        st2 = torch.cuda.Stream()
        p = perm(k)
        assert same(run_device(c, y[:, p], k, evals=True, bitrev_=True, stream=st2.cuda_stream), xy[:, p], inf[:, p],
                    y[:, p])
    finally:
        c.close()


def test_caller_buffers(ctx):
    k = 3
    n, tau = 1 << k, K.default_tau(BLS)
    ctx.gen_srs(tau, n)
    coeffs, xy, inf, y = case(k, tau)
    assert same(run_device(ctx, coeffs, k), xy, inf, y)
    assert same(run_device(ctx, y, k, evals=True), xy, inf, y)
    got = run_device(ctx, coeffs, k, with_y=False)
    assert same(got, xy, inf)


# ---- 7. one chunk of polynomials, and one polynomial more ----------------------------------------------------
@pytest.mark.parametrize("extra", [0, 1])
def test_chunk_threshold(ctx, extra):
    k = 3
    n, tau = 1 << k, K.default_tau(BLS)
    ctx.gen_srs(tau, n)
    batch = (kzgx.G1_NTT_CHUNK_POINTS >> (k + 1)) + extra
    coeffs, xy, inf, y = case(k, tau)
    idx = np.arange(batch) % 3
    idx[-1] = 2  # the polynomial past the threshold is the one with 0, 1, r - 1
    got = ctx.prove_all(coeffs[idx])
    assert same(got, xy[idx], inf[idx], y[idx])
    got = ctx.prove_all(y[idx], evals=True, want_y=False)
    assert same(got, xy[idx], inf[idx])


# ---- 8. statuses ---------------------------------------------------------------------------------------------
def test_statuses(ctx):
    ctx.gen_srs(K.default_tau(BLS), 8)
    lib = kzgx.lib()
    d = torch.zeros((2, 16, 4), dtype=torch.int64, device="cuda")
    o = torch.zeros((32, 12), dtype=torch.int64, device="cuda")
    f = torch.zeros((32,), dtype=torch.int32, device="cuda")
    p, q, fl = d.data_ptr(), o.data_ptr(), f.data_ptr()
    assert lib.kzgx_prove_all_batch_device(ctx.h, p, 3, 0, 8, 0, q, fl, None, None) == 0  # batch 0
    assert lib.kzgx_prove_all_batch_device(ctx.h, p, 3, 2, 8, 0, q, fl, None, None) == 0
    assert lib.kzgx_prove_all_batch_device(ctx.h, p, 3, 2, 7, 0, q, fl, None, None) == ERR_ARG  # stride < n
    assert lib.kzgx_prove_all_batch_device(ctx.h, p, 3, 2, 8, 8, q, fl, None, None) == ERR_ARG  # unknown flag
    assert lib.kzgx_prove_all_batch_device(ctx.h, p, 3, 2, 8, kzgx.NTT_INVERSE, q, fl, None, None) == ERR_ARG
    assert lib.kzgx_prove_all_batch_device(ctx.h, p, 22, 1, 1 << 22, 0, q, fl, None, None) == ERR_ARG  # no 2^23 domain
    assert lib.kzgx_prove_all_batch_device(ctx.h, p, 4, 1, 16, 0, q, fl, None, None) == ERR_DEGREE  # 16 > 8 points
    assert lib.kzgx_prove_all_batch_device(ctx.h, None, 3, 2, 8, 0, q, fl, None, None) == ERR_ARG
    ctx.sync()
    with pytest.raises(kzgx.KzgxError) as e:
        ctx.prove_all(np.zeros((16, 4), dtype=np.uint64))
    assert e.value.status == ERR_DEGREE
    c = kzgx.Context("BLS12381")
    try:
        with pytest.raises(kzgx.KzgxError) as e:
            c.prove_all(np.zeros((4, 4), dtype=np.uint64))
        assert e.value.status == ERR_NO_SRS
    finally:
        c.close()


# ---- 9. BN254: the size-2n domain exists for n <= 2 ------------------------------------------------------------
def test_bn254():
    C = K.BN254
    c = kzgx.Context("BN254")
    try:
        c.set_default_table(0)
        tau = K.default_tau(C)
        c.gen_srs(tau, 4)
        for k in (0, 1):
            P = K.random_scalars(C, 1 << k, 0xB7 + k)
            xy, inf, y, ys = oracle("BN254", tau, P, k)
            assert same(c.prove_all(to_limbs(P)), xy, inf, y)
            assert same(c.prove_all(y, evals=True, bitrev=True), xy, inf, y)  # n <= 2: bit reversal is the identity
        with pytest.raises(kzgx.KzgxError) as e:
            c.prove_all(np.zeros((4, 4), dtype=np.uint64))  # log2n = 2: no size-8 domain
        assert e.value.status == ERR_ARG
        with pytest.raises(kzgx.KzgxError) as e:
            c.prove_all_prepare(2)
        assert e.value.status == ERR_ARG
    finally:
        c.close()
