"""GPU: coset (cell) openings (kzgx_prove_cosets_batch / _device / _prepare, csrc/g1_ntt.hip): one proof
per coset of l points of the size-n or size-2n domain, by the multi-point Feist-Khovratovich.

Checker: with a known tau the proof of P on the coset {x : x^l = a} is [(P(tau) - I(tau)) / (tau^l - a)]G,
I = P mod (X^l - a) by the oracle's poly_divmod, one K.scalar_mul per proof, and y by the oracle's Horner;
bit-exact on canonical limbs and infinity flags.  Larger sizes are compared limb for limb with
kzgx_prove_range over kzgx_coset_points and run through kzgx_verify_proof."""
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
EXT = kzgx.PROVE_COSETS_EXTENDED


def to_limbs(vals) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


@functools.lru_cache(maxsize=None)
def perm(k):
    return np.array([bitrev(i, k) for i in range(1 << k)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def mulG(curve, a):
    C = K.CURVES[curve]
    return K.scalar_mul(C, (C.gx, C.gy), a)


def oracle(curve, tau, coeffs, k, kl, ext):
    """-> (proof limbs (R, 2 w64), flags (R,), y limbs (R, l, 4)), natural order"""
    C = K.CURVES[curve]
    r, kr, l = C.r, k - kl + ext, 1 << kl
    R = 1 << kr
    w = kzgx.domain_root(curve, kr + kl)
    P = list(coeffs)
    ptau, taul = K.poly_eval(C, P, tau), pow(tau, l, r)
    pts, ys = [], []
    for i in range(R):
        a = pow(w, i * l, r)
        _, rem = K.poly_divmod(C, P, [(-a) % r] + [0] * (l - 1) + [1])
        pts.append(mulG(curve, (ptau - K.poly_eval(C, list(rem), tau)) * pow(taul - a, -1, r) % r))
        ys.append(to_limbs([K.poly_eval(C, P, pow(w, i + R * j, r)) for j in range(l)]))
    return corc.points_to_array(curve, pts), np.array([p is None for p in pts]), np.stack(ys)


@functools.lru_cache(maxsize=None)
def polys(k):
    """three polynomials of 2^k coefficients, the third with 0, 1, r - 1 forced in (test_gpu_prove_all.case)"""
    n = 1 << k
    ps = [K.random_scalars(BLS, n, 0xF20 + 16 * k + j) for j in range(3)]
    for i, v in enumerate((0, 1, BLS.r - 1)):
        if i < n:
            ps[2][(i + 1) % n] = v
    return ps


@functools.lru_cache(maxsize=None)
def case(k, kl, ext, tau):
    """-> coefficients (3, n, 4), their values on the size-n domain (3, n, 4), proofs (3, R, 2 w64),
    flags (3, R), y (3, R, l, 4); everything in natural order"""
    ps = polys(k)
    w = kzgx.domain_root("BLS12381", k)
    ev = [to_limbs([K.poly_eval(BLS, P, pow(w, i, BLS.r)) for i in range(1 << k)]) for P in ps]
    exp = [oracle("BLS12381", tau, P, k, kl, ext) for P in ps]
    return (np.stack([to_limbs(P) for P in ps]), np.stack(ev), np.stack([e[0] for e in exp]),
            np.stack([e[1] for e in exp]), np.stack([e[2] for e in exp]))


def cells(y, kr, kl):
    """natural coset order (.., R, l, 4) -> the cells of the bit-reversed evaluation array"""
    return y[..., perm(kr), :, :][..., perm(kl), :]


@pytest.fixture(scope="module")
def ctx():
    c = kzgx.Context("BLS12381")
    c.set_default_table(0)  # small SRSs below: keep the setups quick (the MSM paths have their own tests)
    yield c
    c.close()


def same(got, want_xy, want_inf, want_y=None):
    ok = (got[0] == want_xy).all() and (got[1] == want_inf).all()
    return ok and (want_y is None or (got[2] == want_y).all())


# ---- 1. against the oracle: both domains, both orders, coefficient and evaluation input ----------------
SHAPES = [(1, 0), (1, 1), (2, 1), (3, 0), (3, 1), (3, 2), (3, 3), (4, 2), (5, 2), (5, 4)]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("k,kl", SHAPES)
def test_against_the_oracle(ctx, k, kl, ext, batch):
    n, tau, kr = 1 << k, K.default_tau(BLS), k - kl + ext
    ctx.gen_srs(tau, n)  # exactly n points
    coeffs, ev, xy, inf, y = (x[:batch] for x in case(k, kl, ext, tau))
    p, pn = perm(kr), perm(k)
    e = bool(ext)
    assert same(ctx.prove_cosets(coeffs, kl, extended=e), xy, inf, y)
    assert same(ctx.prove_cosets(coeffs, kl, extended=e, bitrev=True), xy[:, p], inf[:, p], cells(y, kr, kl))
    assert same(ctx.prove_cosets(ev, kl, extended=e, evals=True), xy, inf, y)
    assert same(ctx.prove_cosets(ev[:, pn], kl, extended=e, evals=True, bitrev=True), xy[:, p], inf[:, p],
                cells(y, kr, kl))
    got = ctx.prove_cosets(coeffs[0], kl, extended=e, want_y=False)  # one polynomial, no y
    assert same(got, xy[0], inf[0]) and got[2] is None
    if k == kl:
        assert inf.all()  # m = 1: every quotient is zero


# ---- 2. against the existing path: kzgx_prove_range over kzgx_coset_points -----------------------------
@pytest.mark.parametrize("k,kl,ext", [(8, 3, 0), (8, 3, 1), (9, 7, 1)])
def test_against_prove_range(ctx, k, kl, ext):
    n, tau, R = 1 << k, K.default_tau(BLS), 1 << (k - kl + ext)
    ctx.gen_srs(tau, n + 37)
    coeffs = to_limbs(K.random_scalars(BLS, n, 0xC05 + 16 * k + kl))
    xy, inf, y = ctx.prove_cosets(coeffs, kl, extended=bool(ext))
    assert xy.shape[0] == R and not inf.any()
    for i in range(R):
        xs = kzgx.coset_points("BLS12381", k, kl, i, extended=bool(ext))
        ref, ref_inf = ctx.prove_range(coeffs, xs)
        assert (xy[i] == ref).all() and inf[i] == ref_inf, i
        if i in (0, R - 1):
            assert (y[i] == ctx.poly_eval(coeffs, xs)).all()


# ---- 3. the data-availability shape: 4096 values, extended, 128 cells of 64 -------------------------------
def test_data_availability_shape(ctx):
    k, kl, batch = 12, 6, 2
    n, tau, R, l = 1 << k, K.default_tau(BLS), 128, 64
    ctx.gen_srs(tau, n)
    ctx.gen_srs_g2(tau, l + 1)
    coeffs = np.stack([to_limbs(K.random_scalars(BLS, n, 0xDA5 + b)) for b in range(batch)])
    blob = ctx.ntt(coeffs, bitrev=True)  # the values on the size-n domain, bit-reversed
    xy, inf, y = ctx.prove_cosets(blob, kl, extended=True, evals=True, bitrev=True)
    assert xy.shape == (batch, R, 2 * ctx.w64) and y.shape == (batch, R, l, 4) and not inf.any()
    # brev_2n(e) = 2 brev_n(e) for e < n: the first half of the cells is the blob itself
    assert (y.reshape(batch, 2 * n, 4)[:, :n] == blob).all()
    for b in range(batch):
        c_xy, c_inf = ctx.msm(coeffs[b])
        for idx, p in enumerate((0, 42, 85, R - 1)):
            xs = kzgx.coset_points("BLS12381", k, kl, p, extended=True, bitrev=True)
            ref, ref_inf = ctx.prove_range(coeffs[b], xs)
            assert (xy[b, p] == ref).all() and inf[b, p] == ref_inf, (b, p)
            if idx % 2 == b:
                assert ctx.verify_proof(c_xy, c_inf, xy[b, p], bool(inf[b, p]), xs, y[b, p])
                bad = y[b, p].copy()
                bad[[5, 9]] = bad[[9, 5]]
                assert not ctx.verify_proof(c_xy, c_inf, xy[b, p], bool(inf[b, p]), xs, bad)


# ---- 4. l = 1 on the size-n domain is the all-domain opening ------------------------------------------------
def test_single_point_cosets_equal_prove_all(ctx):
    k = 5
    n, tau = 1 << k, K.default_tau(BLS)
    ctx.gen_srs(tau, n)
    coeffs = np.stack([to_limbs(P) for P in polys(k)])
    for rev in (False, True):
        axy, ainf, ay = ctx.prove_all(coeffs, bitrev=rev)
        got = ctx.prove_cosets(coeffs, 0, bitrev=rev)
        assert same(got, axy, ainf, ay.reshape(3, n, 1, 4))


# ---- 5. degenerate polynomials --------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [0, 1])
def test_degenerate_polynomials(ctx, ext):
    k, kl = 4, 2
    n, l, tau = 1 << k, 1 << kl, K.default_tau(BLS)
    ctx.gen_srs(tau, n)
    c = K.random_scalars(BLS, n, 0xDE7)
    rows = [[0] * n, [c[0]] + [0] * (n - 1), c[:l] + [0] * (n - l), c[:l + 1] + [0] * (n - l - 1)]
    exp = [oracle("BLS12381", tau, P, k, kl, ext) for P in rows]
    xy, inf, y = ctx.prove_cosets(np.stack([to_limbs(P) for P in rows]), kl, extended=bool(ext))
    for b in range(4):
        assert same((xy[b], inf[b], y[b]), *exp[b]), b
    assert inf[:3].all() and not inf[3].any()  # zero, a constant, degree < l: no quotient; degree l: a constant one
    assert not y[0].any() and (y[1] == to_limbs([c[0]])[0]).all()
    assert (xy[3] == xy[3, 0]).all()  # q = f_l whatever the coset


@pytest.mark.parametrize("ext", [0, 1])
def test_one_coset_is_the_whole_domain(ctx, ext):
    k = 3
    tau = K.default_tau(BLS)
    ctx.gen_srs(tau, 1 << k)
    coeffs, ev, xy, inf, y = case(k, k, ext, tau)
    assert inf.all() and inf.shape == (3, 1 << ext)
    for rev in (False, True):
        got = ctx.prove_cosets(coeffs, k, extended=bool(ext), bitrev=rev)
        assert same(got, xy, inf, cells(y, ext, k) if rev else y)


# ---- 6. the setup cache -------------------------------------------------------------------------------------------
def test_two_coset_sizes_share_a_context(ctx):
    k, tau = 3, K.default_tau(BLS)
    ctx.gen_srs(tau, 1 << k)
    for kl in (1, 2, 1, 0, 2):
        coeffs, _, xy, inf, y = case(k, kl, 0, tau)
        assert same(ctx.prove_cosets(coeffs, kl), xy, inf, y), kl


def test_srs_change(ctx):
    k, kl = 3, 1
    n, tau = 1 << k, K.default_tau(BLS)
    tau2 = (tau * 3 + 11) % BLS.r
    coeffs = case(k, kl, 0, tau)[0]
    for t in (tau, tau2, tau):
        ctx.gen_srs(t, n + 5)
        _, _, xy, inf, y = case(k, kl, 0, t)
        assert same(ctx.prove_cosets(coeffs, kl), xy, inf, y)
    assert not (case(k, kl, 0, tau)[2] == case(k, kl, 0, tau2)[2]).all()
    srs = ctx.get_srs()
    ctx.gen_srs(tau2, n)
    assert same(ctx.prove_cosets(coeffs, kl), *case(k, kl, 0, tau2)[2:])
    ctx.load_srs(srs)  # tau's points again, through the loader
    assert same(ctx.prove_cosets(coeffs, kl), *case(k, kl, 0, tau)[2:])


def test_prepare():
    c = kzgx.Context("BLS12381")
    try:
        c.set_default_table(0)
        with pytest.raises(kzgx.KzgxError) as e:
            c.prove_cosets_prepare(3, 1)
        assert e.value.status == ERR_NO_SRS
        tau = K.default_tau(BLS)
        c.gen_srs(tau, 8)
        c.prove_cosets_prepare(3, 1)
        c.prove_cosets_prepare(3, 1)
        c.prove_cosets_prepare(3, 3)  # m = 1: nothing to build
        coeffs, _, xy, inf, y = case(3, 1, 0, tau)
        assert same(c.prove_cosets(coeffs, 1), xy, inf, y)
        with pytest.raises(kzgx.KzgxError) as e:
            c.prove_cosets_prepare(4, 1)  # 16 > the 8 SRS points
        assert e.value.status == ERR_DEGREE
        for shape in ((22, 0), (3, 4)):
            with pytest.raises(kzgx.KzgxError) as e:
                c.prove_cosets_prepare(*shape)
            assert e.value.status == ERR_ARG
    finally:
        c.close()


# ---- 7. device entry: the first call on a fresh stream, strided input, poisoned padding ----------------------
def run_device(c, rows, k, kl, ext, evals=False, bitrev_=False, stream=None, with_y=True):
    batch, n, w = rows.shape[0], 1 << k, 2 * c.w64
    R, l = 1 << (k - kl + ext), 1 << kl
    stride, pad = n + 3, 4
    buf = np.full((batch, stride, 4), POISON, dtype=np.int64)
    buf[:, :n] = rows.view(np.int64)
    d_in = torch.from_numpy(buf).cuda()
    before = d_in.clone()
    d_out = torch.full((batch * R + 2 * pad, w), POISON, dtype=torch.int64, device="cuda")
    d_inf = torch.full((batch * R + 2 * pad,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_y = torch.full((batch * R * l + 2 * pad, 4), POISON, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    c.prove_cosets_device(d_in.data_ptr(), k, kl, batch, stride, d_out[pad:].data_ptr(), d_inf[pad:].data_ptr(),
                          d_y[pad:].data_ptr() if with_y else None, extended=bool(ext), evals=evals, bitrev=bitrev_,
                          stream=stream)
    torch.cuda.synchronize()
    assert torch.equal(d_in, before), "input changed"
    out, oi, oy = d_out.cpu().numpy(), d_inf.cpu().numpy(), d_y.cpu().numpy()
    for edge in (slice(0, pad), slice(pad + batch * R, None)):
        assert (out[edge] == POISON).all() and (oi[edge] == 0x5A5A5A5A).all()
    for edge in (slice(0, pad), slice(pad + batch * R * l, None)):
        assert (oy[edge] == POISON).all()
    if not with_y:
        assert (oy == POISON).all()
    return (out[pad:pad + batch * R].view(np.uint64).reshape(batch, R, w),
            oi[pad:pad + batch * R].reshape(batch, R).astype(bool),
            oy[pad:pad + batch * R * l].view(np.uint64).reshape(batch, R, l, 4))


def test_first_call_on_a_fresh_stream():
    k, kl, ext = 5, 2, 1
    n, tau, kr = 1 << k, K.default_tau(BLS), k - kl + ext
    coeffs, ev, xy, inf, y = case(k, kl, ext, tau)
    c = kzgx.Context("BLS12381")
    try:
        c.set_default_table(0)
        c.gen_srs(tau, n)
        st = torch.cuda.Stream()
        assert same(run_device(c, coeffs, k, kl, ext, stream=st.cuda_stream), xy, inf, y)  # builds run on st
        assert same(c.prove_cosets(coeffs, kl, extended=True), xy, inf, y)  # the context's stream, behind the builds
        st2 = torch.cuda.Stream()
        p = perm(kr)
        got = run_device(c, ev[:, perm(k)], k, kl, ext, evals=True, bitrev_=True, stream=st2.cuda_stream)
        assert same(got, xy[:, p], inf[:, p], cells(y, kr, kl))
    finally:
        c.close()


@pytest.mark.parametrize("ext", [0, 1])
def test_caller_buffers(ctx, ext):
    k, kl = 3, 1
    tau = K.default_tau(BLS)
    ctx.gen_srs(tau, 1 << k)
    coeffs, ev, xy, inf, y = case(k, kl, ext, tau)
    assert same(run_device(ctx, coeffs, k, kl, ext), xy, inf, y)
    assert same(run_device(ctx, ev, k, kl, ext, evals=True), xy, inf, y)
    assert same(run_device(ctx, coeffs, k, kl, ext, with_y=False), xy, inf)
    assert same(run_device(ctx, coeffs, k, kl, ext, bitrev_=True, with_y=False), xy[:, perm(k - kl + ext)],
                inf[:, perm(k - kl + ext)])


# ---- 8. one chunk of polynomials, and one polynomial more ----------------------------------------------------
@pytest.mark.parametrize("extra", [0, 1])
def test_chunk_threshold(ctx, extra):
    k, kl = 3, 1
    n, tau = 1 << k, K.default_tau(BLS)
    ctx.gen_srs(tau, n)
    batch = (kzgx.G1_NTT_CHUNK_POINTS >> (k + 1)) + extra
    coeffs, ev, xy, inf, y = case(k, kl, 0, tau)
    idx = np.arange(batch) % 3
    idx[-1] = 2  # the polynomial past the threshold is the one with 0, 1, r - 1
    assert same(ctx.prove_cosets(coeffs[idx], kl), xy[idx], inf[idx], y[idx])
    assert same(ctx.prove_cosets(ev[idx], kl, evals=True, want_y=False), xy[idx], inf[idx])


# ---- 9. statuses ---------------------------------------------------------------------------------------------
def test_statuses(ctx):
    ctx.gen_srs(K.default_tau(BLS), 8)
    f_ = kzgx.lib().kzgx_prove_cosets_batch_device
    d = torch.zeros((2, 16, 4), dtype=torch.int64, device="cuda")
    o = torch.zeros((32, 12), dtype=torch.int64, device="cuda")
    f = torch.zeros((32,), dtype=torch.int32, device="cuda")
    yy = torch.zeros((64, 4), dtype=torch.int64, device="cuda")
    p, q, fl, py = d.data_ptr(), o.data_ptr(), f.data_ptr(), yy.data_ptr()
    assert f_(ctx.h, p, 3, 1, 0, 8, 0, q, fl, None, None) == 0  # batch 0
    assert f_(ctx.h, p, 3, 1, 2, 8, 0, q, fl, py, None) == 0
    assert f_(ctx.h, p, 3, 1, 2, 8, EXT | kzgx.NTT_BITREV | kzgx.PROVE_ALL_EVALS, q, fl, py, None) == 0
    assert f_(ctx.h, p, 3, 1, 2, 7, 0, q, fl, None, None) == ERR_ARG  # stride < n
    assert f_(ctx.h, p, 3, 1, 2, 8, 16, q, fl, None, None) == ERR_ARG  # unknown flag
    assert f_(ctx.h, p, 3, 1, 2, 8, kzgx.NTT_INVERSE, q, fl, None, None) == ERR_ARG
    assert f_(ctx.h, p, 3, 4, 2, 8, 0, q, fl, None, None) == ERR_ARG  # l > n
    assert f_(ctx.h, p, 22, 0, 1, 1 << 22, 0, q, fl, None, None) == ERR_ARG  # no 2^23 domain for the products
    assert f_(ctx.h, p, 22, 4, 1, 1 << 22, EXT, q, fl, None, None) == ERR_ARG  # no 2^23 domain to open on
    assert f_(ctx.h, p, 22, 4, 1, 1 << 22, 0, q, fl, None, None) == ERR_DEGREE  # a valid shape past the SRS
    assert f_(ctx.h, p, 4, 1, 1, 16, 0, q, fl, None, None) == ERR_DEGREE  # 16 > 8 points
    assert f_(ctx.h, None, 3, 1, 2, 8, 0, q, fl, None, None) == ERR_ARG
    assert f_(ctx.h, p, 3, 1, 2, 8, 0, None, fl, None, None) == ERR_ARG
    assert f_(ctx.h, p, 3, 1, 2, 8, 0, q, None, None, None) == ERR_ARG
    ctx.sync()
    with pytest.raises(kzgx.KzgxError) as e:
        ctx.prove_cosets(np.zeros((16, 4), dtype=np.uint64), 1)
    assert e.value.status == ERR_DEGREE
    with pytest.raises(kzgx.KzgxError) as e:
        ctx.prove_cosets(np.zeros((8, 4), dtype=np.uint64), 4)
    assert e.value.status == ERR_ARG
    c = kzgx.Context("BLS12381")
    try:
        with pytest.raises(kzgx.KzgxError) as e:
            c.prove_cosets(np.zeros((4, 4), dtype=np.uint64), 1)
        assert e.value.status == ERR_NO_SRS
    finally:
        c.close()


# ---- 10. BN254: domains of at most 4 points --------------------------------------------------------------------
def test_bn254():
    C = K.BN254
    c = kzgx.Context("BN254")
    try:
        c.set_default_table(0)
        tau = K.default_tau(C)
        c.gen_srs(tau, 4)
        for k, kl, ext in ((2, 1, 0), (1, 0, 0), (1, 0, 1), (2, 2, 0), (1, 1, 0), (1, 1, 1)):
            P = K.random_scalars(C, 1 << k, 0xB7 + 4 * k + kl)
            xy, inf, y = oracle("BN254", tau, P, k, kl, ext)
            kr = k - kl + ext
            assert same(c.prove_cosets(to_limbs(P), kl, extended=bool(ext)), xy, inf, y), (k, kl, ext)
            got = c.prove_cosets(to_limbs(P), kl, extended=bool(ext), bitrev=True)
            assert same(got, xy[perm(kr)], inf[perm(kr)], cells(y, kr, kl)), (k, kl, ext)
            if k == kl:
                assert inf.all()
        for k, kl, ext in ((2, 0, 0), (2, 1, 1), (2, 2, 1)):
            with pytest.raises(kzgx.KzgxError) as e:
                c.prove_cosets(np.zeros((1 << k, 4), dtype=np.uint64), kl, extended=bool(ext))
            assert e.value.status == ERR_ARG
        with pytest.raises(kzgx.KzgxError) as e:
            c.prove_cosets_prepare(2, 0)
        assert e.value.status == ERR_ARG
    finally:
        c.close()
