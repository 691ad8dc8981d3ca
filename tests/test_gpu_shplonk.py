"""GPU tests of the Shplonk openings (kzgx_shplonk_commit / _open / _verify and their _device /
_checked forms; csrc/shplonk.hip): many polynomials opened at different point sets under one
two-point proof.

Expected values never come from the GPU path under test.  tests/shplonk_model.py works in Python
integers mod r: h coefficient by coefficient from a schoolbook floor division, the values, G, t,
and -- with the known tau, every commitment and proof being a known multiple of G -- the exponents
of W = [h(tau)]G and W' = [(G(tau) - G(z)) / (tau - z)]G and the verifier's equation.
corc.scalar_mul gives the expected point limbs."""
import copy
import ctypes

import numpy as np
import pytest

import corc
import kzg_ref as K
import shplonk_model as M

pytestmark = pytest.mark.gpu

CURVES = [("BN254", K.BN254), ("BLS12381", K.BLS12381)]
U64 = 0xFFFFFFFFFFFFFFFF
SRS_N = 2064  # the largest n below is KZGX_SHPLONK_TILE + 1


def w64(C):
    return 4 if C.name == "BN254" else 6


def scalars(vals):
    vals = list(vals)
    return corc.ints_to_limbs(vals, 4) if vals else np.zeros((0, 4), dtype=np.uint64)


def point(name, C, e):
    return corc.scalar_mul(name, (C.gx, C.gy), e % C.r) if e % C.r else None


def points(name, C, exps, cache):
    for e in exps:
        if e not in cache:
            cache[e] = point(name, C, e)
    P = [cache[e] for e in exps]
    return corc.points_to_array(name, P), np.array([q is None for q in P], dtype=np.int32)


def coeff_array(tab, stride):
    """(n_polys, stride, 4): the rows' padding holds non-canonical words that must never be read"""
    a = np.full((len(tab.polys), stride, 4), U64, dtype=np.uint64)
    for j, P in enumerate(tab.polys):
        a[j, :tab.n] = scalars(P)
    return a


@pytest.fixture(scope="module")
def env():
    import kzgx
    made = {}

    def get(name, C):
        if name not in made:
            tau = K.default_tau(C)
            ctx = kzgx.Context(name)
            ctx.gen_srs(tau, SRS_N)
            ctx.gen_srs_g2(tau, 2)
            made[name] = (ctx, tau, {})
        return made[name]

    yield get
    for ctx, _, _ in made.values():
        ctx.close()


def standard_sets():
    """(a) one point, one claim; (b) three points sharing one with (a), three claims with a polynomial
    repeated; (c) KZGX_SHPLONK_SET_MAX = 64 points; (d) no claims; (e) the repeated value at its other index"""
    return [([2], [2]), ([2, 0, 1], [0, 3, 0]), (list(range(3, 67)), [1, 4]), ([68], []), ([69, 67], [3])]


def standard_table(C, n, weights=None):
    """5 polynomials; T: 70 points with 0, r - 1 and one value at the indices 2 and 69"""
    r = C.r
    polys = [K.random_scalars(C, n, seed=1000 * n + j) for j in range(5)]
    T = K.random_scalars(C, 70, seed=17)
    T[0], T[1], T[69] = 0, r - 1, T[2]
    assert len(set(T)) == 69
    if weights is None:
        weights = K.random_scalars(C, 7, seed=31 * n + 5)
        weights[1], weights[2], weights[3] = 0, 1, r - 1
    return M.Table(r, polys, T, standard_sets(), weights)


def proof_exponents(tab, tau, h, z):
    r = tab.r
    G = tab.G(h, z)
    Gz = M.ev(r, G, z)
    return M.ev(r, h, tau), (M.ev(r, G, tau) - Gz) * pow(tau - z, -1, r) % r, G, Gz


def run_prover(ctx, tab, z, stride, weights=None, powers=False):
    c = coeff_array(tab, stride)
    w = scalars(tab.w if weights is None else weights)
    W, Winf, h, y = ctx.shplonk_commit(c, scalars(tab.T), tab.sets, w, powers=powers, n=tab.n)
    Wp, Wpinf, Gz = ctx.shplonk_open(c, scalars(tab.T), tab.sets, w, h, scalars([z]), powers=powers, n=tab.n)
    return W, Winf, h, y, Wp, Wpinf, Gz


def check_against_model(name, C, ctx, tau, cache, tab, z, got):
    W, Winf, h, y, Wp, Wpinf, Gz = got
    r = C.r
    mh = tab.h()
    assert corc.limbs_to_ints(h) == mh and mh[tab.n - 1] == 0
    assert corc.limbs_to_ints(y) == tab.values()
    eW, eWp, G, mGz = proof_exponents(tab, tau, mh, z)
    ys = tab.values()
    _, t = tab.verifier_scalars(ys, z, len(tab.polys))
    assert mGz == t and corc.limbs_to_ints(Gz.reshape(1, 4)) == [t]
    ex, ei = points(name, C, [eW, eWp], cache)
    assert [Winf, Wpinf] == [bool(v) for v in ei]
    assert np.array_equal(W, ex[0]) and np.array_equal(Wp, ex[1])
    return G, eW, eWp


@pytest.mark.parametrize("name,C", CURVES)
@pytest.mark.parametrize("n", [1, 2, 5, 63, 64, 65, 257, 1030, 2048, 2049])
def test_standard_model(name, C, n, env):
    """n <= 64 gives set (c) a zero share, n = 65 a constant one; 2048 / 2049 sit on both sides of
    KZGX_SHPLONK_TILE (one tile; two tiles with carries across)"""
    import kzgx
    assert kzgx.SHPLONK_TILE == 2048 and kzgx.SHPLONK_SET_MAX == 64
    ctx, tau, cache = env(name, C)
    r = C.r
    tab = standard_table(C, n)
    z = K.random_scalars(C, 1, seed=n + 99)[0]
    assert z != tau and z not in tab.T
    got = run_prover(ctx, tab, z, n + 3)
    G, eW, eWp = check_against_model(name, C, ctx, tau, cache, tab, z, got)
    if n <= 64:
        assert not any(M.floor_div(r, tab.folded(2), tab.vanishing(2)))
    # W' is bit for bit kzgx_prove_single_batch of the host-built G at z
    o2, i2, y2 = ctx.prove_single_batch(scalars(G).reshape(1, n, 4), scalars([z]), shared=False)
    assert np.array_equal(got[4], o2[0]) and bool(i2[0]) == got[5] and np.array_equal(got[6], y2[0])
    # the verifier accepts, through both entries
    commits, cinf = points(name, C, [M.ev(r, P, tau) for P in tab.polys], cache)
    proof = np.stack([got[0], got[4]])
    pinf = np.array([got[1], got[5]], dtype=np.int32)
    kw = dict(commit_inf=cinf, proof_inf=pinf)
    assert ctx.shplonk_verify(commits, scalars(tab.T), tab.sets, got[3], scalars(tab.w), scalars([z]), proof, **kw)
    assert ctx.shplonk_verify(commits, scalars(tab.T), tab.sets, got[3], scalars(tab.w), scalars([z]), proof,
                              checked=True, subgroup=1, **kw)
    # the other weight mode: one gamma, w_k = gamma^k, against the model under the explicit powers
    gamma = K.random_scalars(C, 1, seed=n + 7)[0]
    ptab = standard_table(C, n, weights=M.powers(r, gamma, 7))
    pgot = run_prover(ctx, ptab, z, n, weights=[gamma], powers=True)
    check_against_model(name, C, ctx, tau, cache, ptab, z, pgot)
    assert ctx.shplonk_verify(commits, scalars(ptab.T), ptab.sets, pgot[3], scalars([gamma]), scalars([z]),
                              np.stack([pgot[0], pgot[4]]), powers=True,
                              proof_inf=np.array([pgot[1], pgot[5]], dtype=np.int32), commit_inf=cinf)


@pytest.mark.parametrize("name,C", CURVES)
@pytest.mark.parametrize("n", [1, 33, 2049])
def test_single_claim_equals_prove_single_batch(name, C, n, env):
    """one set {t} with one claim of weight 1: W is bit-equal to kzgx_prove_single_batch(P, t)"""
    ctx, tau, cache = env(name, C)
    P = K.random_scalars(C, n, seed=4000 + n)
    t = K.random_scalars(C, 1, seed=4001)[0]
    tab = M.Table(C.r, [P], [t], [([0], [0])], [1])
    W, Winf, h, y = ctx.shplonk_commit(coeff_array(tab, n), scalars(tab.T), tab.sets, scalars([1]))
    o, i, yy = ctx.prove_single_batch(scalars(P).reshape(1, n, 4), scalars([t]), shared=False)
    assert np.array_equal(W, o[0]) and Winf == bool(i[0]) and np.array_equal(y[0], yy[0])
    assert corc.limbs_to_ints(h) == M.single_quotient(C.r, P, t) + [0]


def small_table(C, n=9, seed=500):
    """4 polynomials, 6 points, 4 sets; index 5 repeats index 1's value"""
    r = C.r
    polys = [K.random_scalars(C, n, seed=seed + j) for j in range(4)]
    T = K.random_scalars(C, 6, seed=seed + 9)
    T[5] = T[1]
    sets = [([0], [0, 1]), ([0, 1, 2], [2, 0]), ([3, 4], [3]), ([5, 2], [1])]
    return M.Table(r, polys, T, sets, K.random_scalars(C, 6, seed=seed + 10))


@pytest.mark.parametrize("name,C", CURVES)
def test_chunk_knob(name, C, env):
    """one set per chunk (and two): bits identical to the default; one fold and one quotient per chunk"""
    ctx, tau, cache = env(name, C)
    tab = small_table(C, n=65)
    z = 12345
    whole = run_prover(ctx, tab, z, 65)
    check_against_model(name, C, ctx, tau, cache, tab, z, whole)
    for chunk, launches in ((65, 4), (2 * 65, 2)):
        ctx.set_shplonk_chunk(chunk)
        try:
            ctx.prof_enable(True)
            ctx.prof_clear()
            c = coeff_array(tab, 65)
            part = ctx.shplonk_commit(c, scalars(tab.T), tab.sets, scalars(tab.w))
            ctx.sync()
            assert ctx.prof_read("shplonk_quotient")[1] == launches and ctx.prof_read("multi_fold")[1] == launches
        finally:
            ctx.prof_enable(False)
            ctx.prof_clear()
            ctx.set_shplonk_chunk(0)
        assert np.array_equal(part[0], whole[0]) and part[1] == whole[1]
        assert np.array_equal(part[2], whole[2]) and np.array_equal(part[3], whole[3])


# ---- verify ---------------------------------------------------------------------------------------
class Claims:
    """the verifier's view in exponents"""

    def __init__(self, name, C, tau, tab, z):
        self.name, self.C, self.tau, self.tab, self.z = name, C, tau, tab, z
        self.c = [M.ev(C.r, P, tau) for P in tab.polys]
        self.y = tab.values()
        self.W, self.Wp, _, _ = proof_exponents(tab, tau, tab.h(), z)

    def copy(self):
        return copy.deepcopy(self)

    def truth(self):
        return self.tab.verify(self.tau, self.c, self.y, self.z, self.W, self.Wp)

    def run(self, ctx, cache, **kw):
        cx, ci = points(self.name, self.C, self.c, cache)
        px, pi = points(self.name, self.C, [self.W, self.Wp], cache)
        return ctx.shplonk_verify(cx, scalars(self.tab.T), self.tab.sets, scalars(self.y), scalars(self.tab.w),
                                  scalars([self.z]), px, commit_inf=ci, proof_inf=pi, **kw)


def retable(tab, sets=None, w=None):
    return M.Table(tab.r, tab.polys, tab.T, tab.sets if sets is None else sets, tab.w if w is None else w)


@pytest.mark.parametrize("name,C", CURVES)
def test_verify_accepts_honest_and_rejects_each_single_mutation(name, C, env):
    ctx, tau, cache = env(name, C)
    r = C.r
    v = Claims(name, C, tau, small_table(C), 777)
    assert v.truth() and v.run(ctx, cache) is True and v.run(ctx, cache, checked=True, subgroup=1) is True
    cases = []
    t = v.copy()
    t.y[4] = (t.y[4] + 1) % r
    cases.append(("one y", t))
    t = v.copy()
    t.W = (t.W + 1) % r
    cases.append(("W", t))
    t = v.copy()
    t.Wp = (t.Wp + 1) % r
    cases.append(("W'", t))
    t = v.copy()
    t.z = (t.z + 1) % r
    cases.append(("z", t))
    t = v.copy()
    w = list(t.tab.w)
    w[3] = (w[3] + 1) % r
    t.tab = retable(t.tab, w=w)
    cases.append(("one weight", t))
    t = v.copy()
    t.c[2] = (t.c[2] + 1) % r
    cases.append(("one commitment", t))
    t = v.copy()
    sets = copy.deepcopy(t.tab.sets)
    sets[0][1][0] = 3  # claim 0 names commitment 3 instead of 0
    t.tab = retable(t.tab, sets=sets)
    cases.append(("one commit_index", t))
    t = v.copy()
    sets = copy.deepcopy(t.tab.sets)
    sets[2][0].remove(4)  # point 4 moves from set 2 to set 0: the values keep their order, the layout shifts
    sets[0][0].append(4)
    t.tab = retable(t.tab, sets=sets)
    assert t.tab.n_values == len(t.y) + 1
    t.y = t.y + [5]
    cases.append(("one point moved between sets", t))
    for label, t in cases:
        assert not t.truth(), label
        assert t.run(ctx, cache) is False, label


@pytest.mark.parametrize("name,C", CURVES)
def test_verify_equals_the_model_on_random_inputs_and_for_z_in_T(name, C, env):
    """the entry computes the stated equation and nothing else"""
    ctx, tau, cache = env(name, C)
    r = C.r
    base = Claims(name, C, tau, small_table(C, seed=600), 31337)
    # z in T: product form, no division by (z - t_i); honest proofs still pass
    for i in (0, 2, 5):
        v = Claims(name, C, tau, base.tab, base.tab.T[i])
        assert v.truth() and v.run(ctx, cache) is True, i
    # z = T[3]: zeta_s = 0 for every set but set 2, whose claims alone the equation still sees
    v = Claims(name, C, tau, base.tab, base.tab.T[3])
    blind = v.copy()
    blind.y[0] = (blind.y[0] + 1) % r  # a claim of set 0
    seen = v.copy()
    seen.y[8] = (seen.y[8] + 1) % r  # the claim of set 2 (values 8, 9), its value at T[3] = z
    assert blind.truth() and blind.run(ctx, cache) is True
    assert not seen.truth() and seen.run(ctx, cache) is False
    # random, invalid inputs: small exponents for the points keep the expected limbs cheap
    rnd = np.random.RandomState(5)
    for trial in range(4):
        t = base.copy()
        t.y = [int(x) for x in rnd.randint(0, 1 << 30, size=len(t.y))]
        t.c = [int(x) for x in rnd.randint(1, 1 << 20, size=len(t.c))]
        t.W, t.Wp = int(rnd.randint(1, 1 << 20)), int(rnd.randint(1, 1 << 20))
        assert t.truth() is False and t.run(ctx, cache) is False
    # two wrong values in one claim whose errors cancel under the interpolation weights pass
    t = base.copy()
    L = t.tab.lagrange_at(2, t.z)  # set 2: claim 4 holds the values 8, 9
    t.y[8] = (t.y[8] + L[1]) % r
    t.y[9] = (t.y[9] - L[0]) % r
    assert t.truth() and t.run(ctx, cache) is True


def g1_row(C, P):
    nl = w64(C)
    return np.concatenate([corc.ints_to_limbs([P[0]], nl)[0], corc.ints_to_limbs([P[1]], nl)[0]])


@pytest.mark.parametrize("name,C", CURVES)
def test_checked_rejects_bad_points(name, C, env):
    """a commitment no claim names enters the MSM under the scalar 0, so the equation holds whatever the
    point is -- the _checked forms still reject it off the curve and, on BLS12-381, outside the subgroup"""
    ctx, tau, cache = env(name, C)
    tab = small_table(C)
    tab = M.Table(tab.r, tab.polys + [K.random_scalars(C, tab.n, seed=9)], tab.T, tab.sets, tab.w)
    v = Claims(name, C, tau, tab, 4242)
    assert 4 not in tab.index and v.truth()
    cx, ci = points(name, C, v.c, cache)
    px, pi = points(name, C, [v.W, v.Wp], cache)

    def run(c, **kw):
        return ctx.shplonk_verify(c, scalars(tab.T), tab.sets, scalars(v.y), scalars(tab.w), scalars([v.z]), px,
                                  commit_inf=ci, proof_inf=pi, **kw)

    assert run(cx) is True and run(cx, checked=True, subgroup=1) is True
    good = corc.array_to_points(name, cx[4:5])[0]
    off = cx.copy()
    off[4] = g1_row(C, (good[0], (good[1] + 1) % C.p))
    assert not K.on_curve(C, (good[0], (good[1] + 1) % C.p))
    assert run(off) is True
    assert run(off, checked=True, subgroup=0) is False and run(off, checked=True, subgroup=1) is False
    if name == "BLS12381":
        from test_subgroup_consts import g1_member, g1_order_point
        P = K.point_add(C, good, g1_order_point(3))
        assert K.on_curve(C, P) and not g1_member(C, P)
        out = cx.copy()
        out[4] = g1_row(C, P)
        assert run(out) is True and run(out, checked=True, subgroup=0) is True
        assert run(out, checked=True, subgroup=1) is False


# ---- device entries -------------------------------------------------------------------------------
def dev_tensor(a, dev):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).to(dev)


def back(t, dtype):
    return t.cpu().numpy().view(dtype)


def u32(v):
    return np.array(list(v), dtype=np.uint32)


class DevTable:
    """a table's arrays on the device, any of them replaceable"""

    def __init__(self, tab, dev, stride, **over):
        self.tab = tab
        a = dict(coeffs=coeff_array(tab, stride), T=scalars(tab.T), sps=u32(tab.set_point_start),
                 sp=u32(tab.set_points), cs=u32(tab.claim_start), index=u32(tab.index), w=scalars(tab.w))
        a.update(over)
        self.n_sp, self.count = len(a["sp"]), len(a["index"])
        self.t = {k: dev_tensor(v, dev) for k, v in a.items()}

    def p(self, k):
        return self.t[k].data_ptr()


def device_commit(ctx, d, n, stride, n_polys, n_points, n_values, st, dev, nl):
    import torch
    out = torch.full((2, 2 * nl), 7, dtype=torch.int64, device=dev)  # one canary row behind each output
    inf = torch.full((2,), 7, dtype=torch.int32, device=dev)
    h = torch.full((n + 1, 4), 7, dtype=torch.int64, device=dev)
    y = torch.full((n_values + 1, 4), 7, dtype=torch.int64, device=dev)
    ok = torch.full((2,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.shplonk_commit_device(d.p("coeffs"), n, stride, n_polys, d.p("T"), n_points, d.p("sps"), d.p("sp"), d.n_sp,
                              d.p("cs"), d.p("index"), len(d.tab.sets), d.p("w"), d.count, n_values, out.data_ptr(),
                              inf.data_ptr(), h.data_ptr(), y.data_ptr(), ok.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    for canary in (out[1], inf[1:], h[n], y[n_values], ok[1:]):
        assert (canary == 7).all()
    return (back(out, np.uint64)[0], bool(back(inf, np.int32)[0]), back(h, np.uint64)[:n],
            back(y, np.uint64)[:n_values], int(back(ok, np.int32)[0]), h)


@pytest.mark.parametrize("name,C", CURVES)
def test_device_entries_on_a_caller_stream(name, C, env):
    """the device forms give the host forms' bits; guard words around every output stay"""
    import torch
    ctx, tau, cache = env(name, C)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    nl = w64(C)
    n = 65
    tab = standard_table(C, n)
    z = 987654321
    host = run_prover(ctx, tab, z, 68)
    d = DevTable(tab, dev, 68)
    W, Winf, h, y, ok, d_h = device_commit(ctx, d, n, 68, 5, 70, tab.n_values, st, dev, nl)
    assert ok == 1 and np.array_equal(W, host[0]) and Winf == host[1]
    assert np.array_equal(h, host[2]) and np.array_equal(y, host[3])
    out = torch.full((2, 2 * nl), 7, dtype=torch.int64, device=dev)
    inf = torch.full((2,), 7, dtype=torch.int32, device=dev)
    gz = torch.full((2, 4), 7, dtype=torch.int64, device=dev)
    okk = torch.full((2,), 7, dtype=torch.int32, device=dev)
    dz = dev_tensor(scalars([z]), dev)
    torch.cuda.synchronize(dev)
    ctx.shplonk_open_device(d.p("coeffs"), n, 68, 5, d.p("T"), 70, d.p("sps"), d.p("sp"), d.n_sp, d.p("cs"),
                            d.p("index"), 5, d.p("w"), d.count, d_h.data_ptr(), dz.data_ptr(), out.data_ptr(),
                            inf.data_ptr(), gz.data_ptr(), okk.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(back(out, np.uint64)[0], host[4]) and bool(back(inf, np.int32)[0]) == host[5]
    assert np.array_equal(back(gz, np.uint64)[0], host[6]) and back(okk, np.int32).tolist() == [1, 7]
    for canary in (out[1], inf[1:], gz[1]):
        assert (canary == 7).all()
    # the verifier through device pointers: the honest proof and one wrong value, plain and checked
    v = Claims(name, C, tau, tab, z)
    bad = v.copy()
    bad.y[40] = (bad.y[40] + 1) % C.r
    assert v.truth() and not bad.truth()
    cx, ci = points(name, C, v.c, cache)
    proof = dev_tensor(np.stack([host[0], host[4]]), dev)
    pinf = dev_tensor(np.array([host[1], host[5]], dtype=np.int32), dev)
    dcx, dci = dev_tensor(cx, dev), dev_tensor(ci, dev)
    oks, keep = [], []
    for case, checked in ((v, False), (bad, False), (v, True), (bad, True)):
        dy = dev_tensor(scalars(case.y), dev)
        o = torch.full((2,), 7, dtype=torch.int32, device=dev)
        keep.append(dy)
        oks.append(o)
        torch.cuda.synchronize(dev)
        ctx.shplonk_verify_device(dcx.data_ptr(), dci.data_ptr(), 5, d.p("index"), d.p("T"), 70, d.p("sps"),
                                  d.p("sp"), d.n_sp, d.p("cs"), 5, dy.data_ptr(), tab.n_values, d.p("w"), d.count,
                                  dz.data_ptr(), proof.data_ptr(), pinf.data_ptr(), o.data_ptr(), checked=checked,
                                  subgroup=1, stream=st.cuda_stream)
    st.synchronize()
    assert [back(o, np.int32).tolist() for o in oks] == [[1, 7], [0, 7], [1, 7], [0, 7]]


@pytest.mark.parametrize("name,C", CURVES)
def test_device_entries_flag_malformed_tables(name, C, env):
    """indices out of range and malformed starts: KZGX_OK, d_ok = 0, nothing read or written out of bounds
    (the canaries stay).  A claim naming a polynomial out of range adds nothing and its values are 0: h
    and the other values are those of the table with that claim's weight 0."""
    import torch
    ctx, tau, cache = env(name, C)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    nl = w64(C)
    tab = small_table(C, n=33)
    n, nv = 33, tab.n_values
    good = device_commit(ctx, DevTable(tab, dev, 33), n, 33, 4, 6, nv, st, dev, nl)
    assert good[4] == 1 and corc.limbs_to_ints(good[2]) == tab.h()
    # claim 2 (the first of set 1, three values from offset 2) names polynomial 4 of 4
    idx = list(tab.index)
    idx[2] = 4
    got = device_commit(ctx, DevTable(tab, dev, 33, index=u32(idx)), n, 33, 4, 6, nv, st, dev, nl)
    w0 = list(tab.w)
    w0[2] = 0
    want_y = tab.values()
    want_y[2:5] = [0, 0, 0]
    assert got[4] == 0 and corc.limbs_to_ints(got[2]) == retable(tab, w=w0).h()
    assert corc.limbs_to_ints(got[3]) == want_y
    # a point index out of range; malformed starts; a wrong n_values; equal values in one set
    sp = list(tab.set_points)
    sp[1] = 6
    sps_dec = list(tab.set_point_start)
    sps_dec[2] = sps_dec[1] - 1
    sps_end = list(tab.set_point_start)
    sps_end[-1] += 1
    cs_dec = list(tab.claim_start)
    cs_dec[2] = cs_dec[3] + 1
    cs_first = list(tab.claim_start)
    cs_first[0] = 1
    T_eq = list(tab.T)
    T_eq[4] = T_eq[3]
    for label, over, values in (("point index", dict(sp=u32(sp)), nv), ("decreasing set_point_start", dict(sps=u32(sps_dec)), nv),
                                ("set_point_start past the total", dict(sps=u32(sps_end)), nv),
                                ("decreasing claim_start", dict(cs=u32(cs_dec)), nv),
                                ("claim_start not from 0", dict(cs=u32(cs_first)), nv), ("n_values", {}, nv - 1),
                                ("equal values in set 2", dict(T=scalars(T_eq)), nv)):
        got = device_commit(ctx, DevTable(tab, dev, 33, **over), n, 33, 4, 6, values, st, dev, nl)
        assert got[4] == 0, label
    # the verifier: a commitment index out of range, a malformed start and equal values force 0 although
    # everything else is the honest proof's
    z = 2024
    v = Claims(name, C, tau, tab, z)
    cx, ci = points(name, C, v.c, cache)
    px, pi = points(name, C, [v.W, v.Wp], cache)
    fixed = [dev_tensor(a, dev) for a in (cx, ci, scalars(v.y), scalars([z]), px, pi)]
    oks, keep = [], []
    for over in ({}, dict(index=u32(idx)), dict(cs=u32(cs_dec)), dict(sp=u32(sp)), dict(T=scalars(T_eq))):
        d = DevTable(tab, dev, 33, **over)
        o = torch.full((2,), 7, dtype=torch.int32, device=dev)
        keep.append(d)
        oks.append(o)
        torch.cuda.synchronize(dev)
        p = [x.data_ptr() for x in fixed]
        ctx.shplonk_verify_device(p[0], p[1], 4, d.p("index"), d.p("T"), 6, d.p("sps"), d.p("sp"), d.n_sp, d.p("cs"),
                                  4, p[2], nv, d.p("w"), d.count, p[3], p[4], p[5], o.data_ptr(),
                                  stream=st.cuda_stream)
    st.synchronize()
    assert [back(o, np.int32).tolist() for o in oks] == [[1, 7], [0, 7], [0, 7], [0, 7], [0, 7]]


# ---- statuses -------------------------------------------------------------------------------------
def status(fn):
    import kzgx
    try:
        fn()
    except kzgx.KzgxError as e:
        return e.status
    return 0


@pytest.mark.parametrize("name,C", CURVES)
def test_host_entry_statuses(name, C, env):
    import kzgx
    ctx, tau, cache = env(name, C)
    r = C.r
    L = kzgx.lib()
    u64p, u32p, intp = kzgx.u64p, kzgx.u32p, kzgx.intp
    tab = small_table(C, n=33)
    nv = tab.n_values
    z = 55
    v = Claims(name, C, tau, tab, z)
    cx, ci = points(name, C, v.c, cache)
    px, pi = points(name, C, [v.W, v.Wp], cache)
    base = dict(coeffs=coeff_array(tab, 36), n=33, stride=36, n_polys=4, T=scalars(tab.T), n_points=6,
                sps=u32(tab.set_point_start), sp=u32(tab.set_points), n_sp=len(tab.set_points),
                cs=u32(tab.claim_start), index=u32(tab.index), n_sets=4, w=scalars(tab.w), count=6, nv=nv, flags=0,
                h=scalars(tab.h()), z=scalars([z]), commits=cx, nc=4, ys=scalars(v.y), proof=px)
    out = np.zeros(2 * w64(C), dtype=np.uint64)
    inf = ctypes.c_int(7)
    hh = np.zeros((33, 4), dtype=np.uint64)
    okv = ctypes.c_int(7)

    def P(a, t=u64p):
        return None if a is None else a.ctypes.data_as(t)

    def commit_rc(c=None, **kw):
        a = dict(base, **kw)
        return L.kzgx_shplonk_commit((c or ctx).h, P(a["coeffs"]), a["n"], a["stride"], a["n_polys"], P(a["T"]),
                                     a["n_points"], P(a["sps"], u32p), P(a["sp"], u32p), a["n_sp"], P(a["cs"], u32p),
                                     P(a["index"], u32p), a["n_sets"], P(a["w"]), a["count"], a["nv"], a["flags"],
                                     P(a.get("out", out)), ctypes.byref(inf) if a.get("inf", 1) else None,
                                     P(a.get("hout", hh)), None)

    def open_rc(c=None, **kw):
        a = dict(base, **kw)
        return L.kzgx_shplonk_open((c or ctx).h, P(a["coeffs"]), a["n"], a["stride"], a["n_polys"], P(a["T"]),
                                   a["n_points"], P(a["sps"], u32p), P(a["sp"], u32p), a["n_sp"], P(a["cs"], u32p),
                                   P(a["index"], u32p), a["n_sets"], P(a["w"]), a["count"], a["flags"], P(a["h"]),
                                   P(a["z"]), P(a.get("out", out)), ctypes.byref(inf) if a.get("inf", 1) else None,
                                   None)

    def verify_rc(c=None, ok=True, **kw):
        a = dict(base, **kw)
        return L.kzgx_shplonk_verify((c or ctx).h, P(a["commits"]), P(ci, intp), a["nc"], P(a["index"], u32p),
                                     P(a["T"]), a["n_points"], P(a["sps"], u32p), P(a["sp"], u32p), a["n_sp"],
                                     P(a["cs"], u32p), a["n_sets"], P(a["ys"]), a["nv"], P(a["w"]), a["count"],
                                     P(a["z"]), P(a["proof"]), P(pi, intp), a["flags"],
                                     ctypes.byref(okv) if ok else None)

    def edited(a, i, val):
        b = a.copy()
        b[i] = val
        return b

    assert commit_rc() == 0 and open_rc() == 0 and verify_rc() == 0 and okv.value == 1
    calls = (("commit", commit_rc), ("open", open_rc), ("verify", verify_rc))
    # a NULL required pointer
    for key in ("coeffs", "T", "sps", "sp", "cs", "index", "w", "out", "inf", "hout"):
        assert commit_rc(**{key: None}) == -1, key
    for key in ("coeffs", "T", "sps", "sp", "cs", "index", "w", "h", "z", "out", "inf"):
        assert open_rc(**{key: None}) == -1, key
    for key in ("commits", "T", "sps", "sp", "cs", "index", "w", "ys", "z", "proof"):
        assert verify_rc(**{key: None}) == -1, key
    assert verify_rc(ok=False) == -1
    # n == 0, stride < n, unknown flags
    for fn in (commit_rc, open_rc):
        assert fn(n=0) == -1 and fn(stride=32) == -1
    sp_dup = edited(base["sp"], 2, base["sp"][1])              # set 1 = {0, 0, 2}
    T_eq = edited(base["T"], 4, base["T"][3])                  # set 2 = {3, 4} with equal values
    for label, fn in calls:
        assert fn(flags=2) == -1, label
        assert fn(n_sets=0) == -1 and fn(n_sets=1 << 16) == -1, label
        assert fn(sps=edited(base["sps"], 0, 1)) == -1, label                       # not from 0
        assert fn(sps=edited(base["sps"], 4, base["n_sp"] - 1)) == -1, label        # not to its total
        assert fn(sps=edited(base["sps"], 2, base["sps"][1])) == -1, label          # d_1 == 0
        assert fn(cs=edited(base["cs"], 0, 1)) == -1, label
        assert fn(cs=edited(base["cs"], 4, 5)) == -1, label
        assert fn(cs=edited(base["cs"], 2, base["cs"][3] + 1)) == -1, label         # decreasing
        assert fn(n_points=0) == -1 and fn(n_points=4097) == -1, label
        assert fn(n_points=5) == -1, label                                          # index 5 out of range
        assert fn(sp=edited(base["sp"], 0, 6)) == -1, label
        assert fn(index=edited(base["index"], 1, 4)) == -1, label
        assert fn(sp=sp_dup) == -1, label                                           # the same index twice in a set
        assert fn(T=edited(base["T"], 1, scalars([r])[0])) == -1, label             # a scalar >= r
        assert fn(w=edited(base["w"], 5, scalars([r + 1])[0])) == -1, label
        assert fn(count=1 << 31) == -1, label
        assert fn(T=T_eq) == -8, label                                              # KZGX_ERR_DIV_ZERO
        assert fn(T=T_eq, flags=2) == -1, label                                     # arguments first
        assert fn(flags=kzgx.SHPLONK_WEIGHT_POWERS) == 0, label                     # the first weight as gamma
    # d_s > KZGX_SHPLONK_SET_MAX: one set of 65 points
    big = dict(T=scalars(range(1, 71)), n_points=70, sps=u32([0, 65]), sp=u32(range(65)), n_sp=65, cs=u32([0, 1]),
               index=u32([0]), n_sets=1, w=scalars([1]), count=1)
    assert commit_rc(nv=65, **big) == -1 and open_rc(**big) == -1 and verify_rc(nv=65, ys=scalars(range(65)), **big) == -1
    # a wrong n_values (the open entry has none); values and z >= r
    assert commit_rc(nv=nv + 1) == -1 and verify_rc(nv=nv - 1) == -1
    assert verify_rc(ys=edited(base["ys"], 3, scalars([r])[0])) == -1
    assert verify_rc(z=scalars([r])) == -1 and open_rc(z=scalars([r])) == -1
    assert open_rc(h=edited(base["h"], 0, scalars([r])[0])) == -1
    assert verify_rc(nc=3) == -1  # index 3 is now out of range
    assert verify_rc(nc=(1 << 22) - 2) == -1  # n_commits + 3 > KZGX_MSM_POINTS_MAX
    # the setup
    one = dict(coeffs=np.zeros((1, SRS_N + 4, 4), dtype=np.uint64), n_polys=1, stride=SRS_N + 4, T=scalars([3]),
               n_points=1, sps=u32([0, 1]), sp=u32([0]), n_sp=1, cs=u32([0, 1]), index=u32([0]), n_sets=1,
               w=scalars([1]), count=1, nv=1)
    big_h = np.zeros((SRS_N + 2, 4), dtype=np.uint64)
    assert commit_rc(n=SRS_N + 1, hout=big_h, **one) == 0      # degree SRS_N = the setup's size
    assert commit_rc(n=SRS_N + 2, hout=big_h, **one) == -5     # KZGX_ERR_DEGREE
    del one["nv"]
    assert open_rc(n=SRS_N + 2, h=big_h, **one) == -5
    bare = kzgx.Context(name)
    try:
        assert commit_rc(c=bare) == -4 and open_rc(c=bare) == -4 and verify_rc(c=bare) == -4  # KZGX_ERR_NO_SRS
        assert commit_rc(c=bare, n=0) == -1                    # arguments first
        bare.gen_srs(tau, 8)                                   # G1 only: the verify needs G2[0..1] too
        assert verify_rc(c=bare) == -4
    finally:
        bare.close()
    # device entries: what the host can see
    import torch
    dev = torch.device("cuda", 0)
    buf = torch.zeros(4096, dtype=torch.int64, device=dev)
    b = buf.data_ptr()
    assert status(lambda: ctx.shplonk_commit_device(b, 4, 4, 1, b, 1, b, b, 1, b, b, 1, None, 1, 1, b, b, b)) == -1
    assert status(lambda: ctx.shplonk_commit_device(b, 4, 3, 1, b, 1, b, b, 1, b, b, 1, b, 1, 1, b, b, b)) == -1
    assert status(lambda: ctx.shplonk_commit_device(b, 4, 4, 1, b, 1, b, b, 65, b, b, 1, b, 1, 1, b, b, b)) == -1
    assert status(lambda: ctx.shplonk_open_device(b, 4, 4, 1, b, 1, b, b, 1, b, b, 1, b, 1, b, None, b, b)) == -1
    assert status(lambda: ctx.shplonk_verify_device(b, None, 1, b, b, 1, b, b, 1, b, 1, b, 1, b, 1, b, b, None,
                                                    None)) == -1
    torch.cuda.synchronize(dev)
