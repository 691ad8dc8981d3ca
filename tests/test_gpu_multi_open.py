"""GPU tests of the batch openings (kzgx_prove_multi_batch / kzgx_verify_multi_batch and their
_device / _checked forms; csrc/multi_open.hip): many polynomials opened at shared points, one
proof per point.

Expected values never come from the GPU path under test.  With the known tau every commitment
and proof is a known multiple of G, so Python integers give
  y_k = P_k(z_g),  F_g(tau) = sum w_k P_k(tau),  Y_g = sum w_k y_k,
  the proof's exponent q_g(tau) = (F_g(tau) - Y_g) / (tau - z_g)                      (mod r)
  the verify equation  tau sum r_g p_g == sum_c s_c c_c + sum r_g z_g p_g - t          (mod r)
and corc.scalar_mul the expected proof limbs."""
import ctypes

import numpy as np
import pytest

import corc
import kzg_ref as K

pytestmark = pytest.mark.gpu

CURVES = [("BN254", K.BN254), ("BLS12381", K.BLS12381)]
U64 = 0xFFFFFFFFFFFFFFFF


def w64(C):
    return 4 if C.name == "BN254" else 6


def scalars(vals):
    return corc.ints_to_limbs(list(vals), 4)


def ev(C, P, x):
    acc = 0
    for a in reversed(P):
        acc = (acc * x + a) % C.r
    return acc


class Model:
    """claims as integers: polys (lists of n coefficients), groups (lists of polynomial indices),
    zs (one per group), weights (one per claim, group by group)"""

    def __init__(self, name, C, tau, polys, groups, zs, weights):
        self.name, self.C, self.tau = name, C, tau
        self.polys, self.groups, self.zs, self.w = polys, groups, list(zs), list(weights)
        self.index = [j for g in groups for j in g]
        self.start = [0]
        for g in groups:
            self.start.append(self.start[-1] + len(g))
        assert len(self.w) == len(self.index) and len(self.zs) == len(groups)
        self.n = len(polys[0])

    def rng(self, g):
        return range(self.start[g], self.start[g + 1])

    def ys(self):
        return [ev(self.C, self.polys[self.index[k]], self.zs[g]) for g in range(len(self.groups)) for k in self.rng(g)]

    def folded(self, g):
        """F_g's coefficients"""
        r = self.C.r
        return [sum(self.w[k] * self.polys[self.index[k]][i] for k in self.rng(g)) % r for i in range(self.n)]

    def Ys(self):
        y = self.ys()
        return [sum(self.w[k] * y[k] for k in self.rng(g)) % self.C.r for g in range(len(self.groups))]

    def proof_exps(self):
        r, t = self.C.r, self.tau
        Y = self.Ys()
        out = []
        for g in range(len(self.groups)):
            Ft = sum(self.w[k] * ev(self.C, self.polys[self.index[k]], t) for k in self.rng(g)) % r
            out.append((Ft - Y[g]) * pow(t - self.zs[g], -1, r) % r)
        return out

    def commit_exps(self):
        return [ev(self.C, P, self.tau) for P in self.polys]

    def coeff_array(self, stride):
        """(n_polys, stride, 4): the rows' padding holds non-canonical words that must never be read"""
        a = np.full((len(self.polys), stride, 4), U64, dtype=np.uint64)
        for j, P in enumerate(self.polys):
            a[j, :self.n] = scalars(P)
        return a


def point(name, C, e):
    return corc.scalar_mul(name, (C.gx, C.gy), e % C.r) if e % C.r else None


def points(name, C, exps, cache):
    for e in exps:
        if e not in cache:
            cache[e] = point(name, C, e)
    P = [cache[e] for e in exps]
    return corc.points_to_array(name, P), np.array([q is None for q in P], dtype=np.int32)


def verify_model(C, tau, c, p, index, start, zs, ys, w, ch):
    """the header's equation on exponents"""
    r = C.r
    ng = len(zs)
    lhs = tau * sum(ch[g] * p[g] for g in range(ng))
    rhs = sum(ch[g] * zs[g] * p[g] for g in range(ng))
    for g in range(ng):
        for k in range(start[g], start[g + 1]):
            rhs += ch[g] * w[k] * (c[index[k]] - ys[k])
    return (lhs - rhs) % r == 0


def standard_model(name, C, tau, n):
    """5 polynomials, 4 groups: one claim; three claims with a repeated polynomial, opened at a root of
    F_g (the last weight is solved for Y_g = 0); 70 claims (more than a wavefront) with the weights 0, 1
    and r - 1 among them; an empty group.  z = 0, the root, r - 3, 5 (0 and 5 trade places with n)."""
    r = C.r
    polys = [K.random_scalars(C, n, seed=1000 * n + j) for j in range(5)]
    groups = [[2], [0, 3, 0], [k % 5 for k in range(70)], []]
    root = 7
    zs = [0, root, r - 3, 5] if n % 2 else [5, root, r - 3, 0]
    w = K.random_scalars(C, 74, seed=31 * n + 5)
    w[4 + 0], w[4 + 1], w[4 + 2] = 0, 1, r - 1
    y0, y3 = ev(C, polys[0], root), ev(C, polys[3], root)
    assert y0 != 0
    w[3] = -(w[1] * y0 + w[2] * y3) * pow(y0, -1, r) % r
    m = Model(name, C, tau, polys, groups, zs, w)
    assert m.Ys()[1] == 0 and m.Ys()[3] == 0 and all(z != tau for z in zs)
    return m


@pytest.fixture(scope="module")
def env():
    import kzgx
    made = {}

    def get(name, C):
        if name not in made:
            tau = K.default_tau(C)
            ctx = kzgx.Context(name)
            ctx.gen_srs(tau, 260)
            ctx.gen_srs_g2(tau, 2)
            made[name] = (ctx, tau, {})
        return made[name]

    yield get
    for ctx, _, _ in made.values():
        ctx.close()


def prove(ctx, m, stride=None, weights=None, powers=False):
    stride = m.n if stride is None else stride
    return ctx.prove_multi(m.coeff_array(stride), m.index, m.start, scalars(m.zs),
                           scalars(m.w if weights is None else weights), powers=powers, n=m.n)


@pytest.mark.parametrize("name,C", CURVES)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_proofs_and_values_against_the_exponent_model(name, C, n, env):
    ctx, tau, cache = env(name, C)
    m = standard_model(name, C, tau, n)
    out, inf, y, Y = prove(ctx, m, stride=n + 3)
    assert corc.limbs_to_ints(y) == m.ys()
    assert corc.limbs_to_ints(Y) == m.Ys()
    exps = m.proof_exps()
    ex, ei = points(name, C, exps, cache)
    assert exps[3] == 0 and (n > 1 or not any(exps))  # the empty group; constants have no quotient
    assert inf.tolist() == [bool(v) for v in ei]
    assert np.array_equal(out, ex)
    # the old route: kzgx_prove_single_batch of the host-folded F_g, limb for limb; y_k = kzgx_poly_eval
    F = np.stack([scalars(m.folded(g)) for g in range(4)])
    o2, i2, Y2 = ctx.prove_single_batch(F, scalars(m.zs), shared=False)
    assert np.array_equal(out, o2) and inf.tolist() == i2.tolist() and np.array_equal(Y, Y2)
    for j in (0, 3):
        got = ctx.poly_eval(scalars(m.polys[j]), scalars(m.zs))
        for g in range(4):
            for k in m.rng(g):
                if m.index[k] == j:
                    assert np.array_equal(y[k], got[g])


@pytest.mark.parametrize("name,C", CURVES)
def test_weight_powers_equal_explicit_powers(name, C, env):
    ctx, tau, _ = env(name, C)
    r = C.r
    base = standard_model(name, C, tau, 65)
    gammas = [K.random_scalars(C, 1, seed=3)[0], 0, r - 1, 12345]
    w = [pow(gammas[g], k - base.start[g], r) for g in range(4) for k in base.rng(g)]
    assert w[1:4] == [1, 0, 0]  # gamma = 0: 0^0 = 1
    m = Model(name, C, tau, base.polys, base.groups, base.zs, w)
    a = prove(ctx, m, stride=68)
    b = prove(ctx, m, stride=68, weights=gammas, powers=True)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert corc.limbs_to_ints(a[3]) == m.Ys() and corc.limbs_to_ints(a[2]) == m.ys()


def nine_groups(name, C, tau, n=65):
    polys = [K.random_scalars(C, n, seed=70 + j) for j in range(4)]
    groups = [[(g + j) % 4 for j in range(1 + g % 3)] for g in range(9)]
    zs = K.random_scalars(C, 9, seed=71)
    w = K.random_scalars(C, sum(len(g) for g in groups), seed=72)
    return Model(name, C, tau, polys, groups, zs, w)


@pytest.mark.parametrize("name,C", CURVES)
def test_chunking(name, C, env):
    """set_multi_chunk(4 * 65) at n = 65: 9 groups run as chunks of 4, 4 and 1"""
    ctx, tau, cache = env(name, C)
    m = nine_groups(name, C, tau)
    whole = prove(ctx, m)
    ctx.set_multi_chunk(4 * 65)
    try:
        ctx.prof_enable(True)
        ctx.prof_clear()
        parts = prove(ctx, m)
        ctx.sync()
        assert ctx.prof_read("quotient_single")[1] == 3 and ctx.prof_read("multi_fold")[1] == 3
    finally:
        ctx.prof_enable(False)
        ctx.prof_clear()
        ctx.set_multi_chunk(0)
    for u, v in zip(whole, parts):
        assert np.array_equal(u, v)
    assert corc.limbs_to_ints(whole[3]) == m.Ys()
    assert np.array_equal(whole[0], points(name, C, m.proof_exps(), cache)[0])


@pytest.mark.parametrize("name,C", CURVES)
def test_sliced_evaluation(name, C):
    """n = 2 KZGX_MULTI_EVAL_SLICE + 5: three slices per claim, the last one ragged"""
    import kzgx
    n = 2 * kzgx.MULTI_EVAL_SLICE + 5
    tau = K.default_tau(C)
    ctx = kzgx.Context(name)
    try:
        ctx.set_default_table(0)
        ctx.gen_srs(tau, n)
        polys = [K.random_scalars(C, n, seed=55 + j) for j in range(2)]
        m = Model(name, C, tau, polys, [[1], [0]], [C.r - 2, 3], [5, C.r - 1])
        ctx.prof_enable(True)
        out, inf, y, Y = prove(ctx, m, stride=n + 3)
        ctx.sync()
        assert ctx.prof_read("multi_eval")[1] == 1
        ctx.prof_enable(False)
        assert corc.limbs_to_ints(y) == m.ys()
        assert corc.limbs_to_ints(Y) == m.Ys()
        ex, ei = points(name, C, m.proof_exps(), {})
        assert np.array_equal(out, ex) and not inf.any() and not ei.any()
    finally:
        ctx.close()


@pytest.mark.parametrize("name,C", CURVES)
def test_one_quotient_launch_per_chunk(name, C, env):
    """3 groups x 8 claims: the call folds -- one quotient launch, not 24"""
    ctx, tau, _ = env(name, C)
    polys = [K.random_scalars(C, 33, seed=90 + j) for j in range(8)]
    m = Model(name, C, tau, polys, [list(range(8))] * 3, [11, 12, 13], K.random_scalars(C, 24, seed=91))
    ctx.prof_enable(True)
    ctx.prof_clear()
    try:
        _, _, _, Y = prove(ctx, m)
        ctx.sync()
        assert ctx.prof_read("quotient_single")[1] == 1
        assert ctx.prof_read("multi_fold")[1] == 1 and ctx.prof_read("multi_eval")[1] == 1
    finally:
        ctx.prof_enable(False)
        ctx.prof_clear()
    assert corc.limbs_to_ints(Y) == m.Ys()


# ---- verify ---------------------------------------------------------------------------------------
class Claims:
    """the verifier's view in exponents: commitments c, proofs p, values y, weights w, per-group z"""

    def __init__(self, m):
        self.name, self.C, self.tau = m.name, m.C, m.tau
        self.c, self.p, self.y, self.w = m.commit_exps(), m.proof_exps(), m.ys(), list(m.w)
        self.index, self.start, self.zs = list(m.index), list(m.start), list(m.zs)

    def copy(self):
        import copy
        return copy.deepcopy(self)

    def truth(self, ch):
        return verify_model(self.C, self.tau, self.c, self.p, self.index, self.start, self.zs, self.y, self.w, ch)

    def run(self, ctx, ch, cache, **kw):
        cx, ci = points(self.name, self.C, self.c, cache)
        px, pi = points(self.name, self.C, self.p, cache)
        return ctx.verify_multi(cx, self.index, self.start, scalars(self.zs), scalars(self.y), scalars(self.w), px,
                                None if ch is None else scalars(ch), commit_inf=ci, proof_inf=pi, **kw)


def verify_case(name, C, tau):
    """6 commitments (one of the zero polynomial: infinite; one constant), 5 groups: the third opens only
    the constant and the zero polynomial (infinite proof), the fourth is empty"""
    r = C.r
    polys = [K.random_scalars(C, 9, seed=200 + j) for j in range(4)] + [[0] * 9, [77] + [0] * 8]
    groups = [[0, 1, 2, 3, 5, 1], [3, 0], [5, 4], [], [2, 4, 0]]
    zs = [9, r - 4, 0, 1, 123456789]
    w = K.random_scalars(C, sum(len(g) for g in groups), seed=201)
    m = Model(name, C, tau, polys, groups, zs, w)
    v = Claims(m)
    assert v.c[4] == 0 and v.p[2] == 0 and v.p[3] == 0 and v.p[0] != 0
    return v


def challenges128(C, n, seed):
    ch = [s % (1 << 128) for s in K.random_scalars(C, n, seed=seed)]
    ch[0] = 1
    assert all(ch)
    return ch


@pytest.mark.parametrize("name,C", CURVES)
def test_verify_valid_and_tampered(name, C, env):
    ctx, tau, cache = env(name, C)
    v = verify_case(name, C, tau)
    ch = challenges128(C, 5, seed=300)
    assert v.truth(ch) and v.run(ctx, ch, cache) is True
    assert v.run(ctx, None, cache) is True  # library-drawn challenges; infinite commitment and proof inside
    assert v.run(ctx, ch, cache, checked=True, subgroup=1) is True
    tampered = []
    t = v.copy()
    t.y[7] = (t.y[7] + 1) % C.r
    tampered.append(("one wrong y", t))
    t = v.copy()
    t.p[1] = (t.p[1] + 1) % C.r
    tampered.append(("one wrong proof", t))
    t = v.copy()
    t.c[3] = (t.c[3] + 1) % C.r
    tampered.append(("one wrong commitment", t))
    t = v.copy()
    assert t.c[t.index[0]] != t.c[t.index[1]]
    t.index[0], t.index[1] = t.index[1], t.index[0]
    tampered.append(("swapped commit_index", t))
    for label, t in tampered:
        assert not t.truth(ch), label
        assert t.run(ctx, ch, cache) is False, label
        assert t.run(ctx, None, cache) is False, label


@pytest.mark.parametrize("name,C", CURVES)
def test_errors_that_cancel_under_the_given_weights_and_challenges(name, C, env):
    """the entry computes the stated equation and nothing else: two wrong values in two groups whose
    errors cancel under (w, r) pass under those and fail under other challenges; two in one group that
    cancel under w pass under every r"""
    ctx, tau, cache = env(name, C)
    r = C.r
    v = verify_case(name, C, tau)
    ch = challenges128(C, 5, seed=301)
    a, b = 2, 7  # claims of groups 0 and 1
    t = v.copy()
    t.y[a] = (t.y[a] + 5) % r
    t.y[b] = (t.y[b] - 5 * ch[0] * t.w[a] * pow(ch[1] * t.w[b], -1, r)) % r
    other = list(ch)
    other[1] += 1
    assert t.truth(ch) and not t.truth(other)
    assert t.run(ctx, ch, cache) is True
    assert t.run(ctx, other, cache) is False
    assert t.run(ctx, None, cache) is False
    t = v.copy()
    t.y[0] = (t.y[0] + 5 * t.w[1]) % r
    t.y[1] = (t.y[1] - 5 * t.w[0]) % r
    assert t.truth(ch) and t.truth(other)
    assert t.run(ctx, ch, cache) is True and t.run(ctx, None, cache) is True


@pytest.mark.parametrize("name,C", CURVES)
def test_no_groups(name, C, env):
    ctx, _, _ = env(name, C)
    e = np.zeros((0, 2 * w64(C)), dtype=np.uint64)
    s = np.zeros((0, 4), dtype=np.uint64)
    assert ctx.verify_multi(e, [], [0], s, s, s, e, s) is True
    assert ctx.verify_multi(e, [], [0], s, s, s, e, None, checked=True, subgroup=1) is True
    out, inf, y, Y = ctx.prove_multi(np.zeros((1, 4, 4), dtype=np.uint64), [], [0], s, s)
    assert out.shape[0] == 0 and Y.shape[0] == 0


def g1_row(C, P):
    nl = w64(C)
    return np.concatenate([corc.ints_to_limbs([P[0]], nl)[0], corc.ints_to_limbs([P[1]], nl)[0]])


@pytest.mark.parametrize("name,C", CURVES)
def test_checked_rejects_points_the_equation_does_not_see(name, C, env):
    """group 1 under the challenge 0: its proof enters neither MSM, so the equation holds whatever the
    point is -- the _checked forms still reject an off-curve proof, and on BLS12-381 one outside the
    prime-order subgroup"""
    ctx, tau, cache = env(name, C)
    v = verify_case(name, C, tau)
    ch = challenges128(C, 5, seed=302)
    ch[1] = 0
    assert v.truth(ch)
    cx, ci = points(name, C, v.c, cache)
    px, pi = points(name, C, v.p, cache)
    args = (v.index, v.start, scalars(v.zs), scalars(v.y), scalars(v.w))

    def run(p, **kw):
        return ctx.verify_multi(cx, *args, p, scalars(ch), commit_inf=ci, proof_inf=pi, **kw)

    assert run(px) is True and run(px, checked=True, subgroup=1) is True
    good = corc.array_to_points(name, px[1:2])[0]
    off = px.copy()
    off[1] = g1_row(C, (good[0], (good[1] + 1) % C.p))
    assert not K.on_curve(C, (good[0], (good[1] + 1) % C.p))
    assert run(off) is True
    assert run(off, checked=True, subgroup=0) is False and run(off, checked=True, subgroup=1) is False
    if name == "BLS12381":
        from test_subgroup_consts import g1_member, g1_order_point
        P = K.point_add(C, good, g1_order_point(3))
        assert K.on_curve(C, P) and not g1_member(C, P)
        out = px.copy()
        out[1] = g1_row(C, P)
        assert run(out) is True and run(out, checked=True, subgroup=0) is True
        assert run(out, checked=True, subgroup=1) is False


# ---- device entries -------------------------------------------------------------------------------
def dev_tensor(a, dev):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).to(dev)


def back(t, dtype):
    return t.cpu().numpy().view(dtype)


@pytest.mark.parametrize("name,C", CURVES)
def test_device_entries_on_a_caller_stream(name, C, env):
    import torch
    ctx, tau, cache = env(name, C)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    nl = w64(C)
    m = standard_model(name, C, tau, 65)
    host = prove(ctx, m, stride=68)
    count, ng = len(m.index), 4
    t = [dev_tensor(a, dev) for a in (m.coeff_array(68), np.array(m.index, dtype=np.uint32),
                                      np.array(m.start, dtype=np.uint32), scalars(m.zs), scalars(m.w))]
    out = torch.full((ng + 1, 2 * nl), 7, dtype=torch.int64, device=dev)  # one canary row behind each output
    inf = torch.full((ng + 1,), 7, dtype=torch.int32, device=dev)
    y = torch.full((count + 1, 4), 7, dtype=torch.int64, device=dev)
    Y = torch.full((ng + 1, 4), 7, dtype=torch.int64, device=dev)
    ok = torch.full((2,), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.prove_multi_device(t[0].data_ptr(), 65, 68, 5, t[1].data_ptr(), t[2].data_ptr(), ng, t[3].data_ptr(),
                           t[4].data_ptr(), count, out.data_ptr(), inf.data_ptr(), y.data_ptr(), Y.data_ptr(),
                           ok.data_ptr(), stream=st.cuda_stream)
    st.synchronize()
    assert np.array_equal(back(out, np.uint64)[:ng], host[0]) and back(inf, np.int32)[:ng].tolist() == host[1].tolist()
    assert np.array_equal(back(y, np.uint64)[:count], host[2]) and np.array_equal(back(Y, np.uint64)[:ng], host[3])
    assert back(ok, np.int32).tolist() == [1, 7]
    for canary in (out[ng], inf[ng:], y[count], Y[ng]):
        assert (canary == 7).all()
    # the verifier through device pointers: a valid batch and one wrong value
    v = Claims(m)
    ch = challenges128(C, ng, seed=400)
    bad = v.copy()
    bad.y[40] = (bad.y[40] + 1) % C.r
    assert v.truth(ch) and not bad.truth(ch)
    cx, ci = points(name, C, v.c, cache)
    oks, keep = [], []
    for case, checked in ((v, False), (bad, False), (v, True), (bad, True)):
        a = [dev_tensor(x, dev) for x in (cx, ci, np.array(case.index, dtype=np.uint32),
                                          np.array(case.start, dtype=np.uint32), scalars(case.zs), scalars(case.y),
                                          scalars(case.w), host[0], host[1].astype(np.int32), scalars(ch))]
        keep.append(a)
        oks.append(torch.full((1,), 7, dtype=torch.int32, device=dev))
    torch.cuda.synchronize(dev)
    for a, o, checked in zip(keep, oks, (False, False, True, True)):
        p = [x.data_ptr() for x in a]
        ctx.verify_multi_device(p[0], p[1], 5, p[2], p[3], ng, p[4], p[5], p[6], p[7], p[8], p[9], count,
                                o.data_ptr(), checked=checked, subgroup=1, stream=st.cuda_stream)
    st.synchronize()
    assert [int(o.item()) for o in oks] == [1, 0, 1, 0]


@pytest.mark.parametrize("name,C", CURVES)
def test_device_entries_flag_malformed_claims(name, C, env):
    """an index out of range or a decreasing group_start: KZGX_OK, d_ok = 0, nothing read or written out
    of bounds (ranges are clamped, the bad claim adds nothing), the other groups' outputs intact"""
    import torch
    ctx, tau, cache = env(name, C)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    nl = w64(C)
    m = nine_groups(name, C, tau, n=33)
    host = prove(ctx, m)
    count, ng = len(m.index), 9
    coeffs, zs, w = (dev_tensor(a, dev) for a in (m.coeff_array(33), scalars(m.zs), scalars(m.w)))
    bad_index = list(m.index)
    bad_index[m.start[4]] = 4  # group 4's first claim: one past the last polynomial
    bad_start = list(m.start)
    bad_start[6] = bad_start[5] - 1  # groups 5 (now decreasing: empty) and 6 (one claim more) change
    runs = []
    for index, start, touched in ((bad_index, m.start, {4}), (m.index, bad_start, {5, 6})):
        ti, ts = dev_tensor(np.array(index, dtype=np.uint32), dev), dev_tensor(np.array(start, dtype=np.uint32), dev)
        out = torch.full((ng + 1, 2 * nl), 7, dtype=torch.int64, device=dev)
        inf = torch.full((ng + 1,), 7, dtype=torch.int32, device=dev)
        y = torch.full((count + 1, 4), 7, dtype=torch.int64, device=dev)
        ok = torch.full((2,), 7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        ctx.prove_multi_device(coeffs.data_ptr(), 33, 33, 4, ti.data_ptr(), ts.data_ptr(), ng, zs.data_ptr(),
                               w.data_ptr(), count, out.data_ptr(), inf.data_ptr(), y.data_ptr(), None,
                               ok.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        runs.append((ti, ts))
        assert back(ok, np.int32).tolist() == [0, 7]
        o = back(out, np.uint64)
        for g in range(ng):
            if g not in touched:
                assert np.array_equal(o[g], host[0][g]), g
        assert (out[ng] == 7).all() and (inf[ng:] == 7).all() and (y[count] == 7).all()
        if touched == {4}:  # the bad claim's value is 0, every other claim's is right
            want = host[2].copy()
            want[m.start[4]] = 0
            assert np.array_equal(back(y, np.uint64)[:count], want)
    # the verifier: the same two defects force 0 although every value and proof is right
    v = Claims(m)
    ch = challenges128(C, ng, seed=401)
    cx, ci = points(name, C, v.c, cache)
    fixed = [dev_tensor(a, dev) for a in (cx, ci, scalars(v.zs), scalars(v.y), scalars(v.w), host[0],
                                          host[1].astype(np.int32), scalars(ch))]
    good = (dev_tensor(np.array(m.index, dtype=np.uint32), dev), dev_tensor(np.array(m.start, dtype=np.uint32), dev))
    oks = []
    for ti, ts in [good] + runs:
        ok = torch.full((1,), 7, dtype=torch.int32, device=dev)
        p = [x.data_ptr() for x in fixed]
        ctx.verify_multi_device(p[0], p[1], 4, ti.data_ptr(), ts.data_ptr(), ng, p[2], p[3], p[4], p[5], p[6], p[7],
                                count, ok.data_ptr(), stream=st.cuda_stream)
        oks.append(ok)
    st.synchronize()
    assert [int(o.item()) for o in oks] == [1, 0, 0]


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
    import torch
    import kzgx
    ctx, tau, cache = env(name, C)
    r = C.r
    L = kzgx.lib()
    u64p, u32p, intp = kzgx.u64p, kzgx.u32p, kzgx.intp
    m = nine_groups(name, C, tau, n=33)
    ng, count = 9, len(m.index)
    base = dict(coeffs=m.coeff_array(36), n=33, stride=36, n_polys=4, index=np.array(m.index, dtype=np.uint32),
                start=np.array(m.start, dtype=np.uint32), ng=ng, zs=scalars(m.zs), w=scalars(m.w), count=count,
                flags=0)
    out = np.zeros((ng, 2 * w64(C)), dtype=np.uint64)
    inf = np.zeros(ng, dtype=np.int32)

    def P(a, t=u64p):
        return None if a is None else a.ctypes.data_as(t)

    def prove_rc(c=None, **kw):
        a = dict(base, **kw)
        return L.kzgx_prove_multi_batch((c or ctx).h, P(a["coeffs"]), a["n"], a["stride"], a["n_polys"],
                                        P(a["index"], u32p), P(a["start"], u32p), a["ng"], P(a["zs"]), P(a["w"]),
                                        a["count"], a["flags"], P(a.get("out", out)), P(a.get("inf", inf), intp),
                                        None, None)

    def edited(a, i, val):
        b = a.copy()
        b[i] = val
        return b

    assert prove_rc() == 0
    for key in ("coeffs", "index", "start", "zs", "w", "out", "inf"):
        assert prove_rc(**{key: None}) == -1, key
    assert prove_rc(n=0) == -1 and prove_rc(stride=32) == -1 and prove_rc(flags=2) == -1
    assert prove_rc(start=edited(base["start"], 0, 1)) == -1      # does not start at 0
    assert prove_rc(start=edited(base["start"], ng, count - 1)) == -1  # does not end at count
    assert prove_rc(start=edited(base["start"], 3, base["start"][4] + 1)) == -1  # decreasing
    assert prove_rc(index=edited(base["index"], 5, 4)) == -1
    assert prove_rc(zs=edited(base["zs"], 2, scalars([r])[0])) == -1
    assert prove_rc(w=edited(base["w"], count - 1, scalars([r + 1])[0])) == -1
    assert prove_rc(flags=kzgx.MULTI_WEIGHT_POWERS, w=edited(base["w"], 8, scalars([r])[0])) == -1
    assert prove_rc(flags=kzgx.MULTI_WEIGHT_POWERS) == 0  # the first n_groups weights as gammas
    big = np.zeros((1, 300, 4), dtype=np.uint64)
    one = dict(coeffs=big, n_polys=1, index=np.zeros(1, dtype=np.uint32), start=np.array([0, 1], dtype=np.uint32),
               ng=1, count=1)
    assert prove_rc(n=261, stride=300, **one) == 0       # degree 260 = the setup's size
    assert prove_rc(n=262, stride=300, **one) == -5      # KZGX_ERR_DEGREE
    bare = kzgx.Context(name)
    try:
        assert prove_rc(c=bare) == -4                    # KZGX_ERR_NO_SRS
        assert prove_rc(c=bare, n=0) == -1               # arguments first
        bare.gen_srs(tau, 8)                             # G1 only: the verify needs G2[0..1] too
        v = Claims(m)
        assert status(lambda: v.run(bare, None, cache)) == -4
    finally:
        bare.close()
    # the verifier
    v = Claims(m)
    cx, ci = points(name, C, v.c, cache)
    px, pi = points(name, C, v.p, cache)
    vb = dict(commits=cx, nc=4, index=base["index"], start=base["start"], ng=ng, zs=base["zs"], ys=scalars(v.y),
              w=base["w"], proofs=px, ch=scalars(challenges128(C, ng, seed=402)), count=count, flags=0)
    okv = ctypes.c_int(7)

    def verify_rc(ok=True, **kw):
        a = dict(vb, **kw)
        return L.kzgx_verify_multi_batch(ctx.h, P(a["commits"]), P(ci, intp), a["nc"], P(a["index"], u32p),
                                         P(a["start"], u32p), a["ng"], P(a["zs"]), P(a["ys"]), P(a["w"]),
                                         P(a["proofs"]), P(pi, intp), P(a["ch"]), a["count"], a["flags"],
                                         ctypes.byref(okv) if ok else None)

    assert verify_rc() == 0 and okv.value == 1
    assert verify_rc(ch=None) == 0 and okv.value == 1
    for key in ("commits", "index", "start", "zs", "ys", "w", "proofs"):
        assert verify_rc(**{key: None}) == -1, key
    assert verify_rc(ok=False) == -1 and verify_rc(flags=4) == -1
    assert verify_rc(start=edited(vb["start"], 2, vb["start"][3] + 1)) == -1
    assert verify_rc(index=edited(vb["index"], 0, 4)) == -1
    assert verify_rc(nc=3) == -1  # index 3 is now out of range
    assert verify_rc(zs=edited(vb["zs"], 0, scalars([r])[0])) == -1
    assert verify_rc(w=edited(vb["w"], 1, scalars([r])[0])) == -1
    assert verify_rc(ch=edited(vb["ch"], 8, scalars([r])[0])) == -1
    assert kzgx._header_define("KZGX_MULTI_CHUNK_SCALARS") == 1 << 21
    assert verify_rc(nc=(1 << 22) - ng) == -1  # n_commits + n_groups + 1 > KZGX_MSM_POINTS_MAX = 2^22
    # device entries: NULL challenges, NULL weights
    dev = torch.device("cuda", 0)
    buf = torch.zeros(4096, dtype=torch.int64, device=dev)
    b = buf.data_ptr()
    ok = torch.full((1,), 7, dtype=torch.int32, device=dev)
    assert status(lambda: ctx.verify_multi_device(b, None, 1, b, b, 1, b, b, b, b, None, None, 1, ok.data_ptr())) == -1
    assert status(lambda: ctx.verify_multi_device(b, None, 1, b, b, 1, b, b, None, b, None, b, 1, ok.data_ptr())) == -1
    assert status(lambda: ctx.prove_multi_device(b, 4, 4, 1, b, b, 1, b, None, 1, b, b)) == -1
    assert status(lambda: ctx.prove_multi_device(b, 4, 3, 1, b, b, 1, b, b, 1, b, b)) == -1
    torch.cuda.synchronize(dev)
    assert int(ok.item()) == 7
