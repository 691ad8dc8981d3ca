"""Single field and point primitives on the device (kzgx_debug_prim,
csrc/selftest.hip) against the exact integer model (oracle/field_model.py):
every product form, carry helper, zero test, conversion and inverse of
csrc/field29.hpp, csrc/field.hpp on both of its fields, and the XYZZ formulas
of csrc/curve.hpp, on raw limbs at the documented bounds -- non-canonical
representatives, the one lazy operand, forced reduction digits, exact
landings on 0 / m / 2m - 1, the equal-x branches.  No tolerances: every
comparison is exact, and every tuple passes the model's precondition check
before it is sent.

Not reachable: a SINGLE product landing exactly on 2m - 1 (it needs a b in a
window of width R just under R m with both factors below R, a factorisation);
the two-product forms land there (field_model.landing_quads)."""
import ctypes

import numpy as np
import pytest

import field_model as M
import kzg_ref as K

pytestmark = pytest.mark.gpu

CURVES = ["BN254", "BLS12381"]
KZGX_ERR_ARG = -1


class Harness:
    def __init__(self, curve):
        import kzgx
        self.curve = curve
        self.ctx = kzgx.Context(curve)
        self.fn = kzgx.lib().kzgx_debug_prim
        self.fn.restype = ctypes.c_int
        self.fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32),
                            ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)]

    def raw(self, op, mode, inp, count, out):
        u32p = ctypes.POINTER(ctypes.c_uint32)
        return self.fn(self.ctx.h, op, mode, inp.ctypes.data_as(u32p) if inp is not None else None, count,
                       out.ctypes.data_as(u32p) if out is not None else None)

    def run(self, name, tuples, mode=0):
        """tuples: flat word lists, one per tuple -> the flat word list of every result"""
        nin, nout = M.prim_words(self.curve, name)
        inp = np.ascontiguousarray(np.array(tuples, dtype=np.uint64).astype(np.uint32))
        assert inp.shape == (len(tuples), nin), (name, inp.shape, nin)
        out = np.full((len(tuples), nout), 0xDEADBEEF, dtype=np.uint32)
        assert self.raw(M.PRIM_OPS[name], mode, inp, len(tuples), out) == 0, name
        return out.tolist()


@pytest.fixture(scope="module")
def harness():
    made = {}

    def get(curve):
        if curve not in made:
            made[curve] = Harness(curve)
        return made[curve]

    yield get
    for h in made.values():
        h.ctx.close()


def flat(*elems):
    return [x for e in elems for x in e]


def split(F, row, n):
    return [row[i * F.L:(i + 1) * F.L] for i in range(n)]


# ---- products ------------------------------------------------------------------
class Products:
    """the operand lists of one curve and their model values, computed once"""

    def __init__(self, curve):
        F = self.F = M.FP29[curve]
        lp, lq = M.landing_pairs(F), M.landing_quads(F)
        self.named = {"landing_%s" % ("0 1 m-1 m m+1".split()[i]): p for i, p in enumerate(lp.values())}
        norm = M.product_pairs(F) + M.digit_pairs(F) + list(lp.values())
        lazy = M.lazy_product_pairs(F)
        # the lazy operand first and second
        self.singles = norm + lazy + [(b, z) for z, b in lazy]
        self.squares = M.square_operands(F) + [a for a, b in lp.values() if a == b]
        Rm = F.R * F.m
        pv = lambda p: M.val(p[0]) * M.val(p[1])
        quads = []
        n = len(norm)
        for i, p in enumerate(norm):
            q = norm[(3 * i + 7) % n]
            if pv(p) + pv(q) < Rm:
                quads.append(p + q)
        for i, (z, b) in enumerate(lazy):  # the one lazy operand first and second, in either product
            q = norm[(5 * i + 2) % n]
            if pv((z, b)) + pv(q) < Rm:
                quads += [(z, b) + q, (b, z) + q, [q + (z, b), q + (b, z)][i % 2]]
        # both products large: a b + c d just under R m
        for a, b in norm:
            T = Rm - 1 - pv((a, b))
            if pv((a, b)) > Rm // 2 and T // F.m < F.R:
                quads.append((a, b, F.limbs(F.m), F.limbs(T // F.m)))
        self.quads = quads + list(lq.values())
        self.landing_quads = lq
        self._m1, self._m2 = {}, {}

    def mul(self, a, b):
        k = (tuple(a), tuple(b))
        if k not in self._m1:
            self._m1[k] = M.mul(self.F, a, b)
        return self._m1[k]

    def sqr(self, a):
        M.sqr(self.F, a)  # the square forms' own precondition
        return self.mul(a, a)

    def mul2(self, q):
        k = tuple(tuple(x) for x in q)
        if k not in self._m2:
            self._m2[k] = M.mul2(self.F, *q)
        return self._m2[k]


_products = {}


def products(curve):
    if curve not in _products:
        _products[curve] = Products(curve)
    return _products[curve]


def check_product_limbs(F, got, want, what):
    assert got == want, what
    assert all(x <= M.M29 for x in got) and M.val(got) < 2 * F.m, what


@pytest.mark.parametrize("curve", CURVES)
def test_single_products_all_forms(curve, harness):
    """f29_mul = f29_mul_lat = f29_mul_chain = each slot of f29_mul_x2 / _x3 and
    the single slots of f29_mul2_mul / f29_mul2_x3 = the model, limb for limb"""
    h, P = harness(curve), products(curve)
    F, S = P.F, P.singles
    n = len(S)
    want = [P.mul(a, b) for a, b in S]
    digits = set()
    for a, b in S:
        digits |= set(M.reduction_digits(F, [(a, b)]))
    assert {0, M.M29} <= digits
    assert {M.val(w) for w in want} >= {0, 1, F.m - 1, F.m, F.m + 1}
    for name in ("mul", "mul_lat", "mul_chain"):
        got = h.run(name, [flat(a, b) for a, b in S])
        for i in range(n):
            check_product_limbs(F, got[i], want[i], (name, i))
    # multi-slot forms: slot s of tuple i takes single (i + s * step) % n
    step = n // 3 + 1
    idx = lambda i, s: (i + s * step) % n
    got = h.run("mul_x2", [flat(*S[i], *S[idx(i, 1)]) for i in range(n)])
    for i in range(n):
        r = split(F, got[i], 2)
        check_product_limbs(F, r[0], want[i], ("mul_x2", 0, i))
        check_product_limbs(F, r[1], want[idx(i, 1)], ("mul_x2", 1, i))
    got = h.run("mul_x3", [flat(*S[i], *S[idx(i, 1)], *S[idx(i, 2)]) for i in range(n)])
    for i in range(n):
        r = split(F, got[i], 3)
        for s in range(3):
            check_product_limbs(F, r[s], want[idx(i, s)], ("mul_x3", s, i))
    # named regression tuples: the exact landings 0, 1, m - 1, m, m + 1
    for tag, (a, b) in P.named.items():
        assert h.run("mul", [flat(a, b)])[0] == P.mul(a, b), tag


@pytest.mark.parametrize("curve", CURVES)
def test_squares_all_forms(curve, harness):
    """f29_sqr = f29_sqr_chain = both slots of f29_sqr_x2 / f29_sqr_x2_pair = f29_mul(a, a)"""
    h, P = harness(curve), products(curve)
    F, S = P.F, P.squares
    n = len(S)
    want = [P.sqr(a) for a in S]
    for name in ("sqr", "sqr_chain"):
        got = h.run(name, S)
        for i in range(n):
            check_product_limbs(F, got[i], want[i], (name, i))
    got = h.run("mul", [flat(a, a) for a in S])  # equal operands through the general form
    assert got == want
    for name in ("sqr_x2", "sqr_x2_pair"):
        got = h.run(name, [flat(S[i], S[(i + n // 2 + 1) % n]) for i in range(n)])
        for i in range(n):
            r = split(F, got[i], 2)
            check_product_limbs(F, r[0], want[i], (name, 0, i))
            check_product_limbs(F, r[1], want[(i + n // 2 + 1) % n], (name, 1, i))


@pytest.mark.parametrize("curve", CURVES)
def test_double_products_all_forms(curve, harness):
    """f29_mul2 = f29_mul2_lat = f29_mul2_chain = slot 0 of f29_mul2_mul /
    f29_mul2_x3 = the model; their single slots equal f29_mul"""
    h, P = harness(curve), products(curve)
    F, Q, S = P.F, P.quads, P.singles
    n, ns = len(Q), len(P.singles)
    want = [P.mul2(q) for q in Q]
    assert {M.val(w) for w in want} >= {0, F.m - 1, F.m, F.m + 1, 2 * F.m - 1}
    for name in ("mul2", "mul2_lat", "mul2_chain"):
        got = h.run(name, [flat(*q) for q in Q])
        for i in range(n):
            check_product_limbs(F, got[i], want[i], (name, i))
    s1 = lambda i: S[(7 * i + 1) % ns]
    s2 = lambda i: S[(11 * i + 5) % ns]
    got = h.run("mul2_mul", [flat(*Q[i], *s1(i)) for i in range(n)])
    for i in range(n):
        r = split(F, got[i], 2)
        check_product_limbs(F, r[0], want[i], ("mul2_mul", 0, i))
        check_product_limbs(F, r[1], P.mul(*s1(i)), ("mul2_mul", 1, i))
    got = h.run("mul2_x3", [flat(*Q[i], *s1(i), *s2(i)) for i in range(n)])
    for i in range(n):
        r = split(F, got[i], 3)
        check_product_limbs(F, r[0], want[i], ("mul2_x3", 0, i))
        check_product_limbs(F, r[1], P.mul(*s1(i)), ("mul2_x3", 1, i))
        check_product_limbs(F, r[2], P.mul(*s2(i)), ("mul2_x3", 2, i))
    # named regression tuples: a b + c d landing exactly on 0, m - 1, m, m + 1, 2m - 1
    for t, q in P.landing_quads.items():
        assert M.val(h.run("mul2", [flat(*q)])[0]) == t


# ---- carry helpers, reductions, zero tests, conversions -------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_add_sub_and_lazy_helpers(curve, harness):
    h, F = harness(curve), M.FP29[curve]
    m = F.m
    ts = M.add_tuples(F)
    assert h.run("add", [flat(a, b) for a, b in ts]) == [M.add(F, a, b) for a, b in ts]
    for k in (2, 4, 6, 8, 10, 16):
        ts = M.sub_tuples(F, k)
        got = h.run("sub_p%d" % k, [flat(a, b) for a, b in ts])
        assert got == [M.sub(F, a, b, k) for a, b in ts], k
    V = M.corner_values(F)
    a1 = [F.limbs(v) for v in V]
    assert h.run("neg_lazy", a1) == [M.neg_lazy(F, a) for a in a1]
    a4 = [F.limbs(v + k * m) for v in V for k in range(4)] + [F.limbs(4 * m - 1)]
    assert h.run("neg8_lazy", a4) == [M.neg8_lazy(F, a) for a in a4]
    ts = [(F.limbs(v + (i % 8) * m), F.limbs(V[(i + 3) % len(V)] + (i % 5) * m)) for i, v in enumerate(V)]
    ts.append(([M.M29] * F.L, [M.M29] * F.L))
    assert h.run("add_2x_lazy", [flat(a, b) for a, b in ts]) == [M.add_2x_lazy(F, a, b) for a, b in ts]
    ts = M.normalize_operands(F)
    assert h.run("normalize", ts) == [M.normalize(F, a) for a in ts]


@pytest.mark.parametrize("curve", CURVES)
def test_csub_reduce_and_zero_tests(curve, harness):
    h, F = harness(curve), M.FP29[curve]
    m = F.m
    for k in (1, 2, 4, 6, 8, 10, 16):
        ts = [F.limbs(v) for v in M.csub_values(F, k)]
        name = "csub_p" if k == 1 else "csub_p%d" % k
        assert h.run(name, ts) == [M.csub(F, a, k) for a in ts], k
    vs = M.zero_test_values(F, 16) + [v + k * m for i, v in enumerate(M.corner_values(F)) for k in (i % 16, 15)]
    ts = [F.limbs(v) for v in vs]
    got = h.run("reduce", ts)
    assert got == [M.reduce(F, a) for a in ts] == [F.limbs(v % m) for v in vs]
    assert h.run("is_zero", ts) == [[int(v % m == 0)] for v in vs]
    assert sum(v % m == 0 for v in vs) >= 16
    vs = M.zero_test_values(F, 2) + [v + k * m for v in M.corner_values(F) for k in (0, 1)]
    ts = [F.limbs(v) for v in vs]
    assert h.run("is_zero_lt2m", ts) == [[int(M.is_zero_lt2m(F, a))] for a in ts]
    # named regression cases: m itself (low limb LOW[1]), and nonzero values that pass the one-limb filter
    assert h.run("is_zero_lt2m", [F.limbs(m), F.limbs(0), F.limbs(m + (1 << 29)), F.limbs(1 << 29)]) == [[1], [1], [0], [0]]


@pytest.mark.parametrize("curve", CURVES)
def test_montgomery_and_word_conversions(curve, harness):
    h, F = harness(curve), M.FP29[curve]
    m, NW = F.m, M.FP32[curve].N
    V = M.corner_values(F)
    ts = [F.limbs(v + (i % 14) * m) for i, v in enumerate(V)] + [F.limbs(m), F.limbs(15 * m + m - 1)]
    got = h.run("to_mont", ts)
    assert got == [M.to_mont(F, a) for a in ts]
    assert all(M.val(g) % m == M.val(a) * F.R % m for g, a in zip(got, ts))
    got = h.run("from_mont", ts)
    assert got == [M.from_mont(F, a) for a in ts] == [F.limbs(M.val(a) * pow(F.R, -1, m) % m) for a in ts]
    W32 = M.FP32[curve]
    ws = [W32.words(v) for v in M.word_values(F, NW)]
    limbs = h.run("from_words", ws)
    assert limbs == [M.from_words(F, w) for w in ws]
    assert h.run("to_words", limbs) == ws  # f29_to_words(f29_from_words(w)) == w
    # to_words on limbs that no from_words produced: values above 32 NW bits are cut
    ts = [F.limbs(v) for v in (F.R - 1, 16 * m - 1, (1 << (32 * NW)) + 5)]
    assert h.run("to_words", ts) == [M.to_words(F, a, NW) for a in ts]


# ---- inverses -------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_inverses_all_forms_and_modes(curve, harness):
    """f29_inv (Fermat), f29_inv_vt (per lane, a different value in every
    lane), f29_inv_uniform and f29_inv_uniform_raw with all 64 lanes, lanes
    0-3 (combine4) and lane 0 alone (the sequential fallback): all equal
    pow(x, -1, m) after full reduction; 0 and k m give exact zero"""
    h, F = harness(curve), M.FP29[curve]
    ts = M.inverse_operands(F)
    want = [M.inv_mont(F, a) for a in ts]
    want_raw = [M.inv_raw(F, a) for a in ts]
    assert max(M.inv_vt_trace(F, a)[1] for a in ts) > (16 if F.L == 9 else 21)  # beyond the random-input figure
    vt = h.run("inv_vt", ts)
    assert all(M.val(r) < 2 * F.m and M.is_norm(F, r) for r in vt)
    vt = [M.reduce(F, r) for r in vt]
    assert vt == want
    fa = [i for i, a in enumerate(ts) if M.fermat_admits(F, a)]
    fer = h.run("inv", [ts[i] for i in fa])
    assert all(M.val(r) < 2 * F.m and M.is_norm(F, r) for r in fer)
    assert [M.reduce(F, r) for r in fer] == [vt[i] for i in fa] == [want[i] for i in fa]
    for mode in (0, 1, 2):
        got = h.run("inv_uniform", ts, mode)
        assert [M.reduce(F, r) for r in got] == want, mode
        got = h.run("inv_uniform_raw", ts, mode)
        assert [M.reduce(F, r) for r in got] == want_raw, mode
    zeros = [i for i, a in enumerate(ts) if M.val(a) % F.m == 0]
    assert len(zeros) == 16 and all(want[i] == [0] * F.L for i in zeros)


# ---- field.hpp ------------------------------------------------------------------
@pytest.mark.parametrize("field", ["fr", "fp"])
@pytest.mark.parametrize("curve", CURVES)
def test_fe_ops(curve, field, harness):
    h = harness(curve)
    F32 = (M.FR32 if field == "fr" else M.FP32)[curve]
    V = M.fe_values(F32)
    n = len(V)
    ws = [F32.words(v) for v in V]
    pairs = [(ws[i], ws[(5 * i + 2) % n]) for i in range(n)] + [(w, w) for w in ws]
    pairs += [(ws[i], F32.words(F32.m - V[i])) for i in range(1, n)]  # a + b = m, a - b across zero
    for op in ("add", "sub", "mul"):
        got = h.run("%s_%s" % (field, op), [flat(a, b) for a, b in pairs])
        assert got == [M.fe_model(F32, op, a, b) for a, b in pairs], op
    for op in ("neg", "dbl", "sqr", "to_mont", "from_mont", "inv"):
        assert h.run("%s_%s" % (field, op), ws) == [M.fe_model(F32, op, a) for a in ws], op


# ---- points ---------------------------------------------------------------------
class Points:
    def __init__(self, curve):
        C, F = self.C, self.F = K.CURVES[curve], M.FP29[curve]
        G = (C.gx, C.gy)
        g = K.splitmix64(0x9017)
        ks = [1, 2, 3, 4, 5, 7, 8, 16, C.r - 1, C.r - 2, C.r - 3, (C.r + 1) // 2]
        ks += [(next(g) << 192 | next(g) << 128 | next(g) << 64 | next(g)) % C.r for _ in range(24)]
        self.ks = ks
        self.pts = [K.scalar_mul(C, G, k) for k in ks]
        self.lams = [1, 2, F.m - 1, (next(g) << 200 | next(g)) % F.m, F.R % F.m]
        self.shifts = [(0, 0, 0, 0), (7, 3, 1, 1), (1, 0, 1, 0), (4, 2, 0, 1), (0, 3, 0, 0)]

    def xyzz(self, i, v=0):
        """point i in variant v: a scaling and a shift of representatives"""
        return M.xyzz_limbs(self.F, self.pts[i % len(self.pts)], self.lams[v % len(self.lams)],
                            *self.shifts[(v // 2) % len(self.shifts)])

    def infs(self):
        F = self.F
        return [M.inf_limbs(F), M.inf_limbs(F, 0, 0), M.inf_limbs(F, 8 * F.m - 1, 4 * F.m - 1), M.inf_limbs(F, 12345, F.m)]

    def check(self, row, want, what):
        """a raw XYZZ result: the oracle's point, infinity exactly by ZZ = 0,
        ZZ^3 = ZZZ^2, normalized limbs, curve.hpp's bounds"""
        F = self.F
        m = F.m
        got, (X, Y, ZZ, ZZZ) = M.decode_xyzz(F, row)
        assert got == want, what
        assert (ZZ == 0) == (want is None), what
        assert pow(M.from_m(F, ZZ), 3, m) == pow(M.from_m(F, ZZZ), 2, m), what
        assert all(x <= M.M29 for x in row), what
        assert X < 8 * m and Y < 4 * m and ZZ < 2 * m and ZZZ < 2 * m, what


_points = {}


def points(curve):
    if curve not in _points:
        _points[curve] = Points(curve)
    return _points[curve]


@pytest.mark.parametrize("curve", CURVES)
def test_point_doublings_and_negation(curve, harness):
    h, S = harness(curve), points(curve)
    C, F = S.C, S.F
    n = len(S.pts)
    dbl = [K.point_add(C, P, P) for P in S.pts]
    # affine doubling: x, y < 2m
    ts, want = [], []
    for i, P in enumerate(S.pts):
        for kx, ky in ((0, 0), (1, 1), (1, 0), (0, 1)):
            ts.append(M.affine_limbs(F, P, kx, ky))
            want.append(dbl[i])
    for row, w in zip(h.run("pt_dbl_affine", ts), want):
        S.check(row, w, "dbl_affine")
    ts = [S.xyzz(i, v) for i in range(n) for v in range(10)] + S.infs()
    want = [dbl[i] for i in range(n) for v in range(10)] + [None] * 4
    out = h.run("pt_dbl", ts)
    for row, w in zip(out, want):
        S.check(row, w, "dbl")
    # chained: the outputs are valid inputs again (closed under their own bounds)
    for row, w in zip(h.run("pt_dbl", out), want):
        S.check(row, None if w is None else K.point_add(C, w, w), "dbl of dbl")
    ts = [S.xyzz(i, v) for i in range(n) for v in range(10)] + S.infs()
    neg = h.run("pt_neg", ts)
    for j, row in enumerate(neg[:-4]):
        S.check(row, K.point_neg(C, S.pts[j // 10]), "neg")
    for row in neg[-4:]:
        assert M.decode_xyzz(F, row)[0] is None
    assert h.run("pt_neg", neg[:-4]) == ts[:-4]  # twice: the very same limbs


@pytest.mark.parametrize("curve", CURVES)
def test_mixed_addition_both_variants(curve, harness):
    h, S = harness(curve), points(curve)
    C, F = S.C, S.F
    n = len(S.pts)
    ts, want, tags = [], [], []

    def case(p_limbs, A, w, tag):
        ts.append(p_limbs + M.affine_limbs(F, A))
        want.append(w)
        tags.append(tag)

    for i in range(n):
        P = S.pts[i]
        for v in range(10):
            A = S.pts[(i + 1 + v) % n]
            if A != P and A != K.point_neg(C, P):
                case(S.xyzz(i, v), A, K.point_add(C, P, A), "finite + finite")
            if v:  # ZZ != 1 or shifted representatives
                case(S.xyzz(i, v), P, K.point_add(C, P, P), "a = P: doubles")
            case(S.xyzz(i, v), K.point_neg(C, P), None, "a = -P: infinity")
        for q in S.infs():
            case(q, P, P, "p = infinity")
    assert {"finite + finite", "a = P: doubles", "a = -P: infinity", "p = infinity"} == set(tags)
    classic = h.run("pt_add_affine_classic", ts)
    nway = h.run("pt_add_affine_nway", ts)
    for row, w, tag in zip(classic, want, tags):
        S.check(row, w, tag)
    assert classic == nway  # identical limbs on identical input
    # chained: each sum takes another term (and its own negation's x: P + A then + A)
    ts2 = [row + t[4 * F.L:] for row, t in zip(classic, ts)]
    want2 = [K.point_add(C, w, M_affine(F, t)) for w, t in zip(want, ts)]
    out2 = h.run("pt_add_affine_nway", ts2)
    for row, w in zip(out2, want2):
        S.check(row, w, "chained")
    assert out2 == h.run("pt_add_affine_classic", ts2)


def M_affine(F, t):
    L = F.L
    return (M.from_m(F, M.val(t[4 * L:5 * L]) % F.m), M.from_m(F, M.val(t[5 * L:6 * L]) % F.m))


@pytest.mark.parametrize("curve", CURVES)
def test_full_addition(curve, harness):
    h, S = harness(curve), points(curve)
    C, F = S.C, S.F
    n = len(S.pts)
    ts, want, tags = [], [], []

    def case(p, q, w, tag):
        ts.append(p + q)
        want.append(w)
        tags.append(tag)

    for i in range(n):
        P = S.pts[i]
        for v in range(10):
            j = (i + 1 + v) % n
            Q = S.pts[j]
            if Q != P and Q != K.point_neg(C, P):
                case(S.xyzz(i, v), S.xyzz(j, v + 3), K.point_add(C, P, Q), "finite + finite")
            case(S.xyzz(i, v), S.xyzz(i, v + 1), K.point_add(C, P, P), "p = q, other scaling")
            neg = h_neg(F, S.xyzz(i, v + 2))
            case(S.xyzz(i, v), neg, None, "p = -q")
        for q in S.infs():
            case(q, S.xyzz(i, i), P, "p infinite")
            case(S.xyzz(i, i + 1), q, P, "q infinite")
    for p in S.infs():
        for q in S.infs():
            case(p, q, None, "both infinite")
    out = h.run("pt_add", ts)
    for row, w, tag in zip(out, want, tags):
        S.check(row, w, tag)
    # chained: (p + q) + q
    ts2 = [row + t[4 * F.L:] for row, t in zip(out, ts)]
    for row, w, t in zip(h.run("pt_add", ts2), want, ts):
        S.check(row, K.point_add(C, w, M.decode_xyzz(F, t[4 * F.L:])[0]), "chained")


def h_neg(F, w):
    """-P on raw XYZZ limbs, host side: Y -> 4m - Y (Y < 4m, nonzero)"""
    L = F.L
    return w[:L] + F.limbs(4 * F.m - M.val(w[L:2 * L])) + w[2 * L:]


@pytest.mark.parametrize("curve", CURVES)
def test_to_affine_both_forms(curve, harness):
    h, S = harness(curve), points(curve)
    F = S.F
    n = len(S.pts)
    ts = [S.xyzz(i, v) for i in range(n) for v in range(10)] + S.infs()
    want = [M.affine_limbs(F, S.pts[i]) + [1] for i in range(n) for v in range(10)] + [[0] * (2 * F.L + 1)] * 4
    assert h.run("pt_to_affine", ts) == want
    for mode in (0, 1, 2):
        assert h.run("pt_to_affine_uniform", ts, mode) == want, mode


# ---- the entry point's argument checks ------------------------------------------
def test_argument_validation(harness):
    h = harness("BN254")
    F = M.FP29["BN254"]
    inp = np.zeros(2 * F.L, dtype=np.uint32)
    out = np.zeros(4 * F.L, dtype=np.uint32)
    assert h.raw(M.PRIM_OPS["mul"], 0, inp, 1, out) == 0
    assert h.raw(-1, 0, inp, 1, out) == KZGX_ERR_ARG
    assert h.raw(len(M.PRIM_NAMES), 0, inp, 1, out) == KZGX_ERR_ARG
    assert h.raw(M.PRIM_OPS["mul"], 1, inp, 1, out) == KZGX_ERR_ARG  # mode only for the uniform forms
    assert h.raw(M.PRIM_OPS["inv_uniform"], 3, inp, 1, out) == KZGX_ERR_ARG
    assert h.raw(M.PRIM_OPS["inv_uniform"], -1, inp, 1, out) == KZGX_ERR_ARG
    assert h.raw(M.PRIM_OPS["mul"], 0, inp, 0, out) == KZGX_ERR_ARG
    assert h.raw(M.PRIM_OPS["mul"], 0, inp, (1 << 16) + 1, out) == KZGX_ERR_ARG
    assert h.raw(M.PRIM_OPS["mul"], 0, None, 1, out) == KZGX_ERR_ARG
    assert h.raw(M.PRIM_OPS["mul"], 0, inp, 1, None) == KZGX_ERR_ARG
