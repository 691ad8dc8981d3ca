"""CPU: the exact integer model of the field primitives (oracle/field_model.py)
checked against number theory, its operand generators against its own
preconditions, and the 64-bit column sums of every product form of
csrc/field29.hpp at the documented operand classes.

Column-sum headroom.  The largest column sum over the class, as a fraction of
2^64 (real modulus limbs, reduction digits <= 2^29 - 1, the incoming carry
included; M.worst_column_sum):

    form class                                         BN254 (L=9)  BLS12-381 (L=14)
    one product,  normalized x normalized                 0.165        0.328
      f29_mul, f29_mul_lat, f29_mul_chain, f29_sqr, f29_sqr_chain,
      f29_mul_x2, f29_sqr_x2, f29_sqr_x2_pair, f29_mul_x3 (per chain)
    one product,  one operand with limbs < 2^30           0.305        0.547
      the f29_mul forms above (not the squares: their doubled limb must stay 30 bits)
    two products, normalized                              0.305        0.547
      f29_mul2, f29_mul2_lat, f29_mul2_chain, f29_mul2_mul, f29_mul2_x3
    two products, one operand with limbs < 2^30           0.446        0.766
    two products, TWO operands with limbs < 2^30          0.586        0.985 (*)

(*) not a documented class: it fits by 1.5 %, and a third lazy operand, or two
lazy operands of ONE product (limbs < 2^30 on both sides), overflow on
BLS12-381.  The headers allow one lazy operand per call; the model rejects
more."""
import pytest

import field_model as M
import kzg_ref as K

CURVES = ["BN254", "BLS12381"]
HEADROOM = {  # (products, lazy operands) -> fraction of 2^64, from the docstring
    "BN254": {(1, 0): 0.165, (1, 1): 0.305, (2, 0): 0.305, (2, 1): 0.446},
    "BLS12381": {(1, 0): 0.328, (1, 1): 0.547, (2, 0): 0.547, (2, 1): 0.766},
}


@pytest.mark.parametrize("name", CURVES)
def test_field_parameters(name):
    F = M.FP29[name]
    assert F.m == K.CURVES[name].p and F.R == 1 << (29 * F.L)
    assert (F.m * F.ninv + 1) % F.R == 0
    assert F.R >= 64 * F.m and 16 * F.m < F.R


@pytest.mark.parametrize("name", CURVES)
def test_redc_value_and_bound(name):
    F = M.FP29[name]
    m, R = F.m, F.R
    Ri = pow(R, -1, m)
    for a, b in M.product_pairs(F) + M.lazy_product_pairs(F) + M.digit_pairs(F):
        T = M.val(a) * M.val(b)
        t, q = M.redc(F, T)
        assert t % m == T * Ri % m
        assert T < R * m and t < 2 * m
        assert M.val(M.mul(F, a, b)) == t  # the column-by-column transcription agrees
    # the bound is sharp from both sides: just under R m the result reaches
    # 2m - 1, at R m + m it is 2m
    T = (2 * m - 1) * R - (R - 1) * m
    assert T < R * m and M.redc(F, T)[0] == 2 * m - 1
    T = R * m + m
    assert M.redc(F, T)[0] == 2 * m
    for T in (R * m, 2 * R * m - 1, 2 * R * m, 5 * R * m + 12345):
        t, _ = M.redc(F, T)
        assert T // R <= t < T // R + m + 1 and t % m == T * Ri % m
    assert M.redc(F, 2 * R * m)[0] >= 2 * m


@pytest.mark.parametrize("name", CURVES)
def test_generators_stay_inside_preconditions(name):
    """every generator's tuples pass the model's precondition checks (a
    ModelError would fail the test) and cover what they are meant to cover"""
    F = M.FP29[name]
    m, R = F.m, F.R
    V = M.corner_values(F)
    assert all(0 <= v < m for v in V) and len(set(V)) == len(V)
    assert {0, 1, m - 1, R % m, R * R % m} <= set(V)
    for a, b in M.product_pairs(F):
        assert M.is_norm(F, a) and M.is_norm(F, b)
        M.mul(F, a, b)
    assert any(R * m - M.val(a) * M.val(b) <= M.val(a) for a, b in M.product_pairs(F))  # just under R m
    for a in M.square_operands(F):
        M.sqr(F, a)
    assert any((M.val(a) + 1) ** 2 >= R * m for a in M.square_operands(F))
    for z in M.lazy_operands(F):
        assert M.is_lazy30(F, z)
    assert any(max(z) == (1 << 30) - 1 for z in M.lazy_operands(F))
    for z, b in M.lazy_product_pairs(F):
        assert not M.is_norm(F, z) or M.val(z) >= 0
        M.mul(F, z, b)
        M.mul(F, b, z)
    digits = set()
    for a, b in M.digit_pairs(F):
        M.mul(F, a, b)
        digits |= set(M.reduction_digits(F, [(a, b)]))
    assert {0, M.M29} <= digits
    lp = M.landing_pairs(F)
    assert set(lp) == {0, 1, m - 1, m, m + 1}
    for t, (a, b) in lp.items():
        assert M.val(M.mul(F, a, b)) == t
    lq = M.landing_quads(F)
    assert set(lq) == {0, m - 1, m, m + 1, 2 * m - 1}
    for t, q in lq.items():
        assert M.val(M.mul2(F, *q)) == t
    for a, b in M.add_tuples(F):
        M.add(F, a, b)
    for k in (2, 4, 6, 8, 10, 16):
        ts = M.sub_tuples(F, k)
        for a, b in ts:
            M.sub(F, a, b, k)
        assert any(max(b) == 3 * M.M29 for a, b in ts) and any(max(a) >= 1 << 29 for a, b in ts)
    for k in (1, 2, 4, 6, 8, 10, 16):
        for v in M.csub_values(F, k):
            M.csub(F, F.limbs(v), k)
    for a in M.normalize_operands(F):
        M.normalize(F, a)
    for kmax, fn in ((2, M.is_zero_lt2m), (16, M.is_zero)):
        vs = M.zero_test_values(F, kmax)
        assert all(0 <= v < kmax * m for v in vs)
        assert sum(fn(F, F.limbs(v)) for v in vs) == kmax
        filt = [v for v in vs if v % m and (v & M.M29) in (0, F.LOW[1])]
        assert {v & M.M29 for v in filt} == {0, F.LOW[1]}
    for a in M.inverse_operands(F):
        M.inv_mont(F, a)
        M.inv_raw(F, a)
    assert any(0 < M.val(a) < 1 << 60 for a in M.inverse_operands(F))
    assert any(M.fermat_admits(F, a) and M.val(a) > 8 * m for a in M.inverse_operands(F))
    NW = M.FP32[name].N
    for v in M.word_values(F, NW):
        w = M.FP32[name].words(v)
        assert M.to_words(F, M.from_words(F, w), NW) == w
    for j in range(NW):
        assert any((v >> (32 * j)) & 0xFFFFFFFF == 0xFFFFFFFF for v in M.word_values(F, NW))
    for F32 in (M.FP32[name], M.FR32[name]):
        assert all(0 <= v < F32.m for v in M.fe_values(F32))


@pytest.mark.parametrize("name", CURVES)
def test_model_rejects_undefined_input(name):
    F = M.FP29[name]
    m, R = F.m, F.R
    lazy = M.neg_lazy(F, F.limbs(5))
    one = F.limbs(1)
    with pytest.raises(M.ModelError):
        M.mul(F, lazy, lazy)  # two lazy operands
    with pytest.raises(M.ModelError):
        M.sqr(F, lazy)
    with pytest.raises(M.ModelError):
        M.mul(F, [1 << 30] + [0] * (F.L - 1), one)  # beyond the lazy class
    with pytest.raises(M.ModelError):
        M.mul(F, F.limbs(R - 1), F.limbs(m + 1))  # a b >= R m
    with pytest.raises(M.ModelError):
        M.mul2(F, lazy, one, one, lazy)
    with pytest.raises(M.ModelError):
        M.reduce(F, F.limbs(16 * m))
    with pytest.raises(M.ModelError):
        M.sub(F, F.limbs(0), F.limbs(2 * m + 1), 2)  # negative
    with pytest.raises(M.ModelError):
        M.neg_lazy(F, F.limbs(m))
    with pytest.raises(M.ModelError):
        M.neg8_lazy(F, F.limbs(4 * m))
    with pytest.raises(M.ModelError):
        M.is_zero_lt2m(F, F.limbs(2 * m))
    with pytest.raises(M.ModelError):
        M.csub(F, lazy, 1)
    with pytest.raises(M.ModelError):
        M.inv_mont(F, F.limbs(16 * m))


@pytest.mark.parametrize("name", CURVES)
def test_column_sums_fit_64_bits(name):
    """every product form, at its documented operand classes, keeps every
    64-bit column sum below 2^64; the figures are those of the module docstring"""
    F = M.FP29[name]
    for form, (nprod, lazy_ok) in M.PRODUCT_FORMS.items():
        for lazy in ((False, True) if lazy_ok else (False,)):
            s = M.worst_column_sum(F, nprod, lazy)
            assert s < 1 << 64, (form, lazy)
            assert abs(s / 2 ** 64 - HEADROOM[name][(nprod, int(lazy))]) < 0.0006, (form, lazy, s / 2 ** 64)
    # the class bound is reached by real operands: the all-maximum tuple's trace
    top, ones = [(1 << 30) - 1] * F.L, [M.M29] * F.L
    peak, _ = M.column_trace(F, [(top, ones), (ones, ones)])
    assert peak <= M.worst_column_sum(F, 2, True) and peak > 0.9 * M.worst_column_sum(F, 2, True)
    # beyond the documented class: two lazy operands of one product overflow on BLS12-381
    peak, _ = M.column_trace(F, [(top, top), (ones, ones)])
    assert (peak >= 1 << 64) == (name == "BLS12381")


@pytest.mark.parametrize("name", CURVES)
def test_inv_vt_transcription(name):
    """the pass-for-pass transcription of f29_inv_vt inverts, and stays inside
    the kernel's pass limit on the adversarial operands -- but not inside the
    "most passes seen" figure of its comment (16 / 21), which random inputs gave"""
    F = M.FP29[name]
    worst = 0
    for a in M.inverse_operands(F):
        x = M.val(a) % F.m
        v, passes = M.inv_vt_trace(F, a)
        assert v * x % F.m == (1 if x else 0)
        assert (passes == 0) == (x == 0)
        worst = max(worst, passes)
    assert worst <= M.inv_vt_pass_limit(F) // 3 + 2  # the limit is 3x a bound with room
    assert worst == {"BN254": 18, "BLS12381": 27}[name]
    assert worst > {"BN254": 16, "BLS12381": 21}[name]


@pytest.mark.parametrize("name", CURVES)
def test_fe_model(name):
    for F32 in (M.FP32[name], M.FR32[name]):
        m = F32.m
        x, y = M.fe_values(F32)[-1], M.fe_values(F32)[-2]
        wx, wy = F32.words(x), F32.words(y)
        mont = lambda v: v * F32.R % m
        assert M.fe_model(F32, "mul", F32.words(mont(x)), F32.words(mont(y))) == F32.words(mont(x * y % m))
        assert M.fe_model(F32, "to_mont", wx) == F32.words(mont(x))
        assert M.fe_model(F32, "from_mont", F32.words(mont(x))) == wx
        assert M.fe_model(F32, "inv", F32.words(mont(x))) == F32.words(mont(pow(x, -1, m)))
        assert M.fe_model(F32, "sub", wx, wy) == F32.words((x - y) % m)
        assert M.fe_model(F32, "inv", F32.words(0)) == F32.words(0)
        with pytest.raises(M.ModelError):
            M.fe_model(F32, "neg", F32.words(m))


@pytest.mark.parametrize("name", CURVES)
def test_point_encoding_round_trip(name):
    C, F = K.CURVES[name], M.FP29[name]
    P = K.scalar_mul(C, (C.gx, C.gy), 5)
    for lam, ks in ((1, (0, 0, 0, 0)), (12345, (7, 3, 1, 1)), (F.m - 2, (3, 1, 0, 1))):
        w = M.xyzz_limbs(F, P, lam, *ks)
        got, (X, Y, ZZ, ZZZ) = M.decode_xyzz(F, w)
        assert got == P and X < 8 * F.m and Y < 4 * F.m and ZZ < 2 * F.m and ZZZ < 2 * F.m
        assert pow(M.from_m(F, ZZ), 3, F.m) == pow(M.from_m(F, ZZZ), 2, F.m)
    assert M.decode_xyzz(F, M.inf_limbs(F))[0] is None
    with pytest.raises(M.ModelError):
        M.xyzz_limbs(F, P, 1, kx=8)
    assert len(M.PRIM_NAMES) == 69 and M.PRIM_OPS["pt_to_affine_uniform"] == 68


@pytest.mark.parametrize("name", CURVES)
def test_point_formulas_closed_under_their_bounds(name):
    """curve.hpp's formulas on the limb-exact model, operands at the documented
    bounds (X + 7m, Y + 3m, ZZ + m, ZZZ + m): every inner operation meets its
    precondition (a ModelError would fail the test), the result is the oracle's
    point and is again inside X < 8m, Y < 4m, ZZ, ZZZ < 2m, also when chained"""
    C, F = K.CURVES[name], M.FP29[name]
    X = M.XyzzModel(F)
    m, L = F.m, F.L
    G = (C.gx, C.gy)
    pts = [K.scalar_mul(C, G, k) for k in (1, 2, 3, 5, C.r - 1, C.r - 2, 0x1234567 << 150)]
    cut = lambda w: tuple(w[i * L:(i + 1) * L] for i in range(len(w) // L))
    flat = lambda p: [x for e in p for x in e]

    def check(p, want):
        got, (vx, vy, vzz, vzzz) = M.decode_xyzz(F, flat(p))
        assert got == want and (vzz == 0) == (want is None)
        assert all(M.is_norm(F, e) for e in p)
        assert vx < 8 * m and vy < 4 * m and vzz < 2 * m and vzzz < 2 * m
        return p

    reps = [(1, (0, 0, 0, 0)), (2, (7, 3, 1, 1)), (m - 1, (7, 3, 1, 1)), (F.R % m, (7, 0, 0, 1))]
    inf = cut(M.inf_limbs(F, 8 * m - 1, 4 * m - 1))
    for i, P in enumerate(pts):
        Q = pts[(i + 1) % len(pts)]
        for lam, ks in reps:
            p = cut(M.xyzz_limbs(F, P, lam, *ks))
            q = cut(M.xyzz_limbs(F, Q, 3 * lam + 1, *ks))
            d = check(X.dbl(p), K.point_add(C, P, P))
            check(X.dbl(d), K.scalar_mul(C, P, 4))
            check(X.dbl_affine(*cut(M.affine_limbs(F, P, 1, 1))), K.point_add(C, P, P))
            s = check(X.add_affine(p, cut(M.affine_limbs(F, Q))), K.point_add(C, P, Q))
            check(X.add_affine(s, cut(M.affine_limbs(F, Q))), K.point_add(C, K.point_add(C, P, Q), Q))
            check(X.add_affine(p, cut(M.affine_limbs(F, P))), K.point_add(C, P, P))
            check(X.add_affine(p, cut(M.affine_limbs(F, K.point_neg(C, P)))), None)
            check(X.add_affine(inf, cut(M.affine_limbs(F, P))), P)
            s = check(X.add(p, q), K.point_add(C, P, Q))
            check(X.add(s, q), K.point_add(C, K.point_add(C, P, Q), Q))
            check(X.add(p, cut(M.xyzz_limbs(F, P, lam + 2, 0, 0, 0, 0))), K.point_add(C, P, P))
            check(X.add(p, X.neg(cut(M.xyzz_limbs(F, P, lam + 2, 1, 1, 1, 0)))), None)
            check(X.add(inf, q), Q)
            check(X.add(p, inf), P)
            assert X.neg(X.neg(p)) == p
            x, y, fin = X.to_affine(p)
            assert fin and x + y == M.affine_limbs(F, P)
    assert X.to_affine(inf)[2] is False
