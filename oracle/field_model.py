"""Exact integer model of the device field primitives, in plain Python ints.

csrc/field29.hpp (radix-2^29 lazy-reduction Montgomery Fp) is modelled limb for
limb: a Montgomery product of operands with integer values a, b (and c, d) is

    t = (T + ((T * (-m^-1)) mod R) * m) / R,   T = a b (+ c d),  R = 2^(29 L),

as an integer, not only as a residue, so every product form must return exactly
limbs(t).  The carry helpers are transcribed from the code's definition.  Each
function states its precondition and raises ModelError on a tuple outside it:
a test can never "pass" on undefined input, and nothing outside a documented
bound is ever sent to the device.  csrc/field.hpp (32-bit CIOS, values always
in [0, m)) is modelled on values.  The inverses' oracle is pow(x, -1, m).

Also here, shared by tests/test_field_model.py (CPU) and
tests/test_gpu_primitives.py: the operation ids of the device harness
(csrc/selftest.hip PrimOp), the operand generators, the worst-case column
sums, and a transcription of f29_inv_vt that counts its passes.
"""
import math

import kzg_ref as K

W = 29
M29 = (1 << W) - 1


class ModelError(ValueError):
    """an operand tuple outside the operation's documented precondition"""


def need(cond, what):
    if not cond:
        raise ModelError(what)


# --------------------------------------------------------------------------
# fields
# --------------------------------------------------------------------------
class Field29:
    """radix-2^29 constants computed from the modulus alone"""

    def __init__(self, name, m, L):
        self.name, self.m, self.L = name, m, L
        self.R = 1 << (W * L)
        self.ninv = (-pow(m, -1, self.R)) % self.R  # -m^-1 mod R
        self.INV = self.ninv & M29
        self.P = self.limbs(m)
        self.K = {k: self.limbs(k * m) for k in (1, 2, 4, 6, 8, 10, 16)}
        # 2m / 8m with a unit borrowed into every limb from the one above
        self.P2B = self._borrowed(2 * m)
        self.P8B = self._borrowed(8 * m)
        self.R2 = self.limbs(self.R * self.R % m)
        self.R3 = self.limbs(pow(self.R, 3, m))
        self.ONE = self.limbs(self.R % m)
        self.LOW = [(k * m) & M29 for k in range(4)]

    def limbs(self, v):
        need(0 <= v < self.R, "value does not fit L limbs")
        return [(v >> (W * i)) & M29 for i in range(self.L)]

    def _borrowed(self, v):
        t = self.limbs(v)
        return [t[0] + (1 << W)] + [x + M29 for x in t[1:-1]] + [t[-1] - 1]


def val(a):
    return sum(x << (W * i) for i, x in enumerate(a))


class FieldW32:
    """csrc/field.hpp: N 32-bit words, R = 2^(32 N), values in [0, m)"""

    def __init__(self, name, m, N):
        self.name, self.m, self.N = name, m, N
        self.R = 1 << (32 * N)

    def words(self, v):
        need(0 <= v < self.R, "value does not fit N words")
        return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(self.N)]


def wval(w):
    return sum(x << (32 * i) for i, x in enumerate(w))


FP29 = {"BN254": Field29("BN254Fp29", K.BN254.p, 9), "BLS12381": Field29("BLS12381Fp29", K.BLS12381.p, 14)}
FR29 = {"BN254": Field29("BN254Fr29", K.BN254.r, 9), "BLS12381": Field29("BLS12381Fr29", K.BLS12381.r, 9)}
FP32 = {"BN254": FieldW32("BN254Fp", K.BN254.p, 8), "BLS12381": FieldW32("BLS12381Fp", K.BLS12381.p, 12)}
FR32 = {"BN254": FieldW32("BN254Fr", K.BN254.r, 8), "BLS12381": FieldW32("BLS12381Fr", K.BLS12381.r, 8)}


# --------------------------------------------------------------------------
# limb classes
# --------------------------------------------------------------------------
def is_norm(F, a):
    return len(a) == F.L and all(0 <= x <= M29 for x in a)


def is_lazy30(F, a):
    """limbs < 2^30: the output class of f29_neg_lazy / f29_neg8_lazy"""
    return len(a) == F.L and all(0 <= x < (1 << 30) for x in a)


def need_norm(F, a, what="operand"):
    need(is_norm(F, a), what + ": limbs not normalized (< 2^29)")


# --------------------------------------------------------------------------
# Montgomery products
# --------------------------------------------------------------------------
def redc(F, T):
    """(T + ((T ninv) mod R) m) / R as an integer, and the reduction digits q[k]"""
    q = (T * F.ninv) % F.R
    s = T + q * F.m
    assert s % F.R == 0
    return s // F.R, [(q >> (W * k)) & M29 for k in range(F.L)]


def column_trace(F, pairs):
    """the 64-bit accumulator of the product-scanning forms, column by column:
    the largest value it takes and the output limbs (the code's arithmetic,
    without the 2^64 wrap)"""
    L = F.L
    q = [0] * L
    t = [0] * L
    acc = 0
    peak = 0
    for k in range(2 * L - 1):
        for a, b in pairs:
            for i in range(L):
                j = k - i
                if 0 <= j < L:
                    acc += a[i] * b[j]
        for i in range(L):
            j = k - i
            if i < k and 1 <= j < L:
                acc += q[i] * F.P[j]
        if k < L:
            q[k] = ((acc & 0xFFFFFFFF) * F.INV) & M29
            acc += q[k] * F.P[0]
        peak = max(peak, acc)
        if k >= L:
            t[k - L] = acc & M29
        acc >>= W
    t[L - 1] = acc
    return peak, t


def mont(F, pairs, lazy_ok=True):
    """limbs of (sum of a b over pairs) / R mod m as the product forms compute it.

    Precondition (field29.hpp header, f29_neg_lazy / f29_neg8_lazy): every
    operand has normalized limbs except at most ONE operand of the call, whose
    limbs are < 2^30; sum a b < R m (then the result is < 2m); every 64-bit
    column sum stays below 2^64.  One or two products per reduction."""
    need(1 <= len(pairs) <= 2, "one or two products per reduction")
    ops = [x for p in pairs for x in p]
    lazy = [x for x in ops if not is_norm(F, x)]
    need(len(lazy) <= (1 if lazy_ok else 0), "more unnormalized operands than the form admits")
    need(all(is_lazy30(F, x) for x in lazy), "lazy operand: limbs not < 2^30")
    T = sum(val(a) * val(b) for a, b in pairs)
    need(T < F.R * F.m, "sum of products not below R m")
    peak, t = column_trace(F, pairs)
    need(peak < (1 << 64), "column sum overflows 64 bits")
    tv, _ = redc(F, T)
    assert val(t) == tv and tv < 2 * F.m and is_norm(F, t)
    return t


def mul(F, a, b):
    return mont(F, [(a, b)])


def sqr(F, a):
    """f29_sqr and its chained / paired forms: the doubled operand 2 a[j] must
    stay a 30-bit factor, so the operand is normalized"""
    return mont(F, [(a, a)], lazy_ok=False)


def mul2(F, a, b, c, d):
    return mont(F, [(a, b), (c, d)])


def reduction_digits(F, pairs):
    return redc(F, sum(val(a) * val(b) for a, b in pairs))[1]


# the product forms: (products per reduction, may take the one lazy operand)
PRODUCT_FORMS = {
    "f29_mul": (1, True), "f29_mul_lat": (1, True), "f29_mul_chain": (1, True),
    "f29_sqr": (1, False), "f29_sqr_chain": (1, False),
    "f29_mul2": (2, True), "f29_mul2_lat": (2, True), "f29_mul2_chain": (2, True),
    "f29_mul_x2": (1, True), "f29_sqr_x2": (1, False), "f29_sqr_x2_pair": (1, False), "f29_mul_x3": (1, True),
    "f29_mul2_mul": (2, True), "f29_mul2_x3": (2, True),
}


def worst_column_sum(F, nprod, lazy):
    """the largest 64-bit column sum of a product form over its documented
    operand class: nprod products of normalized operands (limbs <= 2^29 - 1),
    one operand of one product with limbs <= 2^30 - 1 if lazy; the reduction
    terms q[i] P[j] with q[i] <= 2^29 - 1 and the real modulus limbs; the carry
    of the column before"""
    L = F.L
    big = ((1 << 30) - 1) * M29 if lazy else M29 * M29
    peak = 0
    carry = 0
    for k in range(2 * L - 1):
        cnt = sum(1 for i in range(L) if 0 <= k - i < L)
        s = carry + cnt * (big + (nprod - 1) * M29 * M29)
        s += sum(M29 * F.P[k - i] for i in range(L) if i < k and 1 <= k - i < L)
        if k < L:
            s += M29 * F.P[0]
        peak = max(peak, s)
        carry = s >> W
    return peak


# --------------------------------------------------------------------------
# carry and reduction helpers (limb-exact transcriptions)
# --------------------------------------------------------------------------
def add(F, a, b):
    """f29_add.  Pre: limbs < 2^30 (its uint32 sums absorb a lazy operand),
    a + b < R (the top limb is masked)."""
    need(is_lazy30(F, a) and is_lazy30(F, b), "f29_add: limbs not < 2^30")
    need(val(a) + val(b) < F.R, "f29_add: sum does not fit L limbs")
    r, c = [], 0
    for i in range(F.L):
        s = a[i] + b[i] + c
        r.append(s & M29)
        c = s >> W
    assert val(r) == val(a) + val(b)
    return r


def sub(F, a, b, k):
    """f29_sub(a, b, k m) = a + k m - b.  Pre: a's limbs < 2^30, the subtrahend's
    < 3 2^29 (f29_add_2x_lazy's output class), 0 <= a + k m - b < R."""
    need(is_lazy30(F, a), "f29_sub: minuend limbs not < 2^30")
    need(len(b) == F.L and all(0 <= x <= 3 * M29 for x in b), "f29_sub: subtrahend limbs not < 3 2^29")
    v = val(a) + k * F.m - val(b)
    need(0 <= v < F.R, "f29_sub: a + K - b negative or too large")
    Kl = F.K[k]
    r, c = [], 0
    for i in range(F.L):
        s = a[i] + Kl[i] - b[i] + c
        assert -(1 << 31) <= s < (1 << 31)
        r.append(s & M29)
        c = s >> W  # arithmetic shift
    assert val(r) == v
    return r


def csub(F, a, k):
    """f29_csub(a, k m): a - k m if a >= k m, else a.  Pre: normalized limbs."""
    need_norm(F, a, "f29_csub")
    Kl = F.K[k]
    r, c = [], 0
    for i in range(F.L):
        s = a[i] - Kl[i] + c
        r.append(s & M29)
        c = s >> W
    out = list(a) if c < 0 else r
    assert val(out) == (val(a) - k * F.m if val(a) >= k * F.m else val(a))
    return out


def reduce(F, a):
    """f29_reduce.  Pre: normalized limbs, a < 16 m."""
    need_norm(F, a, "f29_reduce")
    need(val(a) < 16 * F.m, "f29_reduce: operand not < 16 m")
    r = a
    for k in (8, 4, 2, 1):
        r = csub(F, r, k)
    assert val(r) == val(a) % F.m
    return r


def neg_lazy(F, a):
    """f29_neg_lazy: 2m - a limb-wise.  Pre: normalized, a < m."""
    need_norm(F, a, "f29_neg_lazy")
    need(val(a) < F.m, "f29_neg_lazy: operand not < m")
    r = [F.P2B[i] - a[i] for i in range(F.L)]
    assert is_lazy30(F, r) and val(r) == 2 * F.m - val(a)
    return r


def neg8_lazy(F, a):
    """f29_neg8_lazy: 8m - a limb-wise.  Pre: normalized, a < 4m."""
    need_norm(F, a, "f29_neg8_lazy")
    need(val(a) < 4 * F.m, "f29_neg8_lazy: operand not < 4 m")
    r = [F.P8B[i] - a[i] for i in range(F.L)]
    assert is_lazy30(F, r) and val(r) == 8 * F.m - val(a)
    return r


def add_2x_lazy(F, a, b):
    """f29_add_2x_lazy: a + 2 b limb-wise.  Pre: both normalized."""
    need_norm(F, a, "f29_add_2x_lazy")
    need_norm(F, b, "f29_add_2x_lazy")
    return [a[i] + 2 * b[i] for i in range(F.L)]


def normalize(F, a):
    """f29_normalize.  Pre: limbs < 2^31.  The top limb is not masked."""
    need(len(a) == F.L and all(0 <= x < (1 << 31) for x in a), "f29_normalize: limbs not < 2^31")
    r, c = [], 0
    for i in range(F.L):
        s = a[i] + c
        r.append(s & M29 if i + 1 < F.L else s)
        c = s >> W
    need(r[-1] < (1 << 32), "f29_normalize: top limb overflows")
    assert val(r) == val(a)
    return r


def is_zero_lt2m(F, a):
    """f29_is_zero_lt2m.  Pre: normalized, a < 2m."""
    need_norm(F, a, "f29_is_zero_lt2m")
    need(val(a) < 2 * F.m, "f29_is_zero_lt2m: operand not < 2 m")
    return val(a) % F.m == 0


def is_zero(F, a):
    """f29_is_zero.  Pre: f29_reduce's."""
    return val(reduce(F, a)) == 0


def to_mont(F, a):
    return mul(F, a, F.R2)


def from_mont(F, a):
    return reduce(F, mul(F, a, [1] + [0] * (F.L - 1)))


def from_words(F, w):
    """f29_from_words: canonical 32-bit words -> limbs.  Pre: the value fits L limbs."""
    need(all(0 <= x <= 0xFFFFFFFF for x in w), "f29_from_words: not 32-bit words")
    return F.limbs(wval(w))


def to_words(F, a, nw):
    """f29_to_words.  Pre: normalized limbs (overlapping bits are OR-ed); bits
    above 32 nw are dropped."""
    need_norm(F, a, "f29_to_words")
    v = val(a)
    return [(v >> (32 * j)) & 0xFFFFFFFF for j in range(nw)]


def inv_mont(F, a):
    """the oracle of f29_inv / f29_inv_vt / f29_inv_uniform: for the Montgomery
    value a (= A R) the canonical Montgomery form of A^-1, a^-1 R^2 mod m
    (0 -> 0).  Pre: normalized limbs, a < 16 m."""
    need_norm(F, a, "inverse")
    need(val(a) < 16 * F.m, "inverse: operand not < 16 m")
    x = val(a) % F.m
    return F.limbs(pow(x, -1, F.m) * F.R * F.R % F.m if x else 0)


def inv_raw(F, a):
    """f29_inv_uniform_raw: the plain residue A^-1 = a^-1 R mod m"""
    need_norm(F, a, "inverse")
    need(val(a) < 16 * F.m, "inverse: operand not < 16 m")
    x = val(a) % F.m
    return F.limbs(pow(x, -1, F.m) * F.R % F.m if x else 0)


def fermat_admits(F, a):
    """f29_inv (a^(m-2) by f29_sqr / f29_mul): its first square needs a a < R m"""
    return is_norm(F, a) and val(a) < 16 * F.m and val(a) ** 2 < F.R * F.m


# --------------------------------------------------------------------------
# f29_inv_vt, transcribed (Pornin's binary GCD with 60-bit approximations)
# --------------------------------------------------------------------------
def inv_vt_pass_limit(F):
    return 3 * (2 * 29 * F.L // 29 + 2)


def inv_vt_trace(F, a_limbs):
    """(v, passes): the algorithm of f29_inv_vt on integers, pass for pass --
    v = y^-1 mod m for y = a mod m, and the number of passes its main loop
    makes (no pass limit here; the kernel's is inv_vt_pass_limit)"""
    m = F.m
    a = val(reduce(F, a_limbs))
    if a == 0:
        return 0, 0
    b, u, v = m, 1, 0
    half = pow(1 << W, -1, m)
    passes = 0
    while a != 0:
        n = max((a | b).bit_length(), 60)
        p = n - 31
        ab = (((a >> p) & 0x7FFFFFFF) << W) | (a & M29)
        bb = (((b >> p) & 0x7FFFFFFF) << W) | (b & M29)
        f0, g0, f1, g1 = 1, 0, 0, 1
        rem = W
        while rem > 0:
            if ab & 1:
                if ab < bb:
                    ab, bb = bb, ab
                    f0, f1 = f1, f0
                    g0, g1 = g1, g0
                ab -= bb
                f0 -= f1
                g0 -= g1
            z = rem
            if ab:
                z = min((ab & -ab).bit_length() - 1, rem)
            ab >>= z
            f1 <<= z
            g1 <<= z
            rem -= z
        assert all(abs(x) <= (1 << W) for x in (f0, g0, f1, g1))
        na, nb = a * f0 + b * g0, a * f1 + b * g1
        assert na % (1 << W) == 0 and nb % (1 << W) == 0
        na >>= W
        nb >>= W
        if na < 0:
            na, f0, g0 = -na, -f0, -g0
        if nb < 0:
            nb, f1, g1 = -nb, -f1, -g1
        u, v = (u * f0 + v * g0) * half % m, (u * f1 + v * g1) * half % m
        a, b = na, nb
        passes += 1
        assert passes < 10 * inv_vt_pass_limit(F), "no convergence"
    assert b == 1
    return v, passes


# --------------------------------------------------------------------------
# csrc/field.hpp on values
# --------------------------------------------------------------------------
def fe_model(F, op, a, b=None):
    """the fully reduced result of fe_<op> on words a (, b).  Pre: values in [0, m)."""
    x = wval(a)
    need(len(a) == F.N and 0 <= x < F.m, "fe operand not in [0, m)")
    y = None
    if b is not None:
        y = wval(b)
        need(len(b) == F.N and 0 <= y < F.m, "fe operand not in [0, m)")
    m, Ri = F.m, pow(F.R, -1, F.m)
    r = {
        "add": lambda: (x + y) % m, "sub": lambda: (x - y) % m, "neg": lambda: (-x) % m, "dbl": lambda: 2 * x % m,
        "mul": lambda: x * y * Ri % m, "sqr": lambda: x * x * Ri % m, "to_mont": lambda: x * F.R % m,
        "from_mont": lambda: x * Ri % m, "inv": lambda: pow(x, -1, m) * F.R * F.R % m if x else 0,
    }[op]()
    return F.words(r)


# --------------------------------------------------------------------------
# the device harness's operations (csrc/selftest.hip PrimOp, in order) and
# their shapes: (elements in, unit in, elements out, unit out, extra words out),
# units "L" = Fp29 limbs, "NP" = Fp words, "NR" = Fr words, "1" = one word
# --------------------------------------------------------------------------
_FE = ("add", "sub", "neg", "dbl", "mul", "sqr", "to_mont", "from_mont", "inv")
PRIM_NAMES = (
    ["mul", "mul_lat", "mul_chain", "sqr", "sqr_chain", "mul2", "mul2_lat", "mul2_chain", "mul_x2", "sqr_x2",
     "sqr_x2_pair", "mul_x3", "mul2_mul", "mul2_x3", "add", "sub_p2", "sub_p4", "sub_p6", "sub_p8", "sub_p10",
     "sub_p16", "neg_lazy", "neg8_lazy", "add_2x_lazy", "normalize", "csub_p", "csub_p2", "csub_p4", "csub_p6",
     "csub_p8", "csub_p10", "csub_p16", "reduce", "is_zero_lt2m", "is_zero", "to_mont", "from_mont", "from_words",
     "to_words", "inv", "inv_vt", "inv_uniform", "inv_uniform_raw"]
    + ["fr_" + s for s in _FE] + ["fp_" + s for s in _FE]
    + ["pt_dbl_affine", "pt_dbl", "pt_add_affine_classic", "pt_add_affine_nway", "pt_add", "pt_neg", "pt_to_affine",
       "pt_to_affine_uniform"])
PRIM_OPS = {n: i for i, n in enumerate(PRIM_NAMES)}
UNIFORM_OPS = ("inv_uniform", "inv_uniform_raw", "pt_to_affine_uniform")


def prim_shape(name):
    two = ("mul", "mul_lat", "mul_chain", "add", "add_2x_lazy", "sqr_x2", "sqr_x2_pair")
    if name in two or name.startswith("sub_p"):
        return (2, "L", 2 if name.startswith("sqr_x2") else 1, "L", 0)
    if name in ("mul2", "mul2_lat", "mul2_chain"):
        return (4, "L", 1, "L", 0)
    if name == "mul_x2":
        return (4, "L", 2, "L", 0)
    if name == "mul_x3":
        return (6, "L", 3, "L", 0)
    if name == "mul2_mul":
        return (6, "L", 2, "L", 0)
    if name == "mul2_x3":
        return (8, "L", 3, "L", 0)
    if name in ("is_zero_lt2m", "is_zero"):
        return (1, "L", 1, "1", 0)
    if name == "from_words":
        return (1, "NP", 1, "L", 0)
    if name == "to_words":
        return (1, "L", 1, "NP", 0)
    if name.startswith("fr_") or name.startswith("fp_"):
        u = "NR" if name.startswith("fr_") else "NP"
        return (2 if name[3:] in ("add", "sub", "mul") else 1, u, 1, u, 0)
    if name == "pt_dbl_affine":
        return (2, "L", 4, "L", 0)
    if name in ("pt_dbl", "pt_neg"):
        return (4, "L", 4, "L", 0)
    if name in ("pt_add_affine_classic", "pt_add_affine_nway"):
        return (6, "L", 4, "L", 0)
    if name == "pt_add":
        return (8, "L", 4, "L", 0)
    if name in ("pt_to_affine", "pt_to_affine_uniform"):
        return (4, "L", 2, "L", 1)
    return (1, "L", 1, "L", 0)


def prim_words(curve, name):
    """(words in, words out) per tuple"""
    unit = {"L": FP29[curve].L, "NP": FP32[curve].N, "NR": FR32[curve].N, "1": 1}
    ni, ui, no, uo, xo = prim_shape(name)
    return ni * unit[ui], no * unit[uo] + xo


# --------------------------------------------------------------------------
# operand generators (every tuple inside its operation's precondition)
# --------------------------------------------------------------------------
def _fit(F, lim, bound):
    """limbs with the top limbs cut so that the value is < bound"""
    lim = list(lim)
    i = F.L - 1
    while val(lim) >= bound:
        top = (bound - 1) >> (W * i)
        if lim[i] > top:
            lim[i] = top
        if val(lim) >= bound:
            lim[i] = max(lim[i] - 1, 0)
        i -= 1
    return val(lim)


def corner_values(F, nrand=32, seed=0x29F1E1D):
    """canonical values in [0, m) where limb arithmetic goes wrong"""
    m, L, R = F.m, F.L, F.R
    vs = [0, 1, 2, m - 2, m - 1, (m + 1) // 2, (m - 1) // 2, R % m, R * R % m]
    for j in range(L + 1):
        for k in (W * j - 1, W * j, W * j + 1):
            if k >= 0:
                vs += [v for v in ((1 << k), (1 << k) - 1) if v < m]
    vs.append(_fit(F, [M29] * L, m))
    for i in range(L):
        vs.append(_fit(F, [M29 if j == i else 0 for j in range(L)], m))
        vs.append(_fit(F, [1 if j == i else 0 for j in range(L)], m))
    vs.append(_fit(F, [M29 if j % 2 == 0 else 0 for j in range(L)], m))
    vs.append(_fit(F, [M29 if j % 2 == 1 else 0 for j in range(L)], m))
    g = K.splitmix64(seed)
    for _ in range(nrand):
        v = 0
        for w in range((m.bit_length() + 63) // 64):
            v |= next(g) << (64 * w)
        vs.append(v % m)
    out, seen = [], set()
    for v in vs:
        assert 0 <= v < m
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


def representatives(F, x, kmax):
    """x + k m for k = 0 .. kmax - 1 (all < kmax m when x < m)"""
    return [x + k * F.m for k in range(kmax)]


def product_pairs(F):
    """(a, b) limb pairs of normalized operands with a b < R m: the corner values
    against each other and themselves, their non-canonical representatives at
    the bounds curve.hpp documents (X < 8m, P < 10m, reduce < 16m), and pairs
    just under R m"""
    m, R = F.m, F.R
    V = corner_values(F)
    n = len(V)
    prs = []
    for i, v in enumerate(V):
        prs.append((v, V[(7 * i + 3) % n]))
        prs.append((v, v))
    reps = (0, 1, 3, 7, 9, 13, 15)
    for i, v in enumerate(V[:40]):
        w = V[(5 * i + 1) % n]
        ka, kb = reps[i % len(reps)], reps[(i // len(reps) + i) % len(reps)]
        prs.append((v + ka * m, w + kb * m))
        prs.append((v + ka * m, v + ka * m))
    # just under R m: b the largest cofactor of a
    for a in (m - 1, 2 * m - 1, 8 * m - 1, 10 * m - 1, 16 * m - 1, R - 1, (R - 1) // 3):
        b = (R * m - 1) // a
        if b < R:
            prs += [(a, b), (b, a), (a, b - 1)]
    out = []
    for a, b in prs:
        if a < R and b < R and a * b < R * m:
            out.append((F.limbs(a), F.limbs(b)))
    return out


def square_operands(F):
    """normalized a with a a < R m"""
    m = F.m
    out = [a for a, b in product_pairs(F) if a == b]
    k = 1
    while (k * m - 1) ** 2 < F.R * m and k <= 16:
        out.append(F.limbs(k * m - 1))
        out.append(F.limbs(k * m - m))
        k += 1
    r = math.isqrt(F.R * m - 1)  # the largest admissible
    if r < F.R:
        out.append(F.limbs(r))
    return out


def lazy_operands(F):
    """unnormalized operands of the class limbs < 2^30: f29_neg_lazy and
    f29_neg8_lazy outputs on the corner values, and hand-built class maxima"""
    m = F.m
    out = []
    for i, v in enumerate(corner_values(F, nrand=8)):
        out.append(neg_lazy(F, F.limbs(v)))
        out.append(neg8_lazy(F, F.limbs(v + (i % 4) * m)))
    top = (1 << 30) - 1
    out.append([top] * F.L)
    out.append([top] * (F.L - 1) + [0])
    out.append([top if j % 2 == 0 else 0 for j in range(F.L)])
    return out


def lazy_product_pairs(F):
    """(lazy, normalized partner) with lazy * partner < R m, partners from the
    corner values and the largest admissible cofactor"""
    m, R = F.m, F.R
    V = corner_values(F, nrand=8)
    out = []
    for i, z in enumerate(lazy_operands(F)):
        zv = val(z)
        cands = [V[(3 * i + 1) % len(V)] + (i % 8) * m, (R * m - 1) // zv, _fit(F, [M29] * F.L, min(R, (R * m - 1) // zv + 1))]
        for b in cands:
            if b < R and zv * b < R * m:
                out.append((z, F.limbs(b)))
    return out


def digit_pairs(F):
    """normalized (a, b), a b < R m, whose reduction digits q[k] are forced: all
    zero with a nonzero product, all 2^29 - 1, and alternating patterns"""
    L, R, m = F.L, F.R, F.m
    out = []
    # a b = a multiple of R: every digit zero
    out.append((F.limbs(1 << W), F.limbs(3 << (W * (L - 1)))))
    pats = [[M29] * L, [M29 if k % 2 == 0 else 0 for k in range(L)], [0 if k % 2 == 0 else M29 for k in range(L)],
            [0] * (L - 1) + [M29], [M29] + [0] * (L - 1)]
    for qd in pats:
        q = val(qd)
        for a in (1, 3, (1 << W) - 1):
            b = (-q * m * pow(a, -1, R)) % R  # a b = -q m mod R  =>  digits = q
            if a * b < R * m:
                out.append((F.limbs(a), F.limbs(b)))
    for a, b in out:
        assert reduction_digits(F, [(a, b)]) in pats + [[0] * L]
    return out


def landing_pairs(F):
    """{t: (a, b)}: normalized pairs, a b < R m, whose REDC result is exactly t,
    for t = 0, 1, m - 1, m, m + 1.  (A single product landing on 2m - 1 needs
    a b in a window of width R just under R m with both factors below R, that
    is, a factorisation; landing_quads reaches it with two products.)"""
    m, R = F.m, F.R
    out = {0: (0, 0), 1: (1, R % m), m - 1: (1, (m - 1) * R % m), m: (m, R - 1)}
    # t = m + 1: a b = R + m b' with b' = -R / m mod a
    a = 3
    bp = (-R * pow(m, -1, a)) % a or a
    out[m + 1] = (a, (R + m * bp) // a)
    res = {}
    for t, (a, b) in out.items():
        assert a * b < R * m and redc(F, a * b)[0] == t
        res[t] = (F.limbs(a), F.limbs(b))
    return res


def landing_quads(F):
    """{t: (a, b, c, d)}: a b + c d < R m with REDC result exactly t, for
    t = 0, m, m - 1, m + 1, 2m - 1 (T = t R - q m, split as m (T // m) + 1 (T % m))"""
    m, R = F.m, F.R
    res = {}
    for t in (0, m - 1, m, m + 1, 2 * m - 1):
        q = R - 1 if t >= m else t * R // m
        T = t * R - q * m
        assert 0 <= T < R * m and redc(F, T)[0] == t
        res[t] = (F.limbs(m), F.limbs(T // m), F.limbs(1), F.limbs(T % m))
    return res


def zero_test_values(F, kmax):
    """k m - 1, k m, k m + 1 for k < kmax, kmax m - 1, and nonzero values whose
    low limb is 0 or LOW[1] (they pass the one-limb filter of
    f29_is_zero_lt2m and must still be answered no); all < kmax m"""
    m = F.m
    vs = []
    for k in range(kmax):
        vs += [v for v in (k * m - 1, k * m, k * m + 1) if 0 <= v < kmax * m]
    vs.append(kmax * m - 1)
    bound = kmax * m
    for hi in (1, 2, M29, (m >> W) - 1, m >> W, (m >> W) + 1, ((bound - 1) >> W) - 1):
        for lo in (0, F.LOW[1]):
            v = (hi << W) + lo
            if 0 < v < bound and v % m != 0:
                vs.append(v)
    return sorted(set(vs))


def inverse_operands(F):
    """values < 16 m for the four inverse forms: the corner values and their
    representatives up to 16 m, Montgomery representatives shorter than 60
    bits, x 2^k, m - 2^k, and the multiples of m (-> 0)"""
    m = F.m
    V = corner_values(F, nrand=12)
    vs = []
    for i, v in enumerate(V):
        vs.append(v + (i % 16) * m)
    vs += [v + 15 * m for v in V[:12]]
    vs += [1, 2, 3, 5, (1 << 29) - 1, 1 << 29, (1 << 30) + 1, (1 << 58) + 3, (1 << 59) - 1, (1 << 60) - 1, 1 << 60]
    x = V[-1] | 1
    for k in range(0, m.bit_length(), 23):
        vs.append((x << k) % m)
        vs.append((3 << k) % m)
        vs.append(m - (1 << k))
    vs += [k * m for k in range(16)]
    vs.append(16 * m - 1)
    out, seen = [], set()
    for v in vs:
        assert 0 <= v < 16 * m
        if v not in seen:
            seen.add(v)
            out.append(F.limbs(v))
    return out


def word_values(F, nw):
    """word-form values for f29_from_words / f29_to_words: each 32-bit word all
    ones in turn (the others zero, or from a fixed pattern), plus the corner
    values.  The conversions do not reduce, so the values only fit nw words
    (with the top word all ones they exceed m)."""
    vs = list(corner_values(F, nrand=8))
    base = int.from_bytes(bytes((37 * i + 11) & 0xFF for i in range(4 * nw)), "little")
    for j in range(nw):
        for b in (0, base):
            vs.append(b | (0xFFFFFFFF << (32 * j)))
    vs.append((1 << (32 * nw)) - 1)
    assert all(0 <= v < 1 << (32 * nw) for v in vs)
    return vs


def fe_values(F32, nrand=16, seed=0xFE32):
    """values in [0, m) for field.hpp: the edges of the 32-bit carry chains"""
    m, N = F32.m, F32.N
    vs = [0, 1, 2, m - 2, m - 1, (m + 1) // 2, (m - 1) // 2, F32.R % m, F32.R * F32.R % m]
    for j in range(N + 1):
        for k in (32 * j - 1, 32 * j, 32 * j + 1):
            if k >= 0:
                vs += [v % m for v in ((1 << k), (1 << k) - 1)]
    for j in range(N):
        vs.append((0xFFFFFFFF << (32 * j)) % m)
        vs.append(((1 << (32 * N)) - 1 - (0xFFFFFFFF << (32 * j))) % m)
        vs.append((m | (0xFFFFFFFF << (32 * j))) % m)
    g = K.splitmix64(seed)
    for _ in range(nrand):
        v = 0
        for w in range((m.bit_length() + 63) // 64):
            v |= next(g) << (64 * w)
        vs.append(v % m)
    out, seen = [], set()
    for v in vs:
        if v not in seen:
            seen.add(v)
            out.append(v)
    return out


# --------------------------------------------------------------------------
# points: XYZZ / affine limbs <-> the oracle's affine points
# --------------------------------------------------------------------------
def to_m(F, x):
    return x * F.R % F.m


def from_m(F, x):
    return x * pow(F.R, -1, F.m) % F.m


def xyzz_limbs(F, P, lam=1, kx=0, ky=0, kzz=0, kzzz=0):
    """the affine point P scaled by lam (X = lam^2 x, Y = lam^3 y, ZZ = lam^2,
    ZZZ = lam^3, Montgomery form), each coordinate shifted by its k multiples of
    m; within curve.hpp's bounds X < 8m, Y < 4m, ZZ, ZZZ < 2m"""
    m = F.m
    need(P is not None and lam % m != 0, "finite point, nonzero scaling")
    need(0 <= kx <= 7 and 0 <= ky <= 3 and 0 <= kzz <= 1 and 0 <= kzzz <= 1, "representative beyond the bound")
    l2, l3 = lam * lam % m, pow(lam, 3, m)
    vals = (to_m(F, l2 * P[0] % m) + kx * m, to_m(F, l3 * P[1] % m) + ky * m, to_m(F, l2) + kzz * m,
            to_m(F, l3) + kzzz * m)
    return [x for v in vals for x in F.limbs(v)]


def inf_limbs(F, X=None, Y=None):
    """infinity: ZZ = ZZZ = 0, X = Y = R mod m (the canonical form) or the given values"""
    one = F.R % F.m
    return F.limbs(one if X is None else X) + F.limbs(one if Y is None else Y) + [0] * (2 * F.L)


def affine_limbs(F, P, kx=0, ky=0):
    return F.limbs(to_m(F, P[0]) + kx * F.m) + F.limbs(to_m(F, P[1]) + ky * F.m)


def decode_xyzz(F, w):
    """(affine point, None for infinity, or "not a point" when ZZ or ZZZ is a
    nonzero multiple of m; the four integer values) of raw XYZZ limbs"""
    L = F.L
    X, Y, ZZ, ZZZ = (val(w[i * L:(i + 1) * L]) for i in range(4))
    if ZZ == 0:
        return None, (X, Y, ZZ, ZZZ)
    m = F.m
    if ZZ % m == 0 or ZZZ % m == 0:
        return "not a point", (X, Y, ZZ, ZZZ)
    return (X * pow(ZZ, -1, m) % m, Y * pow(ZZZ, -1, m) % m), (X, Y, ZZ, ZZZ)


class XyzzModel:
    """csrc/curve.hpp's formulas transcribed onto the limb-exact model: every
    inner product, sum and difference passes its own precondition check, so
    running a formula on operands at the documented bounds (X < 8m, Y < 4m,
    ZZ, ZZZ < 2m, affine < m; < 2m for the affine doubling) shows that the
    bounds the comments give for the intermediate values hold.  Points are
    (X, Y, ZZ, ZZZ) limb lists; the default (classic) negation of Y1."""

    def __init__(self, F):
        self.F = F
        self.Z = [0] * F.L

    def is_inf(self, p):
        return all(x == 0 for x in p[2])

    def inf(self):
        return (self.F.ONE, self.F.ONE, self.Z, self.Z)

    def dbl_affine(self, x, y):
        F = self.F
        U = add(F, y, y)
        V = sqr(F, U)
        Wv = mul(F, U, V)
        S = mul(F, x, V)
        xx = sqr(F, x)
        Mm = add(F, add(F, xx, xx), xx)
        X3 = sub(F, sqr(F, Mm), add(F, S, S), 4)
        Y3 = mul2(F, Mm, sub(F, S, X3, 8), Wv, sub(F, self.Z, y, 4))
        return (X3, Y3, V, Wv)

    def dbl(self, p):
        if self.is_inf(p):
            return p
        F = self.F
        X3, Y3, V, Wv = self.dbl_affine(p[0], p[1])
        return (X3, Y3, mul(F, V, p[2]), mul(F, Wv, p[3]))

    def add_affine(self, p, a):
        F = self.F
        if self.is_inf(p):
            return (a[0], a[1], F.ONE, F.ONE)
        X, Y, ZZ, ZZZ = p
        U2 = mul(F, a[0], ZZ)
        S2 = mul(F, a[1], ZZZ)
        P = sub(F, U2, X, 8)
        R = sub(F, S2, Y, 4)
        PP = sqr(F, P)
        if is_zero_lt2m(F, PP):
            return self.dbl_affine(a[0], a[1]) if is_zero(F, R) else self.inf()
        PPP = mul(F, P, PP)
        Q = mul(F, X, PP)
        X3 = sub(F, sqr(F, R), add_2x_lazy(F, PPP, Q), 6)
        Y3 = mul2(F, R, sub(F, Q, X3, 8), sub(F, self.Z, Y, 4), PPP)
        return (X3, Y3, mul(F, ZZ, PP), mul(F, ZZZ, PPP))

    def add(self, p, q):
        F = self.F
        if self.is_inf(p):
            return q
        if self.is_inf(q):
            return p
        U1 = mul(F, p[0], q[2])
        U2 = mul(F, q[0], p[2])
        S1 = mul(F, p[1], q[3])
        S2 = mul(F, q[1], p[3])
        P = sub(F, U2, U1, 2)
        R = sub(F, S2, S1, 2)
        PP = sqr(F, P)
        if is_zero_lt2m(F, PP):
            return self.dbl(p) if is_zero(F, R) else self.inf()
        PPP = mul(F, P, PP)
        Q = mul(F, U1, PP)
        X3 = sub(F, sqr(F, R), add(F, PPP, add(F, Q, Q)), 6)
        Y3 = mul2(F, R, sub(F, Q, X3, 8), sub(F, self.Z, S1, 2), PPP)
        return (X3, Y3, mul(F, mul(F, p[2], q[2]), PP), mul(F, mul(F, p[3], q[3]), PPP))

    def neg(self, p):
        return (p[0], sub(self.F, self.Z, p[1], 4), p[2], p[3])

    def to_affine(self, p):
        """(x limbs, y limbs, finite)"""
        F = self.F
        if self.is_inf(p):
            return self.Z, self.Z, False
        i = inv_mont(F, mul(F, p[2], p[3]))
        return reduce(F, mul(F, p[0], mul(F, i, p[3]))), reduce(F, mul(F, p[1], mul(F, i, p[2]))), True


# --------------------------------------------------------------------------
# operands of the carry helpers
# --------------------------------------------------------------------------
def add_tuples(F):
    """(a, b) for f29_add: normalized representatives up to 8m each, carries
    through every limb, and a lazy operand (limbs < 2^30) on either side"""
    m, R = F.m, F.R
    V = corner_values(F, nrand=12)
    n = len(V)
    out = []
    for i, v in enumerate(V):
        a, b = v + (i % 8) * m, V[(3 * i + 2) % n] + ((i // 8) % 8) * m
        out.append((F.limbs(a), F.limbs(b)))
    ones = _fit(F, [M29] * F.L, R)
    out += [(F.limbs(ones), F.limbs(0)), (F.limbs(ones - 1), F.limbs(1)), (F.limbs(R - 1 - 16 * m), F.limbs(16 * m))]
    for i, z in enumerate(lazy_operands(F)):
        b = F.limbs(V[i % n] + (i % 6) * m)
        if val(z) + val(b) < R:
            out += [(z, b), (b, z)]
    return out


def sub_tuples(F, k):
    """(a, b) for f29_sub(a, b, k m) with 0 <= a + k m - b < R: normalized
    representatives b <= k m, the exact landings a + k m - b = 0, f29_neg_lazy
    minuends, f29_add_2x_lazy subtrahends, and hand-built subtrahends at the
    class maximum 3 (2^29 - 1) per limb with the top limb cut to fit"""
    m, R = F.m, F.R
    V = corner_values(F, nrand=12)
    n = len(V)
    out = []
    for i, v in enumerate(V):
        b = v + (i % k) * m
        a = V[(5 * i + 1) % n] + ((i // 3) % 10) * m
        out.append((F.limbs(a), F.limbs(b)))
    out += [(F.limbs(0), F.limbs(k * m)), (F.limbs(1), F.limbs(k * m)), (F.limbs(0), F.limbs(k * m - 1)),
            (F.limbs(0), F.limbs(0)), (F.limbs(m), F.limbs((k + 1) * m)), (F.limbs(R - 1 - k * m), F.limbs(0))]
    for i, z in enumerate(lazy_operands(F)):
        b = F.limbs(V[i % n] + (i % k) * m)
        if val(z) + k * m - val(b) < R:
            out.append((z, b))
    for i, v in enumerate(V):  # subtrahend p + 2 q without carries
        p, q = v, V[(7 * i + 5) % n]
        kk = (k - 1) // 3  # p + kk m + 2 (q + kk m) < (3 kk + 3) m <= k m + ... checked below
        z = add_2x_lazy(F, F.limbs(p + kk * m), F.limbs(q + kk * m))
        a = V[(i + 9) % n] + (i % 4) * m
        if val(z) <= a + k * m:
            out.append((F.limbs(a), z))
    low = [3 * M29] * (F.L - 1)
    for a in (0, m - 1, 9 * m):
        room = a + k * m - val(low)
        if room >= 0:
            top = min(room >> (W * (F.L - 1)), 3 * M29)
            out.append((F.limbs(a), low + [top]))
    return out


def csub_values(F, k):
    """normalized values for f29_csub(a, k m): around every multiple of m up to
    16 m, around k m, the corner values, all limbs 2^29 - 1"""
    m = F.m
    vs = [v for j in range(17) for v in (j * m - 1, j * m, j * m + 1) if v >= 0]
    vs += [k * m - 1, k * m, k * m + 1, 2 * k * m, F.R - 1, F.R - 2]
    vs += [v + (i % 16) * m for i, v in enumerate(corner_values(F, nrand=8))]
    return sorted(set(vs))


def normalize_operands(F):
    """limbs < 2^31 for f29_normalize: the lazy classes, f29_add_2x_lazy outputs,
    a carry through every limb, and the class maximum"""
    V = corner_values(F, nrand=8)
    out = list(lazy_operands(F))
    for i, v in enumerate(V):
        out.append(add_2x_lazy(F, F.limbs(v + (i % 8) * F.m), F.limbs(V[(i + 3) % len(V)] + (i % 5) * F.m)))
    top = (1 << 31) - 1
    out += [[top] * F.L, [M29 + 1] + [M29] * (F.L - 1), [3 * M29] * F.L, [0] * F.L, [top] + [0] * (F.L - 1)]
    return out
