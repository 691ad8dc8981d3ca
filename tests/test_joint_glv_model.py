"""The block table's endomorphism split (msm_joint.hip, GLV) as a pure-Python model.

Both curves have j = 0: phi(x, y) = (beta x, y) = [lambda]P on the order-r
subgroup.  k_joint_index writes every scalar k = k1 + lambda k2 (mod r) with
both halves odd and |k_i| <= 2^128 - 1, and recodes each half in 128 regular
+-1 digits; the MSM is S_1 + phi(S_2), each S_h a 128-plane block-table sum.

The model, derived here from the oracle's curve parameters alone:

* (v1, v2) = ((a1, b1), (a2, b2)): Euclid's short basis of the lattice
  {(a, b): a + b lambda = 0 mod r}, signs chosen so that the coordinates of
  (k, 0), x1 = k n1 / r and x2 = k n2 / r with n1 = |b2|, n2 = |b1|, are >= 0;
* f_i = floor(k g_i / 2^SHIFT) with g_i = floor(2^SHIFT n_i / r).  For k < r <
  2^255: 0 <= x_i - k g_i / 2^SHIFT < k / 2^SHIFT < 2^(255 - SHIFT) = eps, so
  f_i <= x_i < f_i + 1 + eps;
* c_i is the one of f_i, f_i + 1 with the parity that makes both halves odd
  (the parity rule: (c1, c2) = basis^-1 (k + 1, 1) mod 2, the basis'
  determinant +-r being odd), so x_i - c_i = e_i lies in (-1, 1 + eps);
* (k1, k2) = (k, 0) - c1 v1 - c2 v2 = e1 v1 + e2 v2.

The bound, from the basis entries and the parity rule alone (no sampling):
|k1| < (1 + eps)(|a1| + |a2|) and |k2| < (1 + eps)(|b1| + |b2|); both right
sides are asserted <= 2^128, so |k_i| <= 2^128 - 1 for every k < r.
"""
import os
import re
from fractions import Fraction

import pytest

import kzg_ref as K

CURVES = [K.BN254, K.BLS12381]
SHIFT = 288
HALF_BITS = 128
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kzg-commitments_amd", "csrc",
                      "curve_consts.h")


def cube_roots(m):
    g = 2
    while pow(g, (m - 1) // 3, m) == 1:
        g += 1
    w = pow(g, (m - 1) // 3, m)
    return w, w * w % m


_PARAMS = {}


def params(C):
    """beta, lambda, the sign-normalised short basis, the rounding multipliers"""
    if C.name in _PARAMS:
        return _PARAMS[C.name]
    G = (C.gx, C.gy)
    # one fixed beta per curve (BLS12-381: the subgroup test's, [-x^2]P = phi(P)); lambda follows from it
    if C.name == "BN254":
        beta = min(cube_roots(C.p))
    else:
        x2 = K._BLS_X ** 2
        want = K.scalar_mul(C, G, (-x2) % C.r)
        beta = [b for b in cube_roots(C.p) if (b * C.gx % C.p, C.gy) == want][0]
    lam = [l for l in cube_roots(C.r) if K.scalar_mul(C, G, l) == (beta * C.gx % C.p, C.gy)]
    assert len(lam) == 1
    lam = lam[0]
    rows = [(C.r, 0), (lam, 1)]  # remainder s = (...) r + t lambda: s - t lambda = 0 mod r
    while rows[-1][0] ** 2 >= C.r:
        q = rows[-2][0] // rows[-1][0]
        rows.append((rows[-2][0] - q * rows[-1][0], rows[-2][1] - q * rows[-1][1]))
    q = rows[-2][0] // rows[-1][0]
    nxt = (rows[-2][0] - q * rows[-1][0], rows[-2][1] - q * rows[-1][1])
    a1, b1 = rows[-1][0], -rows[-1][1]
    a2, b2 = min([(rows[-2][0], -rows[-2][1]), (nxt[0], -nxt[1])], key=lambda v: max(abs(v[0]), abs(v[1])))
    det = a1 * b2 - a2 * b1
    if b2 * det < 0:
        a1, b1, det = -a1, -b1, -det
    if -b1 * det < 0:
        a2, b2, det = -a2, -b2, -det
    n1, n2 = abs(b2), abs(b1)
    d = dict(beta=beta, lam=lam, basis=((a1, b1), (a2, b2)), det=det, n=(n1, n2),
             g=((n1 << SHIFT) // C.r, (n2 << SHIFT) // C.r))
    _PARAMS[C.name] = d
    return d


def split(C, k):
    """(k1, k2) of a scalar k (any 256-bit value: reduced first), as the device forms them"""
    d = params(C)
    (a1, b1), (a2, b2) = d["basis"]
    k %= C.r
    c1, c2 = (k * d["g"][0]) >> SHIFT, (k * d["g"][1]) >> SHIFT
    c1 += (c1 ^ (b2 * (k + 1) + a2)) & 1
    c2 += (c2 ^ (b1 * (k + 1) + a1)) & 1
    return k - c1 * a1 - c2 * a2, -c1 * b1 - c2 * b2


def recode_half(v):
    """plus-bits of an odd half's 128 planes: bit w = 1 iff digit w is +1"""
    assert v & 1 and abs(v) < 1 << HALF_BITS
    p = (abs(v) >> 1) | (1 << (HALF_BITS - 1))
    return p ^ (((1 << HALF_BITS) - 1) if v < 0 else 0)


def planes(C, k):
    """the 256 plus-bits of scalar k: planes 0..127 half 0, 128..255 half 1"""
    k1, k2 = split(C, k)
    return recode_half(k1) | (recode_half(k2) << HALF_BITS)


def proved_bound(C):
    """strict upper bounds on |k1|, |k2| over every k < r"""
    (a1, b1), (a2, b2) = params(C)["basis"]
    assert C.r < 1 << 255
    e = 1 + Fraction(1, 1 << (SHIFT - 255))
    return e * (abs(a1) + abs(a2)), e * (abs(b1) + abs(b2))


def edge_scalars(C):
    r, lam = C.r, params(C)["lam"]
    return [0, 1, 2, 3, r - 1, r - 2, lam, lam + 1, lam - 1, r - lam, (r + 1) // 2, (r - 1) // 2, 1 << 253,
            lam * lam % r]


def boundary_scalars(C):
    """scalars on both sides of the rounding boundaries of c1 and c2: where x_i = k n_i / r crosses an integer
    (the floor steps) and a half-integer (Babai's rounding steps), k = ceil((j + 1/2) r / n) +- 1 included"""
    out = []
    for n in params(C)["n"]:
        for j in (0, 1, 2, 7, n // 2, n - 2, n - 1):
            for num in (2 * j + 1, 2 * j + 2):  # (j + 1/2) r / n and (j + 1) r / n
                k0 = -((-num * C.r) // (2 * n))
                out += [k for k in (k0 - 1, k0, k0 + 1) if 0 <= k < C.r]
    return out


def check(C, k):
    d = params(C)
    k1, k2 = split(C, k)
    assert (k1 + d["lam"] * k2 - k) % C.r == 0, k
    assert k1 & 1 and k2 & 1, k
    assert abs(k1) <= (1 << HALF_BITS) - 1 and abs(k2) <= (1 << HALF_BITS) - 1, k
    for v in (k1, k2):
        p = recode_half(v)
        assert sum((1 if (p >> w) & 1 else -1) << w for w in range(HALF_BITS)) == v, k
    return k1, k2


@pytest.mark.parametrize("C", CURVES, ids=lambda C: C.name)
def test_basis_and_endomorphism(C):
    d = params(C)
    (a1, b1), (a2, b2) = d["basis"]
    assert (d["lam"] ** 2 + d["lam"] + 1) % C.r == 0 and pow(d["beta"], 3, C.p) == 1 and d["beta"] != 1
    assert abs(d["det"]) == C.r and d["det"] == a1 * b2 - a2 * b1
    for a, b in d["basis"]:
        assert (a + b * d["lam"]) % C.r == 0
    assert b2 * d["det"] >= 0 and -b1 * d["det"] >= 0  # x1, x2 >= 0
    # phi = [lambda] on a point that is not the generator
    P = K.scalar_mul(C, (C.gx, C.gy), 0xC0FFEE)
    assert K.scalar_mul(C, P, d["lam"]) == (d["beta"] * P[0] % C.p, P[1])
    bits = sorted(v.bit_length() for v in (a1, b1, a2, b2))
    assert bits == ([64, 64, 127, 127] if C.name == "BN254" else [1, 1, 128, 128])


@pytest.mark.parametrize("C", CURVES, ids=lambda C: C.name)
def test_bound_from_the_basis_and_the_parity_rule(C):
    """|k_i| <= 2^128 - 1 for every k < r: e_i in (-1, 1 + eps) by the floor's error and the parity rule's choice
    between f_i and f_i + 1, so |k_i| < (1 + eps) (sum of the basis' entries in coordinate i) <= 2^128"""
    d = params(C)
    for n, g in zip(d["n"], d["g"]):
        # 0 <= 2^SHIFT n / r - g < 1: the computed floor is at most eps below x_i
        assert 0 <= Fraction(n << SHIFT, C.r) - g < 1
    # the parity rule: c = basis^-1 (k + 1, 1) mod 2 makes both halves odd for either parity of k
    (a1, b1), (a2, b2) = d["basis"]
    for kp in (0, 1):
        c1, c2 = (b2 * (kp + 1) + a2) & 1, (b1 * (kp + 1) + a1) & 1
        assert (kp - c1 * a1 - c2 * a2) & 1 and (-c1 * b1 - c2 * b2) & 1
    B1, B2 = proved_bound(C)
    assert B1 <= 1 << HALF_BITS and B2 <= 1 << HALF_BITS
    # the figures DESIGN.md states (units of 2^127)
    worst = max(B1, B2) / (1 << 127)
    assert (C.name == "BN254" and 0.76 < worst < 0.77) or (C.name == "BLS12381" and 1.34 < worst < 1.35)


@pytest.mark.parametrize("C", CURVES, ids=lambda C: C.name)
def test_split_edges_and_boundaries(C):
    for k in edge_scalars(C) + boundary_scalars(C) + [C.r, C.r + 5, (1 << 256) - 1]:
        check(C, k)
    k1, k2 = split(C, 0)  # an odd pair that sums to 0 mod r
    assert (k1 + params(C)["lam"] * k2) % C.r == 0 and k1 & 1 and k2 & 1


@pytest.mark.parametrize("C", CURVES, ids=lambda C: C.name)
def test_split_random(C):
    B1, B2 = proved_bound(C)
    m1 = m2 = 0
    for k in K.random_scalars(C, 100000, seed=0x61C7):
        k1, k2 = check(C, k)
        m1, m2 = max(m1, abs(k1)), max(m2, abs(k2))
    assert m1 < B1 and m2 < B2


@pytest.mark.parametrize("C", CURVES, ids=lambda C: C.name)
def test_planes_sum_to_the_scalar(C):
    """sum over the 256 planes with phi standing in as lambda gives k back"""
    lam = params(C)["lam"]
    for k in edge_scalars(C) + K.random_scalars(C, 64, seed=5):
        p = planes(C, k)
        s = [sum((1 if (p >> (HALF_BITS * h + w)) & 1 else -1) << w for w in range(HALF_BITS)) for h in (0, 1)]
        assert (s[0] + lam * s[1] - k) % C.r == 0


def header_struct(name):
    text = open(HEADER).read()
    body = re.search(r"struct %sGlv \{(.*?)\n\};" % name, text, re.S).group(1)
    out = {}
    for m in re.finditer(r"static constexpr (?:uint32_t|int) (\w+)((?:\[\d+\])*) = (.*?);", body):
        words = [int(w.rstrip("u"), 0) for w in re.findall(r"0x[0-9a-f]+u?|\b\d+u?\b", m.group(3))]
        out[m.group(1)] = words
    return out


@pytest.mark.parametrize("C", CURVES, ids=lambda C: C.name)
def test_header_constants_are_the_models(C):
    d = params(C)
    h = header_struct(C.name)
    L = 9 if C.name == "BN254" else 14

    def w32(v, n):
        return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]

    beta_m = d["beta"] * (1 << (29 * L)) % C.p
    assert h["BETA29"] == [(beta_m >> (29 * i)) & ((1 << 29) - 1) for i in range(L)]
    assert h["LAMBDA"] == w32(d["lam"], 8)
    assert h["SHIFT"] == [SHIFT]
    assert h["G"] == w32(d["g"][0], 6) + w32(d["g"][1], 6)
    (a1, b1), (a2, b2) = d["basis"]
    assert h["NEG"] == sum((w32((-v) % (1 << 160), 5) for v in (a1, a2, b1, b2)), [])
    assert h["PAR"] == [(b2 & 1) | ((a2 & 1) << 1) | ((b1 & 1) << 2) | ((a1 & 1) << 3)]
    if C.name == "BLS12381":  # the subgroup test's beta and the split's are one constant
        g1 = re.search(r"struct BLS12381G1 \{(.*?)\n\};", open(HEADER).read(), re.S).group(1)
        sub = re.search(r"BETA29\[14\] = \{(.*?)\}", g1).group(1)
        assert [int(w.rstrip("u"), 16) for w in sub.split(", ")] == h["BETA29"]
