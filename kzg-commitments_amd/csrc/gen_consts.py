#!/usr/bin/env python3
"""Generate curve_consts.h: Montgomery constants for the device field code.

Curves: miracl-core BN254 (Nogami; config/curve_BN254/kzg_config.h) and
BLS12-381 (config/curve_BLS12381/kzg_config.h).  p and r are re-derived from
the curve parameters (u / x) rather than typed in, and the generators are
checked on the curve.  Limbs are 32-bit little-endian (device word size)."""
import os

U = -(2**62 + 2**55 + 1)
BN_P = 36 * U**4 + 36 * U**3 + 24 * U**2 + 6 * U + 1
BN_R = 36 * U**4 + 36 * U**3 + 18 * U**2 + 6 * U + 1
X = -0xD201000000010000
BLS_P = (X - 1) ** 2 * (X**4 - X**2 + 1) // 3 + X
BLS_R = X**4 - X**2 + 1
BLS_GX = 0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB
BLS_GY = 0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1

assert (1 - ((BN_P - 1) ** 3 + 2)) % BN_P == 0
assert (BLS_GY**2 - BLS_GX**3 - 4) % BLS_P == 0


# --------------------------------------------------------------------------
# Prime-order subgroup test on G1 (subgroup.hip).  BN254 (Nogami): #E(Fp) =
# p + 1 - t = r with t = 6u^2 + 1, cofactor 1, nothing to test.  BLS12-381:
# #E(Fp) = r (x - 1)^2 / 3; phi(x, y) = (beta x, y) with beta a primitive
# cube root of 1 in Fp acts on the order-r subgroup as a cube root of 1 mod r,
# -x^2 for one beta and x^2 - 1 for the other.  The device test wants the
# first: [x^2]P = -phi(P).
# --------------------------------------------------------------------------
assert BN_P + 1 - (6 * U * U + 1) == BN_R
assert (BLS_P + 1 - (X + 1)) == BLS_R * ((X - 1) ** 2 // 3)


def _g1_smul(p, P, k):
    """[k]P on y^2 = x^3 + b (a = 0), affine, None = infinity"""
    def add(A, B):
        if A is None:
            return B
        if B is None:
            return A
        if A[0] == B[0]:
            if (A[1] + B[1]) % p == 0:
                return None
            lam = 3 * A[0] * A[0] * pow(2 * A[1], -1, p) % p
        else:
            lam = (B[1] - A[1]) * pow(B[0] - A[0], -1, p) % p
        x3 = (lam * lam - A[0] - B[0]) % p
        return (x3, (lam * (A[0] - x3) - A[1]) % p)

    R = None
    for bit in bin(k)[2:]:
        R = add(R, R)
        if bit == "1":
            R = add(R, P)
    return R


def _bls_beta():
    g = 2
    while pow(g, (BLS_P - 1) // 3, BLS_P) == 1:
        g += 1
    b = pow(g, (BLS_P - 1) // 3, BLS_P)
    want = _g1_smul(BLS_P, (BLS_GX, BLS_GY), (-X * X) % BLS_R)
    roots = [c for c in (b, b * b % BLS_P) if (c * BLS_GX % BLS_P, BLS_GY) == want]
    assert len(roots) == 1
    return roots[0]


BLS_BETA = _bls_beta()
assert BLS_BETA != 1 and pow(BLS_BETA, 3, BLS_P) == 1
BLS_X2 = X * X  # the subgroup test's exponent: [x^2]P = (beta x, -y)
assert (BLS_X2 * BLS_X2 - BLS_X2 + 1) == BLS_R

# --------------------------------------------------------------------------
# Endomorphism split of the block-table MSM (msm_joint.hip, GLV).  Both curves
# have j = 0: phi(x, y) = (beta x, y) = [lambda]P on the order-r subgroup,
# beta^3 = 1 in Fp, lambda^3 = 1 mod r.  A scalar k < r is written
# k = k1 + lambda k2 (mod r) with both halves odd and |k1|, |k2| < 2^128:
#   * (v1, v2) = ((a1, b1), (a2, b2)) is the Euclid short basis of the lattice
#     {(a, b): a + b lambda = 0 mod r}, signs chosen so that the coordinates of
#     (k, 0) in it, x1 = k n1 / r and x2 = k n2 / r with n1 = |b2|, n2 = |b1|,
#     are not negative;
#   * f_i = floor(k g_i / 2^SHIFT), g_i = floor(2^SHIFT n_i / r): f_i <= x_i <
#     f_i + 1 + 2^(255 - SHIFT) for k < r < 2^255;
#   * c_i is the one of f_i, f_i + 1 whose parity makes both halves odd:
#     c1 = b2 (k + 1) + a2, c2 = b1 (k + 1) + a1 (mod 2), the inverse of the
#     basis mod 2 (its determinant +-r is odd) applied to (k + 1, 1);
#   * (k1, k2) = (k, 0) - c1 v1 - c2 v2 = e1 v1 + e2 v2 with |e_i| < 1 + 2^(255 -
#     SHIFT), so |k1| < (1 + 2^(255 - SHIFT)) (|a1| + |a2|) and likewise k2 with
#     the b's: asserted below to be at most 2^128.
# The device computes both halves mod 2^160 in two's complement: NEG[j] = the
# words of -a1, -a2, -b1, -b2 mod 2^160.
# --------------------------------------------------------------------------
GLV_SHIFT = 288


def _cube_roots(m):
    g = 2
    while pow(g, (m - 1) // 3, m) == 1:
        g += 1
    w = pow(g, (m - 1) // 3, m)
    return w, w * w % m


def glv_data(name):
    if name == "BN254":
        p, r, G = BN_P, BN_R, (BN_P - 1, 1)
        beta = min(_cube_roots(p))
        lams = [l for l in _cube_roots(r) if _g1_smul(p, G, l) == (beta * G[0] % p, G[1])]
        assert len(lams) == 1
        lam = lams[0]
    else:  # the subgroup test's beta: lambda = -x^2
        p, r, G = BLS_P, BLS_R, (BLS_GX, BLS_GY)
        beta, lam = BLS_BETA, (-BLS_X2) % BLS_R
        assert _g1_smul(p, G, lam) == (beta * G[0] % p, G[1])
    assert (lam * lam + lam + 1) % r == 0 and pow(beta, 3, p) == 1 and beta != 1
    # Euclid on (r, lambda): every remainder row (s, t) has s + (-t) lambda = 0 mod r
    rows = [(r, 0), (lam, 1)]
    while rows[-1][0] * rows[-1][0] >= r:
        q = rows[-2][0] // rows[-1][0]
        rows.append((rows[-2][0] - q * rows[-1][0], rows[-2][1] - q * rows[-1][1]))
    v1 = (rows[-1][0], -rows[-1][1])
    cand = [(rows[-2][0], -rows[-2][1])]
    q = rows[-2][0] // rows[-1][0]
    cand.append((rows[-2][0] - q * rows[-1][0], -(rows[-2][1] - q * rows[-1][1])))
    v2 = min(cand, key=lambda v: max(abs(v[0]), abs(v[1])))
    (a1, b1), (a2, b2) = v1, v2
    det = a1 * b2 - a2 * b1
    assert abs(det) == r
    if b2 * det < 0:  # x1 = k b2 / det
        a1, b1, det = -a1, -b1, -det
    if -b1 * det < 0:  # x2 = -k b1 / det
        a2, b2, det = -a2, -b2, -det
    assert b2 * det >= 0 and -b1 * det >= 0
    for a, b in ((a1, b1), (a2, b2)):
        assert (a + b * lam) % r == 0
    n1, n2 = abs(b2), abs(b1)
    g1, g2 = (n1 << GLV_SHIFT) // r, (n2 << GLV_SHIFT) // r
    assert r < 1 << 255 and max(g1, g2) < 1 << 192
    # |k_i| < (1 + 2^(255 - SHIFT)) (sum of the basis' entries in that coordinate) <= 2^128
    for s in (abs(a1) + abs(a2), abs(b1) + abs(b2)):
        assert s * ((1 << (GLV_SHIFT - 255)) + 1) <= 1 << (128 + GLV_SHIFT - 255)
    par = (b2 & 1) | ((a2 & 1) << 1) | ((b1 & 1) << 2) | ((a1 & 1) << 3)
    return dict(p=p, r=r, beta=beta, lam=lam, basis=((a1, b1), (a2, b2)), g=(g1, g2), par=par)


def glv_split(name, k, d=None):
    """the device's decomposition of k < r: (k1, k2), both odd, k1 + lambda k2 = k mod r"""
    d = d or glv_data(name)
    (a1, b1), (a2, b2) = d["basis"]
    c1, c2 = (k * d["g"][0]) >> GLV_SHIFT, (k * d["g"][1]) >> GLV_SHIFT
    c1 += (c1 ^ (b2 * (k + 1) + a2)) & 1
    c2 += (c2 ^ (b1 * (k + 1) + a1)) & 1
    return k - c1 * a1 - c2 * a2, -c1 * b1 - c2 * b2


def glv_struct(name, L):
    d = glv_data(name)
    (a1, b1), (a2, b2) = d["basis"]
    for k in (0, 1, 2, d["r"] - 1, d["lam"], d["r"] // 2):
        k1, k2 = glv_split(name, k, d)
        assert (k1 + d["lam"] * k2 - k) % d["r"] == 0 and k1 & 1 and k2 & 1 and max(abs(k1), abs(k2)) < 1 << 128
    neg = ", ".join(arr((-v) % (1 << 160), 5) for v in (a1, a2, b1, b2))
    return "\n".join([
        "// endomorphism split (msm_joint.hip): phi(x, y) = (BETA x, y) = [LAMBDA]P; k = k1 + LAMBDA k2 mod r",
        "struct %sGlv {" % name,
        "  static constexpr uint32_t BETA29[%d] = %s;  // radix-2^29 Montgomery" % (L, arr29(mont29(d["beta"], d["p"], L), L)),
        "  static constexpr uint32_t LAMBDA[8] = %s;  // canonical" % arr(d["lam"], 8),
        "  static constexpr int SHIFT = %d;  // f_i = floor(k G[i] / 2^SHIFT)" % GLV_SHIFT,
        "  static constexpr uint32_t G[2][6] = {%s, %s};  // floor(2^SHIFT |b2| / r), floor(2^SHIFT |b1| / r)" % (
            arr(d["g"][0], 6), arr(d["g"][1], 6)),
        "  static constexpr uint32_t NEG[4][5] = {%s};  // -a1, -a2, -b1, -b2 mod 2^160" % neg,
        "  static constexpr uint32_t PAR = %du;  // parities: bit 0 b2, bit 1 a2, bit 2 b1, bit 3 a1" % d["par"],
        "};",
    ])


# --------------------------------------------------------------------------
# Compressed points (codec.hip).  Both primes are 3 mod 4, so a square a of Fp
# has the root a^((p + 1) / 4); a is a square iff that power squares back to a.
# In Fp2 = Fp[i] (p = 3 mod 4, complex method): a1 = a^((p - 3) / 4),
# alpha = a1^2 a, x0 = a1 a; the root is i x0 when alpha = -1 and
# (1 + alpha)^((p - 1) / 2) x0 otherwise.  (p - 1) / 2 is also the boundary of
# the lexicographic sign: y is "large" when y > (p - 1) / 2.
# --------------------------------------------------------------------------
assert BN_P % 4 == 3 and BLS_P % 4 == 3


def sqrt_consts(p, n):
    return [
        "  // compressed points: the Fp root's exponent, the sign boundary, the Fp2 root's first exponent",
        "  static constexpr uint32_t SQRT_EXP[%d] = %s;  // (p + 1) / 4" % (n, arr((p + 1) // 4, n)),
        "  static constexpr uint32_t HALF[%d] = %s;  // (p - 1) / 2" % (n, arr((p - 1) // 2, n)),
        "  static constexpr uint32_t SQRT2_EXP[%d] = %s;  // (p - 3) / 4" % (n, arr((p - 3) // 4, n)),
    ]


def limbs(v, n):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def arr(v, n):
    return "{" + ", ".join("0x%08xu" % w for w in limbs(v, n)) + "}"


def field(name, m, n):
    R = 1 << (32 * n)
    inv = (-pow(m, -1, 1 << 32)) % (1 << 32)
    lines = [
        "struct %s {" % name,
        "  static constexpr int N = %d;" % n,
        "  static constexpr int BITS = %d;" % m.bit_length(),
        "  static constexpr uint32_t INV = 0x%08xu;  // -m^-1 mod 2^32" % inv,
        "  static constexpr uint32_t P[N] = %s;" % arr(m, n),
        "  static constexpr uint32_t P2[N] = %s;  // 2m" % arr(2 * m, n),
        "  static constexpr uint32_t R2[N] = %s;  // R^2 mod m" % arr(R * R % m, n),
        "  static constexpr uint32_t ONE[N] = %s;  // R mod m" % arr(R % m, n),
        "  static constexpr uint32_t PM2[N] = %s;  // m - 2 (Fermat exponent)" % arr(m - 2, n),
        "};",
    ]
    return "\n".join(lines)


def limbs29(v, n):
    return [(v >> (29 * i)) & ((1 << 29) - 1) for i in range(n)]


def arr29(v, n):
    assert v < (1 << (29 * n))
    return "{" + ", ".join("0x%08xu" % w for w in limbs29(v, n)) + "}"


def field29(name, m, L):
    """radix-2^29 Montgomery constants (R = 2^(29 L)) for field29.hpp"""
    R = 1 << (29 * L)
    assert R >= 64 * m, "lazy-reduction headroom"
    inv = (-pow(m, -1, 1 << 29)) % (1 << 29)
    lines = [
        "struct %s {" % name,
        "  static constexpr int L = %d;  // 29-bit limbs" % L,
        "  static constexpr uint32_t INV = 0x%08xu;  // -m^-1 mod 2^29" % inv,
        "  static constexpr uint32_t P[L] = %s;" % arr29(m, L),
    ]
    for k in (2, 4, 6, 8, 10, 16):
        lines.append("  static constexpr uint32_t P%d[L] = %s;  // %dm" % (k, arr29(k * m, L), k))
    # 2m with every limb borrowed up into [2^29 - 1, 2^30): K - a needs no
    # carry for any a < m with normalized limbs (lazy negation, field29.hpp)
    t = limbs29(2 * m, L)
    b = [t[0] + (1 << 29)] + [t[i] + (1 << 29) - 1 for i in range(1, L - 1)] + [t[L - 1] - 1]
    assert sum(v << (29 * i) for i, v in enumerate(b)) == 2 * m and all(v < (1 << 30) for v in b)
    assert b[L - 1] >= (m - 1) >> (29 * (L - 1)) and all(v >= (1 << 29) - 1 for v in b[:L - 1])
    lines.append("  static constexpr uint32_t P2B[L] = {%s};  // 2m, limbs borrowed into [2^29-1, 2^30)" %
                 ", ".join("0x%08xu" % v for v in b))
    t = limbs29(8 * m, L)
    b = [t[0] + (1 << 29)] + [t[i] + (1 << 29) - 1 for i in range(1, L - 1)] + [t[L - 1] - 1]
    assert sum(v << (29 * i) for i, v in enumerate(b)) == 8 * m and all(v < (1 << 30) for v in b)
    # limb-wise >= every normalized a < 4m: middle limbs >= 2^29 - 1, top limb
    # >= the top limb of 4m - 1 >= a's top limb
    assert b[L - 1] >= (4 * m - 1) >> (29 * (L - 1)) and all(v >= (1 << 29) - 1 for v in b[:L - 1])
    lines.append("  static constexpr uint32_t P8B[L] = {%s};  // 8m, limbs borrowed into [2^29-1, 2^30)" %
                 ", ".join("0x%08xu" % v for v in b))
    lines += [
        "  static constexpr uint32_t R2[L] = %s;  // R^2 mod m" % arr29(R * R % m, L),
        "  static constexpr uint32_t R3[L] = %s;  // R^3 mod m" % arr29(R * R * R % m, L),
        "  static constexpr uint32_t ONE[L] = %s;  // R mod m" % arr29(R % m, L),
        "  // low limb of k m, k = 0..3 (zero filter for values < 4m)",
        "  static constexpr uint32_t LOW[4] = {0u, 0x%08xu, 0x%08xu, 0x%08xu};" % tuple(
            (k * m) & ((1 << 29) - 1) for k in (1, 2, 3)),
        "};",
    ]
    return "\n".join(lines)


def mont(v, m, n):
    return v * (1 << (32 * n)) % m


def mont29(v, m, L):
    return v * (1 << (29 * L)) % m


# --------------------------------------------------------------------------
# Radix-2 NTT domains of the scalar fields (ntt.hip).  r - 1 = 2^s * odd; the
# size-2^k domain (k <= s) is generated by g^((r - 1) / 2^k) for a quadratic
# non-residue g, so the root has order exactly 2^k.  BLS12-381: s = 32, g = 7;
# BN254 (Nogami): s = 2, g = 2.
# --------------------------------------------------------------------------
def two_adicity(r):
    s = 0
    while (r - 1) >> s & 1 == 0:
        s += 1
    return s


NTT_GEN = {"BN254": 2, "BLS12381": 7}


def domain_root(name, k):
    r = BN_R if name == "BN254" else BLS_R
    assert k <= two_adicity(r)
    return pow(NTT_GEN[name], (r - 1) >> k, r)


assert two_adicity(BLS_R) == 32 and two_adicity(BN_R) == 2
assert all(pow(NTT_GEN[n], (r - 1) // 2, r) == r - 1 for n, r in (("BN254", BN_R), ("BLS12381", BLS_R)))
assert domain_root("BLS12381", 32) == 0x16A2A19EDFE81F20D09B681922C813B4B63683508C2280B93829971F439F0D2B
assert domain_root("BN254", 2) == 0x9366C4800000000555150000000000122400000000000015
assert domain_root("BN254", 1) == BN_R - 1


def ntt_struct(name):
    """domain roots w_k (canonical and Montgomery) and 2^-k (Montgomery), k = 0..2-adicity"""
    r = BN_R if name == "BN254" else BLS_R
    s = two_adicity(r)

    def rows(vals):
        return "{\n" + ",\n".join("      " + arr(v, 8) for v in vals) + "}"

    roots = [domain_root(name, k) for k in range(s + 1)]
    return "\n".join([
        "struct %sFrNtt {" % name,
        "  static constexpr int TWO_ADICITY = %d;  // r - 1 = 2^TWO_ADICITY * odd" % s,
        "  // w_k = %d^((r - 1) / 2^k), of order exactly 2^k; canonical" % NTT_GEN[name],
        "  static constexpr uint32_t ROOT[%d][8] = %s;" % (s + 1, rows(roots)),
        "  // the same in Montgomery form (the device twiddle table is built from these)",
        "  static constexpr uint32_t ROOT_M[%d][8] = %s;" % (s + 1, rows(mont(v, r, 8) for v in roots)),
        "  // 2^-k in Montgomery form (the inverse transform's scale)",
        "  static constexpr uint32_t NINV_M[%d][8] = %s;" % (s + 1, rows(mont(pow(1 << k, -1, r), r, 8) for k in range(s + 1))),
        "};",
    ])


# --------------------------------------------------------------------------
# G2 / pairing constants (verify path: trusted_setup.cpp:123-135, 176-201,
# 230-254).  Fp2 = Fp[i]/(i^2+1), xi = 1 + i, Fp6 = Fp2[v]/(v^3 - xi),
# Fp12 = Fp6[w]/(w^2 - v).  The twist type is selected by group order: the
# sextic twist whose order is divisible by r (BN254: D-type y^2 = x^3 + b/xi,
# BLS12-381: M-type y^2 = x^3 + b xi).
# --------------------------------------------------------------------------
def _f2mul(p, a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % p, (a[0] * b[1] + a[1] * b[0]) % p)


def _f2pow(p, a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = _f2mul(p, r, a)
        a = _f2mul(p, a, a)
        e >>= 1
    return r


def _f2inv(p, a):
    ni = pow((a[0] * a[0] + a[1] * a[1]) % p, -1, p)
    return (a[0] * ni % p, (-a[1]) * ni % p)


def _f2add(p, a, b):
    return ((a[0] + b[0]) % p, (a[1] + b[1]) % p)


def _f2sqrt(p, a):
    a1 = _f2pow(p, a, (p - 3) // 4)
    alpha = _f2mul(p, _f2mul(p, a1, a1), a)
    if _f2mul(p, _f2pow(p, alpha, p), alpha) == (p - 1, 0):
        return None
    x0 = _f2mul(p, a1, a)
    if alpha == (p - 1, 0):
        return _f2mul(p, (0, 1), x0)
    return _f2mul(p, _f2pow(p, _f2add(p, (1, 0), alpha), (p - 1) // 2), x0)


def _twist(p, r, b, trace):
    import math
    t2 = trace * trace - 2 * p
    f = math.isqrt((4 * p * p - t2 * t2) // 3)
    orders = {p * p + 1 - (s1 * 3 * f + s2 * t2) // 2 for s1 in (1, -1) for s2 in (1, -1)}
    orders = [n for n in orders if n % r == 0]
    assert len(orders) == 1
    return orders[0]


def _g2_smul(p, Q, k):
    def add(P, Q):
        if P is None:
            return Q
        if Q is None:
            return P
        if P[0] == Q[0]:
            if _f2add(p, P[1], Q[1]) == (0, 0):
                return None
            lam = _f2mul(p, _f2mul(p, (3, 0), _f2mul(p, P[0], P[0])), _f2inv(p, _f2mul(p, (2, 0), P[1])))
        else:
            lam = _f2mul(p, ((Q[1][0] - P[1][0]) % p, (Q[1][1] - P[1][1]) % p),
                         _f2inv(p, ((Q[0][0] - P[0][0]) % p, (Q[0][1] - P[0][1]) % p)))
        l2 = _f2mul(p, lam, lam)
        x3 = ((l2[0] - P[0][0] - Q[0][0]) % p, (l2[1] - P[0][1] - Q[0][1]) % p)
        t = _f2mul(p, lam, ((P[0][0] - x3[0]) % p, (P[0][1] - x3[1]) % p))
        return (x3, ((t[0] - P[1][0]) % p, (t[1] - P[1][1]) % p))

    R = None
    for bit in bin(k)[2:]:
        R = add(R, R)
        if bit == "1":
            R = add(R, Q)
    return R


BLS_G2 = ((0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
           0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E),
          (0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
           0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE))


def g2_data(name):
    """twist, G2 generator, Frobenius constants, loop and hard-part digits"""
    if name == "BN254":
        p, r, b, trace = BN_P, BN_R, 2, 6 * U * U + 1
    else:
        p, r, b, trace = BLS_P, BLS_R, 4, X + 1
    order = _twist(p, r, b, trace)
    xi = (1, 1)
    d_type = name == "BN254"
    b2 = _f2mul(p, (b, 0), _f2inv(p, xi)) if d_type else _f2mul(p, (b, 0), xi)
    if name == "BLS12381":
        gen = BLS_G2
    else:  # deterministic: first x = k + i on the twist, smaller root, cofactor cleared
        k = 1
        while True:
            x = (k, 1)
            y = _f2sqrt(p, _f2add(p, _f2mul(p, _f2mul(p, x, x), x), b2))
            if y is not None:
                ny = ((-y[0]) % p, (-y[1]) % p)
                if (ny[1], ny[0]) < (y[1], y[0]):
                    y = ny
                gen = _g2_smul(p, (x, y), order // r)
                if gen is not None:
                    break
            k += 1
    assert _g2_smul(p, gen, r) is None
    frob = [_f2pow(p, xi, kk * (p - 1) // 6) for kk in range(6)]
    twx = _f2pow(p, xi, (p - 1) // 3)
    twy = _f2pow(p, xi, (p - 1) // 2)
    loop = 6 * U + 2 if name == "BN254" else X
    hard = (p ** 4 - p ** 2 + 1) // r
    digits = []
    for _ in range(4):
        digits.append(hard % p)
        hard //= p
    assert hard == 0
    z = U if name == "BN254" else X
    k3 = (X - 1) ** 2 // 3 if name == "BLS12381" else 0
    return dict(p=p, b2=b2, gen=gen, frob=frob, twx=twx, twy=twy, loop=loop, digits=digits, d_type=d_type, z=z, k3=k3)


def pairing_struct(name, L, nw):
    d = g2_data(name)
    p = d["p"]

    def m29(v):
        return arr29(mont29(v, p, L), L)

    def f2(a):
        return "{%s, %s}" % (m29(a[0]), m29(a[1]))

    lines = [
        "struct %sPair {" % name,
        "  static constexpr bool D_TWIST = %s;  // D: y^2 = x^3 + b/xi, M: y^2 = x^3 + b xi" % (
            "true" if d["d_type"] else "false"),
        "  static constexpr uint32_t B2[2][%d] = %s;  // twist b' (radix-2^29 Montgomery)" % (L, f2(d["b2"])),
        "  static constexpr uint32_t G2X[2][%d] = %s;" % (L, f2(d["gen"][0])),
        "  static constexpr uint32_t G2Y[2][%d] = %s;" % (L, f2(d["gen"][1])),
        "  // Fp12 Frobenius: coefficient of w^k picks up xi^(k (p-1)/6)",
        "  static constexpr uint32_t FROB[6][2][%d] = {%s};" % (L, ", ".join(f2(g) for g in d["frob"])),
        "  // twist Frobenius (D-type): x -> conj(x) xi^((p-1)/3), y -> conj(y) xi^((p-1)/2)",
        "  static constexpr uint32_t TWX[2][%d] = %s;" % (L, f2(d["twx"])),
        "  static constexpr uint32_t TWY[2][%d] = %s;" % (L, f2(d["twy"])),
        "  // Miller loop count |%s| (LOOP_BITS bits, two 64-bit words)" % ("6u+2" if name == "BN254" else "x"),
        "  static constexpr uint64_t LOOP[2] = {0x%016xull, 0x%016xull};" % (abs(d["loop"]) & (2**64 - 1), abs(d["loop"]) >> 64),
        "  static constexpr int LOOP_BITS = %d;" % abs(d["loop"]).bit_length(),
        "  static constexpr bool LOOP_NEG = %s;" % ("true" if d["loop"] < 0 else "false"),
        "  static constexpr int NW = %d;" % nw,
        "  // (p^4 - p^2 + 1)/r = sum_i HARD[i] p^i (canonical words)",
        "  static constexpr uint32_t HARD[4][%d] = {%s};" % (nw, ", ".join(arr(v, nw) for v in d["digits"])),
        "  static constexpr int HARD_BITS = %d;" % max(v.bit_length() for v in d["digits"]),
        "  // curve parameter z (BN: u, BLS: x) for the hard part of the final exponentiation",
        "  static constexpr bool IS_BN = %s;" % ("true" if name == "BN254" else "false"),
        "  static constexpr uint64_t Z_ABS = 0x%016xull;" % abs(d["z"]),
        "  static constexpr bool Z_NEG = %s;" % ("true" if d["z"] < 0 else "false"),
        "  // BLS12: (p^4 - p^2 + 1)/r = K3 (x + p)(x^2 + p^2 - 1) + 1, K3 = (x - 1)^2 / 3",
        "  static constexpr uint64_t K3[2] = {0x%016xull, 0x%016xull};" % (d["k3"] & (2**64 - 1), d["k3"] >> 64),
        "  static constexpr int K3_BITS = %d;" % d["k3"].bit_length(),
        "};",
    ]
    return "\n".join(lines)


def main():
    out = [
        "// GENERATED by gen_consts.py -- do not edit.",
        "#pragma once",
        "#include <stdint.h>",
        "namespace kzgx {",
        field("BN254Fp", BN_P, 8),
        field("BN254Fr", BN_R, 8),
        field("BLS12381Fp", BLS_P, 12),
        field("BLS12381Fr", BLS_R, 8),
        field29("BN254Fp29", BN_P, 9),
        field29("BLS12381Fp29", BLS_P, 14),
        # the scalar fields in radix 2^29: their inversion by f29_inv_uniform
        # (poly.hip fe_inv_wave, the interpolation weights)
        field29("BN254Fr29", BN_R, 9),
        field29("BLS12381Fr29", BLS_R, 9),
        glv_struct("BN254", 9),
        glv_struct("BLS12381", 14),
        "struct BN254G1 {",
        "  using Glv = BN254Glv;",
        "  using Fp = BN254Fp;",
        "  using Fp29 = BN254Fp29;",
        "  using Fr = BN254Fr;",
        "  static constexpr int ID = 0;",
        "  static constexpr uint32_t BSMALL = 2;  // y^2 = x^3 + 2",
        "  static constexpr int SCALAR_BITS = %d;" % BN_R.bit_length(),
        "  static constexpr uint32_t GX[8] = %s;  // Montgomery" % arr(mont(BN_P - 1, BN_P, 8), 8),
        "  static constexpr uint32_t GY[8] = %s;" % arr(mont(1, BN_P, 8), 8),
        "  static constexpr uint32_t B[8] = %s;" % arr(mont(2, BN_P, 8), 8),
        "  static constexpr uint32_t GX29[9] = %s;  // radix-2^29 Montgomery" % arr29(mont29(BN_P - 1, BN_P, 9), 9),
        "  static constexpr uint32_t GY29[9] = %s;" % arr29(mont29(1, BN_P, 9), 9),
        "  static constexpr bool COFACTOR_ONE = true;  // #E(Fp) = r: on the curve is in the subgroup",
        *sqrt_consts(BN_P, 8),
        "};",
        "struct BLS12381G1 {",
        "  using Glv = BLS12381Glv;",
        "  using Fp = BLS12381Fp;",
        "  using Fp29 = BLS12381Fp29;",
        "  using Fr = BLS12381Fr;",
        "  static constexpr int ID = 1;",
        "  static constexpr uint32_t BSMALL = 4;  // y^2 = x^3 + 4",
        "  static constexpr int SCALAR_BITS = %d;" % BLS_R.bit_length(),
        "  static constexpr uint32_t GX[12] = %s;" % arr(mont(BLS_GX, BLS_P, 12), 12),
        "  static constexpr uint32_t GY[12] = %s;" % arr(mont(BLS_GY, BLS_P, 12), 12),
        "  static constexpr uint32_t B[12] = %s;" % arr(mont(4, BLS_P, 12), 12),
        "  static constexpr uint32_t GX29[14] = %s;" % arr29(mont29(BLS_GX, BLS_P, 14), 14),
        "  static constexpr uint32_t GY29[14] = %s;" % arr29(mont29(BLS_GY, BLS_P, 14), 14),
        "  static constexpr bool COFACTOR_ONE = false;  // #E(Fp) = r (x - 1)^2 / 3",
        "  // subgroup test [x^2]P = (beta x, -y): beta^3 = 1, (beta x, y) = [-x^2]P on the order-r subgroup",
        "  static constexpr uint32_t BETA29[14] = %s;  // radix-2^29 Montgomery" % arr29(mont29(BLS_BETA, BLS_P, 14), 14),
        "  static constexpr uint64_t X2[2] = {0x%016xull, 0x%016xull};  // x^2" % (BLS_X2 & (2**64 - 1), BLS_X2 >> 64),
        "  static constexpr int X2_BITS = %d;" % BLS_X2.bit_length(),
        *sqrt_consts(BLS_P, 12),
        "};",
        pairing_struct("BN254", 9, 8),
        pairing_struct("BLS12381", 14, 12),
        ntt_struct("BN254"),
        ntt_struct("BLS12381"),
        "}  // namespace kzgx",
        "",
    ]
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "curve_consts.h")
    text = "\n".join(out)
    # unchanged constants leave the header (and its mtime) alone: every object
    # includes it, so a rewrite would make build() recompile everything
    if os.path.exists(path):
        with open(path) as f:
            if f.read() == text:
                return
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
