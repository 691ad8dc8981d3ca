"""CPU: the constants of the G1 prime-order subgroup test (csrc/gen_consts.py ->
curve_consts.h, read by csrc/subgroup.hip) and the criterion itself.

The device test on BLS12-381 is  P != O and [x^2]P = (beta x, -y).  Checked here
with the Python oracle only: beta is the cube root whose endomorphism acts as
-x^2 on the subgroup, |x| has the six stated bits, and the criterion agrees with
the definitional [r]P = O (K._jac_mul_raw: K.scalar_mul reduces k mod r and
cannot serve) on members and on points of every small prime order dividing the
cofactor.  The vector builders below are shared with tests/test_gpu_subgroup.py."""
import functools
import os
import sys

import kzg_ref as K
import pairing_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kzg-commitments_amd", "csrc"))

BLS = K.BLS12381
G1_COFACTOR_PRIMES = (3, 11, 10177, 859267, 52437899)  # (x - 1)^2 / 3 = 3 * 11^2 * 10177^2 * 859267^2 * 52437899^2


# ---- oracle-side helpers --------------------------------------------------------
def g1_raw_mul(C, P, k):
    """[k]P with no reduction of k (None = infinity)"""
    return K.to_affine(C, K._jac_mul_raw(C, P, k)) if P is not None and k else None


def g1_member(C, P):
    """the definitional test: [r]P = O"""
    return P is None or K.to_affine(C, K._jac_mul_raw(C, P, C.r)) is None


def g1_curve_point(C, seed):
    """a curve point from x = seed, seed + 1, ... by a square root (p = 3 mod 4 on both curves);
    not cofactor-cleared"""
    assert C.p % 4 == 3
    x = seed
    while True:
        rhs = (x * x * x + C.b) % C.p
        y = pow(rhs, (C.p + 1) // 4, C.p)
        if y * y % C.p == rhs:
            return (x, y)
        x += 1


def _prime_order_point(order, ell, mul, seeds):
    """a point of exact order ell in a group of the given order: [order / ell^e]R multiplied up"""
    e, co = 0, order
    while co % ell == 0:
        co //= ell
        e += 1
    assert e >= 1
    for R in seeds:
        T = mul(R, co)
        if T is None:
            continue
        while True:
            nxt = mul(T, ell)
            if nxt is None:
                break
            T = nxt
        assert mul(T, ell) is None and T is not None  # exact order ell (ell prime)
        return T
    raise AssertionError("no point of order %d found" % ell)


@functools.lru_cache(maxsize=None)
def g1_order_point(ell):
    """T_ell on BLS12-381 G1, exact order ell"""
    C = BLS
    n = C.r * ((K._BLS_X - 1) ** 2 // 3)  # #E(Fp)
    seeds = (g1_curve_point(C, 1000 * ell + 7 * j) for j in range(1, 64))
    T = _prime_order_point(n, ell, lambda P, k: g1_raw_mul(C, P, k), seeds)
    assert K.on_curve(C, T)
    return T


@functools.lru_cache(maxsize=None)
def g2_order13_point(name):
    """T_13 on the twist of either curve, exact order 13"""
    C = K.CURVES[name]
    T = PR.twist(C)
    assert T.h2 % 13 == 0

    def seeds():
        k = 2
        while True:
            Q = g2_raw_point(C, k)
            k = Q[0][0] + 1
            yield Q

    P13 = _prime_order_point(T.order, 13, lambda Q, k: PR.g2_mul_raw(C, Q, k), seeds())
    assert PR.g2_on_curve(C, P13)
    return P13


def g2_raw_point(C, k):
    """a twist point with x = k' + i, k' >= k the first that has a square root; not cofactor-cleared"""
    p, b2 = C.p, PR.twist(C).b2
    while True:
        x = (k % p, 1)
        y = PR.f2sqrt(p, PR.f2add(p, PR.f2mul(p, PR.f2mul(p, x, x), x), b2))
        if y is not None:
            return (x, y)
        k += 1


def g2_member(C, Q):
    return Q is None or PR.g2_mul_raw(C, Q, C.r) is None


def bls_g1_vectors():
    """[(label, point, member)] on BLS12-381: members, a raw curve point, T_ell and [777]G + T_ell"""
    C = BLS
    G = (C.gx, C.gy)
    out = [("G", G, True), ("[2]G", K.scalar_mul(C, G, 2), True), ("[r-1]G", K.scalar_mul(C, G, C.r - 1), True)]
    raw = g1_curve_point(C, 424242)
    out.append(("raw curve point", raw, g1_member(C, raw)))
    g777 = K.scalar_mul(C, G, 777)
    for ell in G1_COFACTOR_PRIMES:
        T = g1_order_point(ell)
        out.append(("T_%d" % ell, T, False))
        out.append(("[777]G + T_%d" % ell, K.point_add(C, g777, T), False))
    return out


def fast_criterion(beta, P):
    """P != O and [x^2]P == (beta x, -y)"""
    C = BLS
    if P is None:
        return False
    x2 = K._BLS_X ** 2
    return g1_raw_mul(C, P, x2) == (beta * P[0] % C.p, (-P[1]) % C.p)


# ---- tests ---------------------------------------------------------------------------
def test_emitted_beta_is_the_minus_x2_root():
    import gen_consts as g
    C = BLS
    beta = g.BLS_BETA
    assert pow(beta, 3, C.p) == 1 and beta != 1
    G = (C.gx, C.gy)
    assert (beta * C.gx % C.p, C.gy) == K.scalar_mul(C, G, (-K._BLS_X ** 2) % C.r)
    # the value the header carries: radix-2^29 Montgomery limbs of beta
    assert g.BLS_X2 == K._BLS_X ** 2 and g.BLS_X2.bit_length() == 128 and bin(g.BLS_X2).count("1") == 17
    with open(os.path.join(ROOT, "kzg-commitments_amd", "csrc", "curve_consts.h")) as f:
        text = f.read()
    assert "BETA29[14] = %s;" % g.arr29(g.mont29(beta, C.p, 14), 14) in text
    assert "X2[2] = {0x%016xull, 0x%016xull};" % (g.BLS_X2 & (2**64 - 1), g.BLS_X2 >> 64) in text


def test_bn254_g1_has_cofactor_one():
    import gen_consts as g
    assert g.BN_P + 1 - (6 * g.U * g.U + 1) == g.BN_R == K.BN254.r


def test_x_has_the_six_bits():
    import gen_consts as g
    assert g.X == K._BLS_X < 0
    assert [b for b in range(64) if (abs(g.X) >> b) & 1] == [16, 48, 57, 60, 62, 63]
    assert abs(g.X).bit_length() == 64


def test_cofactor_factorisation():
    h = (K._BLS_X - 1) ** 2 // 3
    f = 3
    for ell in G1_COFACTOR_PRIMES[1:]:
        f *= ell * ell
    assert f == h
    assert BLS.r * h == BLS.p + 1 - (K._BLS_X + 1)  # #E(Fp) = p + 1 - t, t = x + 1, odd


def test_fast_criterion_agrees_with_the_definition():
    import gen_consts as g
    C = BLS
    vecs = bls_g1_vectors()
    assert sum(1 for _, _, m in vecs if m) == 3 and len(vecs) == 14
    for label, P, member in vecs:
        assert K.on_curve(C, P), label
        assert g1_member(C, P) == member, label
        assert fast_criterion(g.BLS_BETA, P) == member, label
    # the other cube root (eigenvalue x^2 - 1) fails on members: the choice matters
    other = g.BLS_BETA * g.BLS_BETA % C.p
    assert not fast_criterion(other, (C.gx, C.gy))


def test_order_points_have_exact_order():
    C = BLS
    for ell in G1_COFACTOR_PRIMES:
        T = g1_order_point(ell)
        assert T is not None and g1_raw_mul(C, T, ell) is None
    T3 = g1_order_point(3)
    assert g1_raw_mul(C, T3, 2) == K.point_neg(C, T3)  # [2]T = -T: the addition's equal-x branch
