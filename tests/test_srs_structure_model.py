"""CPU tests of the exponent model behind the setup-ceremony GPU tests
(tests/test_gpu_srs_ceremony.py), and the builders those tests share.

A setup is described by discrete logs: P_i = [a_i]G, Q_j = [b_j]G2.  The
documented equations of kzgx_srs_verify_structure then read, in exponents,
  g1_ok  <=>  sum_{i<n-1} rho^i (a_(i+1) b_0 - a_i b_1) == 0 mod r
              and a_0 != 0 and (n < 2 or a_1 != 0)
  g2_ok  <=>  sum_{j<m-1} sigma^j (a_1 b_j - a_0 b_(j+1)) == 0 mod r
              and b_0 != 0            (n >= 2; with n = 1 there is no P_1: 0)
and, with the generator flag, both also need a_0 == b_0 == 1.  The GPU tests
take every expected boolean from structure_model(); this file pins the model
once against the oracle's real points and its definitional pairing, at
n = m = 3, on a valid and on a corrupted setup, and pins the update identity
(tau -> tau s) against corc.gen_srs."""
import numpy as np
import pytest

import corc
import kzg_ref as K
import pairing_ref as PR

CURVES = [("BN254", K.BN254), ("BLS12381", K.BLS12381)]


def w64(C):
    return 4 if C.name == "BN254" else 6


def structure_model(C, a, b, rho, sigma, generators=False):
    """(g1_ok, g2_ok) of the documented equations, from the discrete logs"""
    r, n, m = C.r, len(a), len(b)
    assert n >= 1 and m >= 2
    a = [v % r for v in a]
    b = [v % r for v in b]
    s1 = sum(pow(rho, i, r) * (a[i + 1] * b[0] - a[i] * b[1]) for i in range(n - 1)) % r
    g1 = s1 == 0 and a[0] != 0 and (n < 2 or a[1] != 0)
    g2 = False
    if n >= 2:
        s2 = sum(pow(sigma, j, r) * (a[1] * b[j] - a[0] * b[j + 1]) for j in range(m - 1)) % r
        g2 = s2 == 0 and b[0] != 0
    if generators:
        gens = a[0] == 1 and b[0] == 1
        g1, g2 = g1 and gens, g2 and gens
    return g1, g2


def update_model(C, a_prev, a_new, w):
    """kzgx_srs_verify_update in exponents: prev = [a_prev]G, new = [a_new]G, W = [w]G2"""
    r = C.r
    return (a_new - a_prev * w) % r == 0 and w % r != 0 and a_new % r != 0


def powers(C, tau, n, start=0, c=1):
    """the logs of a setup: c tau^(start + i)"""
    return [c * pow(tau, start + i, C.r) % C.r for i in range(n)]


def g1_point(C, k):
    """[k]G by the C oracle (None = infinity)"""
    k %= C.r
    return None if k == 0 else corc.scalar_mul(C.name, (C.gx, C.gy), k)


_G2_POINTS = {}


def g2_point(C, k):
    """[k]G2 by the Python oracle (None = infinity), cached"""
    k %= C.r
    key = (C.name, k)
    if key not in _G2_POINTS:
        _G2_POINTS[key] = None if k == 0 else PR.g2_mul(C, PR.g2_generator(C), k)
    return _G2_POINTS[key]


def g1_rows(C, pts):
    return corc.points_to_array(C.name, pts)


def g2_rows(C, pts):
    nl = w64(C)
    out = np.zeros((len(pts), 4 * nl), dtype=np.uint64)
    for i, Q in enumerate(pts):
        if Q is not None:
            for j, v in enumerate((Q[0][0], Q[0][1], Q[1][0], Q[1][1])):
                out[i, j * nl:(j + 1) * nl] = corc.ints_to_limbs([v], nl)[0]
    return out


def g1_msm(C, pts, scalars):
    acc = None
    for P, k in zip(pts, scalars):
        if P is not None and k % C.r:
            acc = K.point_add(C, acc, corc.scalar_mul(C.name, P, k % C.r))
    return acc


def g2_msm(C, pts, scalars):
    acc = None
    for Q, k in zip(pts, scalars):
        if Q is not None and k % C.r:
            acc = PR.g2_add(C, acc, PR.g2_mul(C, Q, k))
    return acc


def pairing_or_one(C, P, Q, one):
    return one if P is None or Q is None else PR.pairing(C, P, Q)


def equations_with_points(C, a, b, rho, sigma):
    """the two documented pairing equations on real points (four pairings)"""
    r = C.r
    P = [g1_point(C, v) for v in a]
    Q = [g2_point(C, v) for v in b]
    n, m = len(P), len(Q)
    rp = [pow(rho, i, r) for i in range(n - 1)]
    sp = [pow(sigma, j, r) for j in range(m - 1)]
    A, B = g1_msm(C, P[:-1], rp), g1_msm(C, P[1:], rp)
    A2, B2 = g2_msm(C, Q[:-1], sp), g2_msm(C, Q[1:], sp)
    one = PR.F12.one(C.p)
    e = [pairing_or_one(C, B, Q[0], one), pairing_or_one(C, A, Q[1], one),
         pairing_or_one(C, P[1], A2, one), pairing_or_one(C, P[0], B2, one)]
    g1 = e[0] == e[1] and P[0] is not None and P[1] is not None
    g2 = e[2] == e[3] and Q[0] is not None
    return g1, g2


@pytest.mark.parametrize("name,C", CURVES)
def test_model_matches_the_pairing_on_a_valid_setup(name, C):
    tau = K.default_tau(C)
    a, b = powers(C, tau, 3), powers(C, tau, 3)
    rho, sigma = 0x1234567, 0x7654321
    assert structure_model(C, a, b, rho, sigma) == (True, True)
    assert equations_with_points(C, a, b, rho, sigma) == (True, True)


@pytest.mark.parametrize("name,C", CURVES)
def test_model_matches_the_pairing_on_a_corrupted_setup(name, C):
    """G1[2] wrong: the G1 equation fails and the G2 equation, which reads only P_0, P_1, holds"""
    tau = K.default_tau(C)
    a, b = powers(C, tau, 3), powers(C, tau, 3)
    a[2] = 0xC0FFEE
    rho, sigma = 0x1234567, 0x7654321
    assert structure_model(C, a, b, rho, sigma) == (False, True)
    assert equations_with_points(C, a, b, rho, sigma) == (False, True)


@pytest.mark.parametrize("name,C", CURVES)
def test_update_identity(name, C):
    """[s^i]([tau^i]G) = [(tau s)^i]G, word for word against corc.gen_srs"""
    tau = K.default_tau(C)
    s = K.random_scalars(C, 1, seed=0x5EED)[0]
    n = 5
    old = corc.array_to_points(name, corc.gen_srs(name, tau, n))
    upd = [corc.scalar_mul(name, P, pow(s, i, C.r)) for i, P in enumerate(old)]
    assert np.array_equal(corc.points_to_array(name, upd), corc.gen_srs(name, tau * s % C.r, n))
    # and in the model: the updated logs are again consecutive powers, of tau s
    a = [v * pow(s, i, C.r) % C.r for i, v in enumerate(powers(C, tau, n))]
    assert a == powers(C, tau * s % C.r, n)
    assert update_model(C, a_prev=tau, a_new=tau * s % C.r, w=s)
    assert not update_model(C, a_prev=tau, a_new=tau * s % C.r, w=s + 1)


def test_model_sees_what_per_point_checks_cannot():
    """a cancellation under one rho is exactly what the documented equation allows"""
    C = K.BN254
    r = C.r
    tau = K.default_tau(C)
    a, b = powers(C, tau, 6), powers(C, tau, 2)
    rho = 0xABCDEF
    # errors d_2, d_4 on P_2, P_4: an error d_k (k <= n - 2) adds rho^(k-1) d_k b_0 - rho^k d_k b_1 to
    # the G1 sum, so both add (b_0 - rho b_1) (rho d_2 + rho^3 d_4), zero iff rho^2 d_2 + rho^4 d_4 == 0
    d2 = 0x1111
    d4 = (-d2 * pow(rho * rho % r, -1, r)) % r
    a[2] = (a[2] + d2) % r
    a[4] = (a[4] + d4) % r
    assert structure_model(C, a, b, rho, 1)[0] is True
    assert structure_model(C, a, b, rho + 1, 1)[0] is False
