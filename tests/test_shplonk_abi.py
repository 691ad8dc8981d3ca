"""CPU tests of the Shplonk openings' boundary: libkzgx.so exports the new entries, the ctypes
binding carries them, the header's constants have the documented values, a NULL context is
rejected -- and a pure-Python model (tests/shplonk_model.py) of the three identities the scheme
rests on:
  1. F div Z_s = sum_(i in S_s) c_(s,i) (F - F(t_i)) / (X - t_i)      (the fused quotient)
  2. G(z) = t for the honest h                                          (step 2's returned value)
  3. tau W' == sum_c s_c C_c - t - Z_T(z) W + z W'  on exponents       (the verifier)
over random shapes: z in T, equal values at different indices of T, sets with no claims, n = 1 and
n <= d_s; and the verifier's equation fails on perturbed inputs."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import kzg_ref as K
import shplonk_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "kzg-commitments_amd", "libkzgx.so")
NAMES = ["kzgx_shplonk_commit", "kzgx_shplonk_commit_device", "kzgx_shplonk_open", "kzgx_shplonk_open_device",
         "kzgx_shplonk_verify", "kzgx_shplonk_verify_device", "kzgx_shplonk_verify_checked",
         "kzgx_shplonk_verify_checked_device", "kzgx_set_shplonk_chunk"]


def test_library_exports_the_shplonk_entries():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(LIB)
    dyn = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    for n in NAMES:
        assert hasattr(lib, n), n
        assert re.search(r"\bT %s\b" % n, dyn), n


def test_binding_carries_them_and_the_constants():
    import kzgx
    for n in NAMES:
        assert n in kzgx.EXPORTS, n
        assert getattr(kzgx.lib(), n).argtypes is not None, n
    assert kzgx.SHPLONK_WEIGHT_POWERS == 1
    assert kzgx.SHPLONK_SET_MAX == 64
    assert kzgx.SHPLONK_POINTS_MAX == 4096
    assert kzgx.SHPLONK_CHUNK_SCALARS == 2097152
    assert kzgx.SHPLONK_TILE == 2048
    for m in ("shplonk_commit", "shplonk_commit_device", "shplonk_open", "shplonk_open_device", "shplonk_verify",
              "shplonk_verify_device", "set_shplonk_chunk"):
        assert callable(getattr(kzgx.Context, m)), m


def test_rejected_before_any_device_work():
    import kzgx
    L = kzgx.lib()
    assert L.kzgx_set_shplonk_chunk(None, 5) == -1  # KZGX_ERR_ARG
    assert L.kzgx_shplonk_commit(None, None, 1, 1, 1, None, 1, None, None, 1, None, None, 1, None, 0, 0, 0, None,
                                 None, None, None) == -1
    assert L.kzgx_shplonk_open(None, None, 1, 1, 1, None, 1, None, None, 1, None, None, 1, None, 0, 0, None, None,
                               None, None, None) == -1
    assert L.kzgx_shplonk_verify(None, None, None, 0, None, None, 1, None, None, 1, None, 1, None, 0, None, 0, None,
                                 None, None, 0, None) == -1
    assert L.kzgx_shplonk_verify_checked(None, None, None, 0, None, None, 1, None, None, 1, None, 1, None, 0, None, 0,
                                         None, None, None, 0, 1, None) == -1


def random_table(r, rnd, n, n_polys):
    """a random table: T with one value repeated at two indices that never share a set"""
    nT = rnd.randint(2, 9)
    T = [rnd.randrange(r) for _ in range(nT - 1)]
    T.append(T[0])  # the same value at index 0 and index nT - 1
    sets = []
    for _ in range(rnd.randint(1, 5)):
        d = rnd.randint(1, min(4, nT - 1))
        pts = rnd.sample(range(nT), d)
        if 0 in pts and nT - 1 in pts:
            pts.remove(0)
        m = rnd.randint(0, 3)  # sets with no claims among them
        sets.append((pts, [rnd.randrange(n_polys) for _ in range(m)]))
    polys = [[rnd.randrange(r) for _ in range(n)] for _ in range(n_polys)]
    count = sum(len(c) for _, c in sets)
    return M.Table(r, polys, T, sets, [rnd.randrange(r) for _ in range(count)])


@pytest.mark.parametrize("C", [K.BN254, K.BLS12381], ids=["BN254", "BLS12381"])
def test_fused_quotient_identity(C):
    """F div Z_s = sum_i c_(s,i) q_(F,t_i), coefficient by coefficient, zero when n <= d_s"""
    r = C.r
    rnd = random.Random(77)
    for trial in range(40):
        n = rnd.choice([1, 2, 3, 4, 5, 9])
        tab = random_table(r, rnd, n, 3)
        for s, (pts, _) in enumerate(tab.sets):
            F = tab.folded(s)
            want = M.floor_div(r, F, tab.vanishing(s))
            want += [0] * (n - len(want))
            got = [0] * n
            for a in pts:
                den = 1
                for b in pts:
                    if b != a:
                        den = den * (tab.T[a] - tab.T[b]) % r
                c = pow(den, -1, r)
                for i, q in enumerate(M.single_quotient(r, F, tab.T[a])):
                    got[i] = (got[i] + c * q) % r
            assert got == want
            if n <= len(pts):
                assert not any(want)


@pytest.mark.parametrize("C", [K.BN254, K.BLS12381], ids=["BN254", "BLS12381"])
def test_step_two_value_and_the_verifier_equation(C):
    """G(z) = t, and the verifier's equation on exponents holds for honest proofs (z in T included) and
    fails for perturbed values, commitments, proofs, z and weights"""
    r = C.r
    rnd = random.Random(78)
    for trial in range(30):
        n = rnd.choice([1, 2, 3, 5, 9])
        tab = random_table(r, rnd, n, 4)
        tau = rnd.randrange(1, r)
        z = tab.T[rnd.randrange(len(tab.T))] if trial % 3 == 0 else rnd.randrange(r)
        h = tab.h()
        assert len(h) == n and h[n - 1] == 0
        ys = tab.values()
        commits = [M.ev(r, P, tau) for P in tab.polys]
        G = tab.G(h, z)
        _, t = tab.verifier_scalars(ys, z, len(commits))
        Gz = M.ev(r, G, z)
        assert Gz == t
        W = M.ev(r, h, tau)
        Wp = M.ev(r, M.single_quotient(r, G, z) or [0], tau) if n > 1 else 0
        assert tab.verify(tau, commits, ys, z, W, Wp)
        if not ys or z in tab.T:
            continue  # with z in T a set's zeta_s may be 0: the equation no longer sees its claims
        bad = list(ys)
        bad[rnd.randrange(len(bad))] += 1
        assert not tab.verify(tau, commits, bad, z, W, Wp)
        assert not tab.verify(tau, commits, ys, z, (W + 1) % r, Wp)
        assert not tab.verify(tau, commits, ys, z, W, (Wp + 1) % r)
        used = sorted(set(tab.index))
        c2 = list(commits)
        c2[used[0]] = (c2[used[0]] + 1) % r
        assert not tab.verify(tau, c2, ys, z, W, Wp)


def test_equal_values_inside_one_set_have_no_interpolant():
    r = K.BN254.r
    tab = M.Table(r, [[1, 2, 3]], [5, 7, 5], [([0, 2], [0])], [1])
    with pytest.raises((ValueError, ZeroDivisionError)):
        tab.lagrange_at(0, 11)
