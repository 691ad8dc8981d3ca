"""GPU tests of the setup ceremony (kzgx_srs_update, kzgx_srs_verify_structure,
kzgx_srs_verify_update; csrc/srs_update.hip).

Update: the updated points are compared word for word with the C oracle's
setup for tau s (G1), with the Python oracle's points (G2) and with a second
context's generated setup for tau s.  Structure and update proof: every
expected boolean comes from the exponent model of
tests/test_srs_structure_model.py (pinned there against real pairings), under
explicit challenges.  Nothing has a tolerance: all results are exact."""
import numpy as np
import pytest

import corc
import kzg_ref as K
import pairing_ref as PR
from test_srs_structure_model import (CURVES, g1_point, g1_rows, g2_point, g2_rows, powers, structure_model,
                                      update_model)

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NO_SRS = -1, -4
RHO, SIGMA = 0x9E3779B97F4A7C15F39CC0605CEDC834, 0xD1B54A32D192ED03C2B2AE3D27D4EB4F


def limbs(vals):
    return corc.ints_to_limbs(list(vals), 4)


def pt(name, out, inf):
    return None if inf else corc.array_to_points(name, np.asarray(out)[None, :])[0]


def oracle_srs(name, tau, n):
    """the C oracle's [tau^i]G, i < n (it generates two points at least)"""
    return corc.gen_srs(name, tau, max(n, 2))[:n]


def secrets(C):
    """1, 2, r - 1 and a random full-width value"""
    v = next(v for v in K.random_scalars(C, 16, seed=0xCE4E) if v >> (C.r.bit_length() - 2))
    return [1, 2, C.r - 1, v]


@pytest.fixture(scope="module")
def env():
    """per curve: a context (default table off) and a second one for cross-checks"""
    import kzgx
    made = {}

    def get(name):
        if name not in made:
            a, b = kzgx.Context(name), kzgx.Context(name)
            a.set_default_table(0)
            b.set_default_table(0)
            made[name] = (a, b)
        return made[name]

    yield get
    for a, b in made.values():
        a.close()
        b.close()


def g2_oracle_rows(C, tau, idx, start=0):
    return g2_rows(C, [g2_point(C, pow(tau, start + j, C.r)) for j in idx])


def check_update(name, C, ctx, other, tau, s, n, m, start=0):
    r = C.r
    ctx.gen_srs(tau, n, start=start)
    ctx.gen_srs_g2(tau, m, start=start)
    w = ctx.srs_update(s, g1_start=start, g2_start=start)
    t2 = tau * s % r
    g1, g2 = ctx.get_srs(), ctx.get_srs_g2()
    assert ctx.srs_size == n and ctx.srs2_size == m
    if start == 0:
        assert np.array_equal(g1, oracle_srs(name, t2, n))
    else:
        assert np.array_equal(g1, g1_rows(C, [g1_point(C, pow(t2, start + i, r)) for i in range(n)]))
    idx = sorted({0, 1, m // 2, m - 1})
    assert np.array_equal(g2[idx], g2_oracle_rows(C, t2, idx, start))
    other.gen_srs(t2, n, start=start)
    other.gen_srs_g2(t2, m, start=start)
    assert np.array_equal(g1, other.get_srs()) and np.array_equal(g2, other.get_srs_g2())
    assert np.array_equal(w, g2_rows(C, [g2_point(C, s)])[0])


# ---- update parity --------------------------------------------------------------------------
# a lone lane, the wave edges, the 256-thread block edge with a ragged tail (G1); the 64-thread
# block edges (G2)
@pytest.mark.parametrize("n,m", [(1, 2), (2, 64), (3, 65), (64, 130), (65, 2), (257, 64), (300, 65)])
@pytest.mark.parametrize("name,C", CURVES)
def test_update_matches_the_oracle(name, C, env, n, m):
    ctx, other = env(name)
    check_update(name, C, ctx, other, K.default_tau(C), secrets(C)[3], n, m)


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("name,C", CURVES)
def test_update_edge_secrets(name, C, env, k):
    ctx, other = env(name)
    check_update(name, C, ctx, other, K.default_tau(C), secrets(C)[k], 65, 3)


@pytest.mark.parametrize("name,C", CURVES)
def test_update_of_a_shard(name, C, env):
    """a context that holds powers 5.. passes start = 5, as to kzgx_gen_srs_g1"""
    ctx, other = env(name)
    check_update(name, C, ctx, other, K.default_tau(C), secrets(C)[3], 66, 3, start=5)


@pytest.mark.parametrize("name,C", CURVES)
def test_update_rejects_bad_secrets_and_leaves_the_setup(name, C, env):
    import kzgx
    ctx, _ = env(name)
    tau = K.default_tau(C)
    ctx.gen_srs(tau, 5)
    ctx.gen_srs_g2(tau, 3)
    g1, g2 = ctx.get_srs(), ctx.get_srs_g2()
    for bad in (0, C.r, C.r + 1, (1 << 256) - 1):
        with pytest.raises(kzgx.KzgxError) as e:
            ctx.srs_update(bad)
        assert e.value.status == ERR_ARG
        assert np.array_equal(ctx.get_srs(), g1) and np.array_equal(ctx.get_srs_g2(), g2)
    P = K.random_scalars(C, 5, seed=77)
    out, inf = ctx.msm(limbs(P))
    assert pt(name, out, inf) == K.commit_via_tau(C, tau, P)
    fresh = kzgx.Context(name)
    try:
        with pytest.raises(kzgx.KzgxError) as e:
            fresh.srs_update(3)
        assert e.value.status == ERR_NO_SRS
        # a G1-only context: updated, and still without a G2 half
        fresh.set_default_table(0)
        fresh.gen_srs(tau, 4)
        fresh.srs_update(3)
        assert np.array_equal(fresh.get_srs(), oracle_srs(name, tau * 3 % C.r, 4)) and fresh.srs2_size == 0
    finally:
        fresh.close()


@pytest.mark.parametrize("name,C", CURVES)
def test_update_keeps_an_infinite_entry(name, C, env):
    ctx, _ = env(name)
    tau, s, r = K.default_tau(C), secrets(C)[3], C.r
    n = 6
    g1 = oracle_srs(name, tau, n)
    g1[3] = 0
    g2 = g2_oracle_rows(C, tau, range(4))
    g2[2] = 0
    ctx.load_srs(g1)
    ctx.load_srs_g2(g2)
    ctx.srs_update(s)
    want1 = oracle_srs(name, tau * s % r, n)
    want1[3] = 0
    want2 = g2_oracle_rows(C, tau * s % r, range(4))
    want2[2] = 0
    assert np.array_equal(ctx.get_srs(), want1) and np.array_equal(ctx.get_srs_g2(), want2)


# ---- derived state follows the update -------------------------------------------------------
def commits_match(name, C, ctx, tau, n, seed):
    P = K.random_scalars(C, n, seed=seed)
    out, inf = ctx.msm(limbs(P))
    return pt(name, out, inf) == K.commit_via_tau(C, tau, P)


@pytest.mark.parametrize("mode", ["default_table", "fixed_base", "table_off"])
@pytest.mark.parametrize("name,C", CURVES)
def test_msm_and_verify_follow_the_update(name, C, mode):
    import kzgx
    tau, s, r, n = K.default_tau(C) + 99, secrets(C)[3], C.r, 130
    t2 = tau * s % r
    ctx = kzgx.Context(name)
    try:
        if mode == "table_off":
            ctx.set_default_table(0)
        if mode == "fixed_base":
            ctx.set_fixed_base(8, n)
        ctx.gen_srs(tau, n)
        ctx.gen_srs_g2(tau, 3)
        assert commits_match(name, C, ctx, tau, n, 901)  # the old setup's tables are built and used
        P = K.random_scalars(C, n - 1, seed=902)
        z = limbs([12345])
        com, _ = ctx.msm(limbs(P))
        proof, _, y = ctx.prove_single_batch(limbs(P), z)
        assert ctx.verify_single_batch(com[None, :], proof, z, y).tolist() == [True]  # the old verify tables
        ctx.srs_update(s)
        if mode == "default_table":
            assert ctx.default_table_info()[1] == n
        assert commits_match(name, C, ctx, t2, n, 903)
        assert commits_match(name, C, ctx, t2, 64, 904)
        # a fresh opening verifies under the new setup and its proof is the tau s oracle's
        com, cinf = ctx.msm(limbs(P))
        proof, pinf, y = ctx.prove_single_batch(limbs(P), z)
        assert pt(name, com, cinf) == K.commit_via_tau(C, t2, P)
        assert pt(name, proof[0], pinf[0]) == K.commit_via_tau(C, t2, K.proof_quotient(C, P, 12345, 1))
        assert ctx.verify_single_batch(com[None, :], proof, z, y).tolist() == [True]
        bad_y = y.copy()
        bad_y[0, 0] ^= 1
        assert ctx.verify_single_batch(com[None, :], proof, z, bad_y).tolist() == [False]
    finally:
        ctx.close()


def test_all_domain_openings_follow_the_update(env):
    from test_gpu_prove_all import oracle, to_limbs
    name, C = "BLS12381", K.BLS12381
    ctx, _ = env(name)
    tau, s = K.default_tau(C), secrets(C)[3]
    ctx.gen_srs(tau, 8)
    ctx.gen_srs_g2(tau, 2)
    coeffs = K.random_scalars(C, 8, seed=0xFA11)
    xy, inf, _, _ = oracle(name, tau, coeffs, 3)
    got = ctx.prove_all(to_limbs(coeffs))  # caches the all-domain setup of the old tau
    assert (got[0] == xy).all() and (got[1] == inf).all()
    ctx.srs_update(s)
    xy, inf, _, _ = oracle(name, tau * s % C.r, coeffs, 3)
    got = ctx.prove_all(to_limbs(coeffs))
    assert (got[0] == xy).all() and (got[1] == inf).all()


@pytest.mark.parametrize("name,C", CURVES)
def test_a_shared_default_table_stays_the_other_contexts(name, C):
    import kzgx
    tau, s, n = K.default_tau(C) + 777, 0xABCDEF0123456789, 200  # an SRS no other test's context holds
    a, b = kzgx.Context(name), kzgx.Context(name)
    try:
        n0 = kzgx.shared_tables(0)[0]
        a.gen_srs(tau, n)
        b.gen_srs(tau, n)
        assert kzgx.shared_tables(0)[0] == n0 + 1 and a.default_table_info() == b.default_table_info()
        a.srs_update(s)
        assert kzgx.shared_tables(0)[0] == n0 + 2
        assert commits_match(name, C, b, tau, n, 911)
        assert commits_match(name, C, a, tau * s % C.r, n, 912)
        assert np.array_equal(b.get_srs(), oracle_srs(name, tau, n))
    finally:
        a.close()
        b.close()


# ---- structure ------------------------------------------------------------------------------
def load_logs(C, ctx, a, b):
    ctx.load_srs(g1_rows(C, [g1_point(C, v) for v in a]))
    ctx.load_srs_g2(g2_rows(C, [g2_point(C, v) for v in b]))


def both(C, ctx, a, b, rho=RHO, sigma=SIGMA):
    """the call's answers without and with the generator flag, checked against the model"""
    rho, sigma = rho % C.r, sigma % C.r
    res = []
    for gen in (False, True):
        got = ctx.srs_verify_structure(rho, sigma, generators=gen)
        assert got == structure_model(C, a, b, rho, sigma, generators=gen), (gen, got)
        res.append(got)
    return res


@pytest.mark.parametrize("n,m", [(2, 2), (3, 65), (130, 130), (130, 2), (2, 130)])
@pytest.mark.parametrize("name,C", CURVES)
def test_generated_setups_are_valid_also_after_an_update(name, C, env, n, m):
    ctx, _ = env(name)
    tau, s = K.default_tau(C), secrets(C)[3]
    ctx.gen_srs(tau, n)
    ctx.gen_srs_g2(tau, m)
    assert ctx.srs_check(True) == (True, True)
    assert both(C, ctx, powers(C, tau, n), powers(C, tau, m)) == [(True, True), (True, True)]
    ctx.srs_update(s)
    t2 = tau * s % C.r
    assert both(C, ctx, powers(C, t2, n), powers(C, t2, m)) == [(True, True), (True, True)]


@pytest.mark.parametrize("name,C", CURVES)
def test_scaled_setups_pass_only_without_the_generator_flag(name, C, env):
    ctx, _ = env(name)
    tau, c = K.default_tau(C), 0xC0DE
    a, b = powers(C, tau, 5, c=c), powers(C, tau, 4, c=c)
    load_logs(C, ctx, a, b)
    assert both(C, ctx, a, b) == [(True, True), (False, False)]


def corruptions(C, tau, n, m):
    """label -> (G1 logs, G2 logs, expected without the flag or None = whatever the model says)"""
    r = C.r
    a0, b0 = powers(C, tau, n), powers(C, tau, m)
    out = {}

    def put(label, a, b, want=None):
        out[label] = (a, b, want)

    a = list(a0)
    a[3], a[4] = a[4], a[3]
    put("adjacent G1 swapped", a, b0, (False, True))
    for i in (2, n - 1, 0):
        a = list(a0)
        a[i] = 0x5EED5
        put("G1[%d] = [k]G" % i, a, b0, (False, True) if i >= 2 else None)
    a = list(a0)
    a[5] = r - a[5]
    put("G1[5] negated", a, b0, (False, True))
    for j in (2, m - 1):
        b = list(b0)
        b[j] = 0xBAD2
        put("G2[%d] wrong" % j, a0, b, (True, False))
    put("G2 from another tau", a0, powers(C, tau + 1, m), (False, False))
    a = list(a0)
    a[1] = 0
    put("G1[1] = O", a, b0, (False, False))
    return out


@pytest.mark.parametrize("name,C", CURVES)
def test_corrupted_setups(name, C, env):
    """every corruption is a valid subgroup point (kzgx_srs_check still passes); the structure
    test answers what the exponent model says"""
    ctx, _ = env(name)
    tau, n, m = K.default_tau(C), 8, 5
    for label, (a, b, want) in corruptions(C, tau, n, m).items():
        load_logs(C, ctx, a, b)
        assert ctx.srs_check(True) == (True, True), label
        got = both(C, ctx, a, b)
        if want is not None:
            assert got[0] == want, label
        assert got[0] != (True, True), label


@pytest.mark.parametrize("name,C", CURVES)
def test_errors_that_cancel_under_one_rho_pass_under_that_rho_only(name, C, env):
    """the call computes the documented equation, nothing stronger: rho^2 d_2 + rho^4 d_4 == 0"""
    ctx, _ = env(name)
    r, tau, rho = C.r, K.default_tau(C), RHO % C.r
    a, b = powers(C, tau, 6), powers(C, tau, 2)
    d2 = 0x1111
    d4 = (-d2 * pow(rho * rho % r, -1, r)) % r
    a[2], a[4] = (a[2] + d2) % r, (a[4] + d4) % r
    load_logs(C, ctx, a, b)
    assert structure_model(C, a, b, rho, SIGMA % r)[0] is True
    assert ctx.srs_verify_structure(rho, SIGMA % r)[0] is True
    assert structure_model(C, a, b, rho + 1, SIGMA % r)[0] is False
    assert ctx.srs_verify_structure(rho + 1, SIGMA % r)[0] is False


@pytest.mark.parametrize("name,C", CURVES)
def test_drawn_challenges(name, C, env):
    ctx, _ = env(name)
    tau = K.default_tau(C)
    ctx.gen_srs(tau, 9)
    ctx.gen_srs_g2(tau, 9)
    assert ctx.srs_verify_structure() == (True, True)
    assert ctx.srs_verify_structure(generators=True) == (True, True)
    a, b = powers(C, tau, 9), powers(C, tau, 9)
    a[4], b[6] = 0x4444, 0x6666
    load_logs(C, ctx, a, b)
    assert ctx.srs_verify_structure() == (False, False)


@pytest.mark.parametrize("name,C", CURVES)
def test_structure_degenerate_sizes_and_arguments(name, C, env):
    import kzgx
    ctx, _ = env(name)
    tau = K.default_tau(C)
    ctx.gen_srs(tau, 1)
    ctx.gen_srs_g2(tau, 2)
    assert both(C, ctx, [1], powers(C, tau, 2)) == [(True, False), (True, False)]  # n = 1: no P_1
    ctx.gen_srs(tau, 4)
    ctx.gen_srs_g2(tau, 1)
    for args in ((RHO % C.r, SIGMA % C.r), (None, None)):
        with pytest.raises(kzgx.KzgxError) as e:
            ctx.srs_verify_structure(*args)
        assert e.value.status == ERR_NO_SRS
    ctx.gen_srs_g2(tau, 2)
    with pytest.raises(kzgx.KzgxError) as e:
        ctx.srs_verify_structure(C.r, 1)
    assert e.value.status == ERR_ARG
    fresh = kzgx.Context(name)
    try:
        with pytest.raises(kzgx.KzgxError) as e:
            fresh.srs_verify_structure(1, 1)
        assert e.value.status == ERR_NO_SRS
    finally:
        fresh.close()


# ---- update proof ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,C", CURVES)
def test_update_proof(name, C, env):
    ctx, other = env(name)
    r, tau, s = C.r, K.default_tau(C), secrets(C)[3]
    ctx.gen_srs(tau, 3)
    ctx.gen_srs_g2(tau, 2)
    prev = ctx.get_srs()[1].copy()
    w = ctx.srs_update(s)
    new = ctx.get_srs()[1].copy()
    t2 = tau * s % r
    g2 = lambda k: g2_rows(C, [g2_point(C, k)])[0]
    cases = [
        ("a real update", prev, new, w, (tau, t2, s)),
        ("W from another s", prev, new, g2(s + 1), (tau, t2, s + 1)),
        ("W = O", prev, new, g2(0), (tau, t2, 0)),
        ("new = prev, s != 1", prev, prev, w, (tau, tau, s)),
        ("new = prev, W = G2", prev, prev, g2(1), (tau, tau, 1)),
        ("new = O", prev, np.zeros_like(prev), g2(0), (tau, 0, 0)),
    ]
    for label, p, q, wit, logs in cases:
        # the call needs no SRS: the second context holds whatever the last test left
        assert other.srs_verify_update(p, q, wit) == update_model(C, *logs), label
    assert [update_model(C, *c[4]) for c in cases] == [True, False, False, False, True, False]
