"""The block-table accumulation's residency reserve (msm_joint.hip,
kzgx_set_fixed_accum_reserve): launches that leave r wave slots per CU free
run the same kernel on the same data, so every output is the same word for
word at every r, and equal to the CPU oracle's naive per-term MSM.

Shape: the forced block table at g = 4 over 13 points (three whole blocks and
a short last block of one point), batch 3.  Scalars: 0, 1, r - 1, 2^127 +- 1
(the halves' boundary under the endomorphism split) and seeded random ones.
Reserves: 0 (the plain launch), 1, 2 and one far beyond what the device can
hold back (clamped).  Once on an SRS with points at infinity (tau = 0: the
accumulation kernel that tests for entries at infinity) and once on the
254 / 255-plane path (KZGX_FIXED_JOINT_GLV=0)."""
import numpy as np
import pytest

import kzg_ref as K

pytestmark = pytest.mark.gpu

CURVES = [("BN254", K.BN254), ("BLS12381", K.BLS12381)]
G, N, BATCH, C_REQ = 4, 13, 3, 8
RESERVES = (0, 1, 2, 1 << 20)
KZGX_ERR_ARG = -1


def limbs(vals):
    import corc
    return corc.ints_to_limbs(vals, 4)


def pt(curve, row, inf):
    import corc
    return None if inf else corc.array_to_points(curve, row[None, :])[0]


def rows_for(C):
    edges = [0, 1, C.r - 1, (1 << 127) - 1, (1 << 127) + 1]
    rows = []
    for b in range(BATCH):
        row = K.random_scalars(C, N, seed=4200 + b)
        for j, v in enumerate(edges):
            row[(3 * j + 5 * b) % N] = v  # the edge scalars move through the blocks, the short one included
        rows.append(row)
    return rows


def run_all_reserves(name, C, tau, oracle_c, variant):
    import kzgx
    srs = oracle_c.gen_srs(name, tau % C.r, N)
    rows = rows_for(C)
    SB = np.concatenate([limbs(r) for r in rows])
    exp = [oracle_c.msm_naive(name, srs, limbs(r)) for r in rows]
    ctx = kzgx.Context(name)
    try:
        ctx.load_srs(srs)
        ctx.set_fixed_joint(G)
        ctx.set_fixed_base(C_REQ, N)
        assert ctx.fixed_joint_info()[:2] == (G, 4)
        assert ctx.fixed_accum_variant() == variant  # bit 0: tests for entries at infinity, bit 1: the split
        res = []
        for r in RESERVES:
            ctx.set_fixed_accum_reserve(r)
            req, eff, lds = ctx.fixed_accum_reserve_info()
            assert req == r
            if r == 0:
                assert (eff, lds) == (0, 0)
            elif r <= 2:
                assert eff == r and 0 < lds <= 65536, (r, eff, lds)
            else:
                assert 2 <= eff < 32 and 0 < lds <= 65536, (r, eff, lds)  # clamped: a CU keeps a workgroup
            res.append((eff, lds) + ctx.msm_batch(SB, N, BATCH))
        assert res[1][1] < res[2][1] <= res[3][1]  # a larger reserve is held by more LDS
        for eff, lds, out, inf in res:
            assert (out == res[0][2]).all() and (inf == res[0][3]).all(), eff
            for b in range(BATCH):
                assert pt(name, out[b], inf[b]) == exp[b], (eff, b)
    finally:
        ctx.close()


@pytest.mark.parametrize("name,C", CURVES)
def test_outputs_identical_at_every_reserve(name, C, oracle_c):
    run_all_reserves(name, C, K.default_tau(C), oracle_c, 2)


@pytest.mark.parametrize("name,C", CURVES)
def test_outputs_identical_with_points_at_infinity(name, C, oracle_c):
    """tau = 0: every SRS point but the first is at infinity, so are table entries"""
    run_all_reserves(name, C, 0, oracle_c, 3)


@pytest.mark.parametrize("name,C", CURVES)
def test_outputs_identical_without_the_split(name, C, oracle_c, monkeypatch):
    monkeypatch.setenv("KZGX_FIXED_JOINT_GLV", "0")
    run_all_reserves(name, C, K.default_tau(C), oracle_c, 0)


@pytest.mark.parametrize("name,C", CURVES)
def test_setter_info_and_environment(name, C, monkeypatch):
    import kzgx
    monkeypatch.delenv("KZGX_FIXED_ACCUM_RESERVE", raising=False)
    ctx = kzgx.Context(name)
    try:
        req, eff0, lds0 = ctx.fixed_accum_reserve_info()
        assert req == -1 and (eff0 == 0) == (lds0 == 0)  # the curve's default
        ctx.set_fixed_accum_reserve(2)
        _, eff, lds = ctx.fixed_accum_reserve_info()
        assert eff == 2 and lds > 0
        ctx.set_fixed_accum_reserve(0)
        assert ctx.fixed_accum_reserve_info() == (0, 0, 0)
        for bad in (-2, -100):
            with pytest.raises(kzgx.KzgxError) as e:
                ctx.set_fixed_accum_reserve(bad)
            assert e.value.status == KZGX_ERR_ARG
            assert ctx.fixed_accum_reserve_info() == (0, 0, 0)  # a refused value changes nothing
        ctx.set_fixed_accum_reserve(-1)
        assert ctx.fixed_accum_reserve_info() == (-1, eff0, lds0)
        assert kzgx.lib().kzgx_set_fixed_accum_reserve(None, 1) == KZGX_ERR_ARG
        assert kzgx.lib().kzgx_fixed_accum_reserve_info(None, None, None, None, None) == KZGX_ERR_ARG
    finally:
        ctx.close()
    # read at context creation, as KZGX_FIXED_JOINT_GLV is; a value that is no reserve is ignored
    for text, want in (("2", (2, eff, lds)), ("0", (0, 0, 0)), ("-1", (-1, eff0, lds0)), ("two", (-1, eff0, lds0)),
                       ("-3", (-1, eff0, lds0)), ("1x", (-1, eff0, lds0))):
        monkeypatch.setenv("KZGX_FIXED_ACCUM_RESERVE", text)
        c2 = kzgx.Context(name)
        try:
            assert c2.fixed_accum_reserve_info() == want, text
        finally:
            c2.close()
