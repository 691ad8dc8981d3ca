"""GPU parity of the block-table ("joint") fixed-base MSM path (msm_joint.hip).

kzgx_set_fixed_joint(g) forces a table of the signed subset sums of blocks of
g consecutive SRS points beside the window table, and every batch >= 1 onto
it: index pass (k_joint_index), plane accumulation (k_joint_accum), Horner
pass.  Every output is compared with the CPU oracle's naive per-term MSM
(corc.msm_naive).  tests/test_joint_recoding.py is the model these kernels
follow, with the index bound idx < 2^(g_b - 1) asserted on the CPU.

Shapes: the block sizes take both builders (g = 2: one thread per entry;
g = 5, 8, 13: the batched affine builder, with a short last block of either
kind), n_use covers whole skipped blocks and a padded partial block, batch 65
crosses the automatic path's threshold, and both block-range counts run."""
import os
import sys

import numpy as np
import pytest

import kzg_ref as K

pytestmark = pytest.mark.gpu

CURVES = [("BN254", K.BN254), ("BLS12381", K.BLS12381)]
C_REQ = 8  # the footprint asked for: fixed_base_bytes(8, n_t) holds both tables


def limbs(vals, nl=4):
    import corc
    return corc.ints_to_limbs(vals, nl)


def pt(curve, row, inf=False):
    import corc
    return None if inf else corc.array_to_points(curve, row[None, :])[0]


@pytest.fixture
def fresh_ctx():
    import kzgx
    made = []

    def get(curve):
        c = kzgx.Context(curve)
        made.append(c)
        return c

    yield get
    for c in made:
        c.close()


def edge_scalars(C):
    return [0, 1, C.r - 1, C.r - 2, (1 << 253) - 1]


def build(ctx, name, g, n_t):
    import kzgx
    ctx.set_fixed_joint(g)
    ctx.set_fixed_base(C_REQ, n_t)
    gg, blocks, jbytes = ctx.fixed_joint_info()
    assert (gg, blocks) == (g, (n_t + g - 1) // g)
    assert jbytes == blocks * (1 << (g - 1)) * (64 if name == "BN254" else 112)
    c, nt, total = ctx.fixed_base_info()
    cw, wbytes = ctx.fixed_window_info()
    assert (c, nt) == (C_REQ, n_t) and 0 < cw <= C_REQ and total == jbytes + wbytes
    assert wbytes == kzgx.fixed_base_bytes(name, cw, n_t)
    assert total <= kzgx.fixed_base_bytes(name, C_REQ, n_t)


@pytest.mark.parametrize("name,C", CURVES)
@pytest.mark.parametrize("g,n_t", [(2, 37), (5, 37), (8, 37), (2, 300), (5, 300), (8, 300), (13, 300)])
def test_joint_matches_naive(name, C, g, n_t, fresh_ctx, oracle_c):
    ctx = fresh_ctx(name)
    srs = oracle_c.gen_srs(name, K.default_tau(C), n_t)
    ctx.load_srs(srs)
    build(ctx, name, g, n_t)
    sc = K.random_scalars(C, n_t, seed=1000 * g + n_t)
    for j, v in enumerate(edge_scalars(C)):
        sc[j] = v
    S = limbs(sc)
    ref = {n_use: oracle_c.msm_naive(name, srs[:n_use], S[:n_use])
           for n_use in (n_t, n_t - 1, 1, g, g + 1, 2 * g + 3)}
    for ranges in (1, 2):
        ctx.set_fixed_joint_ranges(ranges)
        for n_use, exp in ref.items():
            out, inf = ctx.msm(S[:n_use])
            assert pt(name, out, inf) == exp, (ranges, n_use)
    # batches: rows of their own scalars, the edge scalars moving through the blocks
    ctx.set_fixed_joint_ranges(0)
    for batch in (3, 65):
        n_use = n_t if batch == 3 else 2 * g + 3
        rows = []
        for b in range(batch):
            row = K.random_scalars(C, n_use, seed=7000 + 100 * g + b)
            for j, v in enumerate(edge_scalars(C)):
                row[(j * 3 + b) % n_use] = v
            rows.append(row)
        rows[1] = list(rows[0])  # a repeated row
        SB = np.concatenate([limbs(r) for r in rows])
        for ranges in (1, 2):
            ctx.set_fixed_joint_ranges(ranges)
            out, inf = ctx.msm_batch(SB, n_use, batch)
            for b in range(batch):
                assert pt(name, out[b], inf[b]) == oracle_c.msm_naive(name, srs[:n_use], limbs(rows[b])), (batch, b)


@pytest.mark.parametrize("name,C", CURVES)
def test_joint_noncanonical_scalars(name, C, fresh_ctx, oracle_c):
    """scalars >= r (outside the ABI contract) still give (s mod r) P"""
    ctx = fresh_ctx(name)
    n = 40
    tau = K.default_tau(C)
    ctx.load_srs(oracle_c.gen_srs(name, tau, n))
    build(ctx, name, 5, n)
    sc = [C.r, C.r + 5, (1 << 256) - 1, 2 * C.r + 1] + K.random_scalars(C, n - 4, seed=9)
    out, inf = ctx.msm(limbs(sc))
    assert pt(name, out, inf) == K.commit_via_tau(C, tau, [v % C.r for v in sc])


@pytest.mark.parametrize("name,C", CURVES)
@pytest.mark.parametrize("g", [5, 8])
@pytest.mark.parametrize("tau", [0, 1, -1, 2])
def test_joint_degenerate_srs(name, C, tau, g, fresh_ctx, oracle_c):
    """tau = 0: infinite SRS points, whole blocks of entries at infinity;
    tau = +-1: repeated and opposite points, so the builder's affine additions
    meet equal and opposite operands and (tau = -1, even g) entries at
    infinity; tau = 2: a well-formed SRS from a tiny tau.  Rows that cancel
    exactly give infinity; a repeated row repeats its output."""
    ctx = fresh_ctx(name)
    t = tau % C.r
    n = 43
    srs = oracle_c.gen_srs(name, t, n)
    ctx.load_srs(srs)
    build(ctx, name, g, n)
    rows = [K.random_scalars(C, n, seed=50 + b) for b in range(4)]
    rows[0][7] = rows[0][3]
    rows[0][9] = (C.r - rows[0][3]) % C.r
    rows[2] = list(rows[1])
    z = [0] * n  # cancels exactly on repeated points: s P_0 -+ s P_1
    if tau in (1, -1):
        z[0], z[1] = 12345, (C.r - 12345) if tau == 1 else 12345
    rows[3] = z
    SB = np.concatenate([limbs(r) for r in rows])
    out, inf = ctx.msm_batch(SB, n, 4)
    for b in range(4):
        assert pt(name, out[b], inf[b]) == oracle_c.msm_naive(name, srs, limbs(rows[b])), b
    assert inf[3] and (out[1] == out[2]).all()
    out1, inf1 = ctx.msm(limbs(rows[0]))
    assert pt(name, out1, inf1) == K.commit_via_tau(C, t, rows[0])


def _bench():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench
    return bench


@pytest.mark.parametrize("name,C", CURVES)
def test_joint_proof_path(name, C, fresh_ctx):
    """65 commits and 65 single-opening proofs (prove_single_batch_device: the
    quotient, then a 299-point MSM) at n_t = 300, g = 8, on two streams as the
    bench runs them, checked as bench.check_step checks: commit = [P(tau)]G1,
    proof = [q(tau)]G1, y = P(z)"""
    import torch
    bench = _bench()
    ctx = fresh_ctx(name)
    tau = K.default_tau(C)
    n, B = 300, 65
    ctx.gen_srs(tau, n)
    build(ctx, name, 8, n)
    coeffs, zs = bench.bench_inputs(C, "cfg2", B, n)
    coeffs[3] = 0          # zero polynomial: commit and proof at infinity
    coeffs[5, 1:] = 0      # constant polynomial: proof at infinity
    coeffs[7, :] = coeffs[6, :]
    dev = torch.device("cuda", 0)
    bufs = bench.StepBuffers(torch, dev, coeffs, zs, ctx.w64)
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    step = bench.make_step(ctx, "cfg2", n, bufs, streams)
    torch.cuda.synchronize(dev)
    for _ in range(2):
        step()
    torch.cuda.synchronize(dev)
    checked, ok, bad = bench.check_step(name, C, tau, "cfg2", coeffs, zs, bufs, ctx.w64)
    assert checked == 3 * B and ok == checked, bad


def test_joint_lifecycle(fresh_ctx, oracle_c):
    """a new SRS rebuilds both tables; set_fixed_base(0) frees both;
    set_fixed_joint(0) is the window table alone, the same bytes out; the
    automatic choice builds nothing below 1024 points; a block size that does
    not fit the footprint is refused and leaves the tables as they were"""
    import kzgx
    name, C = CURVES[0]
    ctx = fresh_ctx(name)
    tau = K.default_tau(C)
    n = 300
    srs = oracle_c.gen_srs(name, tau, n)
    ctx.load_srs(srs)
    sc = K.random_scalars(C, n, seed=3)
    S = limbs(sc)
    exp = oracle_c.msm_naive(name, srs, S)
    ctx.set_fixed_base(C_REQ, n)  # automatic, 300 points: no block table
    assert ctx.fixed_joint_info() == (0, 0, 0)
    assert ctx.fixed_base_info() == (C_REQ, n, kzgx.fixed_base_bytes(name, C_REQ, n))
    out0, inf0 = ctx.msm(S)
    build(ctx, name, 8, n)
    out1, inf1 = ctx.msm(S)
    assert pt(name, out0, inf0) == exp and not inf1 and (out0 == out1).all()
    # a new SRS rebuilds both (clamped to its size)
    ctx.gen_srs(tau + 1, 200)
    assert ctx.fixed_joint_info()[:2] == (8, 25) and ctx.fixed_base_info()[:2] == (C_REQ, 200)
    out, inf = ctx.msm(S[:200])
    assert pt(name, out, inf) == K.commit_via_tau(C, tau + 1, sc[:200])
    # off: the parent's path and table
    ctx.set_fixed_joint(0)
    assert ctx.fixed_joint_info() == (0, 0, 0)
    assert ctx.fixed_window_info() == (C_REQ, kzgx.fixed_base_bytes(name, C_REQ, 200))
    out2, inf2 = ctx.msm(S[:200])
    assert not inf2 and (out2 == out).all()
    with pytest.raises(kzgx.KzgxError):
        ctx.set_fixed_joint(25)  # 8 blocks x 2^24 entries: far over the c = 8 footprint
    assert ctx.fixed_joint_info() == (0, 0, 0) and ctx.fixed_base_info()[0] == C_REQ
    with pytest.raises(kzgx.KzgxError):
        ctx.set_fixed_joint(1)
    ctx.set_fixed_joint(5)
    assert ctx.fixed_joint_info()[0] == 5
    ctx.set_fixed_base(0)
    assert ctx.fixed_base_info() == (0, 0, 0) and ctx.fixed_joint_info() == (0, 0, 0)
    out3, inf3 = ctx.msm(S[:200])  # Pippenger
    assert not inf3 and (out3 == out).all()


def test_joint_automatic_split_fits_the_request(fresh_ctx):
    """the automatic choice at 4097 points, c = 12: both tables inside
    fixed_base_bytes(12, 4097); batches of >= 64 MSMs take the block table,
    smaller ones the window table, with the same outputs"""
    import kzgx
    name, C = CURVES[0]
    ctx = fresh_ctx(name)
    tau = K.default_tau(C)
    n = 4097
    ctx.gen_srs(tau, n)
    ctx.set_fixed_base(12, n)
    g, blocks, jbytes = ctx.fixed_joint_info()
    cw, wbytes = ctx.fixed_window_info()
    c, nt, total = ctx.fixed_base_info()
    assert (c, nt) == (12, n) and total == jbytes + wbytes
    assert total <= kzgx.fixed_base_bytes(name, 12, n)
    assert 2 <= g <= 25 and blocks == (n + g - 1) // g and 9 <= cw <= 12
    batch = 64
    rows = [K.random_scalars(C, n, seed=600 + b) for b in range(3)]
    SB = np.concatenate([limbs(rows[b % 3]) for b in range(batch)])
    out, inf = ctx.msm_batch(SB, n, batch)  # the block table
    for b in range(3):
        assert pt(name, out[b], inf[b]) == K.commit_via_tau(C, tau, rows[b]), b
    assert (out[3:] == out[[b % 3 for b in range(3, batch)]]).all()
    outw, infw = ctx.msm_batch(SB, n, 3)  # below the threshold: the window table
    assert (outw == out[:3]).all() and not infw.any()
