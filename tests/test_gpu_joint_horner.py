"""GPU parity of the block-table MSM's Horner pass (csrc/joint_horner.hip):
stage 1 folds segments of JOINT_SEG planes in lone lanes, stage 2 folds the
segment sums in one 8-lane cooperative group per MSM (coop.hpp), 8 groups per
workgroup.

The pass's shape depends on the planes (254 on BN254, 255 on BLS12-381: the
short top segment differs), the block ranges R and the batch alone, so the
table is tiny: forced g = 5 inside the c = 8 footprint, n_t <= 40.  Every
output is compared with the CPU oracle's naive per-term MSM, with
[P(tau)]G1, or with the point at infinity.

Batches 1, 7, 8, 9, 65: part of, all of and one more than a workgroup's 8
groups, and a last workgroup with one live group.  Ranges 1, 2, 4, and
n_use <= g where R clamps to the one block.  One-point MSMs make every plane
sum +-P; a degenerate SRS (tau = 1: every point G; -1; 0) makes plane and
segment sums equal, opposite or infinite, which drives the cooperative
addition's infinity operands, its doubling and cancel branches and the
cooperative doubling of O."""
import functools
import os
import sys

import numpy as np
import pytest

import kzg_ref as K

pytestmark = pytest.mark.gpu

CURVES = [("BN254", K.BN254), ("BLS12381", K.BLS12381)]
C_REQ = 8
G = 5
N_T = 37  # 8 blocks, the last of 2 points
BATCHES = (1, 7, 8, 9, 65)
SEG = 16  # joint_horner.hip's JOINT_SEG: the patterned scalars repeat with this period


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


def patterned(C, word):
    """an odd scalar whose recoded digit pattern (the bits of k >> 1) repeats
    with period SEG below the top segment: every full segment sum of a
    one-point MSM is the same multiple of P"""
    u = 0
    for s in range(240 // SEG):
        u |= word << (SEG * s)
    k = 2 * u + 1
    assert k < C.r
    return k


def build(ctx, n_t, g=G):
    ctx.set_fixed_joint(g)
    ctx.set_fixed_base(C_REQ, n_t)
    assert ctx.fixed_joint_info()[:2] == (g, (n_t + g - 1) // g)


def check_batch(ctx, name, rows, n_use, exp, tag):
    SB = np.concatenate([limbs(r[:n_use]) for r in rows])
    out, inf = ctx.msm_batch(SB, n_use, len(rows))
    for b in range(len(rows)):
        assert pt(name, out[b], inf[b]) == exp[b], (tag, b)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the SRS, 65 rows of N_T scalars (the edge scalars moving through the
    blocks, one repeated row) and their naive MSMs over all N_T and over the
    first G points: computed once per curve, read by every case"""
    import corc
    corc.build()
    C = dict(CURVES)[name]
    srs = corc.gen_srs(name, K.default_tau(C), N_T)
    rows = []
    for b in range(max(BATCHES)):
        row = K.random_scalars(C, N_T, seed=31000 + b)
        for j, v in enumerate(edge_scalars(C)):
            row[(j * 7 + b) % N_T] = v
        rows.append(row)
    rows[6] = list(rows[2])
    full = [corc.msm_naive(name, srs, limbs(r)) for r in rows]
    head = [corc.msm_naive(name, srs[:G], limbs(r[:G])) for r in rows[:9]]
    return srs, rows, full, head


@pytest.mark.parametrize("name,C", CURVES)
@pytest.mark.parametrize("ranges", [1, 2, 4])
def test_horner_batches_and_ranges(name, C, ranges, fresh_ctx):
    srs, rows, full, head = reference(name)
    ctx = fresh_ctx(name)
    ctx.load_srs(srs)
    build(ctx, N_T)
    ctx.set_fixed_joint_ranges(ranges)
    for batch in BATCHES:
        check_batch(ctx, name, rows[:batch], N_T, full, (ranges, batch))
    # n_use <= g: one block, R clamps to 1 whatever was set
    check_batch(ctx, name, rows[:9], G, head, (ranges, "n_use = g"))


@pytest.mark.parametrize("name,C", CURVES)
@pytest.mark.parametrize("n_t", [1, N_T])
def test_horner_one_point_edge_and_patterned_scalars(name, C, n_t, fresh_ctx, oracle_c):
    """one-point MSMs.  Over a one-point table (n_t = 1) every plane sum is +P
    or -P; over the 37-point table the block's other points run as scalar 0.
    Scalar 0 runs as r and reaches O only at the end of the chain; the
    patterned scalars give equal segment sums below the top segment."""
    srs = reference(name)[0]
    ctx = fresh_ctx(name)
    ctx.load_srs(srs)
    build(ctx, n_t)
    sc = edge_scalars(C) + [patterned(C, 0xFFFF), patterned(C, 0x0000), patterned(C, 0xA5C3), patterned(C, 0x0001), 2]
    exp = [oracle_c.msm_naive(name, srs[:1], limbs([v])) for v in sc]
    assert exp[0] is None and exp[1] is not None
    for ranges in (1, 4):
        ctx.set_fixed_joint_ranges(ranges)
        check_batch(ctx, name, [[v] for v in sc], 1, exp, (n_t, ranges))
        for k, v in enumerate(sc[:3]):  # batch 1: a workgroup with one live group
            check_batch(ctx, name, [[v]], 1, exp[k:k + 1], (n_t, ranges, "single", k))


@pytest.mark.parametrize("name,C", CURVES)
def test_horner_all_points_equal(name, C, fresh_ctx, oracle_c):
    """tau = 1: every SRS point is G.  n = 2: scalars (k, r - k) make every
    plane sum O and the result O (the whole chain on the point at infinity);
    (k, k) makes the plane sums +-2G; rows of both kinds share a batch.
    n = 2 g with two ranges: the same scalars in both blocks make the two
    ranges' segment sums equal (the cooperative addition's doubling branch),
    opposite scalars make them cancel in every segment, so the doublings that
    follow run on O and the next addition meets an infinite operand."""
    n_t = 2 * G
    srs = oracle_c.gen_srs(name, 1, n_t)
    ctx = fresh_ctx(name)
    ctx.load_srs(srs)
    build(ctx, n_t)
    ks = [12345, 2, C.r - 1, patterned(C, 0x5A3C), K.random_scalars(C, 1, seed=77)[0]]
    rows = []
    for k in ks:
        rows.append([k, (C.r - k) % C.r])
        rows.append([k, k])
    exp = [oracle_c.msm_naive(name, srs[:2], limbs(r)) for r in rows]
    assert all(e is None for e in exp[0::2]) and all(e is not None for e in exp[1::2])
    for ranges in (1, 2):
        ctx.set_fixed_joint_ranges(ranges)
        check_batch(ctx, name, rows, 2, exp, ("n = 2", ranges))
        check_batch(ctx, name, rows[:1], 2, exp[:1], ("n = 2, batch 1", ranges))
    lo = K.random_scalars(C, G, seed=78)
    lo[1], lo[3] = 0, C.r - 2
    rows = [lo + lo, lo + [(C.r - v) % C.r for v in lo], lo + [1] * G]
    rows = rows * 3  # batch 9
    exp = [oracle_c.msm_naive(name, srs, limbs(r)) for r in rows[:3]] * 3
    assert exp[1] is None and exp[0] is not None
    for ranges in (1, 2, 4):
        ctx.set_fixed_joint_ranges(ranges)
        check_batch(ctx, name, rows, n_t, exp, ("n = 2 g", ranges))


@pytest.mark.parametrize("name,C", CURVES)
@pytest.mark.parametrize("tau", [0, -1])
def test_horner_degenerate_srs(name, C, tau, fresh_ctx, oracle_c):
    """tau = 0: infinite SRS points and whole blocks of entries at infinity;
    tau = -1: alternating G, -G.  Batch 9 (a second workgroup with one live
    group), a repeated row and a row that cancels exactly."""
    t = tau % C.r
    srs = oracle_c.gen_srs(name, t, N_T)
    ctx = fresh_ctx(name)
    ctx.load_srs(srs)
    build(ctx, N_T)
    rows = [K.random_scalars(C, N_T, seed=150 + b) for b in range(9)]
    rows[2] = list(rows[1])
    z = [0] * N_T
    if tau == -1:
        z[0], z[1] = 12345, 12345  # s G + s (-G)
    rows[8] = z
    exp = [oracle_c.msm_naive(name, srs, limbs(r)) for r in rows]
    assert exp[8] is None
    for ranges in (1, 2):
        ctx.set_fixed_joint_ranges(ranges)
        check_batch(ctx, name, rows, N_T, exp, (tau, ranges))
    out1, inf1 = ctx.msm(limbs(rows[0]))
    assert pt(name, out1, inf1) == K.commit_via_tau(C, t, rows[0])


def _bench():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench
    return bench


@pytest.mark.parametrize("name,C", CURVES)
def test_horner_interleaved_streams(name, C, fresh_ctx):
    """steps of two batch sizes (9 and 3: a second workgroup with one live
    group, and part of one) interleaved on two streams of one context as the
    bench enqueues them (bench.make_step: proofs, then commits), so each
    stream's segment-sum workspace serves both sizes in turn; every output
    checked as bench.check_step checks"""
    import torch
    bench = _bench()
    ctx = fresh_ctx(name)
    tau = K.default_tau(C)
    n = 40
    ctx.gen_srs(tau, n)
    build(ctx, n)
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    work = []
    for B in (9, 3):
        coeffs, zs = bench.bench_inputs(C, "cfg2", B, n)
        coeffs[1] = 0  # zero polynomial: commit and proof at infinity
        bufs = bench.StepBuffers(torch, dev, coeffs, zs, ctx.w64)
        work.append((B, coeffs, zs, bufs, bench.make_step(ctx, "cfg2", n, bufs, streams)))
    torch.cuda.synchronize(dev)
    for _ in range(3):
        for w in work:
            w[4]()
    torch.cuda.synchronize(dev)
    for B, coeffs, zs, bufs, _ in work:
        checked, ok, bad = bench.check_step(name, C, tau, "cfg2", coeffs, zs, bufs, ctx.w64)
        assert checked == 3 * B and ok == checked, (B, bad)
