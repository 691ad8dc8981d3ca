"""GPU tests of the per-cell verdicts (kzgx_verify_cells_each, its _device, _checked and _checked_device
forms): for every cell k of a batch
  ok[k] = e(pi_k, G2[l]) == e(C_(c_k) - [I_k(tau)]G1 + [a_(i_k)]pi_k, G2[0]).

Expected verdicts never come from the code under test: they are Cells.singles() of
test_gpu_verify_cells.py -- exponent arithmetic mod r with the golden tau on what is supplied, tampered or
not.  Every parametrised case expects at least one True and at least one False among its verdicts, so an
output of all zeros or all ones cannot pass."""
import numpy as np
import pytest

import corc
import kzg_ref as K
import kzgx
from test_gpu_verify_aggregate import scalars
from test_gpu_verify_cells import SHAPES, Cells, env, make_cells, single, tamper  # noqa: F401 (env: a fixture)

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NO_SRS, ERR_DEGREE = -1, -4, -5
EXT, BITREV = kzgx.PROVE_COSETS_EXTENDED, kzgx.NTT_BITREV
KINDS = ("value", "swap", "cell_index", "commit_index", "proof")


def each(ctx, b, checked=None):
    c, cf, ci, idx, p, pf, ys = b.arrays()
    kw = dict(commit_inf=cf, proof_inf=pf, extended=bool(b.ext), bitrev=bool(b.bitrev))
    if checked is None:
        got = ctx.verify_cells_each(c, ci, idx, p, ys, b.k, **kw)
    else:
        got = ctx.verify_cells_each_checked(c, ci, idx, p, ys, b.k, subgroup=checked, **kw)
    assert got.dtype == np.bool_ and got.shape == (len(b),)
    return got.tolist()


def tamper_many(b, spec):
    """several tamperings at once: spec = [(pos, kind), ...]; None where one of them has no room"""
    t = b
    for pos, kind in spec:
        t = tamper(t, pos, kind)
        if t is None:
            return None
    return t


def check_each(ctx, b):
    """the valid batch is all true; every tampering kind at the first, the middle and the last cell equals
    the exponent prediction element for element"""
    n = len(b)
    assert each(ctx, b) == [True] * n
    trues, falses = n, 0
    for pos in sorted({0, n // 2, n - 1}):
        for kind in KINDS:
            t = tamper(b, pos, kind)
            if t is None:
                continue
            want = t.singles()
            if kind in ("value", "proof"):
                assert not want[pos], (pos, kind)
            assert each(ctx, t) == want, (pos, kind)
            trues += want.count(True)
            falses += want.count(False)
    assert trues >= 1 and falses >= 1


# ---- 1. shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bitrev", [0, 1])
@pytest.mark.parametrize("k,kl,ext", SHAPES)
def test_shapes(env, k, kl, ext, bitrev):
    ctx, tau = env("BLS12381")
    check_each(ctx, make_cells("BLS12381", k, kl, ext, bitrev, 8 if kl >= 6 else 7, tau))


@pytest.mark.parametrize("bitrev", [0, 1])
@pytest.mark.parametrize("k,kl,ext", [(2, 1, 0), (1, 0, 1)])
def test_bn254(env, k, kl, ext, bitrev):
    ctx, tau = env("BN254")
    check_each(ctx, make_cells("BN254", k, kl, ext, bitrev, 7, tau))


# ---- 2. counts, several failures at once ------------------------------------------------------------------------
@pytest.mark.parametrize("bitrev", [0, 1])
@pytest.mark.parametrize("count", [1, 2, 3, 65, 300])
def test_counts(env, count, bitrev):
    """one cell to more than one workgroup of every kernel; from 65 cells on cell 3 opens the zero polynomial,
    cell 4 a constant (C' = O and pi = O) and cell 5 a polynomial of degree exactly l"""
    ctx, tau = env("BLS12381")
    b = make_cells("BLS12381", 4, 2, 1, bitrev, count, tau)
    n = len(b)
    assert each(ctx, b) == [True] * n
    specs = [[(0, "value")]]
    if n >= 2:
        specs.append([(0, "proof"), (n - 1, "value")])
    if n >= 3:
        specs.append([(0, "swap"), (n // 2, "cell_index"), (n - 1, "proof")])
    if n >= 65:
        specs.append([(3, "value"), (4, "proof"), (5, "value")])  # the three special cells
        specs.append([(3, "proof"), (4, "value"), (5, "commit_index")])
    falses = 0
    for spec in specs:
        t = tamper_many(b, spec)
        want = t.singles()
        assert want.count(False) >= len([s for s in spec if s[1] in ("value", "proof")])
        assert each(ctx, t) == want, spec
        falses += want.count(False)
    assert falses >= 1


# ---- 3. errors that cancel in the aggregate are two failures here -------------------------------------------------
@pytest.mark.parametrize("bitrev", [0, 1])
def test_cancelling_errors(env, bitrev):
    """make_cells makes the last cell repeat the first: +1 on the first proof exponent and -1 on the last
    cancel under equal challenges -- the aggregate is TRUE, both cells are false"""
    ctx, tau = env("BLS12381")
    b = make_cells("BLS12381", 4, 2, 1, bitrev, 7, tau)
    n, r = len(b), b.C.r
    assert (b.ci[0], b.idx[0], b.y[0]) == (b.ci[n - 1], b.idx[n - 1], b.y[n - 1])
    t = b.copy()
    t.p[0] = (t.p[0] + 1) % r
    t.p[n - 1] = (t.p[n - 1] - 1) % r
    assert t.aggregate([1] * n) is True
    c, cf, ci, idx, p, pf, ys = t.arrays()
    kw = dict(commit_inf=cf, proof_inf=pf, extended=True, bitrev=bool(bitrev))
    assert ctx.verify_cells_aggregate(c, ci, idx, p, ys, t.k, challenges=scalars([1] * n), **kw) is True
    want = [k not in (0, n - 1) for k in range(n)]
    assert t.singles() == want
    assert each(ctx, t) == want


# ---- 4. l = 512 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bitrev", [0, 1])
def test_cosets_larger_than_a_workgroup(bitrev):
    """l = 512 on a setup of exactly l G1 and l + 1 G2 points: all the entry needs"""
    name, C = "BLS12381", K.BLS12381
    tau = K.default_tau(C)
    b = make_cells(name, 10, 9, 1, bitrev, 3, tau)
    t = tamper(b, 1, "value")
    assert t.singles() == [True, False, True]
    ctx = kzgx.Context(name)
    try:
        ctx.set_default_table(0)
        ctx.gen_srs(tau, 512)
        ctx.gen_srs_g2(tau, 513)
        assert each(ctx, b) == [True, True, True]
        assert each(ctx, t) == [True, False, True]
    finally:
        ctx.close()


# ---- 5. chunks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,bad", [(300, (127, 128, 299)), (128, (0, 127))])
def test_chunks(env, count, bad):
    """128 cells per chunk: 300 cells are two whole chunks and a short one, 128 cells exactly one"""
    ctx, tau = env("BLS12381")
    b = make_cells("BLS12381", 4, 2, 1, 1, count, tau)
    t = tamper_many(b, [(pos, "value" if pos % 2 else "proof") for pos in bad])
    want = t.singles()
    assert [k for k, v in enumerate(want) if not v] == list(bad)
    default = each(ctx, t)
    try:
        ctx.set_verify_cells_chunk(128)
        chunked = each(ctx, t)
        chunked_checked = each(ctx, t, checked=True)
        assert each(ctx, b) == [True] * count
    finally:
        ctx.set_verify_cells_chunk(0)
    assert default == want and chunked == want and chunked_checked == want
    with pytest.raises(kzgx.KzgxError):
        ctx.set_verify_cells_chunk(65536)  # kzgx::msm_batch takes at most 65535 MSMs


# ---- 6. the two pairing kernels give the same booleans ---------------------------------------------------------------
@pytest.mark.parametrize("bitrev", [0, 1])
def test_wave_and_lane_paths_agree(env, bitrev):
    ctx, tau = env("BLS12381")
    b = make_cells("BLS12381", 4, 2, 1, bitrev, 65, tau)
    t = tamper_many(b, [(0, "value"), (3, "proof"), (4, "value"), (33, "cell_index"), (64, "proof")])
    want = t.singles()
    assert want.count(False) >= 4 and want.count(True) >= 50
    wave = each(ctx, t)
    try:
        ctx.set_verify_wave_max(0)  # every count takes the lane-per-opening kernel
        lane = each(ctx, t)
        lane_good = each(ctx, b)
    finally:
        ctx.set_verify_wave_max(8192)
    assert wave == want and lane == want and lane_good == [True] * 65


# ---- 7. kzgx_verify_proof gives the same boolean ---------------------------------------------------------------------
@pytest.mark.parametrize("bitrev", [0, 1])
def test_agrees_with_verify_proof(env, bitrev):
    ctx, tau = env("BLS12381")
    b = make_cells("BLS12381", 4, 2, 1, bitrev, 65, tau)
    t = tamper_many(b, [(0, "value"), (4, "proof"), (5, "swap"), (32, "commit_index"), (64, "cell_index")])
    got = each(ctx, t)
    assert got == t.singles() and False in got and True in got
    for j in (0, 1, 3, 4, 5, 32, 40, 64):
        assert single(ctx, t, j) is got[j], j


# ---- 8. the device entries on a caller's stream ----------------------------------------------------------------------
def dev_tensors(a, dev):
    """device copies of arrays(); the commitment and the value arrays get a spare trailing row"""
    import torch
    c, cf, ci, idx, p, pf, ys = a
    c = np.concatenate([c, np.zeros_like(c[:1])])
    cf = np.concatenate([cf, np.zeros_like(cf[:1])])
    ys = np.concatenate([ys, np.zeros_like(ys[:1])])
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.int32): np.int32}
    return [torch.from_numpy(np.ascontiguousarray(v).view(view[v.dtype])).to(dev) for v in (c, cf, ci, idx, p, pf, ys)]


@pytest.mark.parametrize("bitrev", [0, 1])
def test_device_entries_on_a_caller_stream(bitrev):
    """a fresh context and a fresh stream; d_ok is count words inside a buffer of 0xFFFFFFFF whose other
    words stay; an index out of range zeroes its own cell and nothing else"""
    import torch
    name, C = "BLS12381", K.BLS12381
    tau = K.default_tau(C)
    dev = torch.device("cuda", 0)
    good = make_cells(name, 4, 2, 1, bitrev, 65, tau)
    n = len(good)
    bad = tamper_many(good, [(40, "value"), (64, "proof")])
    oob_commit, oob_cell = bad.copy(), bad.copy()
    oob_commit.ci[33] = len(good.commits)
    oob_cell.idx[63] = good.R
    oob_cell.idx[0] = 0xFFFFFFFF

    def gated(b, zeroed):
        s = bad.singles()  # the oracle cannot name an index out of range: those cells are forced to 0
        return [v and k not in zeroed for k, v in enumerate(s)] if b is not good else [True] * n

    cases = [(good, None, gated(good, ())), (bad, None, gated(bad, ())), (oob_commit, None, gated(oob_commit, (33,))),
             (oob_cell, None, gated(oob_cell, (0, 63))), (good, True, gated(good, ())), (bad, False, gated(bad, ())),
             (oob_commit, True, gated(oob_commit, (33,))), (oob_cell, True, gated(oob_cell, (0, 63)))]
    keep, before, oks = [], [], []
    for b, _, _ in cases:
        t = dev_tensors(b.arrays(), dev)
        keep.append(t)
        before.append([x.clone() for x in t])
        oks.append(torch.full((n + 3,), -1, dtype=torch.int32, device=dev))
    ctx = kzgx.Context(name)
    try:
        ctx.set_default_table(0)
        ctx.gen_srs(tau, 8)
        ctx.gen_srs_g2(tau, 8)
        torch.cuda.synchronize(dev)
        st = torch.cuda.Stream(device=dev)
        for (b, checked, _), t, ok in zip(cases, keep, oks):
            c, cf, ci, idx, p, pf, ys = (x.data_ptr() for x in t)
            kw = dict(extended=True, bitrev=bool(bitrev), stream=st.cuda_stream)
            if checked is None:
                ctx.verify_cells_each_device(c, cf, len(b.commits), ci, idx, p, pf, ys, n, b.k, b.kl,
                                             ok[2:].data_ptr(), **kw)
            else:
                ctx.verify_cells_each_checked_device(c, cf, len(b.commits), ci, idx, p, pf, ys, n, b.k, b.kl, checked,
                                                     ok[2:].data_ptr(), **kw)
        st.synchronize()
        for (b, checked, want), ok in zip(cases, oks):
            assert ok.tolist() == [-1, -1] + [int(v) for v in want] + [-1], checked
        for t, t0 in zip(keep, before):
            assert all(bool((x == x0).all()) for x, x0 in zip(t, t0))  # the inputs are only read
        # the host forms: the same verdicts; the same indices are KZGX_ERR_ARG
        assert each(ctx, bad) == cases[1][2] and each(ctx, bad, checked=True) == cases[1][2]
        for b in (oob_commit, oob_cell):
            for checked in (None, True):
                with pytest.raises(kzgx.KzgxError) as e:
                    each(ctx, b, checked)
                assert e.value.status == ERR_ARG
    finally:
        ctx.close()


# ---- 9. the checked forms -------------------------------------------------------------------------------------------
def test_checked_forms(env):
    from test_gpu_subgroup import g1_rows
    from test_subgroup_consts import g1_member, g1_order_point
    ctx, tau = env("BLS12381")
    C = K.BLS12381
    good = make_cells("BLS12381", 4, 2, 1, 1, 9, tau)
    bad = tamper(good, 4, "value")
    oracle = bad.singles()
    assert oracle.count(False) == 1 and not oracle[4]
    for sg in (True, False):
        assert each(ctx, good, checked=sg) == [True] * 9
        assert each(ctx, bad, checked=sg) == oracle
    c, cf, ci, idx, p, pf, ys = bad.arrays()
    assert not pf[1] and not pf[2] and not pf[6]
    pts = corc.array_to_points("BLS12381", p)
    off_curve = (pts[1][0], (pts[1][1] + 1) % C.p)
    non_canon = (pts[2][0] + C.p, pts[2][1])
    non_member = K.point_add(C, pts[6], g1_order_point(3))
    assert not K.on_curve(C, off_curve) and K.on_curve(C, non_member) and not g1_member(C, non_member)
    px = p.copy()
    px[1], px[2], px[6] = g1_rows(C, [off_curve, non_canon, non_member])
    kw = dict(commit_inf=cf, proof_inf=pf, extended=True, bitrev=True)
    got = ctx.verify_cells_each_checked(c, ci, idx, px, ys, 4, subgroup=True, **kw).tolist()
    assert got == [v and k not in (1, 2, 6) for k, v in enumerate(oracle)]
    # without the subgroup test the non-member passes the check (its cell's answer is then not asserted)
    got = ctx.verify_cells_each_checked(c, ci, idx, px, ys, 4, subgroup=False, **kw).tolist()
    want = [v and k not in (1, 2) for k, v in enumerate(oracle)]
    assert got[:6] + got[7:] == want[:6] + want[7:]
    # an off-curve commitment zeroes exactly the cells that name it, under both settings
    cx = c.copy()
    pt = corc.array_to_points("BLS12381", c[1:2])[0]
    cx[1] = g1_rows(C, [(pt[0], (pt[1] + 1) % C.p)])[0]
    named = [k for k in range(9) if ci[k] == 1]
    assert 0 < len(named) < 9
    for sg in (True, False):
        got = ctx.verify_cells_each_checked(cx, ci, idx, p, ys, 4, subgroup=sg, **kw).tolist()
        assert got == [v and k not in named for k, v in enumerate(oracle)]


# ---- 10. statuses ---------------------------------------------------------------------------------------------------
def raw_host(ctx, a, log2n, log2l, flags, checked=False, drop=None, count=None, n_commits=None):
    """(status, ok array) of the host entry called directly (drop: the name of an argument passed as NULL)"""
    c, cf, ci, idx, p, pf, ys = (np.ascontiguousarray(v) for v in a)
    ok = np.full(p.shape[0] + 1, 7, dtype=np.int32)
    ptr = {"commits": kzgx._p(c), "commit_index": ci.ctypes.data_as(kzgx.u32p),
           "cell_index": idx.ctypes.data_as(kzgx.u32p), "proofs": kzgx._p(p), "ys": kzgx._p(ys),
           "ok": ok.ctypes.data_as(kzgx.intp)}
    if drop:
        ptr[drop] = None
    args = [ctx.h, ptr["commits"], cf.ctypes.data_as(kzgx.intp), c.shape[0] if n_commits is None else n_commits,
            ptr["commit_index"], ptr["cell_index"], ptr["proofs"], pf.ctypes.data_as(kzgx.intp), ptr["ys"],
            p.shape[0] if count is None else count, log2n, log2l, flags]
    if checked:
        return kzgx.lib().kzgx_verify_cells_each_checked(*args, 1, ptr["ok"]), ok.tolist()
    return kzgx.lib().kzgx_verify_cells_each(*args, ptr["ok"]), ok.tolist()


def raw_device(ctx, buf, log2n, log2l, flags, count=2, n_commits=2, checked=False, drop=None):
    """the status of the device entry on dummy device pointers: every refusal comes before anything is read"""
    ptr = {n: buf.data_ptr() for n in ("commits", "commit_index", "cell_index", "proofs", "ys", "ok")}
    if drop:
        ptr[drop] = None
    args = [ctx.h, ptr["commits"], None, n_commits, ptr["commit_index"], ptr["cell_index"], ptr["proofs"], None,
            ptr["ys"], count, log2n, log2l, flags]
    if checked:
        return kzgx.lib().kzgx_verify_cells_each_checked_device(*args, 1, ptr["ok"], None)
    return kzgx.lib().kzgx_verify_cells_each_device(*args, ptr["ok"], None)


def test_statuses(env):
    import torch
    ctx, tau = env("BLS12381")
    b = make_cells("BLS12381", 4, 2, 1, 0, 3, tau)
    a = b.arrays()
    buf = torch.zeros(4096, dtype=torch.int64, device=torch.device("cuda", 0))
    assert raw_host(ctx, a, 4, 2, EXT) == (0, [1, 1, 1, 7])
    for checked in (False, True):
        refused = [
            (4, 5, 0),                      # a coset larger than the domain
            (22, 2, EXT),                   # no 2^23 domain
            (23, 2, 0),
            (32, 2, 0),                     # log2n > 31
            (4, 2, EXT | 16),               # an unknown flag
            (4, 2, EXT | kzgx.NTT_INVERSE),
            (4, 2, EXT | kzgx.PROVE_ALL_EVALS),
        ]
        for log2n, log2l, flags in refused:
            assert raw_host(ctx, a, log2n, log2l, flags, checked)[0] == ERR_ARG, (log2n, log2l, flags)
            assert raw_device(ctx, buf, log2n, log2l, flags, checked=checked) == ERR_ARG, (log2n, log2l, flags)
        for drop in ("commits", "commit_index", "cell_index", "proofs", "ys", "ok"):
            assert raw_host(ctx, a, 4, 2, EXT, checked, drop=drop)[0] == ERR_ARG, drop
            assert raw_device(ctx, buf, 4, 2, EXT, checked=checked, drop=drop) == ERR_ARG, drop
        # limits: commitments, cells, n_commits + count + l, count x l values
        pmax = 1 << 22
        assert raw_host(ctx, a, 4, 0, 0, checked, count=0, n_commits=pmax + 1)[0] == ERR_ARG
        assert raw_device(ctx, buf, 4, 0, 0, count=pmax + 1, checked=checked) == ERR_ARG
        assert raw_host(ctx, a, 4, 0, 0, checked, count=0, n_commits=pmax)[0] == ERR_ARG
        assert raw_device(ctx, buf, 4, 0, 0, count=0, n_commits=pmax, checked=checked) == ERR_ARG
        assert raw_device(ctx, buf, 12, 12, 0, count=4097, checked=checked) == ERR_ARG
        # count == 0: OK, nothing written, and no commitment is needed
        assert raw_host(ctx, a, 4, 2, EXT, checked, count=0) == (0, [7, 7, 7, 7])
        assert raw_host(ctx, a, 4, 2, EXT, checked, count=0, n_commits=0, drop="commits") == (0, [7, 7, 7, 7])
        ok = torch.full((2,), 7, dtype=torch.int32, device=buf.device)
        args = [ctx.h, None, None, 0, None, None, None, None, None, 0, 4, 2, EXT]
        if checked:
            assert kzgx.lib().kzgx_verify_cells_each_checked_device(*args, 1, ok.data_ptr(), None) == 0
        else:
            assert kzgx.lib().kzgx_verify_cells_each_device(*args, ok.data_ptr(), None) == 0
        ctx.sync()
        assert ok.tolist() == [7, 7]
        # host-side index errors
        for field, v in (("ci", len(b.commits)), ("idx", b.R)):
            t = b.copy()
            getattr(t, field)[1] = v
            assert raw_host(ctx, t.arrays(), 4, 2, EXT, checked)[0] == ERR_ARG, field
    empty = Cells("BLS12381", 4, 2, 1, 0, tau, [], [], [], [], [])
    assert each(ctx, empty) == [] and each(ctx, empty, checked=True) == []
    assert kzgx.lib().kzgx_set_verify_cells_chunk(None, 0) == ERR_ARG
    # setups: none; G1 only; too few G2 points; too few G1 points
    bare = kzgx.Context("BLS12381")
    try:
        bare.set_default_table(0)
        assert raw_host(bare, a, 4, 2, EXT)[0] == ERR_NO_SRS
        assert raw_device(bare, buf, 4, 2, EXT) == ERR_NO_SRS
        bare.gen_srs(tau, 8)
        assert raw_host(bare, a, 4, 2, EXT)[0] == ERR_NO_SRS  # no G2 setup
        assert raw_device(bare, buf, 4, 2, EXT, checked=True) == ERR_NO_SRS
        bare.gen_srs_g2(tau, 4)
        assert raw_host(bare, a, 4, 2, EXT)[0] == ERR_NO_SRS  # l + 1 = 5 > 4 G2 points
        assert raw_device(bare, buf, 4, 2, EXT) == ERR_NO_SRS
        bare.gen_srs_g2(tau, 5)
        assert raw_host(bare, a, 4, 2, EXT) == (0, [1, 1, 1, 7])  # 8 >= l G1 points, 5 = l + 1 G2 points
        bare.gen_srs(tau, 3)
        assert raw_host(bare, a, 4, 2, EXT, True)[0] == ERR_DEGREE  # l = 4 > 3 G1 points
        assert raw_device(bare, buf, 4, 2, EXT) == ERR_DEGREE
        bare.gen_srs(tau, 4)
        assert raw_host(bare, a, 4, 2, EXT) == (0, [1, 1, 1, 7])  # exactly l G1 points: 2^log2n exceeds the SRS
        # a new G2 setup drops the staged G2[0] || G2[l] and its line tables: another tau refuses every cell
        bare.gen_srs_g2((tau + 1) % K.BLS12381.r, 5)
        assert raw_host(bare, a, 4, 2, EXT) == (0, [0, 0, 0, 7])
        bare.gen_srs_g2(tau, 5)
        assert raw_host(bare, a, 4, 2, EXT) == (0, [1, 1, 1, 7])
    finally:
        bare.close()
