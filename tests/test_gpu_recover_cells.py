"""GPU: cell recovery (kzgx_recover_cells / _device / _and_proofs / _and_proofs_device, csrc/recover.hip):
polynomials of n coefficients rebuilt from any half of the R cells of their size-2n domain.

Checker: the truth is the polynomial's own extended evaluations by the oracle's Horner (K.poly_eval) at the
points kzgx.coset_points lists, and its coefficients; out_y and out_coeffs are compared limb for limb.  The
large shapes are compared byte for byte with prove_cosets(coeffs, extended=True, bitrev=True), which its own
tests pin to the oracle."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import kzg_ref as K
import kzgx
from test_gpu_prove_cosets import perm, polys, to_limbs

pytestmark = pytest.mark.gpu

BLS = K.BLS12381
ERR_ARG, ERR_NO_SRS, ERR_DEGREE = -1, -4, -5
POISON = 0x5A5A5A5AA5A5A5A5
EXT = kzgx.PROVE_COSETS_EXTENDED


def from_limbs(x) -> int:
    return sum(int(x[i]) << (64 * i) for i in range(4))


def horner(curve, P, k, kl):
    """the (R, l, 4) extended evaluations of P in natural coset order, point by point"""
    C = K.CURVES[curve]
    rows = []
    for i in range(1 << (k + 1 - kl)):
        xs = kzgx.coset_points(curve, k, kl, i, extended=True)
        rows.append(to_limbs([K.poly_eval(C, list(P), from_limbs(x)) for x in xs]))
    return np.stack(rows)


@functools.lru_cache(maxsize=None)
def case(k, kl):
    """-> coefficients (3, n, 4) and the natural-order values (3, R, l, 4) of test_gpu_prove_cosets.polys(k)"""
    ps = polys(k)
    return np.stack([to_limbs(P) for P in ps]), np.stack([horner("BLS12381", P, k, kl) for P in ps])


def cells(y, kr, kl):
    """natural coset order (.., R, l, 4) -> the cells of the bit-reversed evaluation array"""
    return y[..., perm(kr), :, :][..., perm(kl), :]


def flat(y, keep, order=None):
    """y (batch, R, l, 4) and keep[b] = the cell numbers of blob b -> (blob_index, cell_index, ys), blob by
    blob, or permuted by order"""
    bi = np.concatenate([np.full(len(kp), b, dtype=np.uint32) for b, kp in enumerate(keep)])
    ci = np.concatenate([np.asarray(kp, dtype=np.uint32) for kp in keep])
    ys = np.concatenate([y[b][np.asarray(kp, dtype=np.int64)] for b, kp in enumerate(keep)])
    if order is not None:
        bi, ci, ys = bi[order], ci[order], ys[order]
    return bi, ci, np.ascontiguousarray(ys)


@pytest.fixture(scope="module")
def ctx():
    c = kzgx.Context("BLS12381")
    c.set_default_table(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bare():
    """a context that never gets an SRS: the plain forms need none"""
    c = kzgx.Context("BLS12381")
    yield c
    c.close()


def half(R, b=0):
    """a seeded random set of exactly R / 2 cells"""
    return np.sort(np.random.default_rng(0x7EC0 + 131 * R + b).permutation(R)[:R // 2])


# ---- 1. against the independent reference: both orders, batch 1 and 3 -------------------------------------------
SHAPES = [(1, 0), (1, 1), (2, 1), (3, 0), (3, 3), (4, 2), (5, 2)]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("k,kl", SHAPES)
def test_against_horner(bare, k, kl, batch):
    kr = k + 1 - kl
    R = 1 << kr
    coeffs, y = (x[3 - batch:] for x in case(k, kl))  # the polynomial with 0, 1, r - 1 is always in
    keep = [half(R, b) for b in range(batch)]
    for rev in (False, True):
        yy = cells(y, kr, kl) if rev else y
        oy, oc, ok = bare.recover_cells(*flat(yy, keep), batch, k, bitrev=rev)
        assert ok.all()
        assert (oy == yy).all() and (oc == coeffs).all()
        oy2, none, ok = bare.recover_cells(*flat(yy, keep), batch, k, bitrev=rev, want_coeffs=False)
        assert none is None and ok.all() and (oy2 == yy).all()
        none, oc2, ok = bare.recover_cells(*flat(yy, keep), batch, k, bitrev=rev, want_y=False)
        assert none is None and ok.all() and (oc2 == coeffs).all()


# ---- 2. erasure patterns -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("k,kl", [(4, 2), (5, 2)])
def test_erasure_patterns(bare, k, kl, rev):
    kr = k + 1 - kl
    R = 1 << kr
    coeffs, y = case(k, kl)
    yy = cells(y, kr, kl) if rev else y
    every = np.arange(R)
    patterns = {
        "nothing missing": every,
        "first half missing": every[R // 2:],
        "second half missing": every[:R // 2],
        # Zs = Y^(R/2) - 1; bit-reversed, the odd cosets that stay are the chunks with the top bit set
        "even cosets missing": every[R // 2:] if rev else every[1::2],
        "random half": half(R),
        "one missing": np.delete(every, 3),
    }
    if rev:
        assert all(perm(kr)[p] % 2 == 1 for p in patterns["even cosets missing"])
    for name, kp in patterns.items():
        oy, oc, ok = bare.recover_cells(*flat(yy[:1], [kp]), 1, k, bitrev=rev)
        assert ok.all() and (oy == yy[:1]).all() and (oc == coeffs[:1]).all(), name
    # a different pattern and a different count per blob in one call
    keep = [every[R // 2:], np.delete(every, [1, R - 1]), half(R, 9)]
    oy, oc, ok = bare.recover_cells(*flat(yy, keep), 3, k, bitrev=rev)
    assert ok.all() and (oy == yy).all() and (oc == coeffs).all()
    # the flat list shuffled, the blobs interleaved
    total = sum(len(kp) for kp in keep)
    order = np.random.default_rng(0x5F1E + k).permutation(total)
    assert len(set(flat(yy, keep, order)[0][:6].tolist())) > 1
    oy, oc, ok = bare.recover_cells(*flat(yy, keep, order), 3, k, bitrev=rev)
    assert ok.all() and (oy == yy).all() and (oc == coeffs).all()


# ---- 3. transform paths: the one-pass transform's largest size, the two-pass one, the cell cap ------------------
@pytest.mark.parametrize("k,kl,batch", [(11, 5, 1), (12, 6, 2)])
def test_transform_paths(ctx, k, kl, batch):
    n, tau, kr = 1 << k, K.default_tau(BLS), k + 1 - kl
    R = 1 << kr
    ctx.gen_srs(tau, n)
    coeffs = np.stack([to_limbs(K.random_scalars(BLS, n, 0x2EC + 16 * k + b)) for b in range(batch)])
    xy, inf, y = ctx.prove_cosets(coeffs, kl, extended=True, bitrev=True)
    keep = [half(R, b) for b in range(batch)]
    oy, oc, ok = ctx.recover_cells(*flat(y, keep), batch, k, bitrev=True)
    assert ok.all() and oy.tobytes() == y.tobytes() and oc.tobytes() == coeffs.tobytes()
    oy, oc, pxy, pinf, ok = ctx.recover_cells_and_proofs(*flat(y, keep), batch, k, bitrev=True, want_coeffs=False)
    assert ok.all() and oc is None and oy.tobytes() == y.tobytes()
    assert pxy.tobytes() == xy.tobytes() and (pinf == inf).all()


def test_cell_cap(bare):
    k, kl = 11, 0  # R = 4096 = the cap, l = 1
    R = 1 << (k + 1)
    coeffs = to_limbs(K.random_scalars(BLS, 1 << k, 0xCA9))
    y = bare.ntt(np.concatenate([coeffs, np.zeros_like(coeffs)])).reshape(1, R, 1, 4)
    oy, oc, ok = bare.recover_cells(*flat(y, [half(R)]), 1, k)
    assert ok.all() and (oy == y).all() and (oc[0] == coeffs).all()
    with pytest.raises(kzgx.KzgxError) as e:  # R = 8192
        bare.recover_cells(np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.zeros((1, 1, 4), np.uint64), 1, 12)
    assert e.value.status == ERR_ARG


# ---- 4. round trip through the aggregated cell verification ------------------------------------------------------
def test_round_trip_verifies(ctx):
    k, kl, batch = 5, 2, 2
    n, l, tau, kr = 1 << k, 1 << kl, K.default_tau(BLS), k + 1 - kl
    R = 1 << kr
    ctx.gen_srs(tau, n)
    ctx.gen_srs_g2(tau, l + 1)
    coeffs, y = (x[:batch] for x in case(k, kl))
    yy = cells(y, kr, kl)
    oy, oc, pxy, pinf, ok = ctx.recover_cells_and_proofs(*flat(yy, [half(R, b) for b in range(batch)]), batch, k,
                                                         bitrev=True)
    assert ok.all() and (oy == yy).all()
    commits = np.stack([ctx.msm(oc[b])[0] for b in range(batch)])
    ci = np.repeat(np.arange(batch, dtype=np.uint32), R)
    ki = np.tile(np.arange(R, dtype=np.uint32), batch)
    r = to_limbs(K.random_scalars(BLS, batch * R, 0xC4A1))
    args = (commits, ci, ki, pxy.reshape(batch * R, -1), oy.reshape(batch * R, l, 4), k)
    assert ctx.verify_cells_aggregate(*args, challenges=r, proof_inf=pinf.reshape(-1), extended=True, bitrev=True)
    bad = oy.reshape(batch * R, l, 4).copy()
    bad[R + 1, 0, 0] ^= 1
    assert not ctx.verify_cells_aggregate(*args[:4], bad, k, challenges=r, proof_inf=pinf.reshape(-1),
                                          extended=True, bitrev=True)


# ---- 5. inconsistent input ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rev", [False, True])
def test_inconsistent_cells(ctx, rev):
    k, kl = 4, 2
    n, tau, kr = 1 << k, K.default_tau(BLS), k + 1 - kl
    R = 1 << kr
    ctx.gen_srs(tau, n)
    coeffs, y = (x[:2] for x in case(k, kl))
    yy = cells(y, kr, kl) if rev else y
    keep = [np.sort(np.append(half(R, 0), [c for c in range(R) if c not in half(R, 0)][0])), half(R, 1)]
    assert len(keep[0]) == R // 2 + 1
    bi, ci, ys = flat(yy, keep)
    ys[2, 1] = to_limbs([(from_limbs(ys[2, 1]) + 1) % BLS.r])[0]  # one value of blob 0 off by one
    before = ys.copy()
    oy, oc, pxy, pinf, ok = ctx.recover_cells_and_proofs(bi, ci, ys, 2, k, bitrev=rev)
    assert (ys == before).all()
    assert ok.tolist() == [False, True]
    assert not oy[0].any() and not oc[0].any() and pinf[0].all()
    assert (oy[1] == yy[1]).all() and (oc[1] == coeffs[1]).all()
    want = ctx.prove_cosets(coeffs[1], kl, extended=True, bitrev=rev, want_y=False)
    assert (pxy[1] == want[0]).all() and (pinf[1] == want[1]).all()
    # exactly R / 2 cells: every input is consistent, and the output agrees with what was supplied
    bi, ci, ys = flat(yy[:1], [half(R, 0)])
    ys[2, 1] = to_limbs([(from_limbs(ys[2, 1]) + 1) % BLS.r])[0]
    oy, oc, ok = ctx.recover_cells(bi, ci, ys, 1, k, bitrev=rev)
    assert ok.all() and (oy[0][ci] == ys).all() and not (oy[0] == yy[0]).all()


# ---- 6. device forms -------------------------------------------------------------------------------------------------
def run_device(c, bi, ci, ys, n_blobs, k, kl, rev, proofs=False, stream=None, with_y=True, with_coeffs=True):
    n, l, R, w, pad = 1 << k, 1 << kl, 1 << (k + 1 - kl), 2 * c.w64, 4
    d_bi = torch.from_numpy(bi.astype(np.int32)).cuda()
    d_ci = torch.from_numpy(ci.astype(np.int32)).cuda()
    d_ys = torch.from_numpy(ys.view(np.int64)).cuda()
    befores = (d_bi.clone(), d_ci.clone(), d_ys.clone())
    d_y = torch.full((n_blobs * R * l + 2 * pad, 4), POISON, dtype=torch.int64, device="cuda")
    d_c = torch.full((n_blobs * n + 2 * pad, 4), POISON, dtype=torch.int64, device="cuda")
    d_ok = torch.full((n_blobs + 2 * pad,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_xy = torch.full((n_blobs * R + 2 * pad, w), POISON, dtype=torch.int64, device="cuda")
    d_inf = torch.full((n_blobs * R + 2 * pad,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    head = (d_bi.data_ptr(), d_ci.data_ptr(), d_ys.data_ptr(), len(bi), n_blobs, k, kl,
            d_y[pad:].data_ptr() if with_y else None, d_c[pad:].data_ptr() if with_coeffs else None)
    if proofs:
        c.recover_cells_and_proofs_device(*head, d_xy[pad:].data_ptr(), d_inf[pad:].data_ptr(),
                                          d_ok[pad:].data_ptr(), bitrev=rev, stream=stream)
    else:
        c.recover_cells_device(*head, d_ok[pad:].data_ptr(), bitrev=rev, stream=stream)
    torch.cuda.synchronize()
    for d, b in zip((d_bi, d_ci, d_ys), befores):
        assert torch.equal(d, b), "input changed"
    oy, oc, ok, xy, inf = (t.cpu().numpy() for t in (d_y, d_c, d_ok, d_xy, d_inf))
    for arr, cnt, poison in ((oy, n_blobs * R * l, POISON), (oc, n_blobs * n, POISON), (ok, n_blobs, 0x5A5A5A5A),
                             (xy, n_blobs * R, POISON), (inf, n_blobs * R, 0x5A5A5A5A)):
        assert (arr[:pad] == poison).all() and (arr[pad + cnt:] == poison).all()
    if not with_y:
        assert (oy == POISON).all()
    if not with_coeffs:
        assert (oc == POISON).all()
    if not proofs:
        assert (xy == POISON).all() and (inf == 0x5A5A5A5A).all()
    return (oy[pad:pad + n_blobs * R * l].view(np.uint64).reshape(n_blobs, R, l, 4),
            oc[pad:pad + n_blobs * n].view(np.uint64).reshape(n_blobs, n, 4), ok[pad:pad + n_blobs],
            xy[pad:pad + n_blobs * R].view(np.uint64).reshape(n_blobs, R, w),
            inf[pad:pad + n_blobs * R].reshape(n_blobs, R))


@pytest.mark.parametrize("rev", [False, True])
def test_device_forms_match_host(ctx, rev):
    k, kl = 5, 2
    kr = k + 1 - kl
    R = 1 << kr
    ctx.gen_srs(K.default_tau(BLS), 1 << k)
    coeffs, y = case(k, kl)
    yy = cells(y, kr, kl) if rev else y
    keep = [half(R, 0), np.delete(np.arange(R), 5), half(R, 2)]
    order = np.random.default_rng(0xD0).permutation(sum(len(kp) for kp in keep))
    bi, ci, ys = flat(yy, keep, order)
    hy, hc, hxy, hinf, hok = ctx.recover_cells_and_proofs(bi, ci, ys, 3, k, bitrev=rev)
    assert hok.all() and (hy == yy).all()
    oy, oc, ok, xy, inf = run_device(ctx, bi, ci, ys, 3, k, kl, rev, proofs=True)
    assert (ok == 1).all() and (oy == hy).all() and (oc == hc).all() and (xy == hxy).all()
    assert (inf.astype(bool) == hinf).all()
    oy, oc, ok, _, _ = run_device(ctx, bi, ci, ys, 3, k, kl, rev)
    assert (ok == 1).all() and (oy == hy).all() and (oc == hc).all()
    oy, _, ok, _, _ = run_device(ctx, bi, ci, ys, 3, k, kl, rev, with_coeffs=False)
    assert (ok == 1).all() and (oy == hy).all()
    _, oc, ok, _, _ = run_device(ctx, bi, ci, ys, 3, k, kl, rev, with_y=False)
    assert (ok == 1).all() and (oc == hc).all()
    _, _, ok, xy, inf = run_device(ctx, bi, ci, ys, 3, k, kl, rev, proofs=True, with_y=False, with_coeffs=False)
    assert (ok == 1).all() and (xy == hxy).all()


def test_device_refusals_are_flags(bare):
    k, kl = 4, 2
    kr = k + 1 - kl
    R = 1 << kr
    coeffs, y = case(k, kl)
    keep = [half(R, 0), half(R, 1), half(R, 2)]
    # blob 1 one cell short
    short = [keep[0], keep[1][:-1], keep[2]]
    oy, oc, ok, _, _ = run_device(bare, *flat(y, short), 3, k, kl, False)
    assert ok.tolist() == [1, 0, 1] and not oy[1].any() and not oc[1].any()
    assert (oy[[0, 2]] == y[[0, 2]]).all() and (oc[[0, 2]] == coeffs[[0, 2]]).all()
    # blob 2 names a cell twice (R / 2 + 1 entries, R / 2 distinct)
    bi, ci, ys = flat(y, keep)
    bi, ci, ys = np.append(bi, 2).astype(np.uint32), np.append(ci, keep[2][0]).astype(np.uint32), np.concatenate(
        [ys, y[2][keep[2][:1]]])
    oy, oc, ok, _, _ = run_device(bare, bi, ci, ys, 3, k, kl, False)
    assert ok.tolist() == [1, 1, 0] and not oy[2].any() and (oy[:2] == y[:2]).all()
    # a cell index past R marks its blob, a blob index past n_blobs the whole call; nothing is read out of bounds
    # (blob 0 still has R / 2 good cells: one more is appended for the one whose index is spoilt)
    bi, ci, ys = flat(y, keep)
    spare = [c for c in range(R) if c not in keep[0]][0]
    bi2, ci2 = np.append(bi, 0).astype(np.uint32), np.append(ci, spare).astype(np.uint32)
    ys2 = np.concatenate([ys, y[0][[spare]]])
    ci2[0] = R
    oy, oc, ok, _, _ = run_device(bare, bi2, ci2, ys2, 3, k, kl, False)
    assert ok.tolist() == [0, 1, 1] and not oy[0].any() and (oy[1:] == y[1:]).all()
    bi4 = bi.copy()
    bi4[-1] = 3
    oy, oc, ok, _, _ = run_device(bare, bi4, ci, ys, 3, k, kl, False)
    assert ok.tolist() == [0, 0, 0] and not oy.any() and not oc.any()
    bi4[-1] = 0xFFFFFFFF
    oy, oc, ok, _, _ = run_device(bare, bi4, ci, ys, 3, k, kl, False)
    assert ok.tolist() == [0, 0, 0] and not oy.any()


def test_a_second_stream():
    k, kl = 5, 2
    kr = k + 1 - kl
    R = 1 << kr
    coeffs, y = case(k, kl)
    yy = cells(y, kr, kl)
    c = kzgx.Context("BLS12381")
    try:
        c.set_default_table(0)
        keep = [half(R, b) for b in range(3)]
        st = torch.cuda.Stream()
        oy, oc, ok, _, _ = run_device(c, *flat(yy, keep), 3, k, kl, True, stream=st.cuda_stream)  # tables built on st
        assert (ok == 1).all() and (oy == yy).all() and (oc == coeffs).all()
        st2 = torch.cuda.Stream()
        oy, oc, ok, _, _ = run_device(c, *flat(y, keep), 3, k, kl, False, stream=st2.cuda_stream)
        assert (ok == 1).all() and (oy == y).all() and (oc == coeffs).all()
        oy, oc, ok = c.recover_cells(*flat(y, keep), 3, k)  # the context's stream, behind the builds
        assert ok.all() and (oy == y).all()
    finally:
        c.close()


def test_more_blobs_than_a_chunk(bare):
    k, kl = 3, 1
    R = 1 << (k + 1 - kl)
    coeffs, y = case(k, kl)
    batch = (kzgx.RECOVER_CHUNK_SCALARS >> (k + 1)) + 1
    idx = np.arange(batch) % 3
    idx[-1] = 2
    pats = np.stack([half(R, j) for j in range(5)])[np.arange(batch) % 5]  # (batch, R / 2) cell numbers
    bi = np.repeat(np.arange(batch, dtype=np.uint32), R // 2)
    ci = pats.reshape(-1).astype(np.uint32)
    order = np.random.default_rng(0xC4).permutation(batch * (R // 2))
    bi, ci = bi[order], ci[order]
    oy, oc, ok = bare.recover_cells(bi, ci, y[idx][bi, ci], batch, k)
    assert ok.all() and (oy == y[idx]).all() and (oc == coeffs[idx]).all()


# ---- 7. statuses -----------------------------------------------------------------------------------------------------
def test_statuses(ctx, bare):
    k, kl = 3, 1
    R = 1 << (k + 1 - kl)
    ctx.gen_srs(K.default_tau(BLS), 8)
    coeffs, y = case(k, kl)
    bi, ci, ys = flat(y[:1], [half(R)])
    cnt = len(bi)
    f_ = kzgx.lib().kzgx_recover_cells_device
    g_ = kzgx.lib().kzgx_recover_cells_and_proofs_device
    d_bi = torch.from_numpy(bi.astype(np.int32)).cuda()
    d_ci = torch.from_numpy(ci.astype(np.int32)).cuda()
    d_ys = torch.from_numpy(ys.view(np.int64)).cuda()
    d_y = torch.zeros((2 << k, 4), dtype=torch.int64, device="cuda")
    d_c = torch.zeros((1 << k, 4), dtype=torch.int64, device="cuda")
    d_ok = torch.zeros((4,), dtype=torch.int32, device="cuda")
    d_xy = torch.zeros((R, 12), dtype=torch.int64, device="cuda")
    d_inf = torch.zeros((R,), dtype=torch.int32, device="cuda")
    a, b, s, py, pc, pk, px, pf = (t.data_ptr() for t in (d_bi, d_ci, d_ys, d_y, d_c, d_ok, d_xy, d_inf))
    assert f_(ctx.h, a, b, s, cnt, 1, k, kl, EXT, py, pc, pk, None) == 0
    assert f_(ctx.h, a, b, s, cnt, 1, k, kl, EXT | kzgx.NTT_BITREV, py, None, pk, None) == 0
    assert f_(ctx.h, None, None, None, 0, 0, k, kl, EXT, None, None, None, None) == 0  # n_blobs == 0
    assert f_(ctx.h, a, b, s, cnt, 1, k, kl, 0, py, pc, pk, None) == ERR_ARG  # EXTENDED missing
    assert f_(ctx.h, a, b, s, cnt, 1, k, kl, kzgx.NTT_BITREV, py, pc, pk, None) == ERR_ARG
    assert f_(ctx.h, a, b, s, cnt, 1, k, kl, EXT | 16, py, pc, pk, None) == ERR_ARG  # unknown flag
    assert f_(ctx.h, a, b, s, cnt, 1, k, kl, EXT | kzgx.NTT_INVERSE, py, pc, pk, None) == ERR_ARG
    assert f_(ctx.h, a, b, s, cnt, 1, k, kl, EXT | kzgx.PROVE_ALL_EVALS, py, pc, pk, None) == ERR_ARG
    assert f_(ctx.h, a, b, s, cnt, 1, 3, 4, EXT, py, pc, pk, None) == ERR_ARG  # l > n
    assert f_(ctx.h, a, b, s, cnt, 1, 22, 12, EXT, py, pc, pk, None) == ERR_ARG  # no 2^23 domain
    assert f_(ctx.h, a, b, s, cnt, 1, 12, 0, EXT, py, pc, pk, None) == ERR_ARG  # R = 8192 cells
    assert f_(ctx.h, None, b, s, cnt, 1, k, kl, EXT, py, pc, pk, None) == ERR_ARG
    assert f_(ctx.h, a, None, s, cnt, 1, k, kl, EXT, py, pc, pk, None) == ERR_ARG
    assert f_(ctx.h, a, b, None, cnt, 1, k, kl, EXT, py, pc, pk, None) == ERR_ARG
    assert f_(ctx.h, a, b, s, cnt, 1, k, kl, EXT, None, None, pk, None) == ERR_ARG  # neither output
    assert f_(ctx.h, a, b, s, cnt, 1, k, kl, EXT, py, pc, None, None) == ERR_ARG
    assert g_(ctx.h, a, b, s, cnt, 1, k, kl, EXT, None, None, px, pf, pk, None) == 0  # proofs alone
    assert g_(ctx.h, a, b, s, cnt, 1, k, kl, EXT, py, pc, None, pf, pk, None) == ERR_ARG
    assert g_(ctx.h, a, b, s, cnt, 1, k, kl, EXT, py, pc, px, None, pk, None) == ERR_ARG
    assert g_(ctx.h, a, b, s, cnt, 1, 4, kl, EXT, py, pc, px, pf, pk, None) == ERR_DEGREE  # 16 > 8 points
    ctx.sync()
    assert g_(bare.h, a, b, s, cnt, 1, k, kl, EXT, py, pc, px, pf, pk, None) == ERR_NO_SRS
    assert f_(bare.h, a, b, s, cnt, 1, k, kl, EXT, py, pc, pk, None) == 0  # the plain form needs no SRS
    ctx.sync()
    bare.sync()
    assert d_ok.cpu()[0] == 1 and (d_y.cpu().numpy().view(np.uint64).reshape(R, 2, 4) == y[0]).all()

    def refused(c, *args, **kw):
        with pytest.raises(kzgx.KzgxError) as e:
            c.recover_cells(*args, **kw)
        return e.value.status

    assert refused(bare, bi, ci, ys, 1, k, extended=False) == ERR_ARG
    bad = ci.copy()
    bad[0] = R
    assert refused(bare, bi, bad, ys, 1, k) == ERR_ARG  # cell index out of range
    bad = bi.copy()
    bad[0] = 1
    assert refused(bare, bad, ci, ys, 1, k) == ERR_ARG  # blob index out of range
    bad = ci.copy()
    bad[0] = bad[1]
    assert refused(bare, bi, bad, ys, 1, k) == ERR_ARG  # a duplicate
    assert refused(bare, bi[1:], ci[1:], ys[1:], 1, k) == ERR_ARG  # fewer than R / 2 cells
    assert refused(bare, bi, ci, ys, 2, k) == ERR_ARG  # blob 1 has none
    assert refused(bare, bi, ci, ys, 1, k, want_y=False, want_coeffs=False) == ERR_ARG
    with pytest.raises(kzgx.KzgxError) as e:
        bare.recover_cells_and_proofs(bi, ci, ys, 1, k)
    assert e.value.status == ERR_NO_SRS
    ok = (ctypes.c_int * 1)(7)
    assert kzgx.lib().kzgx_recover_cells(bare.h, None, None, None, 0, 0, k, kl, EXT, None, None, ok) == 0
    assert ok[0] == 7  # n_blobs == 0 writes nothing


# ---- 8. BN254: the size-4 domain -----------------------------------------------------------------------------------
def test_bn254():
    C = K.BN254
    c = kzgx.Context("BN254")
    try:
        for k, kl in ((1, 0), (1, 1)):
            kr = k + 1 - kl
            R = 1 << kr
            P = K.random_scalars(C, 1 << k, 0xB7E + kl)
            y = horner("BN254", P, k, kl)[None]
            for rev in (False, True):
                yy = cells(y, kr, kl) if rev else y
                for kp in (np.arange(R // 2), np.arange(R // 2, R), np.arange(R)):
                    oy, oc, ok = c.recover_cells(*flat(yy, [kp]), 1, k, bitrev=rev)
                    assert ok.all() and (oy == yy).all() and (oc[0] == to_limbs(P)).all(), (k, kl, rev, kp)
        with pytest.raises(kzgx.KzgxError) as e:  # no size-8 domain
            c.recover_cells(np.zeros(2, np.uint32), np.arange(2, dtype=np.uint32), np.zeros((2, 2, 4), np.uint64), 1, 2)
        assert e.value.status == ERR_ARG
    finally:
        c.close()
