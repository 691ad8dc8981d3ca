"""GPU parity of the variable-base G1 MSM over caller-supplied points
(kzgx_msm_g1_points / _device), both curves.

Checker: the C oracle's naive sum of double-and-add scalar multiplications
(corc.msm_naive over the same point array) and, where the points are known
multiples d_k G, the single scalar multiplication [sum s_k d_k mod r]G.  Every
step of the kernels is an exact group operation, so every comparison is bit
exact on the canonical affine result."""
import numpy as np
import pytest

import corc
import kzg_ref as K

pytestmark = pytest.mark.gpu

CURVES = [("BN254", K.BN254), ("BLS12381", K.BLS12381)]


def w64(C):
    return 4 if C.name == "BN254" else 6


def scalars(vals):
    return corc.ints_to_limbs(list(vals), 4)


def got_point(name, out, inf):
    return None if inf else corc.array_to_points(name, out[None, :])[0]


@pytest.fixture(scope="module")
def ctxs():
    import kzgx
    made = {}

    def get(name):
        if name not in made:
            made[name] = kzgx.Context(name)  # no SRS: the MSM needs none
        return made[name]

    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def powers():
    """[tau^k]G for k < 1500 per curve (the C oracle) and the exponents tau^k mod r"""
    made = {}

    def get(name, C):
        if name not in made:
            tau = K.default_tau(C)
            n = 1500
            d = [pow(tau, k, C.r) for k in range(n)]
            made[name] = (corc.gen_srs(name, tau, n), d)
        return made[name]

    return get


def check(ctx, name, C, pts, sc, d=None, inf=None):
    pts = np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, 2 * w64(C))
    out, oi = ctx.msm_points(pts, scalars(sc), inf)
    got = got_point(name, out, oi)
    ref_pts = pts.copy()
    if inf is not None:
        ref_pts[np.asarray(inf, dtype=bool)] = 0
    if len(sc):
        assert got == corc.msm_naive(name, ref_pts, scalars(sc))
    else:
        assert got is None
    if d is not None:
        e = sum(s * dk for s, dk in zip(sc, d)) % C.r
        assert got == corc.scalar_mul(name, (C.gx, C.gy), e)
    return got


def neg_row(C, row):
    n = w64(C)
    y = sum(int(row[n + i]) << (64 * i) for i in range(n))
    out = row.copy()
    out[n:] = corc.ints_to_limbs([C.p - y], n)[0]
    return out


@pytest.mark.parametrize("name,C", CURVES)
def test_empty_and_single(name, C, ctxs, powers):
    ctx = ctxs(name)
    P, d = powers(name, C)
    assert check(ctx, name, C, np.zeros((0, 2 * w64(C)), dtype=np.uint64), []) is None
    for s in (0, 1, 2, C.r - 1):
        check(ctx, name, C, P[3:4], [s], d[3:4])
    assert check(ctx, name, C, P[3:4], [0]) is None


@pytest.mark.parametrize("name,C", CURVES)
def test_repeated_and_opposite_points(name, C, ctxs, powers):
    """P, P with equal scalars is a doubling inside a bucket; P, -P cancels"""
    ctx = ctxs(name)
    P, d = powers(name, C)
    s = 0x1234567 + (5 << 200)
    check(ctx, name, C, np.stack([P[2], P[2]]), [s, s], [d[2], d[2]])
    assert check(ctx, name, C, np.stack([P[2], neg_row(C, P[2])]), [s, s], [d[2], C.r - d[2]]) is None


@pytest.mark.parametrize("name,C", CURVES)
def test_infinite_points(name, C, ctxs, powers):
    """a flagged-infinity point (coordinates present) and an all-zero point in the middle"""
    ctx = ctxs(name)
    P, d = powers(name, C)
    sc = K.random_scalars(C, 4, seed=77)
    pts = np.stack([P[1], P[5], np.zeros_like(P[0]), P[7]])
    check(ctx, name, C, pts, sc, [d[1], 0, 0, d[7]], inf=[0, 1, 0, 0])
    check(ctx, name, C, pts[1:], sc[1:], [0, 0, d[7]], inf=[1, 0, 0])  # n = 3
    check(ctx, name, C, pts, sc, [d[1], d[5], 0, d[7]])                # no flags


def max_digit_scalar(c):
    """every c-bit window below bit 253 holds the raw digit 2^(c-1) + 1 (< r on both curves), so each
    recodes to a negative digit with a carry into the next"""
    v = 0
    for w in range(253 // c):
        v |= ((1 << (c - 1)) + 1) << (c * w)
    return v


@pytest.mark.parametrize("name,C", CURVES)
def test_n64_short_and_full_scalars(name, C, ctxs, powers):
    ctx = ctxs(name)
    P, d = powers(name, C)
    short = [s % (1 << 128) for s in K.random_scalars(C, 64, seed=5)]
    short[0], short[1], short[2] = (1 << 128) - 1, 0, 1
    check(ctx, name, C, P[:64], short, d[:64])
    full = K.random_scalars(C, 64, seed=6)
    full[0], full[1] = (1 << 253) % C.r, C.r - 1
    full[2] = max_digit_scalar(10) % C.r   # n = 64 runs the 10-bit window
    full[3] = ((1 << 253) - 1) % C.r       # every raw digit all ones
    full[4] = max_digit_scalar(13) % C.r
    check(ctx, name, C, P[:64], full, d[:64])


@pytest.mark.parametrize("name,C", CURVES)
@pytest.mark.parametrize("n", [511, 512, 513])
def test_count_block_boundaries(name, C, n, ctxs, powers):
    ctx = ctxs(name)
    P, d = powers(name, C)
    check(ctx, name, C, P[:n], K.random_scalars(C, n, seed=1000 + n), d[:n])


def tiled_msm_matches_one_scalar_mul(ctx, name, C, P, d, n):
    """64 distinct points repeat, so the expected point is one scalar multiplication:
    [sum s_k d_(k mod 64)]G"""
    sc = K.random_scalars(C, n, seed=n)
    pts = np.tile(P[:64], ((n + 63) // 64, 1))[:n]
    out, oi = ctx.msm_points(pts, scalars(sc))
    sums = [sum(sc[j::64]) for j in range(64)]
    e = sum(s * dk for s, dk in zip(sums, d[:64])) % C.r
    assert got_point(name, out, oi) == corc.scalar_mul(name, (C.gx, C.gy), e)


@pytest.mark.parametrize("name,C", CURVES)
@pytest.mark.parametrize("n", [4095, 4096, 4097, 8193])
def test_point_count_block_boundaries(name, C, n, ctxs, powers):
    """the point path's count block is 4096 points (the 512 above is the SRS path's): one block
    short by a point, full, one point over, and two full blocks and a point"""
    ctx = ctxs(name)
    P, d = powers(name, C)
    tiled_msm_matches_one_scalar_mul(ctx, name, C, P, d, n)


@pytest.mark.parametrize("name,C", CURVES)
def test_one_bucket_spans_many_segments(name, C, ctxs, powers):
    """1000 copies of one (point, scalar) pair among 500 random terms: each window's bucket of that
    pair spans many accumulation segments; with 4-entry segments it also crosses workgroups"""
    ctx = ctxs(name)
    P, d = powers(name, C)
    n = 1500
    rs = K.random_scalars(C, n, seed=31)
    pts, sc, dd = P[:n].copy(), list(rs), list(d[:n])
    for i in range(n):
        if i % 3 != 2:  # 1000 of the 1500, spread over the array
            pts[i], sc[i], dd[i] = P[9], rs[9], d[9]
    ref = check(ctx, name, C, pts, sc, dd)
    ctx.set_segment(4)
    try:
        out, oi = ctx.msm_points(pts, scalars(sc))
        assert got_point(name, out, oi) == ref
    finally:
        ctx.set_segment(128)


@pytest.mark.parametrize("name,C", CURVES)
@pytest.mark.parametrize("n", [20001, 40001, (1 << 17) + 4097])
def test_wider_windows_and_chunks(name, C, n, ctxs, powers):
    """the 11-, 12- and 13-bit windows, and two chunks (2^17 points and an odd rest)"""
    ctx = ctxs(name)
    P, d = powers(name, C)
    tiled_msm_matches_one_scalar_mul(ctx, name, C, P, d, n)


@pytest.mark.parametrize("name,C", CURVES)
def test_device_entry_two_streams(name, C, ctxs, powers):
    """two calls on two caller streams with no sync in between"""
    import torch
    ctx = ctxs(name)
    P, d = powers(name, C)
    dev = torch.device("cuda", 0)
    jobs = []
    for k, n in enumerate((300, 700)):
        sc = K.random_scalars(C, n, seed=500 + k)
        pts = P[k:k + n]
        flags = np.zeros(n, dtype=np.int32)
        flags[5] = 1
        jobs.append(dict(
            n=n, sc=sc, dd=[0 if i == 5 else d[k + i] for i in range(n)],
            d_p=torch.from_numpy(np.ascontiguousarray(pts).view(np.int64)).to(dev),
            d_s=torch.from_numpy(scalars(sc).view(np.int64)).to(dev),
            d_f=torch.from_numpy(flags).to(dev),
            out=torch.zeros(2 * w64(C), dtype=torch.int64, device=dev),
            oi=torch.ones(1, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize(dev)
    streams = [torch.cuda.Stream(device=dev) for _ in jobs]
    for j, st in zip(jobs, streams):
        ctx.msm_points_device(j["d_p"].data_ptr(), j["d_f"].data_ptr(), j["d_s"].data_ptr(), j["n"],
                              j["out"].data_ptr(), j["oi"].data_ptr(), st.cuda_stream)
    torch.cuda.synchronize(dev)
    for j in jobs:
        e = sum(s * dk for s, dk in zip(j["sc"], j["dd"])) % C.r
        got = got_point(name, j["out"].cpu().numpy().view(np.uint64), bool(j["oi"].item()))
        assert got == corc.scalar_mul(name, (C.gx, C.gy), e)


def test_too_many_points_is_an_argument_error(ctxs):
    import kzgx
    ctx = ctxs("BN254")
    with pytest.raises(kzgx.KzgxError) as e:
        ctx.msm_points_device(1 << 12, None, 1 << 12, (1 << 22) + 1, 1 << 12, 1 << 12)  # rejected before any access
    assert e.value.status == -1
