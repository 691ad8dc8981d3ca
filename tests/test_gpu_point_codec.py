"""GPU tests of the compressed point encodings (kzgx_g1_decompress_batch(_device),
kzgx_g1_compress_batch(_device), kzgx_g2_decompress_batch, kzgx_g2_compress_batch,
kzgx_verify_cells_aggregate_bytes(_device); csrc/codec.hip).

Every expected byte, limb and flag comes from the Python codec of
tests/point_codec_ref.py (roots by pow(a, (p + 1) // 4, p) and pairing_ref.f2sqrt)
and from the oracle's membership tests, never from the library."""
import numpy as np
import pytest

import corc
import kzg_ref as K
import pairing_ref as PR
import point_codec_ref as R
from test_gpu_subgroup import g1_rows, g2_rows, w64
from test_gpu_verify_aggregate import challenges128, scalars
from test_subgroup_consts import (G1_COFACTOR_PRIMES, g1_curve_point, g1_member, g1_order_point, g2_member,
                                  g2_order13_point)

pytestmark = pytest.mark.gpu

BLS, BN = K.BLS12381, K.BN254
COMBOS = [("BN254", BN, R.SEC1), ("BLS12381", BLS, R.ZCASH), ("BLS12381", BLS, R.SEC1)]
ERR_ARG = -1


@pytest.fixture(scope="module")
def env():
    import kzgx
    made = {}

    def get(name):
        if name not in made:
            C = K.CURVES[name]
            ctx = kzgx.Context(name)
            ctx.set_default_table(0)
            # 257 members ([tau^i]G from the C oracle) and their negatives: both signs occur
            pool = corc.array_to_points(name, corc.gen_srs(name, K.default_tau(C), 257))
            pool = pool + [K.point_neg(C, P) for P in pool]
            made[name] = (ctx, pool, {})
        return made[name]

    yield get
    for ctx, _, _ in made.values():
        ctx.close()


def records(C, enc, pts):
    return b"".join(R.g1_compress(C, P, enc) for P in pts)


def sec1(C, prefix, x):
    return bytes([prefix]) + x.to_bytes(R.modbytes(C), "big")


def zcash(x, flags):
    b = bytearray(x.to_bytes(48, "big"))
    assert b[0] < 0x20
    b[0] |= flags
    return bytes(b)


def expect_rows(C, recs, enc, subgroup=False):
    """the reference codec's (rows, is_inf, ok) for a list of records"""
    pts, inf, ok = [], [], []
    for rec in recs:
        P = R.g1_decompress(C, rec, enc)
        good = P is None or (P != R.INVALID and (not subgroup or g1_member(C, P)))
        pts.append(P if good else None)
        inf.append(P is None or not good)
        ok.append(good)
    return g1_rows(C, pts), inf, ok


# ---- round trip --------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 63, 64, 65, 514])
@pytest.mark.parametrize("name,C,enc", COMBOS)
def test_g1_round_trip(name, C, enc, count, env):
    ctx, pool, _ = env(name)
    pts = list(pool[:count]) if count < 514 else list(pool)
    if count == 1:
        pts = [pool[300]]  # a negative
    assert len(pts) == count
    rows = g1_rows(C, pts)
    inf = np.zeros(count, dtype=np.int32)
    if count > 10:
        inf[5] = 1  # the identity by its flag, whatever the words
        pts[5] = None
        rows[9] = 0  # and by all-zero words
        pts[9] = None
    want = records(C, enc, pts)
    got = ctx.g1_compress(rows, inf, encoding=enc)
    assert len(got) == count * R.point_bytes(C, 1, enc)
    assert got == want
    if count > 10:
        assert ctx.g1_compress(rows[9:10], None, encoding=enc) == R.g1_compress(C, None, enc)
    xy, oi, ok = ctx.g1_decompress(got, encoding=enc, subgroup=(count % 2 == 0))
    assert (xy == g1_rows(C, pts)).all()
    assert oi.tolist() == [P is None for P in pts] and ok.tolist() == [True] * count
    signs = {(R.sign_lex_g1 if enc == R.ZCASH else R.sign_parity)(C, P[1]) for P in pts if P is not None}
    assert signs == ({0, 1} if count > 1 else signs)


# ---- rejections ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,C,enc", COMBOS)
def test_g1_rejections_inside_a_wave(name, C, enc, env):
    ctx, pool, _ = env(name)
    p, nb = C.p, R.modbytes(C)
    nonres = (0, 1, 3, 8, 9) if name == "BN254" else (1, 2, 3, 7)
    for x in nonres:
        assert pow((x ** 3 + C.b) % p, (p - 1) // 2, p) == p - 1
    gx = pool[1][0]
    if enc == R.SEC1:
        bad = [sec1(C, 2, p), sec1(C, 3, p + 1), sec1(C, 2, (1 << (8 * nb)) - 1)]
        bad += [sec1(C, 2 | (x & 1), x) for x in nonres]
        bad += [sec1(C, 4, gx), sec1(C, 5, gx), sec1(C, 0, 1), sec1(C, 0, gx)]
    else:
        # x = p, p + 1 and 2^384 - 1: the flag bits are part of the top byte, so the all-ones record
        # reads as C = I = S = 1; p and p + 1 fit the 381 bits
        bad = [zcash(p, 0x80), zcash(p + 1, 0xA0), bytes([0xFF] * 48), zcash((1 << 381) - 1, 0x80)]
        bad += [zcash(x, 0x80 | ((x & 1) << 5)) for x in nonres]
        bad += [zcash(gx, 0x00), zcash(gx, 0x20),  # C = 0
                zcash(0, 0xE0),  # I = 1 with S = 1
                zcash(1, 0xC0), zcash(1 << 380, 0xC0)]  # I = 1 with a nonzero x bit
    good = [R.g1_compress(C, P, enc) for P in pool[:70]]
    recs = list(good)
    at = [0, 1, 31, 62, 63, 64, 69] + list(range(10, 10 + len(bad) - 7))
    assert len(at) == len(bad) and len(set(at)) == len(at)
    for i, rec in zip(at, bad):
        assert R.g1_decompress(C, rec, enc) == R.INVALID
        recs[i] = rec
    rows, inf, ok = expect_rows(C, recs, enc)
    assert sorted(i for i, v in enumerate(ok) if not v) == sorted(at)
    for sg in (False, True):
        xy, oi, okg = ctx.g1_decompress(b"".join(recs), encoding=enc, subgroup=sg)
        assert okg.tolist() == ok and oi.tolist() == inf
        assert (xy == rows).all()  # rejected lanes all-zero, their neighbours exact


# ---- subgroup ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bls_nonmembers():
    """the 11 non-members of tests/test_gpu_subgroup.py: T_ell, [k]G + T_ell, a raw curve point"""
    C, out = BLS, []
    G = (C.gx, C.gy)
    for j, ell in enumerate(G1_COFACTOR_PRIMES):
        T = g1_order_point(ell)
        out += [T, K.point_add(C, K.scalar_mul(C, G, 1000003 + j), T)]
    out.append(g1_curve_point(C, 987654321))
    assert len(out) == 11 and all(K.on_curve(C, P) and not g1_member(C, P) for P in out)
    return out


@pytest.mark.parametrize("enc", [R.ZCASH, R.SEC1])
def test_g1_subgroup_flag_bls(enc, env, bls_nonmembers):
    C = BLS
    ctx, pool, _ = env("BLS12381")
    assert K.on_curve(C, (0, 2)) and not g1_member(C, (0, 2))  # x = 0 is on the curve
    non = bls_nonmembers + [(0, 2), (0, C.p - 2)]
    pts = list(pool[:6]) + non + list(pool[300:303])
    recs = [R.g1_compress(C, P, enc) for P in pts]
    member = [g1_member(C, P) for P in pts]
    assert member == [True] * 6 + [False] * 13 + [True] * 3
    xy, oi, ok = ctx.g1_decompress(b"".join(recs), encoding=enc, subgroup=False)
    assert ok.tolist() == [True] * len(pts) and not oi.any() and (xy == g1_rows(C, pts)).all()
    xy, oi, ok = ctx.g1_decompress(b"".join(recs), encoding=enc, subgroup=True)
    assert ok.tolist() == member and oi.tolist() == [not m for m in member]
    assert (xy == g1_rows(C, [P if m else None for P, m in zip(pts, member)])).all()


def test_g1_subgroup_flag_adds_nothing_on_bn254(env):
    C = BN
    ctx, pool, _ = env("BN254")
    raw = [g1_curve_point(C, 5000 + 97 * j) for j in range(6)]  # raw curve points: cofactor 1
    recs = [R.g1_compress(C, P, R.SEC1) for P in raw + pool[:3]] + [sec1(C, 2, 1), sec1(C, 0, 0)]
    res = [ctx.g1_decompress(b"".join(recs), encoding=R.SEC1, subgroup=sg) for sg in (False, True)]
    assert res[0][2].tolist() == res[1][2].tolist() == [True] * 9 + [False, True]
    assert (res[0][0] == res[1][0]).all() and (res[0][1] == res[1][1]).all()
    assert (res[0][0] == expect_rows(C, recs, R.SEC1)[0]).all()


# ---- the sign functions at their boundaries, through compress (which validates nothing) --------------
@pytest.mark.parametrize("name,C,enc", COMBOS)
def test_g1_sign_boundaries(name, C, enc, env):
    ctx = env(name)[0]
    p = C.p
    ys = [1, (p - 1) // 2, (p + 1) // 2, p - 1]
    x = 0x1234567
    got = ctx.g1_compress(g1_rows(C, [(x, y) for y in ys]), None, encoding=enc)
    want = b"".join(R.g1_compress_raw(C, x, y, enc) for y in ys)
    assert got == want
    rb = R.point_bytes(C, 1, enc)
    bits = [(got[i * rb] >> 5) & 1 if enc == R.ZCASH else got[i * rb] & 1 for i in range(4)]
    assert bits == ([0, 0, 1, 1] if enc == R.ZCASH else [y & 1 for y in ys])


def test_g2_sign_boundaries(env):
    C = BLS
    ctx = env("BLS12381")[0]
    p = C.p
    h = (p - 1) // 2
    ys = [(re, im) for im in (1, h, h + 1, p - 1) for re in (1, p - 1)]
    ys += [(1, 0), (h, 0), (h + 1, 0), (p - 1, 0)]  # y.im = 0: y.re on either side of (p - 1) / 2
    x = (0x1234567, 0x89ABCDE)
    got = ctx.g2_compress(g2_rows(C, [(x, y) for y in ys]))
    assert got == b"".join(R.g2_compress_raw(C, x, y) for y in ys)
    bits = [(got[96 * i] >> 5) & 1 for i in range(len(ys))]
    assert bits == [0, 0, 0, 0, 1, 1, 1, 1] + [0, 0, 1, 1]


# ---- G2 ------------------------------------------------------------------------------------------
def test_g2_round_trip_and_rejections(env):
    C = BLS
    ctx = env("BLS12381")[0]
    p = C.p
    Gen = PR.g2_generator(C)
    ks = K.random_scalars(C, 20, seed=0xC0DEC)
    pts = [PR.g2_mul(C, Gen, k) for k in ks]
    pts += [(Q[0], PR.f2neg(p, Q[1])) for Q in pts]
    T13 = g2_order13_point("BLS12381")
    assert PR.g2_mul_raw(C, T13, 13) is None and not g2_member(C, T13)
    pts += [None, T13]
    assert all(g2_member(C, Q) for Q in pts[:-1])
    recs = [R.g2_compress(C, Q) for Q in pts]
    got = ctx.g2_compress(g2_rows(C, pts))
    assert got == b"".join(recs)
    inf = np.zeros(len(pts), dtype=np.int32)
    inf[3] = 1
    assert ctx.g2_compress(g2_rows(C, pts), inf)[3 * 96:4 * 96] == R.g2_compress(C, None)
    assert {R.sign_lex_g2(C, Q[1]) for Q in pts if Q is not None} == {0, 1}
    for rec, Q in zip(recs, pts):
        assert R.g2_decompress(C, rec) == Q
    xy, oi, ok = ctx.g2_decompress(got, subgroup=False)
    assert ok.tolist() == [True] * len(pts) and oi.tolist() == [Q is None for Q in pts]
    assert (xy == g2_rows(C, pts)).all()
    xy, oi, ok = ctx.g2_decompress(got, subgroup=True)
    assert ok.tolist() == [True] * (len(pts) - 1) + [False]  # the order-13 point only with the flag
    assert oi.tolist() == [Q is None for Q in pts[:-1]] + [True]
    assert (xy == g2_rows(C, pts[:-1] + [None])).all()
    # rejections: a non-canonical x component (either one), and a non-residue right side found by
    # counting x.re upward with the oracle
    xre, xim = pts[0][0]
    s = R.sign_lex_g2(C, pts[0][1]) << 5
    bad = [zcash(xim, 0x80 | s) + p.to_bytes(48, "big"), zcash(p, 0x80 | s) + xre.to_bytes(48, "big"),
           zcash(xim, s) + xre.to_bytes(48, "big"),  # C = 0
           zcash(0, 0xE0) + bytes(48), zcash(0, 0xC0) + bytes(47) + b"\x01"]  # I = 1: S = 1, an x bit
    b2 = PR.twist(C).b2
    nonres = None
    for t in range(16):
        x = (xre + t, xim)
        if PR.f2sqrt(p, PR.f2add(p, PR.f2mul(p, PR.f2mul(p, x, x), x), b2)) is None:
            nonres = x
            break
    assert nonres is not None
    bad.append(zcash(nonres[1], 0x80) + nonres[0].to_bytes(48, "big"))
    assert all(R.g2_decompress(C, rec) == R.INVALID for rec in bad)
    mixed = [recs[0]] + bad[:3] + [recs[21]] + bad[3:] + [recs[5]]
    want_ok = [True] + [False] * 3 + [True] + [False] * 3 + [True]
    want = g2_rows(C, [pts[0], None, None, None, pts[21], None, None, None, pts[5]])
    for sg in (False, True):
        xy, oi, ok = ctx.g2_decompress(b"".join(mixed), subgroup=sg)
        assert ok.tolist() == want_ok and oi.tolist() == [not v for v in want_ok]
        assert (xy == want).all()


# ---- device forms --------------------------------------------------------------------------------
@pytest.mark.parametrize("name,C,enc", COMBOS)
def test_device_forms(name, C, enc, env):
    import torch
    ctx, pool, _ = env(name)
    dev = torch.device("cuda", 0)
    n, nl = 130, w64(C)
    clean = [R.g1_compress(C, P, enc) for P in pool[:n]]
    dirty = list(clean)
    dirty[77] = sec1(C, 5, pool[0][0]) if enc == R.SEC1 else zcash(pool[0][0], 0x00)
    st = torch.cuda.Stream(device=dev)
    for recs, all_want in ((clean, 1), (dirty, 0)):
        rows, inf, ok = expect_rows(C, recs, enc)
        d_b = torch.from_numpy(np.frombuffer(b"".join(recs), dtype=np.uint8).copy()).to(dev)
        d_xy = [torch.full((n, 2 * nl), 7, dtype=torch.int64, device=dev) for _ in range(3)]
        d_inf = torch.full((n,), 7, dtype=torch.int32, device=dev)
        d_ok = [torch.full((n,), 7, dtype=torch.int32, device=dev) for _ in range(2)]
        d_all = torch.full((3,), 7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        s = st.cuda_stream
        ctx.g1_decompress_device(d_b.data_ptr(), n, enc, True, d_xy[0].data_ptr(), d_inf.data_ptr(),
                                 d_ok[0].data_ptr(), d_all.data_ptr(), s)
        ctx.g1_decompress_device(d_b.data_ptr(), n, enc, True, d_xy[1].data_ptr(), None, None,
                                 d_all[1:].data_ptr(), s)  # d_ok = NULL, d_out_is_inf = NULL
        ctx.g1_decompress_device(d_b.data_ptr(), n, enc, True, d_xy[2].data_ptr(), None, d_ok[1].data_ptr(), None,
                                 s)  # d_all_ok = NULL
        ctx.g1_decompress_device(None, 0, enc, True, None, None, None, d_all[2:].data_ptr(), s)  # count = 0
        # and back: compress the recovered points on the device
        d_out = torch.zeros((n * len(recs[0]),), dtype=torch.uint8, device=dev)
        ctx.g1_compress_device(d_xy[0].data_ptr(), d_inf.data_ptr(), n, enc, d_out.data_ptr(), s)
        st.synchronize()
        for t in d_xy:
            assert (t.cpu().numpy().view(np.uint64) == rows).all()
        assert d_inf.cpu().tolist() == [int(v) for v in inf]
        assert d_ok[0].cpu().tolist() == d_ok[1].cpu().tolist() == [int(v) for v in ok]
        assert d_all.cpu().tolist() == [all_want, all_want, 1]
        back = bytes(d_out.cpu().numpy())
        rb = len(recs[0])
        assert [back[i * rb:(i + 1) * rb] for i in range(n)] == \
            [r if v else R.g1_compress(C, None, enc) for r, v in zip(recs, ok)]


def test_statuses(env):
    import kzgx
    lib = kzgx.lib()
    bn, bls = env("BN254")[0], env("BLS12381")[0]
    buf = np.zeros(4096, dtype=np.uint8)
    b8 = buf.ctypes.data_as(kzgx.u8p)
    xy = np.zeros(512, dtype=np.uint64)
    fl = np.zeros(64, dtype=np.int32)
    pi = fl.ctypes.data_as(kzgx.intp)
    for ctx in (bn, bls):
        for enc in (-1, 2, 7):  # unknown encodings, count 0 included: raised before any device work
            for count in (0, 1):
                assert lib.kzgx_g1_decompress_batch(ctx.h, b8, count, enc, 0, kzgx._p(xy), pi, pi) == ERR_ARG
                assert lib.kzgx_g1_compress_batch(ctx.h, kzgx._p(xy), None, count, enc, b8) == ERR_ARG
                assert lib.kzgx_g1_decompress_batch_device(ctx.h, 256, count, enc, 0, 256, None, 256, None,
                                                           None) == ERR_ARG
                assert lib.kzgx_g1_compress_batch_device(ctx.h, 256, None, count, enc, 256, None) == ERR_ARG
    # ZCash on BN254, and G2 on BN254
    assert lib.kzgx_g1_decompress_batch(bn.h, b8, 1, kzgx.ENC_ZCASH, 0, kzgx._p(xy), pi, pi) == ERR_ARG
    assert lib.kzgx_g1_compress_batch(bn.h, kzgx._p(xy), None, 1, kzgx.ENC_ZCASH, b8) == ERR_ARG
    assert lib.kzgx_g2_decompress_batch(bn.h, b8, 1, 0, kzgx._p(xy), pi, pi) == ERR_ARG
    assert lib.kzgx_g2_compress_batch(bn.h, kzgx._p(xy), None, 1, b8) == ERR_ARG
    with pytest.raises(kzgx.KzgxError) as err:
        bn.g1_decompress(bytes(48), encoding=kzgx.ENC_ZCASH)
    assert err.value.status == ERR_ARG
    with pytest.raises(kzgx.KzgxError) as err:
        bn.verify_cells_aggregate_bytes(b"", [], [], b"", np.zeros((0, 1, 4), dtype=np.uint64), 2,
                                        encoding=kzgx.ENC_ZCASH)
    assert err.value.status == ERR_ARG
    # NULL pointers, too many records, both flag outputs NULL
    for ctx, enc in ((bn, kzgx.ENC_SEC1), (bls, kzgx.ENC_ZCASH)):
        assert lib.kzgx_g1_decompress_batch(ctx.h, None, 1, enc, 0, kzgx._p(xy), pi, pi) == ERR_ARG
        assert lib.kzgx_g1_decompress_batch(ctx.h, b8, 1, enc, 0, None, pi, pi) == ERR_ARG
        assert lib.kzgx_g1_decompress_batch(ctx.h, b8, 1, enc, 0, kzgx._p(xy), pi, None) == ERR_ARG
        assert lib.kzgx_g1_decompress_batch(ctx.h, b8, (1 << 22) + 1, enc, 0, kzgx._p(xy), pi, pi) == ERR_ARG
        assert lib.kzgx_g1_compress_batch(ctx.h, None, None, 1, enc, b8) == ERR_ARG
        assert lib.kzgx_g1_compress_batch(ctx.h, kzgx._p(xy), None, 1, enc, None) == ERR_ARG
        assert lib.kzgx_g1_decompress_batch_device(ctx.h, 256, 1, enc, 0, 256, None, None, None, None) == ERR_ARG
        assert lib.kzgx_g1_decompress_batch_device(ctx.h, None, 1, enc, 0, 256, None, 256, None, None) == ERR_ARG
        assert lib.kzgx_g1_decompress_batch_device(ctx.h, 256, (1 << 22) + 1, enc, 0, 256, None, 256, None,
                                                   None) == ERR_ARG
        # count == 0 is KZGX_OK, out_is_inf may be NULL
        assert lib.kzgx_g1_decompress_batch(ctx.h, None, 0, enc, 1, None, None, None) == 0
        assert lib.kzgx_g1_compress_batch(ctx.h, None, None, 0, enc, None) == 0
        assert lib.kzgx_g1_compress_batch_device(ctx.h, None, None, 0, enc, None, None) == 0
    assert lib.kzgx_g2_decompress_batch(bls.h, None, 0, 1, None, None, None) == 0
    assert lib.kzgx_g2_decompress_batch(bls.h, None, 1, 1, kzgx._p(xy), pi, pi) == ERR_ARG
    rec = R.g1_compress(BLS, (BLS.gx, BLS.gy), R.ZCASH)
    xy1, oi, ok = bls.g1_decompress(rec)
    assert ok.tolist() == [True] and (xy1 == g1_rows(BLS, [(BLS.gx, BLS.gy)])).all()
    one = np.frombuffer(rec, dtype=np.uint8).copy()
    okf = np.zeros(1, dtype=np.int32)
    assert lib.kzgx_g1_decompress_batch(bls.h, one.ctypes.data_as(kzgx.u8p), 1, 0, 1, kzgx._p(xy), None,
                                        okf.ctypes.data_as(kzgx.intp)) == 0 and okf[0] == 1


# ---- end to end ----------------------------------------------------------------------------------
def test_end_to_end_cells_from_bytes():
    """prove_cosets_batch_device -> g1_compress_batch_device -> verify_cells_aggregate_bytes at
    (log2n = 4, log2l = 2), extended, bit-reversed, 2 blobs, 16 cells"""
    import kzgx
    import torch
    C, name, enc = BLS, "BLS12381", R.ZCASH
    tau = K.default_tau(C)
    dev = torch.device("cuda", 0)
    ctx = kzgx.Context(name)
    try:
        ctx.set_default_table(0)
        ctx.gen_srs(tau, 16)
        ctx.gen_srs_g2(tau, 8)
        blobs = np.stack([scalars(K.random_scalars(C, 16, seed=0xB10B + b)) for b in range(2)])
        coeffs = ctx.ntt(blobs, inverse=True, bitrev=True)
        commits = np.stack([ctx.msm(coeffs[b])[0] for b in range(2)])
        d_in = torch.from_numpy(blobs.view(np.int64)).to(dev)
        d_xy = torch.zeros((16, 12), dtype=torch.int64, device=dev)
        d_inf = torch.zeros((16,), dtype=torch.int32, device=dev)
        d_y = torch.zeros((16, 4, 4), dtype=torch.int64, device=dev)
        d_rec = torch.zeros((16 * 48,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        ctx.prove_cosets_device(d_in.data_ptr(), 4, 2, 2, 16, d_xy.data_ptr(), d_inf.data_ptr(), d_y.data_ptr(),
                                extended=True, evals=True, bitrev=True)
        ctx.g1_compress_device(d_xy.data_ptr(), d_inf.data_ptr(), 16, enc, d_rec.data_ptr())
        ctx.sync()
        torch.cuda.synchronize(dev)
        proofs = d_xy.cpu().numpy().view(np.uint64)
        ys = d_y.cpu().numpy().view(np.uint64)
        prec = bytes(d_rec.cpu().numpy())
        assert not d_inf.cpu().numpy().any()
        ppts = corc.array_to_points(name, proofs)
        assert prec == records(C, enc, ppts)  # the device compress against the reference codec
        crec = records(C, enc, corc.array_to_points(name, commits))
        assert ctx.g1_compress(commits, None, encoding=enc) == crec
        ci = np.repeat(np.arange(2, dtype=np.uint32), 8)
        idx = np.tile(np.arange(8, dtype=np.uint32), 2)
        ch = scalars(challenges128(C, 16, seed=0xE2E))
        kw = dict(challenges=ch, extended=True, bitrev=True)

        def from_bytes(c, p, sg=True):
            return ctx.verify_cells_aggregate_bytes(c, ci, idx, p, ys, 4, encoding=enc, subgroup=sg, **kw)

        for sg in (True, False):
            assert from_bytes(crec, prec, sg) is True
            assert ctx.verify_cells_aggregate_checked(commits, ci, idx, proofs, ys, 4, subgroup=sg, **kw) is True
        assert ctx.verify_cells_aggregate_bytes(crec, ci, idx, prec, ys, 4, encoding=enc, extended=True,
                                                bitrev=True) is True  # library-drawn challenges
        # flip S of one proof: the record still decodes (-pi is a valid point) and the answer is false
        flipped = bytearray(prec)
        flipped[11 * 48] ^= 0x20
        assert R.g1_decompress(C, bytes(flipped[11 * 48:12 * 48]), enc) == K.point_neg(C, ppts[11])
        assert from_bytes(crec, bytes(flipped)) is False
        neg = proofs.copy()
        neg[11] = g1_rows(C, [K.point_neg(C, ppts[11])])[0]
        assert ctx.verify_cells_aggregate_checked(commits, ci, idx, neg, ys, 4, subgroup=True, **kw) is False
        # one proof's x replaced by a non-residue, one commitment's likewise: does not decode -> false
        assert from_bytes(crec, prec[:5 * 48] + zcash(1, 0x80) + prec[6 * 48:]) is False
        assert from_bytes(crec[:48] + zcash(2, 0xA0), prec) is False
        # SEC1 records of the same points
        crec1 = records(C, R.SEC1, corc.array_to_points(name, commits))
        prec1 = records(C, R.SEC1, ppts)
        assert ctx.verify_cells_aggregate_bytes(crec1, ci, idx, prec1, ys, 4, encoding=R.SEC1, subgroup=True,
                                                **kw) is True
        # the device entry: clean, an out-of-range cell index, an out-of-range commit index, a bad record
        st = torch.cuda.Stream(device=dev)
        t_c = torch.from_numpy(np.frombuffer(crec, dtype=np.uint8).copy()).to(dev)
        t_p = torch.from_numpy(np.frombuffer(prec, dtype=np.uint8).copy()).to(dev)
        t_pb = torch.from_numpy(np.frombuffer(bytes(flipped), dtype=np.uint8).copy()).to(dev)
        t_y = torch.from_numpy(ys.view(np.int64)).to(dev)
        t_r = torch.from_numpy(ch.view(np.int64)).to(dev)
        oob_cell, oob_commit = idx.copy(), ci.copy()
        oob_cell[13] = 8
        oob_commit[2] = 2
        t_ci, t_idx, t_oc, t_ox = (torch.from_numpy(v.view(np.int32)).to(dev) for v in (ci, idx, oob_commit, oob_cell))
        cases = [(t_ci, t_idx, t_p, 1), (t_ci, t_ox, t_p, 0), (t_oc, t_idx, t_p, 0), (t_ci, t_idx, t_pb, 0)]
        oks = [torch.full((3,), 7, dtype=torch.int32, device=dev) for _ in cases]
        par = [torch.full((1,), 7, dtype=torch.int32, device=dev) for _ in range(2)]
        torch.cuda.synchronize(dev)
        for (a, b, p, _), ok in zip(cases, oks):
            ctx.verify_cells_aggregate_bytes_device(t_c.data_ptr(), 2, a.data_ptr(), b.data_ptr(), p.data_ptr(),
                                                    t_y.data_ptr(), t_r.data_ptr(), 16, 4, 2, enc, True,
                                                    ok[1:].data_ptr(), extended=True, bitrev=True,
                                                    stream=st.cuda_stream)
        # the parent call on the uncompressed points with the same out-of-range index
        t_cx = torch.from_numpy(commits.view(np.int64)).to(dev)
        t_px = torch.from_numpy(proofs.view(np.int64)).to(dev)
        torch.cuda.synchronize(dev)
        for a, b, ok in ((t_ci, t_ox, par[0]), (t_ci, t_idx, par[1])):
            ctx.verify_cells_aggregate_checked_device(t_cx.data_ptr(), None, 2, a.data_ptr(), b.data_ptr(),
                                                      t_px.data_ptr(), None, t_y.data_ptr(), t_r.data_ptr(), 16, 4, 2,
                                                      True, ok.data_ptr(), extended=True, bitrev=True,
                                                      stream=st.cuda_stream)
        st.synchronize()
        assert [o.tolist() for o in oks] == [[7, want, 7] for _, _, _, want in cases]
        assert [int(o.item()) for o in par] == [0, 1]
    finally:
        ctx.close()
