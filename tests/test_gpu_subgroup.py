"""GPU tests of the batched point validation with prime-order subgroup checks
(kzgx_g1_check_batch(_device), kzgx_g2_check_batch, kzgx_srs_check,
kzgx_verify_aggregate_checked(_device); csrc/subgroup.hip).

Every expected flag comes from the Python oracle, never from the library:
  G1 member  <=>  K.to_affine(K._jac_mul_raw(C, P, r)) is None
  G2 member  <=>  pairing_ref.g2_mul_raw(C, Q, r) is None
Non-members are built here (tests/test_subgroup_consts.py holds the builders):
T_ell = [n / ell^e]R multiplied up to exact order ell, for every prime ell of the
BLS12-381 G1 cofactor and for 13 on both twists; the exact order is asserted."""
import numpy as np
import pytest

import corc
import kzg_ref as K
import pairing_ref as PR
from test_gpu_verify_aggregate import challenges128, make_batch, scalars
from test_subgroup_consts import (G1_COFACTOR_PRIMES, g1_curve_point, g1_member, g1_order_point, g1_raw_mul,
                                  g2_member, g2_order13_point, g2_raw_point)

pytestmark = pytest.mark.gpu

CURVES = [("BN254", K.BN254), ("BLS12381", K.BLS12381)]
BLS = K.BLS12381


def w64(C):
    return 4 if C.name == "BN254" else 6


def g1_rows(C, entries):
    """entries: (x, y) raw integers (not reduced), None = all-zero words"""
    nl = w64(C)
    out = np.zeros((len(entries), 2 * nl), dtype=np.uint64)
    for i, e in enumerate(entries):
        if e is not None:
            out[i, :nl] = corc.ints_to_limbs([e[0]], nl)[0]
            out[i, nl:] = corc.ints_to_limbs([e[1]], nl)[0]
    return out


def g2_rows(C, pts):
    nl = w64(C)
    out = np.zeros((len(pts), 4 * nl), dtype=np.uint64)
    for i, Q in enumerate(pts):
        if Q is not None:
            for j, v in enumerate((Q[0][0], Q[0][1], Q[1][0], Q[1][1])):
                out[i, j * nl:(j + 1) * nl] = corc.ints_to_limbs([v], nl)[0]
    return out


def g1_expected(C, e, flagged, subgroup):
    """the oracle's flag for one entry"""
    if flagged or e is None or e == (0, 0):
        return True
    x, y = e
    if x >= C.p or y >= C.p or not K.on_curve(C, (x, y)):
        return False
    return g1_member(C, (x, y)) if subgroup else True


def g2_expected(C, Q, subgroup):
    if Q is None:
        return True
    if any(v >= C.p for c in Q for v in c) or not PR.g2_on_curve(C, Q):
        return False
    return g2_member(C, Q) if subgroup else True


@pytest.fixture(scope="module")
def env():
    import kzgx
    made = {}

    def get(name):
        if name not in made:
            C = K.CURVES[name]
            tau = K.default_tau(C)
            ctx = kzgx.Context(name)
            ctx.set_default_table(0)
            ctx.gen_srs(tau, 130)
            ctx.gen_srs_g2(tau, 130)
            # 257 members ([tau^i]G from the C oracle): the pool of the batch-shape tests
            pool = corc.array_to_points(name, corc.gen_srs(name, tau, 257))
            made[name] = (ctx, tau, pool, {})
        return made[name]

    yield get
    for ctx, _, _, _ in made.values():
        ctx.close()


@pytest.fixture(scope="module")
def bls_nonmembers():
    """[(label, point)] on BLS12-381 G1: T_ell, [k]G + T_ell for every ell, and a raw curve point"""
    C = BLS
    G = (C.gx, C.gy)
    out = []
    for j, ell in enumerate(G1_COFACTOR_PRIMES):
        T = g1_order_point(ell)
        assert g1_raw_mul(C, T, ell) is None and T is not None  # exact order ell (prime)
        out.append(("T_%d" % ell, T))
        out.append(("[k]G + T_%d" % ell, K.point_add(C, K.scalar_mul(C, G, 1000003 + j), T)))
    raw = g1_curve_point(C, 987654321)
    assert not g1_member(C, raw)
    out.append(("raw curve point", raw))
    for label, P in out:
        assert K.on_curve(C, P) and not g1_member(C, P), label
    return out


# ---- G1 ------------------------------------------------------------------------------
@pytest.mark.parametrize("name,C", CURVES)
def test_g1_members_pass(name, C, env):
    ctx = env(name)[0]
    G = (C.gx, C.gy)
    ks = [1, 2, C.r - 1] + K.random_scalars(C, 20, seed=31337)
    pts = [K.scalar_mul(C, G, k) for k in ks]
    assert all(g1_member(C, P) for P in pts)
    rows = g1_rows(C, pts + [pts[5]])
    inf = np.zeros(len(pts) + 1, dtype=np.int32)
    inf[-1] = 1  # flagged infinity, whatever the words
    for sg in (False, True):
        assert ctx.g1_check(rows, inf, subgroup=sg).tolist() == [True] * (len(pts) + 1)
    # all-zero words without a flag are the identity too
    assert ctx.g1_check(g1_rows(C, [None, pts[0]]), None, subgroup=True).tolist() == [True, True]


def test_g1_bls_nonmembers_rejected_only_with_the_flag(env, bls_nonmembers):
    ctx = env("BLS12381")[0]
    rows = g1_rows(BLS, [P for _, P in bls_nonmembers])
    n = len(bls_nonmembers)
    assert n == 11
    assert ctx.g1_check(rows, None, subgroup=True).tolist() == [False] * n
    assert ctx.g1_check(rows, None, subgroup=False).tolist() == [True] * n  # they are on the curve


@pytest.mark.parametrize("name,C", CURVES)
def test_g1_curve_test(name, C, env):
    ctx = env(name)[0]
    x, y = K.scalar_mul(C, (C.gx, C.gy), 12345)
    bad = [(x, (y + 1) % C.p), (x + C.p, y), (x, y + C.p)]
    assert not K.on_curve(C, bad[0])
    rows = g1_rows(C, bad + [(x, y)])
    for sg in (False, True):
        assert ctx.g1_check(rows, None, subgroup=sg).tolist() == [False, False, False, True]


def test_g1_bn254_flag_adds_nothing(env):
    C = K.BN254
    ctx = env("BN254")[0]
    raw = [g1_curve_point(C, 5000 + 97 * j) for j in range(6)]  # raw curve points: cofactor 1
    x, y = raw[0]
    entries = raw + [(x, (y + 1) % C.p), (x + C.p, y), None]
    rows = g1_rows(C, entries)
    plain = ctx.g1_check(rows, None, subgroup=False).tolist()
    flagged = ctx.g1_check(rows, None, subgroup=True).tolist()
    assert plain == flagged == [True] * 6 + [False, False, True]
    for e, ok in zip(entries, flagged):
        if ok and e is not None:
            assert g1_member(C, e)  # every accepted point satisfies the oracle


@pytest.mark.parametrize("name,C", CURVES)
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_g1_batch_shapes_and_device_entry(name, C, count, env, bls_nonmembers):
    """bad entries at 0, 62, 63, 64 and the last index (two kinds of failure inside the first wave),
    flags element for element, d_all_ok = their AND; device entry on a caller's stream with
    d_ok = NULL once and d_all_ok = NULL once"""
    import torch
    ctx, _, pool, _ = env(name)
    entries = list(pool[:count])
    x, y = pool[3]
    off_curve, non_canon = (x, (y + 1) % C.p), (x + C.p, y)
    second = bls_nonmembers[1][1] if name == "BLS12381" else non_canon  # [k]G + T_3 on BLS12-381
    kinds = {0: off_curve, 62: second, 63: non_canon, 64: second, count - 1: off_curve if count != 63 else second}
    bad_at = sorted(i for i in kinds if 0 <= i < count)
    for i in bad_at:
        entries[i] = kinds[i]
    inf = np.zeros(count, dtype=np.int32)
    if count > 10:
        inf[7] = 1
        entries[7] = (1, 1)  # flagged: passes whatever the words
    rows = g1_rows(C, entries)
    dev = torch.device("cuda", 0)
    for sg in (True, False):
        exp = [g1_expected(C, e, bool(f), sg) for e, f in zip(entries, inf)]
        if sg or name == "BN254":  # without the flag the BLS12-381 non-member is accepted
            assert [i for i, v in enumerate(exp) if not v] == bad_at
        assert ctx.g1_check(rows, inf, subgroup=sg).tolist() == exp
        # an all-good batch of the same size (AND = 1) beside the bad one (AND = 0 unless empty)
        good_rows = g1_rows(C, pool[:count])
        st = torch.cuda.Stream(device=dev)
        res = []
        for r, f in ((rows, inf), (good_rows, None)):
            d_xy = torch.from_numpy(np.ascontiguousarray(r).view(np.int64)).to(dev)
            d_inf = None if f is None else torch.from_numpy(f).to(dev)
            d_ok = torch.full((max(count, 1),), 7, dtype=torch.int32, device=dev)
            d_all = torch.full((2,), 7, dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            pi = None if d_inf is None else d_inf.data_ptr()
            px = d_xy.data_ptr() if count else None
            ctx.g1_check_device(px, pi, count, sg, d_ok.data_ptr(), d_all.data_ptr(), st.cuda_stream)
            ctx.g1_check_device(px, pi, count, sg, None, d_all[1:].data_ptr(), st.cuda_stream)  # d_ok = NULL
            d_ok2 = torch.full((max(count, 1),), 7, dtype=torch.int32, device=dev)
            ctx.g1_check_device(px, pi, count, sg, d_ok2.data_ptr(), None, st.cuda_stream)  # d_all_ok = NULL
            st.synchronize()
            res.append((d_ok.cpu().tolist()[:count], d_ok2.cpu().tolist()[:count], d_all.cpu().tolist()))
        assert res[0][0] == res[0][1] == [int(v) for v in exp]
        assert res[0][2] == [int(all(exp))] * 2
        assert res[1][0] == res[1][1] == [1] * count and res[1][2] == [1, 1]


@pytest.mark.parametrize("name,C", CURVES)
def test_g1_argument_errors(name, C, env):
    import kzgx
    ctx = env(name)[0]
    for fn in (lambda: kzgx.lib().kzgx_g1_check_batch(ctx.h, None, None, 1, 1, None),
               lambda: kzgx.lib().kzgx_g2_check_batch(ctx.h, None, None, 1, 1, None),
               lambda: kzgx.lib().kzgx_g1_check_batch_device(ctx.h, None, None, 0, 1, None, None, None),
               lambda: kzgx.lib().kzgx_g1_check_batch_device(ctx.h, 256, None, (1 << 22) + 1, 1, 256, None, None),
               lambda: kzgx.lib().kzgx_srs_check(ctx.h, 1, None, None)):
        assert fn() == -1
    bare = kzgx.Context(name)
    try:
        with pytest.raises(kzgx.KzgxError) as err:
            bare.srs_check()
        assert err.value.status == -4
    finally:
        bare.close()


# ---- G2 ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g2_vectors():
    made = {}

    def get(name):
        if name not in made:
            C = K.CURVES[name]
            Gen = PR.g2_generator(C)
            T13 = g2_order13_point(name)
            assert T13 is not None and PR.g2_mul_raw(C, T13, 13) is None  # exact order 13
            raw = g2_raw_point(C, 77)
            mixed = PR.g2_add(C, PR.g2_mul(C, Gen, 424243), T13)
            members = [Gen, PR.g2_mul(C, Gen, 2), PR.g2_mul(C, Gen, C.r - 1), PR.g2_mul(C, Gen, 0xDEADBEEFCAFE)]
            non = [raw, T13, mixed]
            off = (Gen[0], PR.f2add(C.p, Gen[1], (1, 0)))
            assert all(g2_member(C, Q) for Q in members) and not any(g2_member(C, Q) for Q in non)
            assert all(PR.g2_on_curve(C, Q) for Q in non) and not PR.g2_on_curve(C, off)
            made[name] = (members, non, off)
        return made[name]

    return get


@pytest.mark.parametrize("name,C", CURVES)
def test_g2_check(name, C, env, g2_vectors):
    ctx = env(name)[0]
    members, non, off = g2_vectors(name)
    noncanon = ((members[0][0][0] + C.p, members[0][0][1]), members[0][1])
    pts = members + non + [off, noncanon, None]
    rows = g2_rows(C, pts)
    for sg in (True, False):
        exp = [g2_expected(C, Q, sg) for Q in pts]
        assert exp == [True] * 4 + [not sg] * 3 + [False, False, True]
        assert ctx.g2_check(rows, None, subgroup=sg).tolist() == exp
    inf = np.zeros(len(pts), dtype=np.int32)
    inf[5] = 1  # T_13 flagged infinite: passes
    assert ctx.g2_check(rows, inf, subgroup=True).tolist() == [True] * 4 + [False, True, False, False, False, True]
    # generated SRS points are members
    srs2 = ctx.get_srs_g2()
    assert srs2.shape[0] == 130
    assert ctx.g2_check(srs2, None, subgroup=True).all()
    assert ctx.g2_check(rows[:0], None, subgroup=True).tolist() == []


# ---- kzgx_srs_check ------------------------------------------------------------------
@pytest.mark.parametrize("name,C", CURVES)
def test_srs_check(name, C, env, g2_vectors, bls_nonmembers):
    import kzgx
    ctx = env(name)[0]
    assert ctx.srs_check(True) == (True, True)
    assert ctx.srs_check(False) == (True, True)
    srs1, srs2 = ctx.get_srs(), ctx.get_srs_g2()
    assert srs1.shape[0] == 130 and srs2.shape[0] == 130

    def reloaded(g1, g2):
        c2 = kzgx.Context(name)
        try:
            c2.set_default_table(0)
            try:
                c2.load_srs(g1)
                c2.load_srs_g2(g2)
            except kzgx.KzgxError as e:  # a loader that refuses the replacement
                assert e.status == -1
                return "refused"
            return c2.srs_check(True), c2.srs_check(False)
        finally:
            c2.close()

    assert reloaded(srs1, srs2) == ((True, True), (True, True))
    T13 = g2_vectors(name)[1][1]
    for idx in (5, 129):
        m2 = srs2.copy()
        m2[idx] = g2_rows(C, [T13])[0]
        assert reloaded(srs1, m2) in ("refused", ((True, False), (True, True)))
    if name == "BLS12381":
        non = g1_rows(C, [bls_nonmembers[1][1]])[0]  # [k]G + T_3
        for idx in (0, 129):
            m1 = srs1.copy()
            m1[idx] = non
            assert reloaded(m1, srs2) in ("refused", ((False, True), (True, True)))
    # a G1-only context: g2_ok = 1
    c3 = kzgx.Context(name)
    try:
        c3.set_default_table(0)
        c3.load_srs(srs1)
        assert c3.srs_check(True) == (True, True)
    finally:
        c3.close()


# ---- checked aggregate, 40 openings ----------------------------------------------------
@pytest.mark.parametrize("name,C", CURVES)
def test_checked_aggregate(name, C, env, bls_nonmembers):
    import torch
    ctx, tau, _, cache = env(name)
    n = 40
    good = make_batch(name, C, tau, n)
    bad = good.copy()
    bad.y[23] = (bad.y[23] + 1) % C.r
    ch = challenges128(C, n, seed=515)
    assert good.aggregate(ch) and not bad.aggregate(ch)
    gx = good.arrays(cache)
    bx = bad.arrays(cache)
    r = scalars(ch)

    def checked(a, sg, px=None, cx=None):
        return ctx.verify_aggregate_checked(a[0] if cx is None else cx, a[1] if px is None else px, a[2], a[3], r,
                                            a[4], a[5], subgroup=sg)

    for sg in (True, False):
        assert checked(gx, sg) is True
        assert checked(bx, sg) is False
    # subgroup = 0 equals kzgx_verify_aggregate on the same member inputs
    for a in (gx, bx):
        assert checked(a, False) == ctx.verify_aggregate(a[0], a[1], a[2], a[3], r, a[4], a[5])
    assert ctx.verify_aggregate_checked(gx[0], gx[1], gx[2], gx[3], None, gx[4], gx[5], subgroup=True) is True
    # an off-curve commit fails under both settings, whatever the pairing says
    cx = gx[0].copy()
    pt = corc.array_to_points(name, cx[9:10])[0]
    cx[9] = g1_rows(C, [(pt[0], (pt[1] + 1) % C.p)])[0]
    for sg in (True, False):
        assert checked(gx, sg, cx=cx) is False
    e = np.zeros((0, 2 * w64(C)), dtype=np.uint64)
    s = np.zeros((0, 4), dtype=np.uint64)
    assert ctx.verify_aggregate_checked(e, e, s, s, s, subgroup=True) is True
    assert ctx.verify_aggregate_checked(e, e, s, s, None, subgroup=True) is True
    tampered = []
    if name == "BLS12381":
        T3 = g1_order_point(3)
        assert not gx[5][17] and not gx[4][0]
        pi17 = corc.array_to_points(name, gx[1][17:18])[0]
        px = gx[1].copy()
        px[17] = g1_rows(C, [K.point_add(C, pi17, T3)])[0]
        assert checked(gx, True, px=px) is False  # the unchecked answer is not asserted
        c0 = corc.array_to_points(name, gx[0][0:1])[0]
        cx0 = gx[0].copy()
        cx0[0] = g1_rows(C, [K.point_add(C, c0, T3)])[0]
        assert checked(gx, True, cx=cx0) is False
        tampered = [(gx[0], px), (cx0, gx[1])]
    # the device form on a caller's stream: stays asynchronous, the AND folded on the device
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(device=dev)
    cases = [(gx[0], gx[1], gx, 1), (bx[0], bx[1], bx, 0)] + [(c, p, gx, 0) for c, p in tampered]
    keep, oks = [], []
    for c, p, a, _ in cases:
        t = [torch.from_numpy(np.ascontiguousarray(v).view(np.int64 if v.dtype == np.uint64 else np.int32)).to(dev)
             for v in (c, a[4], p, a[5], a[2], a[3], r)]
        keep.append(t)
        oks.append(torch.full((1,), 7, dtype=torch.int32, device=dev))
    torch.cuda.synchronize(dev)
    for t, ok in zip(keep, oks):
        ctx.verify_aggregate_checked_device(*[v.data_ptr() for v in t], n, True, ok.data_ptr(), st.cuda_stream)
    st.synchronize()
    assert [int(o.item()) for o in oks] == [c[3] for c in cases]
