"""GPU tests of the aggregated verification (kzgx_verify_aggregate / _device):
one pairing check of  e(sum r_k pi_k, [tau]G2) == e(sum r_k (C_k - [y_k]G + [z_k]pi_k), G2).

Expected booleans never come from the GPU: every commitment and proof is a
known multiple of G (C_k = [c_k]G, pi_k = [p_k]G; infinity = the multiple 0),
so with the known tau
  opening k holds      <=>  (tau - z_k) p_k == c_k - y_k                      (mod r)
  the aggregate holds  <=>  tau sum r_k p_k == sum r_k (c_k - y_k + z_k p_k)  (mod r).
K.verify_proof_tau (the group-side restatement) cross-checks the first of
these on a sample of every batch, kzgx_verify_single_batch on every opening."""
import numpy as np
import pytest

import corc
import kzg_ref as K

pytestmark = pytest.mark.gpu

CURVES = [("BN254", K.BN254), ("BLS12381", K.BLS12381)]
COUNTS = [1, 2, 3, 64, 513]


def w64(C):
    return 4 if C.name == "BN254" else 6


def scalars(vals):
    return corc.ints_to_limbs(list(vals), 4)


class Batch:
    """openings as exponents: c, p (multiples of G), z, y"""

    def __init__(self, name, C, tau, c, p, z, y):
        self.name, self.C, self.tau = name, C, tau
        self.c, self.p, self.z, self.y = list(c), list(p), list(z), list(y)

    def copy(self):
        return Batch(self.name, self.C, self.tau, self.c, self.p, self.z, self.y)

    def __len__(self):
        return len(self.c)

    def point(self, e):
        return corc.scalar_mul(self.name, (self.C.gx, self.C.gy), e % self.C.r) if e % self.C.r else None

    def arrays(self, cache):
        """(commits, proofs, zs, ys, commit_inf, proof_inf) as the ABI takes them"""
        def pts(es):
            for e in es:
                if e not in cache:
                    cache[e] = self.point(e)
            P = [cache[e] for e in es]
            return corc.points_to_array(self.name, P), np.array([q is None for q in P], dtype=np.int32)
        cx, ci = pts(self.c)
        px, pi = pts(self.p)
        return cx, px, scalars(self.z), scalars(self.y), ci, pi

    def singles(self):
        r, t = self.C.r, self.tau
        return [((t - z) * p - (c - y)) % r == 0 for c, p, z, y in zip(self.c, self.p, self.z, self.y)]

    def aggregate(self, ch):
        r, t = self.C.r, self.tau
        lhs = t * sum(rk * p for rk, p in zip(ch, self.p))
        rhs = sum(rk * (c - y + z * p) for rk, c, p, z, y in zip(ch, self.c, self.p, self.z, self.y))
        return (lhs - rhs) % r == 0


def ev(C, P, x):
    acc = 0
    for a in reversed(P):
        acc = (acc * x + a) % C.r
    return acc


def make_batch(name, C, tau, n):
    """n valid openings.  Slots 0..2 open at z = 0, 5, r - 3; from n = 64 on, slot 3 opens a root
    (y = 0), slot 4 the zero polynomial (infinite commitment and proof), slot 5 a constant (infinite
    proof), and slots 10..41 one commitment at 32 different points."""
    r = C.r
    polys = [K.random_scalars(C, 6, seed=900 + j) for j in range(5)]
    root = polys[4][:]
    root[0] = (root[0] - ev(C, root, 7)) % r  # root(7) = 0
    zr = K.random_scalars(C, n, seed=77 + n)
    c, p, z, y = [], [], [], []
    for k in range(n):
        P, zk = polys[k % 4], zr[k]
        if k < 3:
            zk = (0, 5, r - 3)[k]
        elif n >= 64 and k == 3:
            P, zk = root, 7
        elif n >= 64 and k == 4:
            P = [0]
        elif n >= 64 and k == 5:
            P = [12345]
        elif n >= 64 and 10 <= k < 42:
            P, zk = polys[0], 100 + k
        assert zk != tau
        ck, yk = ev(C, P, tau), ev(C, P, zk)
        c.append(ck)
        y.append(yk)
        z.append(zk)
        p.append((ck - yk) * pow(tau - zk, -1, r) % r)  # q(tau), q = (P - y) / (X - z)
    b = Batch(name, C, tau, c, p, z, y)
    assert all(b.singles())
    if n >= 64:
        assert y[3] == 0 and c[4] == 0 and p[4] == 0 and p[5] == 0 and c[5] != 0
    return b


def challenges128(C, n, seed):
    ch = [s % (1 << 128) for s in K.random_scalars(C, n, seed=seed)]
    ch[0] = 1
    assert all(ch)
    return ch


@pytest.fixture(scope="module")
def env():
    import kzgx
    made = {}

    def get(name, C):
        if name not in made:
            tau = K.default_tau(C)
            ctx = kzgx.Context(name)
            ctx.gen_srs(tau, 8)
            ctx.gen_srs_g2(tau, 2)
            made[name] = (ctx, tau, {})
        return made[name]

    yield get
    for ctx, _, _ in made.values():
        ctx.close()


def run(ctx, b, ch, cache):
    cx, px, z, y, ci, pi = b.arrays(cache)
    return ctx.verify_aggregate(cx, px, z, y, None if ch is None else scalars(ch), ci, pi)


def check_sample_against_group_oracle(b, cache):
    """the exponent truth of single openings against K.verify_proof_tau, on a few openings"""
    n = len(b)
    truth = b.singles()
    for k in sorted({0, 1, 2, 3, 4, 5, n // 2, n - 1} & set(range(n))):
        for e in (b.c[k], b.p[k]):
            if e not in cache:
                cache[e] = b.point(e)
        assert K.verify_proof_tau(b.C, b.tau, 8, cache[b.c[k]], cache[b.p[k]], [(b.z[k], b.y[k])]) == truth[k], k


@pytest.mark.parametrize("name,C", CURVES)
@pytest.mark.parametrize("n", COUNTS)
def test_valid_and_single_tampered_batches(name, C, n, env):
    ctx, tau, cache = env(name, C)
    b = make_batch(name, C, tau, n)
    ch = challenges128(C, n, seed=4000 + n)
    check_sample_against_group_oracle(b, cache)
    assert b.aggregate(ch)
    assert run(ctx, b, ch, cache) is True
    cx, px, z, y, ci, pi = b.arrays(cache)
    assert ctx.verify_single_batch(cx, px, z, y, ci, pi).tolist() == [True] * n
    for pos in sorted({0, n // 2, n - 1}):
        for kind in ("y", "z", "commit"):
            t = b.copy()
            if kind == "y":
                t.y[pos] = (t.y[pos] + 1) % C.r
            elif kind == "z":
                t.z[pos] = (t.z[pos] + 1) % C.r
            else:
                t.c[pos] = (t.c[pos] + 1) % C.r  # another known multiple of G
            truth = t.singles()
            assert truth.count(False) == 1 and not truth[pos], (pos, kind)
            assert not t.aggregate(ch)
            assert run(ctx, t, ch, cache) is False, (pos, kind)
            if pos == n // 2:
                check_sample_against_group_oracle(t, cache)
                tx = t.arrays(cache)
                assert ctx.verify_single_batch(tx[0], tx[1], tx[2], tx[3], tx[4], tx[5]).tolist() == truth


@pytest.mark.parametrize("name,C", CURVES)
def test_explicit_challenges_compute_the_stated_equation(name, C, env):
    """two openings of one commitment with y off by +1 and -1: under equal challenges the errors
    cancel and the aggregate is TRUE while both singles are false -- the entry computes the stated
    equation, and challenges a prover can predict prove nothing"""
    ctx, tau, cache = env(name, C)
    b = make_batch(name, C, tau, 3)
    b = Batch(name, C, tau, [b.c[1]] * 2, [b.p[1]] * 2, [b.z[1]] * 2, [b.y[1]] * 2)
    b.y[0] = (b.y[0] + 1) % C.r
    b.y[1] = (b.y[1] - 1) % C.r
    r0 = challenges128(C, 2, seed=99)[1]
    assert b.singles() == [False, False]
    cx, px, z, y, ci, pi = b.arrays(cache)
    assert ctx.verify_single_batch(cx, px, z, y, ci, pi).tolist() == [False, False]
    assert b.aggregate([r0, r0]) and run(ctx, b, [r0, r0], cache) is True
    assert not b.aggregate([r0, r0 + 1]) and run(ctx, b, [r0, r0 + 1], cache) is False


@pytest.mark.parametrize("name,C", CURVES)
def test_library_drawn_challenges(name, C, env):
    ctx, tau, cache = env(name, C)
    b = make_batch(name, C, tau, 64)
    bad = b.copy()
    bad.y[17] = (bad.y[17] + 5) % C.r
    assert bad.singles().count(False) == 1
    for _ in range(2):  # successive calls draw again
        assert run(ctx, b, None, cache) is True
        assert run(ctx, bad, None, cache) is False


@pytest.mark.parametrize("name,C", CURVES)
def test_empty_batch_and_argument_errors(name, C, env):
    import torch
    import kzgx
    ctx, tau, cache = env(name, C)
    e = np.zeros((0, 2 * w64(C)), dtype=np.uint64)
    s = np.zeros((0, 4), dtype=np.uint64)
    assert ctx.verify_aggregate(e, e, s, s, s) is True
    assert ctx.verify_aggregate(e, e, s, s, None) is True
    dev = torch.device("cuda", 0)
    buf = torch.zeros(64, dtype=torch.int64, device=dev)
    with pytest.raises(kzgx.KzgxError) as err:  # a null challenge pointer on the device entry
        ctx.verify_aggregate_device(buf.data_ptr(), None, buf.data_ptr(), None, buf.data_ptr(), buf.data_ptr(), None, 1,
                                    buf.data_ptr())
    assert err.value.status == -1
    bare = kzgx.Context(name)
    try:
        bare.gen_srs(tau, 8)  # G1 only: no G2 setup
        b = make_batch(name, C, tau, 2)
        with pytest.raises(kzgx.KzgxError) as err:
            run(bare, b, [1, 2], cache)
        assert err.value.status == -4
    finally:
        bare.close()


@pytest.mark.parametrize("name,C", CURVES)
def test_device_entry_on_a_caller_stream(name, C, env):
    import torch
    ctx, tau, cache = env(name, C)
    dev = torch.device("cuda", 0)
    n = 64
    good = make_batch(name, C, tau, n)
    bad = good.copy()
    bad.z[40] = (bad.z[40] + 1) % C.r
    ch = challenges128(C, n, seed=8)
    st = torch.cuda.Stream(device=dev)
    oks = []
    keep = []
    for b in (good, bad):
        cx, px, z, y, ci, pi = b.arrays(cache)
        t = [torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.int32)).to(dev)
             for a in (cx, ci, px, pi, z, y, scalars(ch))]
        ok = torch.full((1,), 7, dtype=torch.int32, device=dev)
        keep.append(t)
        oks.append(ok)
    torch.cuda.synchronize(dev)
    for t, ok in zip(keep, oks):
        ctx.verify_aggregate_device(*[x.data_ptr() for x in t], n, ok.data_ptr(), st.cuda_stream)
    st.synchronize()
    assert [int(o.item()) for o in oks] == [1, 0]
    assert good.aggregate(ch) and not bad.aggregate(ch)
