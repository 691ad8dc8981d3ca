"""GPU tests of the aggregated cell verification (kzgx_verify_cells_aggregate, its _device, _checked and
_checked_device forms): one pairing check of many coset openings,
  e(sum r_k pi_k, G2[l]) == e(sum_c rho_c C_c + sum_k r_k a_k pi_k - sum_t S_t G1[t], G2[0]).

Expected booleans never come from the code under test.  Every commitment and proof is a known multiple
of G (C = [P(tau)]G, pi = [p]G; infinity is the multiple 0) with the golden tau, so in arithmetic mod r
  cell k holds         <=>  (tau^l - a_k) p_k == c_k - I_k(tau)
  the aggregate holds  <=>  tau^l sum r_k p_k == sum r_k (c_k - I_k(tau) + a_k p_k)
where I_k is K.interpolate of the values as supplied (tampered or not) at kzgx.coset_points of the index
and flags as supplied, and a_k = x^l for a point x of that coset.  The honest proof exponent is
(P(tau) - (P mod (X^l - a))(tau)) / (tau^l - a) by K.poly_divmod, as in test_gpu_prove_cosets.oracle."""
import ctypes
import functools

import numpy as np
import pytest

import corc
import kzg_ref as K
import kzgx
from test_gpu_verify_aggregate import challenges128, scalars
from test_ntt_consts import bitrev as brev

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NO_SRS, ERR_DEGREE = -1, -4, -5
EXT, BITREV = kzgx.PROVE_COSETS_EXTENDED, kzgx.NTT_BITREV
SRS_POINTS = 130  # > 128 points: kzgx_verify_proof of the largest cell needs more G1 points than it opens


def w64(name):
    return kzgx.BASE_LIMBS[name]


@functools.lru_cache(maxsize=None)
def mulG(name, e):
    C = K.CURVES[name]
    return corc.scalar_mul(name, (C.gx, C.gy), e % C.r) if e % C.r else None


@functools.lru_cache(maxsize=None)
def coset_xs(name, k, kl, ext, bitrev, index):
    """the points of the cell as the library lists them for these flags (host arithmetic, test_coset_points.py)"""
    return tuple(corc.limbs_to_ints(kzgx.coset_points(name, k, kl, index, extended=bool(ext), bitrev=bool(bitrev))))


@functools.lru_cache(maxsize=None)
def interpolant_at_tau(name, k, kl, ext, bitrev, index, ys, tau):
    C = K.CURVES[name]
    xs = coset_xs(name, k, kl, ext, bitrev, index)
    return K.poly_eval(C, K.interpolate(C, list(zip(xs, ys))), tau)


class Cells:
    """a batch as the entry takes it: commits (exponents), and per cell the commit index, the cell index,
    the proof exponent and the l values in the order of the flags"""

    def __init__(self, name, k, kl, ext, bitrev, tau, commits, ci, idx, p, y):
        self.name, self.k, self.kl, self.ext, self.bitrev, self.tau = name, k, kl, ext, bitrev, tau
        self.C = K.CURVES[name]
        self.commits, self.ci, self.idx, self.p = list(commits), list(ci), list(idx), list(p)
        self.y = [tuple(v) for v in y]

    def copy(self):
        return Cells(self.name, self.k, self.kl, self.ext, self.bitrev, self.tau, self.commits, self.ci, self.idx,
                     self.p, self.y)

    def __len__(self):
        return len(self.p)

    @property
    def R(self):
        return 1 << (self.k - self.kl + self.ext)

    def terms(self, j):
        """(c, I(tau), a, p) of cell j from what is supplied"""
        r, l = self.C.r, 1 << self.kl
        xs = coset_xs(self.name, self.k, self.kl, self.ext, self.bitrev, self.idx[j])
        it = interpolant_at_tau(self.name, self.k, self.kl, self.ext, self.bitrev, self.idx[j], self.y[j], self.tau)
        return self.commits[self.ci[j]], it, pow(xs[0], l, r), self.p[j]

    def singles(self):
        r, tl = self.C.r, pow(self.tau, 1 << self.kl, self.C.r)
        out = []
        for j in range(len(self)):
            c, it, a, p = self.terms(j)
            out.append(((tl - a) * p - (c - it)) % r == 0)
        return out

    def aggregate(self, ch):
        r, tl = self.C.r, pow(self.tau, 1 << self.kl, self.C.r)
        lhs = rhs = 0
        for j, rk in enumerate(ch):
            c, it, a, p = self.terms(j)
            lhs += rk * p
            rhs += rk * (c - it + a * p)
        return (tl * lhs - rhs) % r == 0

    def arrays(self):
        """(commits, commit_inf, commit_index, cell_index, proofs, proof_inf, ys) as the ABI takes them"""
        cp = [mulG(self.name, e) for e in self.commits]
        pp = [mulG(self.name, e) for e in self.p]
        ys = np.stack([scalars(v) for v in self.y]) if self.y else np.zeros((0, 1 << self.kl, 4), dtype=np.uint64)
        return (corc.points_to_array(self.name, cp), np.array([q is None for q in cp], dtype=np.int32),
                np.array(self.ci, dtype=np.uint32), np.array(self.idx, dtype=np.uint32),
                corc.points_to_array(self.name, pp), np.array([q is None for q in pp], dtype=np.int32), ys)

    def flags(self):
        return (EXT if self.ext else 0) | (BITREV if self.bitrev else 0)


@functools.lru_cache(maxsize=None)
def honest(name, k, kl, ext, tau, P, i):
    """(proof exponent, values in the natural order j = 0..l-1) of polynomial P on coset i"""
    C = K.CURVES[name]
    r, l, R = C.r, 1 << kl, 1 << (k - kl + ext)
    w = kzgx.domain_root(name, k + ext)
    a = pow(w, i * l, r)
    P = list(P)
    rem = P if len(P) <= l else list(K.poly_divmod(C, P, [(-a) % r] + [0] * (l - 1) + [1])[1])
    p = (K.poly_eval(C, P, tau) - K.poly_eval(C, rem, tau)) * pow(pow(tau, l, r) - a, -1, r) % r
    return p, tuple(K.poly_eval(C, P, pow(w, i + R * j, r)) for j in range(l))


def make_cells(name, k, kl, ext, bitrev, count, tau):
    """count valid cells drawn from 3 polynomials of 2^k coefficients, interleaved; commitment 3 is never
    referenced; the last cell repeats the first; from 65 cells on cell 3 opens the zero polynomial (infinite
    commitment and proof, all values 0), cell 4 a constant (infinite proof) and cell 5 a polynomial of
    degree exactly l"""
    C = K.CURVES[name]
    n, l, kr = 1 << k, 1 << kl, k - kl + ext
    R = 1 << kr
    polys = [tuple(K.random_scalars(C, n, seed=0xCE11 + 64 * k + 8 * kl + j)) for j in range(4)]
    special = count >= 65 and kl < k
    if special:
        top = K.random_scalars(C, l + 1, seed=0xD06 + kl)
        top[l] = top[l] or 1
        polys += [(0,), (777,), tuple(top)]
    commits = [K.poly_eval(C, list(P), tau) for P in polys]
    ci, idx, p, y = [], [], [], []
    for j in range(count):
        pid, i = j % 3, (5 * j + j // 3) % R
        if special and j in (3, 4, 5):
            pid, i = j + 1, (j - 2) % R
        if j == count - 1 and count >= 2:
            pid, i = ci[0], nat0
        if j == 0:
            nat0 = i
        pj, yj = honest(name, k, kl, ext, tau, polys[pid], i)
        ci.append(pid)
        idx.append(brev(i, kr) if bitrev else i)
        p.append(pj)
        y.append([yj[brev(q, kl)] for q in range(l)] if bitrev else yj)
    b = Cells(name, k, kl, ext, bitrev, tau, commits, ci, idx, p, y)
    assert all(b.singles())
    if special:
        assert commits[4] == 0 and p[3] == 0 and not any(y[3]) and p[4] == 0 and commits[5] != 0 and p[5] != 0
    if k == kl:
        assert not any(p)  # one coset per domain: every quotient is zero
    return b


def tamper(b, pos, kind):
    """one tampering of cell pos, or None where the shape has no room for it"""
    t, r, l = b.copy(), b.C.r, 1 << b.kl
    y = list(t.y[pos])
    if kind == "value":
        y[l // 2] = (y[l // 2] + 1) % r
        t.y[pos] = tuple(y)
    elif kind == "swap":
        other = [q for q in range(1, l) if y[q] != y[0]]
        if not other:
            return None
        y[0], y[other[0]] = y[other[0]], y[0]
        t.y[pos] = tuple(y)
    elif kind == "cell_index":
        if b.R < 2:
            return None
        t.idx[pos] = (t.idx[pos] + 1) % b.R
    elif kind == "commit_index":
        t.ci[pos] = (t.ci[pos] + 1) % 4  # another commitment, the unreferenced one included
    else:
        t.p[pos] = (t.p[pos] + 1) % r  # another known multiple of G
    return t


def run(ctx, b, ch, checked=None):
    c, cf, ci, idx, p, pf, ys = b.arrays()
    r = None if ch is None else scalars(ch)
    kw = dict(challenges=r, commit_inf=cf, proof_inf=pf, extended=bool(b.ext), bitrev=bool(b.bitrev))
    if checked is None:
        return ctx.verify_cells_aggregate(c, ci, idx, p, ys, b.k, **kw)
    return ctx.verify_cells_aggregate_checked(c, ci, idx, p, ys, b.k, subgroup=checked, **kw)


def single(ctx, b, j):
    """kzgx_verify_proof of cell j over the points kzgx_coset_points lists"""
    c, cf, ci, idx, p, pf, ys = b.arrays()
    xs = kzgx.coset_points(b.name, b.k, b.kl, b.idx[j], extended=bool(b.ext), bitrev=bool(b.bitrev))
    return ctx.verify_proof(c[b.ci[j]], bool(cf[b.ci[j]]), p[j], bool(pf[j]), xs, ys[j])


@pytest.fixture(scope="module")
def env():
    made = {}

    def get(name):
        if name not in made:
            tau = K.default_tau(K.CURVES[name])
            ctx = kzgx.Context(name)
            ctx.set_default_table(0)  # small SRSs: keep the setups quick (the MSM paths have their own tests)
            ctx.gen_srs(tau, SRS_POINTS)
            ctx.gen_srs_g2(tau, SRS_POINTS)
            made[name] = (ctx, tau)
        return made[name]

    yield get
    for ctx, _ in made.values():
        ctx.close()


def check_batch(ctx, b, seed):
    """a valid batch, every tampering of three positions against the exponent prediction, and
    kzgx_verify_proof on a sample of cells"""
    n = len(b)
    ch = challenges128(b.C, n, seed=seed)
    assert b.aggregate(ch)
    assert run(ctx, b, ch) is True
    sample = sorted({0, n // 2, n - 1})
    for j in sample:
        assert single(ctx, b, j) is True, j
    seen = 0
    for pos in sample:
        for kind in ("value", "swap", "cell_index", "commit_index", "proof"):
            t = tamper(b, pos, kind)
            if t is None:
                continue
            truth = t.singles()
            want = t.aggregate(ch)
            if truth.count(False) == 1:
                assert want is False, (pos, kind)  # one failing cell, nonzero challenges
            if kind in ("value", "proof"):
                assert truth.count(False) >= 1 and not truth[pos], (pos, kind)
            assert run(ctx, t, ch) is want, (pos, kind)
            if pos == n // 2 or kind == "value":
                assert single(ctx, t, pos) is truth[pos], (pos, kind)
            seen += 1
    assert seen >= 4  # one cell of one point, or one coset per domain, still leaves four tamperings


# ---- 1. shapes and counts ---------------------------------------------------------------------------------
SHAPES = [(3, 0, 0), (3, 1, 0), (3, 2, 1), (3, 3, 0), (3, 3, 1), (4, 2, 1), (8, 6, 1), (8, 7, 1)]


@pytest.mark.parametrize("bitrev", [0, 1])
@pytest.mark.parametrize("k,kl,ext", SHAPES)
def test_shapes(env, k, kl, ext, bitrev):
    ctx, tau = env("BLS12381")
    check_batch(ctx, make_cells("BLS12381", k, kl, ext, bitrev, 8 if kl >= 6 else 7, tau), seed=5000 + 8 * k + kl)


@pytest.mark.parametrize("bitrev", [0, 1])
@pytest.mark.parametrize("count", [1, 2, 3, 65, 300])
def test_counts(env, count, bitrev):
    """one cell to more than one workgroup slice of the fold (l = 4: 64 cells side by side in a workgroup)"""
    ctx, tau = env("BLS12381")
    check_batch(ctx, make_cells("BLS12381", 4, 2, 1, bitrev, count, tau), seed=6000 + count)


@pytest.mark.parametrize("bitrev", [0, 1])
def test_cosets_larger_than_a_workgroup(bitrev):
    """l = 512: two column tiles of the fold, one cell per workgroup row"""
    name, C = "BLS12381", K.BLS12381
    tau = K.default_tau(C)
    b = make_cells(name, 10, 9, 1, bitrev, 3, tau)
    ch = challenges128(C, 3, seed=512)
    t = tamper(b, 1, "value")
    assert b.aggregate(ch) and t.singles() == [True, False, True] and not t.aggregate(ch)
    ctx = kzgx.Context(name)
    try:
        ctx.set_default_table(0)
        ctx.gen_srs(tau, 514)  # kzgx_verify_proof of 512 points wants more than 512 G1 points
        ctx.gen_srs_g2(tau, 513)
        assert run(ctx, b, ch) is True
        assert run(ctx, t, ch) is False
        assert single(ctx, b, 1) is True and single(ctx, t, 1) is False
    finally:
        ctx.close()


# ---- 2. explicit challenges compute the stated equation -------------------------------------------------
@pytest.mark.parametrize("bitrev", [0, 1])
def test_explicit_challenges_compute_the_stated_equation(env, bitrev):
    """two copies of one cell with one value off by +d and -d: under equal challenges the errors cancel
    and the aggregate is TRUE while both cells are false -- challenges a prover predicts prove nothing"""
    ctx, tau = env("BLS12381")
    b = make_cells("BLS12381", 4, 2, 1, bitrev, 3, tau)
    r, d = b.C.r, 0xD1FF
    b = Cells(b.name, b.k, b.kl, b.ext, b.bitrev, tau, b.commits, [b.ci[1]] * 2, [b.idx[1]] * 2, [b.p[1]] * 2,
              [b.y[1]] * 2)
    y0, y1 = list(b.y[0]), list(b.y[1])
    y0[2], y1[2] = (y0[2] + d) % r, (y1[2] - d) % r
    b.y = [tuple(y0), tuple(y1)]
    assert b.singles() == [False, False]
    assert single(ctx, b, 0) is False and single(ctx, b, 1) is False
    r0 = challenges128(b.C, 2, seed=99)[1]
    assert b.aggregate([r0, r0]) and run(ctx, b, [r0, r0]) is True
    assert not b.aggregate([r0, r0 + 1]) and run(ctx, b, [r0, r0 + 1]) is False


# ---- 3. log2l = 0 is kzgx_verify_aggregate at z_k = w^(i_k) -----------------------------------------------
@pytest.mark.parametrize("ext,bitrev", [(0, 0), (1, 0), (1, 1)])
def test_single_point_cosets_equal_verify_aggregate(env, ext, bitrev):
    ctx, tau = env("BLS12381")
    good = make_cells("BLS12381", 3, 0, ext, bitrev, 7, tau)
    ch = challenges128(good.C, 7, seed=31)
    for b in (good, tamper(good, 3, "value"), tamper(good, 6, "proof"), tamper(good, 0, "cell_index")):
        c, cf, ci, idx, p, pf, ys = b.arrays()
        zs = np.stack([kzgx.coset_points(b.name, 3, 0, i, extended=bool(ext), bitrev=bool(bitrev))[0] for i in b.idx])
        want = b.aggregate(ch)
        assert ctx.verify_aggregate(c[ci], p, zs, ys[:, 0], scalars(ch), cf[ci], pf) is want
        assert run(ctx, b, ch) is want
    assert good.aggregate(ch)


# ---- 4. library-drawn challenges ------------------------------------------------------------------------------
def test_library_drawn_challenges(env):
    ctx, tau = env("BLS12381")
    b = make_cells("BLS12381", 4, 2, 1, 1, 65, tau)
    bad = tamper(b, 17, "value")
    assert bad.singles().count(False) == 1
    for _ in range(2):  # successive calls draw again
        assert run(ctx, b, None) is True
        assert run(ctx, bad, None) is False


# ---- 5. the data-availability shape: 4096 values, extended, bit-reversed, 128 cells of 64 per blob --------
def test_data_availability_shape():
    """cells, proofs and commitments straight from ctx.ntt / ctx.prove_cosets / ctx.msm (paths with tests of
    their own); a verifier holding only 64 G1 and 65 G2 points gives the same answers"""
    C = K.BLS12381
    tau = K.default_tau(C)
    full, small = kzgx.Context("BLS12381"), kzgx.Context("BLS12381")
    try:
        for c, n1 in ((full, 4096), (small, 64)):
            c.set_default_table(0)
            c.gen_srs(tau, n1)
            c.gen_srs_g2(tau, 65)
        blobs = np.stack([scalars(K.random_scalars(C, 4096, seed=0xDA5 + b)) for b in range(2)])
        coeffs = full.ntt(blobs, inverse=True, bitrev=True)
        commits = np.stack([full.msm(coeffs[b])[0] for b in range(2)])
        xy, inf, y = full.prove_cosets(blobs, 6, extended=True, evals=True, bitrev=True)
        assert xy.shape == (2, 128, 12) and y.shape == (2, 128, 64, 4) and not inf.any()
        proofs, ys = xy.reshape(256, 12), y.reshape(256, 64, 4)
        ci = np.repeat(np.arange(2, dtype=np.uint32), 128)
        idx = np.tile(np.arange(128, dtype=np.uint32), 2)
        ch = scalars(challenges128(C, 256, seed=0xDA))
        swapped = ys.copy()
        swapped[77, [10, 11]] = swapped[77, [11, 10]]
        assert (ys[77, 10] != ys[77, 11]).any()
        exchanged = proofs.copy()
        exchanged[[5, 200]] = exchanged[[200, 5]]
        assert (proofs[5] != proofs[200]).any()
        cases = [(ci, proofs, ys, True), (ci, proofs, swapped, False), (ci, exchanged, ys, False),
                 (1 - ci, proofs, ys, False)]
        for ctx in (full, small):
            got = [ctx.verify_cells_aggregate(commits, a, idx, p, v, 12, challenges=ch, extended=True, bitrev=True)
                   for a, p, v, _ in cases]
            assert got == [w for _, _, _, w in cases], got
        # one cell through the per-cell path the parent commit offers
        xs = kzgx.coset_points("BLS12381", 12, 6, 77, extended=True, bitrev=True)
        assert full.verify_proof(commits[0], False, proofs[77], False, xs, ys[77]) is True
        assert full.verify_proof(commits[0], False, proofs[77], False, xs, swapped[77]) is False
    finally:
        full.close()
        small.close()


# ---- 6. the checked form -------------------------------------------------------------------------------------
def test_checked_form(env):
    from test_gpu_subgroup import g1_rows
    from test_subgroup_consts import g1_member, g1_order_point
    ctx, tau = env("BLS12381")
    C = K.BLS12381
    good = make_cells("BLS12381", 4, 2, 1, 1, 6, tau)
    bad = tamper(good, 4, "value")
    ch = challenges128(C, 6, seed=616)
    # cell 2's challenge: r_2 and r_2 a_2 mod r are multiples of 3, so that an order-3 component of its
    # proof is annihilated in both MSMs and leaves the unchecked equation as it was
    a2 = good.terms(2)[2]
    ch[2] = next(3 * j for j in range(1 << 20, 1 << 21) if (3 * j * a2 % C.r) % 3 == 0)
    assert good.aggregate(ch) and not bad.aggregate(ch)
    for b, want in ((good, True), (bad, False)):
        for sg in (True, False):
            assert run(ctx, b, ch, checked=sg) is want
        assert run(ctx, b, ch) is want  # an all-member batch: the checked answer is the unchecked one
    assert run(ctx, good, None, checked=True) is True
    c, cf, ci, idx, p, pf, ys = good.arrays()
    assert not pf[2]
    T3 = g1_order_point(3)
    off = K.point_add(C, corc.array_to_points("BLS12381", p[2:3])[0], T3)
    assert K.on_curve(C, off) and not g1_member(C, off)
    px = p.copy()
    px[2] = g1_rows(C, [off])[0]
    kw = dict(challenges=scalars(ch), commit_inf=cf, proof_inf=pf, extended=True, bitrev=True)
    assert ctx.verify_cells_aggregate_checked(c, ci, idx, px, ys, 4, subgroup=True, **kw) is False
    # on the curve: only the subgroup test can refuse it (the answer of the equation itself is not asserted)
    print("unchecked with the non-member proof:", ctx.verify_cells_aggregate(c, ci, idx, px, ys, 4, **kw))
    # an off-curve commitment fails under both settings, whatever the pairing says
    cx = c.copy()
    pt = corc.array_to_points("BLS12381", c[1:2])[0]
    cx[1] = g1_rows(C, [(pt[0], (pt[1] + 1) % C.p)])[0]
    for sg in (True, False):
        assert ctx.verify_cells_aggregate_checked(cx, ci, idx, p, ys, 4, subgroup=sg, **kw) is False


# ---- 7. the device entries on a caller's stream -------------------------------------------------------------
def dev_tensors(a, ch, dev, spare=True):
    """device copies of arrays() + challenges; the commitment and the value arrays get a spare trailing row"""
    import torch
    c, cf, ci, idx, p, pf, ys = a
    if spare:
        c = np.concatenate([c, np.zeros_like(c[:1])])
        cf = np.concatenate([cf, np.zeros_like(cf[:1])])
        ys = np.concatenate([ys, np.zeros_like(ys[:1])])
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.int32): np.int32}
    return [torch.from_numpy(np.ascontiguousarray(v).view(view[v.dtype])).to(dev)
            for v in (c, cf, ci, idx, p, pf, ys, scalars(ch))]


def dev_call(ctx, t, b, n_commits, ok, stream, checked=None):
    c, cf, ci, idx, p, pf, ys, r = (x.data_ptr() for x in t)
    kw = dict(extended=bool(b.ext), bitrev=bool(b.bitrev), stream=stream)
    if checked is None:
        ctx.verify_cells_aggregate_device(c, cf, n_commits, ci, idx, p, pf, ys, r, len(b), b.k, b.kl, ok.data_ptr(),
                                          **kw)
    else:
        ctx.verify_cells_aggregate_checked_device(c, cf, n_commits, ci, idx, p, pf, ys, r, len(b), b.k, b.kl,
                                                  checked, ok.data_ptr(), **kw)


@pytest.mark.parametrize("bitrev", [0, 1])
def test_device_entry_on_a_caller_stream(bitrev):
    """a fresh context and a fresh stream: the first call builds the twiddle table on the caller's stream"""
    import torch
    name, C = "BLS12381", K.BLS12381
    tau = K.default_tau(C)
    dev = torch.device("cuda", 0)
    good = make_cells(name, 4, 2, 1, bitrev, 65, tau)
    bad = tamper(good, 40, "value")
    oob_commit, oob_cell = good.copy(), good.copy()
    oob_commit.ci[33] = len(good.commits)
    oob_cell.idx[64] = good.R
    ch = challenges128(C, 65, seed=8)
    assert good.aggregate(ch) and not bad.aggregate(ch)
    cases = [(good, None, 1), (bad, None, 0), (oob_commit, None, 0), (oob_cell, None, 0), (good, True, 1),
             (bad, True, 0), (oob_commit, False, 0), (oob_cell, True, 0)]
    keep, before, oks = [], [], []
    for b, _, _ in cases:
        t = dev_tensors(b.arrays(), ch, dev)
        keep.append(t)
        before.append([x.clone() for x in t])
        oks.append(torch.full((3,), 7, dtype=torch.int32, device=dev))
    ctx = kzgx.Context(name)
    try:
        ctx.set_default_table(0)
        ctx.gen_srs(tau, 8)
        ctx.gen_srs_g2(tau, 8)
        torch.cuda.synchronize(dev)
        st = torch.cuda.Stream(device=dev)
        for (b, checked, _), t, ok in zip(cases, keep, oks):
            dev_call(ctx, t, b, len(b.commits), ok[1:], st.cuda_stream, checked)
        st.synchronize()
        assert [o.tolist() for o in oks] == [[7, want, 7] for _, _, want in cases]
        for t, t0 in zip(keep, before):
            assert all(bool((x == x0).all()) for x, x0 in zip(t, t0))  # the inputs are only read
    finally:
        ctx.close()


# ---- 8. statuses ---------------------------------------------------------------------------------------------------
def raw_host(ctx, a, ch, log2n, log2l, flags, checked=False, drop=None, count=None, n_commits=None):
    """the status of the host entry called directly (drop: the name of an argument passed as NULL)"""
    c, cf, ci, idx, p, pf, ys = (np.ascontiguousarray(v) for v in a)
    ok = ctypes.c_int(7)
    ptr = {"commits": kzgx._p(c), "commit_index": ci.ctypes.data_as(kzgx.u32p), "cell_index": idx.ctypes.data_as(kzgx.u32p),
           "proofs": kzgx._p(p), "ys": kzgx._p(ys), "challenges": None if ch is None else kzgx._p(ch),
           "ok": ctypes.byref(ok)}
    if drop:
        ptr[drop] = None
    args = [ctx.h, ptr["commits"], cf.ctypes.data_as(kzgx.intp), c.shape[0] if n_commits is None else n_commits,
            ptr["commit_index"], ptr["cell_index"], ptr["proofs"], pf.ctypes.data_as(kzgx.intp), ptr["ys"],
            ptr["challenges"], p.shape[0] if count is None else count, log2n, log2l, flags]
    if checked:
        return kzgx.lib().kzgx_verify_cells_aggregate_checked(*args, 1, ptr["ok"]), ok.value
    return kzgx.lib().kzgx_verify_cells_aggregate(*args, ptr["ok"]), ok.value


def raw_device(ctx, buf, log2n, log2l, flags, count=2, n_commits=2, checked=False, drop=None):
    """the status of the device entry on dummy device pointers: every refusal comes before anything is read"""
    ptr = {n: buf.data_ptr() for n in ("commits", "commit_index", "cell_index", "proofs", "ys", "challenges", "ok")}
    if drop:
        ptr[drop] = None
    args = [ctx.h, ptr["commits"], None, n_commits, ptr["commit_index"], ptr["cell_index"], ptr["proofs"], None,
            ptr["ys"], ptr["challenges"], count, log2n, log2l, flags]
    if checked:
        return kzgx.lib().kzgx_verify_cells_aggregate_checked_device(*args, 1, ptr["ok"], None)
    return kzgx.lib().kzgx_verify_cells_aggregate_device(*args, ptr["ok"], None)


def test_statuses(env):
    import torch
    ctx, tau = env("BLS12381")
    C = K.BLS12381
    b = make_cells("BLS12381", 4, 2, 1, 0, 3, tau)
    a, ch = b.arrays(), scalars(challenges128(C, 3, seed=2))
    buf = torch.zeros(4096, dtype=torch.int64, device=torch.device("cuda", 0))
    assert raw_host(ctx, a, ch, 4, 2, EXT) == (0, 1)
    for checked in (False, True):
        refused = [
            (4, 5, 0),                      # a coset larger than the domain
            (22, 2, EXT),                   # no 2^23 domain
            (23, 2, 0),
            (4, 2, EXT | 16),               # an unknown flag
            (4, 2, EXT | kzgx.NTT_INVERSE),
            (4, 2, EXT | kzgx.PROVE_ALL_EVALS),
        ]
        for log2n, log2l, flags in refused:
            assert raw_host(ctx, a, ch, log2n, log2l, flags, checked)[0] == ERR_ARG, (log2n, log2l, flags)
            assert raw_device(ctx, buf, log2n, log2l, flags, checked=checked) == ERR_ARG, (log2n, log2l, flags)
        for drop in ("commits", "commit_index", "cell_index", "proofs", "ys", "ok"):
            assert raw_host(ctx, a, ch, 4, 2, EXT, checked, drop=drop)[0] == ERR_ARG, drop
            assert raw_device(ctx, buf, 4, 2, EXT, checked=checked, drop=drop) == ERR_ARG, drop
        assert raw_device(ctx, buf, 4, 2, EXT, checked=checked, drop="challenges") == ERR_ARG  # host: drawn
        assert raw_host(ctx, a, None, 4, 2, EXT, checked) == (0, 1)
        # limits: n_commits + count + l points in B's MSM; count x l values of workspace
        assert raw_host(ctx, a, ch, 4, 0, 0, checked, count=0, n_commits=1 << 22)[0] == ERR_ARG
        assert raw_device(ctx, buf, 4, 0, 0, count=0, n_commits=1 << 22, checked=checked) == ERR_ARG
        assert raw_device(ctx, buf, 12, 12, 0, count=4097, checked=checked) == ERR_ARG
        # count == 0: true, and no commitment is needed
        assert raw_host(ctx, a, ch, 4, 2, EXT, checked, count=0) == (0, 1)
        assert raw_host(ctx, a, ch, 4, 2, EXT, checked, count=0, n_commits=0, drop="commits") == (0, 1)
        ok = torch.full((1,), 7, dtype=torch.int32, device=buf.device)
        args = [ctx.h, None, None, 0, None, None, None, None, None, buf.data_ptr(), 0, 4, 2, EXT]
        if checked:
            assert kzgx.lib().kzgx_verify_cells_aggregate_checked_device(*args, 1, ok.data_ptr(), None) == 0
        else:
            assert kzgx.lib().kzgx_verify_cells_aggregate_device(*args, ok.data_ptr(), None) == 0
        ctx.sync()
        assert int(ok.item()) == 1
        # host-side index errors
        for field, v in (("ci", len(b.commits)), ("idx", b.R)):
            t = b.copy()
            getattr(t, field)[1] = v
            assert raw_host(ctx, t.arrays(), ch, 4, 2, EXT, checked)[0] == ERR_ARG, field
    empty = Cells("BLS12381", 4, 2, 1, 0, tau, [], [], [], [], [])
    assert run(ctx, empty, None) is True and run(ctx, empty, [], checked=True) is True
    # setups: none; G1 only; too few G2 points; too few G1 points
    bare = kzgx.Context("BLS12381")
    try:
        bare.set_default_table(0)
        assert raw_host(bare, a, ch, 4, 2, EXT)[0] == ERR_NO_SRS
        assert raw_device(bare, buf, 4, 2, EXT) == ERR_NO_SRS
        bare.gen_srs(tau, 8)
        assert raw_host(bare, a, ch, 4, 2, EXT)[0] == ERR_NO_SRS  # no G2 setup
        assert raw_device(bare, buf, 4, 2, EXT, checked=True) == ERR_NO_SRS
        bare.gen_srs_g2(tau, 4)
        assert raw_host(bare, a, ch, 4, 2, EXT)[0] == ERR_NO_SRS  # l + 1 = 5 > 4 G2 points
        assert raw_device(bare, buf, 4, 2, EXT) == ERR_NO_SRS
        bare.gen_srs_g2(tau, 5)
        assert raw_host(bare, a, ch, 4, 2, EXT) == (0, 1)  # 8 >= l G1 points, 5 = l + 1 G2 points
        bare.gen_srs(tau, 3)
        assert raw_host(bare, a, ch, 4, 2, EXT, True)[0] == ERR_DEGREE  # l = 4 > 3 G1 points
        assert raw_device(bare, buf, 4, 2, EXT) == ERR_DEGREE
        bare.gen_srs(tau, 4)
        assert raw_host(bare, a, ch, 4, 2, EXT) == (0, 1)  # exactly l G1 points: 2^log2n exceeds the SRS
    finally:
        bare.close()


# ---- 9. BN254: domains of at most 4 points --------------------------------------------------------------------------
@pytest.mark.parametrize("bitrev", [0, 1])
@pytest.mark.parametrize("k,kl,ext", [(2, 1, 0), (1, 0, 1), (1, 1, 1), (2, 2, 0)])
def test_bn254(env, k, kl, ext, bitrev):
    ctx, tau = env("BN254")
    b = make_cells("BN254", k, kl, ext, bitrev, 5, tau)
    ch = challenges128(b.C, 5, seed=254)
    assert b.aggregate(ch) and run(ctx, b, ch) is True
    assert run(ctx, b, None, checked=True) is True
    t = tamper(b, 2, "value")
    assert t.singles().count(False) >= 1 and not t.aggregate(ch)
    assert run(ctx, t, ch) is False
    assert single(ctx, b, 2) is True and single(ctx, t, 2) is False


def test_bn254_refuses_shapes_beyond_its_domain(env):
    import torch
    ctx, tau = env("BN254")
    b = make_cells("BN254", 2, 1, 0, 0, 3, tau)
    a, ch = b.arrays(), scalars(challenges128(b.C, 3, seed=3))
    buf = torch.zeros(4096, dtype=torch.int64, device=torch.device("cuda", 0))
    assert raw_host(ctx, a, ch, 2, 1, 0) == (0, 1)
    for log2n, log2l, flags in ((2, 1, EXT), (3, 1, 0), (3, 2, 0), (12, 6, EXT)):
        assert raw_host(ctx, a, ch, log2n, log2l, flags)[0] == ERR_ARG
        assert raw_device(ctx, buf, log2n, log2l, flags) == ERR_ARG
