"""The block table's recoding, indexing and summation as a pure-Python model.

This is the specification msm_joint.hip follows (k_joint_halves /
k_joint_entries: the table; k_joint_index: the words; k_joint_accum and the
Horner pass: the sum), over integers mod r with the SRS point P_i stood in by
tau^i, so that an MSM is sum k_i tau^i mod r:

* the n_t tabled points are cut into blocks of g; block b holds g_b =
  min(g, n_t - b g) points, its last one is P_top;
* entry j < 2^(g_b - 1) of a block is P_top + sum_{i < g_b - 1} (2 j_i - 1) P_i;
* a scalar k is recoded in regular +-1 digits: odd k, u = k >> 1, d_w =
  2 u_w - 1 for w < bits - 1 and d_{bits-1} = +1; an even k runs as r - k with
  every sign flipped, 0 as r;
* points [n, blocks_used g) run as scalar 0, whole blocks beyond n are skipped;
* word(block, plane w) = the g_b sign bits (1 = plus), normalised to the
  stored half: a top bit of 0 complements the word and negates the entry;
  the index is masked to g_b - 1 bits, so idx < 2^(g_b - 1) whatever the
  scalars -- asserted here for every word the model forms;
* MSM = sum_w 2^w sum_blocks +- entry[block][idx].
"""
import pytest

import kzg_ref as K

CURVES = [K.BN254, K.BLS12381]


def recode(C, k):
    """plus-bits of scalar k's planes: bit w = 1 iff digit w is +1"""
    bits = C.r.bit_length()
    k %= C.r  # scalar_reduce
    flip = (k & 1) ^ 1  # odd_prepare: an even k (0 included) runs as r - k
    u = (C.r - k if flip else k) >> 1
    assert u < 1 << (bits - 1)
    p = u | (1 << (bits - 1))  # d_{bits-1} = +1
    return p ^ (((1 << bits) - 1) if flip else 0)


def block_table(C, pts, g):
    """entries[b][j] for every block of the tabled points pts"""
    tab = []
    for p0 in range(0, len(pts), g):
        blk = pts[p0:p0 + g]
        gb = len(blk)
        ent = []
        for j in range(1 << (gb - 1)):
            v = blk[gb - 1]
            for i in range(gb - 1):
                v += blk[i] if (j >> i) & 1 else -blk[i]
            ent.append(v % C.r)
        tab.append(ent)
    return tab


def index_word(signs, gb):
    """(idx, neg) of a plane's gb sign bits (bit i: point i of the block)"""
    top = (signs >> (gb - 1)) & 1
    low = (1 << (gb - 1)) - 1
    idx = (signs if top else ~signs) & low
    assert 0 <= idx < 1 << (gb - 1)  # the bound the accumulation's gather relies on
    return idx, top ^ 1


def joint_msm(C, tab, n_t, g, scalars, seen=None):
    bits = C.r.bit_length()
    n = len(scalars)
    nb = (n + g - 1) // g  # whole blocks beyond n are skipped
    total = 0
    for b in range(nb):
        gb = min(g, n_t - b * g)
        assert len(tab[b]) == 1 << (gb - 1)
        planes = [recode(C, scalars[b * g + i] if b * g + i < n else 0) for i in range(gb)]
        for w in range(bits):
            signs = sum(((planes[i] >> w) & 1) << i for i in range(gb))
            idx, neg = index_word(signs, gb)
            if seen is not None:
                if signs == (1 << gb) - 1:
                    seen.add("all_plus")
                if signs == 0:
                    seen.add("all_minus")
            e = tab[b][idx]
            total += (-e if neg else e) << w
    return total % C.r


def direct(C, pts, scalars):
    return sum(k * p for k, p in zip(scalars, pts)) % C.r


@pytest.mark.parametrize("C", CURVES, ids=lambda C: C.name)
@pytest.mark.parametrize("g", [2, 5, 8])
def test_recoding_sums_to_the_scalar(C, g):
    bits = C.r.bit_length()
    for k in [0, 1, 2, 3, C.r - 1, C.r - 2, (1 << 253) - 1, C.r, C.r + 5, (1 << 256) - 1] + K.random_scalars(C, 8, g):
        p = recode(C, k)
        assert sum((1 if (p >> w) & 1 else -1) << w for w in range(bits)) % C.r == k % C.r


@pytest.mark.parametrize("C", CURVES, ids=lambda C: C.name)
@pytest.mark.parametrize("g", [2, 5, 8])
def test_joint_msm_model(C, g):
    tau = K.default_tau(C)
    n_t = 37
    pts = [pow(tau, i, C.r) for i in range(n_t)]
    tab = block_table(C, pts, g)
    assert len(tab) == (n_t + g - 1) // g and len(tab[-1]) == 1 << ((n_t - 1) % g)
    edge = [0, 1, C.r - 1, C.r - 2, (1 << 253) - 1]
    for n in (1, g, g + 1, 2 * g + 3, n_t - 1, n_t):  # n < n_t: empty blocks and a padded partial block
        sc = K.random_scalars(C, n, seed=100 * g + n)
        for j, v in enumerate(edge):
            sc[(3 * j) % n] = v
        assert joint_msm(C, tab, n_t, g, sc) == direct(C, pts, sc), n
        for v in edge:  # every point on the same edge scalar
            assert joint_msm(C, tab, n_t, g, [v] * n) == direct(C, pts, [v] * n), (n, v)


@pytest.mark.parametrize("C", CURVES, ids=lambda C: C.name)
@pytest.mark.parametrize("g", [2, 5, 8])
def test_both_normalisation_branches(C, g):
    """scalars 1: u = 0, so every plane below the top is all-minus (complemented,
    negated entry 0) and the top plane all-plus (the last entry as stored);
    scalars 2 run as r - 2 with the signs flipped"""
    tau = K.default_tau(C)
    n_t = 37
    pts = [pow(tau, i, C.r) for i in range(n_t)]
    tab = block_table(C, pts, g)
    for v in (1, 2, C.r - 1):
        seen = set()
        assert joint_msm(C, tab, n_t, g, [v] * n_t, seen) == direct(C, pts, [v] * n_t)
        assert seen == {"all_plus", "all_minus"}, (v, seen)
    assert index_word((1 << g) - 1, g) == ((1 << (g - 1)) - 1, 0)
    assert index_word(0, g) == ((1 << (g - 1)) - 1, 1)
    assert index_word(1 << (g - 1), g) == (0, 0)
    assert index_word((1 << (g - 1)) - 1, g) == (0, 1)


@pytest.mark.parametrize("C", CURVES, ids=lambda C: C.name)
def test_index_bound_every_block_size(C):
    """idx < 2^(g_b - 1) for every block size up to the widest, the one-point
    block included, for every sign word at the extremes and random ones"""
    for gb in range(1, 26):
        rnd = K.random_scalars(C, 16, seed=gb)
        for signs in [0, 1, (1 << gb) - 1, 1 << (gb - 1), (1 << (gb - 1)) - 1] + [v & ((1 << gb) - 1) for v in rnd]:
            idx, neg = index_word(signs & ((1 << gb) - 1), gb)
            assert idx < 1 << (gb - 1) and neg in (0, 1)


@pytest.mark.parametrize("C", CURVES, ids=lambda C: C.name)
def test_degenerate_points(C):
    """tau = 0 / 1 / -1 / 2: zero, repeated and opposite "points"; the model's
    sums stay exact (the table's entries may be 0, the kernels' infinity)"""
    for tau in (0, 1, C.r - 1, 2):
        for g in (2, 5, 8):
            n_t = 21
            pts = [pow(tau, i, C.r) for i in range(n_t)]
            tab = block_table(C, pts, g)
            sc = K.random_scalars(C, n_t, seed=7 + g)
            sc[0], sc[1] = 12345, C.r - 12345
            assert joint_msm(C, tab, n_t, g, sc) == direct(C, pts, sc), (tau, g)
