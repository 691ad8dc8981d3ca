"""CPU: kzgx_coset_points (host arithmetic, no device) -- the l points whose values sit in chunk
`index` of the coset openings' y, in y's order.

Coset i of the size-D domain (D = R l, R = n / l cosets, 2 n / l extended) holds x(i, j) = w^(i + R j),
w = kzgx_domain_root(curve, log2 D).  Naturally chunk i is coset i, j ascending; with KZGX_NTT_BITREV
chunk p is coset brev_R(p) and offset q holds j = brev_l(q), so that the chunks are the consecutive
slices of the bit-reversed size-D evaluation array."""
import numpy as np
import pytest

import kzg_ref as K
import kzgx
from test_ntt_consts import bitrev

ERR_ARG = -1
SHAPES = [(3, 1), (4, 2), (5, 0), (3, 3)]


def ints(a):
    return [sum(int(v) << (64 * i) for i, v in enumerate(row)) for row in a]


@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("log2n,log2l", SHAPES)
def test_points_bls12381(log2n, log2l, extended):
    r = K.BLS12381.r
    kr = log2n - log2l + int(extended)
    R, l = 1 << kr, 1 << log2l
    w = kzgx.domain_root("BLS12381", kr + log2l)
    nat = [[pow(w, i + R * j, r) for j in range(l)] for i in range(R)]
    for i in range(R):
        assert ints(kzgx.coset_points("BLS12381", log2n, log2l, i, extended=extended)) == nat[i]
    # bit-reversed: the chunks of the bit-reversed size-D array of w^e
    D = R * l
    flat = [pow(w, bitrev(e, kr + log2l), r) for e in range(D)]
    for p in range(R):
        got = ints(kzgx.coset_points("BLS12381", log2n, log2l, p, extended=extended, bitrev=True))
        assert got == flat[p * l:(p + 1) * l]
        assert got == [nat[bitrev(p, kr)][bitrev(q, log2l)] for q in range(l)]
    # every point of coset i is a root of X^l - w^(i l)
    for i in range(R):
        assert {pow(x, l, r) for x in nat[i]} == {pow(w, i * l, r)}


@pytest.mark.parametrize("log2n,log2l,extended", [(2, 1, False), (2, 2, False), (1, 0, True), (1, 1, True),
                                                  (1, 0, False)])
def test_points_bn254(log2n, log2l, extended):
    r = K.BN254.r
    kr = log2n - log2l + int(extended)
    R, l = 1 << kr, 1 << log2l
    w = kzgx.domain_root("BN254", kr + log2l)
    for rev in (False, True):
        for p in range(R):
            i = bitrev(p, kr) if rev else p
            want = [pow(w, i + R * (bitrev(q, log2l) if rev else q), r) for q in range(l)]
            assert ints(kzgx.coset_points("BN254", log2n, log2l, p, extended=extended, bitrev=rev)) == want


def test_evals_flag_is_ignored():
    xs = np.zeros((4, 4), dtype=np.uint64)
    lib = kzgx.lib()
    assert lib.kzgx_coset_points(1, 4, 2, kzgx.PROVE_ALL_EVALS | kzgx.NTT_BITREV, 3, kzgx._p(xs)) == 0
    assert (xs == kzgx.coset_points("BLS12381", 4, 2, 3, bitrev=True)).all()


def test_bad_arguments():
    lib = kzgx.lib()
    xs = np.zeros((16, 4), dtype=np.uint64)
    p = kzgx._p(xs)
    ext = kzgx.PROVE_COSETS_EXTENDED
    assert lib.kzgx_coset_points(1, 3, 1, 0, 3, p) == 0
    assert lib.kzgx_coset_points(1, 3, 1, 0, 4, p) == ERR_ARG  # 4 cosets
    assert lib.kzgx_coset_points(1, 3, 1, ext, 7, p) == 0
    assert lib.kzgx_coset_points(1, 3, 1, ext, 8, p) == ERR_ARG  # 8 cosets
    assert lib.kzgx_coset_points(1, 3, 4, 0, 0, p) == ERR_ARG  # l > n
    assert lib.kzgx_coset_points(1, 3, 1, 16, 0, p) == ERR_ARG  # unknown flag
    assert lib.kzgx_coset_points(1, 3, 1, kzgx.NTT_INVERSE, 0, p) == ERR_ARG
    assert lib.kzgx_coset_points(1, 3, 1, 0, 0, None) == ERR_ARG
    assert lib.kzgx_coset_points(7, 3, 1, 0, 0, p) == ERR_ARG  # unknown curve
    mx = kzgx.ntt_max_log2("BLS12381")
    assert lib.kzgx_coset_points(1, mx, 0, 0, 0, p) == ERR_ARG  # no size-2n domain for the m = n products
    assert lib.kzgx_coset_points(1, mx, mx - 2, ext, 0, p) == ERR_ARG  # no size-2n domain to open on
    assert lib.kzgx_coset_points(1, 2 ** 32 - 1, 2 ** 32 - 1, 0, 0, p) == ERR_ARG
    # BN254: domains up to 4 points
    assert lib.kzgx_coset_points(0, 2, 1, 0, 1, p) == 0
    assert lib.kzgx_coset_points(0, 2, 1, ext, 0, p) == ERR_ARG  # D = 8
    assert lib.kzgx_coset_points(0, 2, 0, 0, 0, p) == ERR_ARG  # 2m = 8
    assert lib.kzgx_coset_points(0, 1, 0, ext, 3, p) == 0
    with pytest.raises(kzgx.KzgxError) as e:
        kzgx.coset_points("BLS12381", 3, 1, 4)
    assert e.value.status == ERR_ARG
