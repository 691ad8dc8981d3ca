"""CPU tests of the blob proofs' host utilities (include/kzg_gpu.h "blob proofs"): kzgx_sha256 and
kzgx_blob_challenge are host arithmetic in libkzgx.so and need no device.  They run the SHA-256 of
csrc/sha256.hpp and the message walk of csrc/blob_msg.hpp -- the code the device kernel runs -- so
the padding boundaries, which no blob message reaches (a blob's last block always holds 16 or 48
bytes), are tested here.  Expected values come from hashlib and the stated byte layout only."""
import hashlib

import numpy as np
import pytest

import kzg_ref as K
import kzgx

NAME = "BLS12381"
R = K.BLS12381.r
ERR_ARG = -1


def limbs(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def be(vals):
    return b"".join(int(v).to_bytes(32, "big") for v in vals)


def expect(vals, rec):
    m = b"FSBLOBVERIFY_V1_" + len(vals).to_bytes(16, "big") + be(vals) + rec
    assert len(m) == 80 + 32 * len(vals)
    d = int.from_bytes(hashlib.sha256(m).digest(), "big")
    return d // R, d % R


def draw(k, seed):
    vals = K.random_scalars(K.BLS12381, 1 << k, seed=seed)
    rec = hashlib.sha256(b"record %d %d" % (k, seed)).digest() + hashlib.sha256(b"tail %d" % seed).digest()[:16]
    return vals, rec


@pytest.mark.parametrize("length", [0, 1, 55, 56, 63, 64, 65, 119, 120, 128, 1000])
def test_sha256_padding_boundaries(length):
    msg = bytes((37 * i + 11) & 0xFF for i in range(length))
    assert kzgx.sha256(msg) == hashlib.sha256(msg).digest()


@pytest.mark.parametrize("k", [0, 1, 2, 6])
def test_blob_challenge_is_the_stated_layout(k):
    """both encodings (the order is the order given: a permuted blob is another message), with seeds searched
    by hashlib so that digest div r = 0, 1 and 2 each occur"""
    assert (1 << 256) // R == 2
    picked, seed = {}, 0
    while len(picked) < 3:
        vals, rec = draw(k, seed)
        picked.setdefault(expect(vals, rec)[0], (vals, rec))
        seed += 1
        assert seed < 400
    for q in (0, 1, 2):
        vals, rec = picked[q]
        for order in (vals, vals[::-1]):
            want = expect(order, rec)
            assert want[0] == q or order is not vals
            assert kzgx.blob_challenge(NAME, be(order), rec) == (want[1], True)
            assert kzgx.blob_challenge(NAME, limbs(order), rec) == (want[1], True)
            # KZGX_NTT_BITREV is accepted and changes nothing: the order is the order given
            assert kzgx.blob_challenge(NAME, be(order), rec, flags=kzgx.BLOB_BYTES | kzgx.NTT_BITREV) == (want[1], True)


@pytest.mark.parametrize("k", [0, 1, 2, 6])
def test_non_canonical_elements(k):
    vals, rec = draw(k, 77)
    n = 1 << k
    for pos in sorted({0, n // 2, n - 1}):
        for bad in (R, (vals[pos] % ((1 << 256) - R)) + R, (1 << 256) - 1):
            assert R <= bad < 1 << 256
            v = list(vals)
            v[pos] = bad
            z, ok = kzgx.blob_challenge(NAME, be(v), rec)
            assert ok is False and z == expect(v, rec)[1]  # still the hash of the bytes as given
    v = list(vals)
    v[n - 1] = R - 1
    assert kzgx.blob_challenge(NAME, be(v), rec) == (expect(v, rec)[1], True)


def test_statuses():
    import ctypes
    L = kzgx.lib()
    vals, rec = draw(1, 5)
    b = np.frombuffer(be(vals), dtype=np.uint8).copy()
    r = np.frombuffer(rec, dtype=np.uint8).copy()
    z = np.zeros(4, dtype=np.uint64)
    ok = ctypes.c_int(7)
    args = lambda curve=1, blob=b.ctypes.data, k=1, flags=kzgx.BLOB_BYTES, record=r.ctypes.data_as(kzgx.u8p), zp=kzgx._p(z): \
        L.kzgx_blob_challenge(curve, blob, k, flags, record, zp, ctypes.byref(ok))
    assert args() == 0 and ok.value == 1
    assert args(curve=0) == ERR_ARG  # BN254
    assert args(curve=5) == ERR_ARG
    assert args(flags=kzgx.BLOB_BYTES | 1) == ERR_ARG  # KZGX_NTT_INVERSE is not a blob flag
    assert args(flags=64) == ERR_ARG
    assert args(k=kzgx.ntt_max_log2(NAME) + 1) == ERR_ARG
    assert args(blob=None) == ERR_ARG and args(record=None) == ERR_ARG and args(zp=None) == ERR_ARG
    out = np.zeros(32, dtype=np.uint8)
    assert L.kzgx_sha256(None, 3, out.ctypes.data_as(kzgx.u8p)) == ERR_ARG
    assert L.kzgx_sha256(None, 0, None) == ERR_ARG
    assert L.kzgx_sha256(None, 0, out.ctypes.data_as(kzgx.u8p)) == 0
    assert out.tobytes() == hashlib.sha256(b"").digest()
