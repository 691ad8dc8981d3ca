"""CPU: the radix-2 NTT domains of the scalar fields -- kzgx_ntt_max_log2 and
kzgx_domain_root (host arithmetic of libkzgx.so, no device) and the constants
csrc/gen_consts.py emits into curve_consts.h for csrc/ntt.hip.

Also the checker of tests/test_gpu_ntt.py: a recursive integer FFT over
K.BLS12381.r written here in plain Python, itself checked against the O(n^2)
definition at n = 64.  It shares nothing with the GPU code."""
import os
import sys

import pytest

import kzg_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kzg-commitments_amd", "csrc"))

BLS = K.BLS12381
BN = K.BN254
ROOT_32 = 0x16A2A19EDFE81F20D09B681922C813B4B63683508C2280B93829971F439F0D2B
BN_ROOT_2 = 0x9366C4800000000555150000000000122400000000000015
ERR_ARG = -1


# ---- the Python checker ---------------------------------------------------------
def bls_root(k):
    return pow(7, (BLS.r - 1) >> k, BLS.r)


def bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def _fft(a, w, r):
    n = len(a)
    if n == 1:
        return list(a)
    w2 = w * w % r
    even, odd = _fft(a[0::2], w2, r), _fft(a[1::2], w2, r)
    out = [0] * n
    t = 1
    for i in range(n // 2):
        x = t * odd[i] % r
        out[i] = (even[i] + x) % r
        out[i + n // 2] = (even[i] - x) % r
        t = t * w % r
    return out


def fft(a, w, r=None):
    """out[i] = sum_j a[j] w^(i j) mod r, len(a) a power of two, w of that order"""
    return _fft([int(v) for v in a], w, BLS.r if r is None else r)


def ifft(a, w, r=None):
    """the inverse: out[j] = n^-1 sum_i a[i] w^(-i j)"""
    r = BLS.r if r is None else r
    ninv = pow(len(a), -1, r)
    return [v * ninv % r for v in _fft([int(v) for v in a], pow(w, -1, r), r)]


def dft_definition(a, w, r):
    n = len(a)
    return [sum(a[j] * pow(w, i * j, r) for j in range(n)) % r for i in range(n)]


def test_python_fft_matches_the_definition():
    r, n = BLS.r, 64
    w = bls_root(6)
    a = K.random_scalars(BLS, n, 0xF0F7)
    a[0], a[1], a[2] = 0, 1, r - 1
    X = fft(a, w)
    assert X == dft_definition(a, w, r)
    assert ifft(X, w) == a
    winv = pow(w, -1, r)
    assert ifft(a, w) == [v * pow(n, -1, r) % r for v in dft_definition(a, winv, r)]
    assert fft([5], 1) == [5]


# ---- the library's host arithmetic -----------------------------------------------
def test_ntt_max_log2():
    import kzgx
    assert kzgx.ntt_max_log2("BLS12381") == 22 == kzgx.NTT_MAX_LOG2
    assert kzgx.ntt_max_log2("BN254") == 2
    assert kzgx.lib().kzgx_ntt_max_log2(7) == -1
    assert kzgx.NTT_TILE_LOG2 in (11, 12)
    assert (kzgx.NTT_INVERSE, kzgx.NTT_BITREV) == (1, 2)


def test_bls_domain_roots():
    import kzgx
    r = BLS.r
    roots = [kzgx.domain_root("BLS12381", k) for k in range(33)]
    for k in range(33):
        assert roots[k] == pow(7, (r - 1) >> k, r), k
    assert roots[32] == ROOT_32
    assert roots[0] == 1
    for k in range(1, 33):
        assert roots[k] * roots[k] % r == roots[k - 1], k
        assert pow(roots[k], 1 << (k - 1), r) == r - 1, k  # order exactly 2^k
    with pytest.raises(kzgx.KzgxError) as e:
        kzgx.domain_root("BLS12381", 33)
    assert e.value.status == ERR_ARG


def test_bn254_domain_roots():
    import kzgx
    r = BN.r
    assert kzgx.domain_root("BN254", 0) == 1
    assert kzgx.domain_root("BN254", 1) == r - 1
    assert kzgx.domain_root("BN254", 2) == BN_ROOT_2 == pow(2, (r - 1) >> 2, r)
    assert BN_ROOT_2 * BN_ROOT_2 % r == r - 1
    with pytest.raises(kzgx.KzgxError) as e:
        kzgx.domain_root("BN254", 3)
    assert e.value.status == ERR_ARG
    assert (r - 1) % 4 == 0 and (r - 1) % 8 != 0  # 2-adicity 2: no domain beyond n = 4


def test_unknown_curve_and_null_root():
    import ctypes
    import kzgx
    w = (ctypes.c_uint64 * 4)()
    assert kzgx.lib().kzgx_domain_root(7, 1, w) == ERR_ARG
    assert kzgx.lib().kzgx_domain_root(1, 1, None) == ERR_ARG


# ---- the emitted constants ---------------------------------------------------------
def test_emitted_twiddle_constants():
    import gen_consts as g
    with open(os.path.join(ROOT, "kzg-commitments_amd", "csrc", "curve_consts.h")) as f:
        text = f.read()
    for name, C, s in (("BN254", BN, 2), ("BLS12381", BLS, 32)):
        r = C.r
        assert g.two_adicity(r) == s
        assert "struct %sFrNtt {" % name in text
        assert "static constexpr int TWO_ADICITY = %d;" % s in text
        body = text[text.index("struct %sFrNtt {" % name):]
        body = body[:body.index("\n};\n")]  # up to the struct's closing line
        R = 1 << 256
        rows = [ln.strip().rstrip(",").rstrip("};") for ln in body.splitlines() if ln.strip().startswith("{0x")]
        assert len(rows) == 3 * (s + 1)
        for k in range(s + 1):
            w = g.domain_root(name, k)
            assert w == pow(g.NTT_GEN[name], (r - 1) >> k, r)
            # canonical root, Montgomery root, Montgomery 2^-k: R = 2^256
            assert rows[k] == g.arr(w, 8).rstrip("}")
            assert rows[s + 1 + k] == g.arr(g.mont(w, r, 8), 8).rstrip("}") == g.arr(w * R % r, 8).rstrip("}")
            assert rows[2 * (s + 1) + k] == g.arr(pow(1 << k, -1, r) * R % r, 8).rstrip("}")
    # the generators are quadratic non-residues: the roots have full order
    assert pow(7, (BLS.r - 1) // 2, BLS.r) == BLS.r - 1
    assert pow(2, (BN.r - 1) // 2, BN.r) == BN.r - 1
