"""Reference arithmetic (TEST INFRASTRUCTURE ONLY) for the blob proofs of include/kzg_gpu.h "blob
proofs": hashlib, plain Python integers mod r, and the oracle's curve arithmetic for the points --
nothing from the library but kzgx.domain_root (host constants, tests/test_ntt_consts.py).

A blob is the list of its n = 2^k values IN THE ORDER GIVEN; with bitrev position p holds the value
at w^brev(p).  Commitments and proofs are exponents (multiples of G), so a verdict is exponent
arithmetic with the golden tau:  p (tau - z) == c - y."""
import functools
import hashlib

import numpy as np

import corc
import kzg_ref as K
import kzgx
import point_codec_ref as PC
from test_ntt_consts import bitrev as brev

NAME = "BLS12381"
C = K.BLS12381
R = C.r
DOMAIN = b"FSBLOBVERIFY_V1_"
assert (1 << 256) // R == 2


def batch_inv(vals):
    """the inverses of nonzero vals mod r with one modular inversion (Montgomery's trick)"""
    pre, acc = [], 1
    for v in vals:
        pre.append(acc)
        acc = acc * v % R
    inv = pow(acc, -1, R)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * pre[i] % R
        inv = inv * vals[i] % R
    return out


@functools.lru_cache(maxsize=None)
def domain(k, bitrev):
    """w^e(p) for every position p of the order given"""
    w = kzgx.domain_root(NAME, k)
    pw, acc = [], 1
    for _ in range(1 << k):
        pw.append(acc)
        acc = acc * w % R
    return tuple(pw[brev(p, k)] for p in range(1 << k)) if bitrev else tuple(pw)


def bary(vals, k, bitrev, z):
    """P(z) from P's values in the order given, O(n); exactly the stored value on a domain point"""
    n, ws = 1 << k, domain(k, bool(bitrev))
    assert len(vals) == n
    z %= R
    for p in range(n):
        if ws[p] == z:
            return vals[p] % R
    inv = batch_inv([(z - x) % R for x in ws])
    s = sum(f * x % R * i for f, x, i in zip(vals, ws, inv)) % R
    return (pow(z, n, R) - 1) * pow(n, -1, R) % R * s % R


def blob_bytes(vals):
    """32-byte big-endian elements (values up to 2^256 - 1: non-canonical ones are representable)"""
    return b"".join(int(v).to_bytes(32, "big") for v in vals)


def blob_limbs(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def message(vals, record):
    assert len(record) == 48
    return DOMAIN + len(vals).to_bytes(16, "big") + blob_bytes(vals) + bytes(record)


def challenge(vals, record):
    """(digest div r in {0, 1, 2}, z)"""
    d = int.from_bytes(hashlib.sha256(message(vals, record)).digest(), "big")
    return d // R, d % R


@functools.lru_cache(maxsize=None)
def mulG(e):
    return corc.scalar_mul(NAME, (C.gx, C.gy), e % R) if e % R else None


def record(e):
    """the ZCash record of [e]G"""
    return PC.g1_compress(C, mulG(e), PC.ZCASH)


def off_curve_record():
    """a well-formed record whose x is on no curve point"""
    x = 5
    while PC.g1_decompress(C, PC.g1_compress_raw(C, x, 0, PC.ZCASH), PC.ZCASH) != PC.INVALID:
        x += 1
    return PC.g1_compress_raw(C, x, 0, PC.ZCASH)


def to_int(row):
    return sum(int(row[i]) << (64 * i) for i in range(4))


class Blobs:
    """a batch as the entries take it: per blob the values in the order given, the commitment record and
    the proof record; c / p are the exponents behind the records, None for a record that decodes to nothing"""

    def __init__(self, k, bitrev, tau, vals, c, p, crec=None, prec=None):
        self.k, self.bitrev, self.tau = k, bitrev, tau
        self.vals = [tuple(v) for v in vals]
        self.c, self.p = list(c), list(p)
        self.crec = list(crec) if crec else [record(e) for e in c]
        self.prec = list(prec) if prec else [record(e) for e in p]

    def copy(self):
        return Blobs(self.k, self.bitrev, self.tau, self.vals, self.c, self.p, self.crec, self.prec)

    def __len__(self):
        return len(self.vals)

    def set_c(self, j, e):
        self.c[j], self.crec[j] = e % R, record(e)

    def set_p(self, j, e):
        self.p[j], self.prec[j] = e % R, record(e)

    def zy(self, j):
        z = challenge(self.vals[j], self.crec[j])[1]
        return z, bary(self.vals[j], self.k, self.bitrev, z)

    def canonical(self, j):
        return all(v < R for v in self.vals[j])

    def residual(self, j):
        z, y = self.zy(j)
        return (self.p[j] * (self.tau - z) - self.c[j] + y) % R

    def singles(self):
        return [self.c[j] is not None and self.p[j] is not None and self.canonical(j) and self.residual(j) == 0
                for j in range(len(self))]

    def aggregate(self, ch):
        if any(c is None for c in self.c) or any(p is None for p in self.p):
            return False
        if not all(self.canonical(j) for j in range(len(self))):
            return False
        return sum(rk * self.residual(j) for j, rk in enumerate(ch)) % R == 0

    def data(self, as_bytes):
        """(blobs, commitment records, proof records) as the binding takes them"""
        flat = [v for b in self.vals for v in b]
        return (blob_bytes(flat) if as_bytes else blob_limbs(flat)), b"".join(self.crec), b"".join(self.prec)


def honest(k, bitrev, tau, vals):
    """(c, p, z, y) of one blob"""
    c = bary(vals, k, bitrev, tau)
    z = challenge(vals, record(c))[1]
    y = bary(vals, k, bitrev, z)
    return c, (c - y) * pow(tau - z, -1, R) % R, z, y


def make_blobs(k, bitrev, count, tau, seed=0xB10B):
    """count valid blobs of 2^k values; from 3 blobs on the last repeats the first; from 65 on blob 3 is all
    zero (identity commitment and proof) and blob 4 a constant (identity proof)"""
    n = 1 << k
    vals = [tuple(K.random_scalars(C, n, seed=seed + 131 * k + j)) for j in range(count)]
    if count >= 65:
        vals[3] = (0,) * n
        vals[4] = (777,) * n
    if count >= 3:
        vals[-1] = vals[0]
    cs, ps = [], []
    for v in vals:
        c, p, _, _ = honest(k, bitrev, tau, v)
        cs.append(c)
        ps.append(p)
    b = Blobs(k, bitrev, tau, vals, cs, ps)
    assert all(b.singles())
    return b


KINDS = ("value", "commit", "proof", "swap", "noncanonical", "offcurve")


def tamper(b, pos, kind):
    """one tampering at blob pos, or None where the batch has no room for it"""
    t, n = b.copy(), 1 << b.k
    if kind == "value":
        v = list(t.vals[pos])
        v[n // 2] = (v[n // 2] + 1) % R
        t.vals[pos] = tuple(v)
    elif kind == "commit":
        t.set_c(pos, t.c[pos] + 1)
    elif kind == "proof":
        t.set_p(pos, t.p[pos] + 1)
    elif kind == "swap":
        other = [q for q in range(len(b)) if b.p[q] != b.p[pos]]
        if not other:
            return None
        q = other[0]
        t.p[pos], t.p[q] = t.p[q], t.p[pos]
        t.prec[pos], t.prec[q] = t.prec[q], t.prec[pos]
    elif kind == "noncanonical":
        v = list(t.vals[pos])
        i = [q for q in range(n) if v[q] + R < 1 << 256]
        if not i:
            return None
        v[i[-1]] += R  # congruent to the valid value, and invalid
        t.vals[pos] = tuple(v)
    else:
        t.c[pos], t.crec[pos] = None, off_curve_record()
    return t
