"""Reference codec (TEST INFRASTRUCTURE ONLY) for the compressed point encodings of
include/kzg_gpu.h "compressed points": plain Python integers, the roots by
pow(a, (p + 1) // 4, p) and pairing_ref.f2sqrt, nothing from the library.

Points are (x, y) integer pairs (G2: ((x.re, x.im), (y.re, y.im))), None is the
identity; a record that does not decode gives the string "invalid".

  ZCASH  BLS12-381.  G1: 48 bytes, x big-endian, byte 0 carries C 0x80 (must be 1),
         I 0x40 (infinity: S = 0 and every other bit zero), S 0x20 (y > (p - 1) / 2).
         G2: 96 bytes, x.im || x.re; S by y.im, or by y.re when y.im = 0.
  SEC1   both curves, G1: 0x02 | (y mod 2), then x big-endian in MODBYTES bytes;
         0x00 || 0 is the identity."""
import kzg_ref as K
import pairing_ref as PR

ZCASH, SEC1 = 0, 1
INVALID = "invalid"


def modbytes(C):
    return 32 if C.name == "BN254" else 48


def point_bytes(C, group, enc):
    """the record length, 0 where the combination is not offered"""
    if enc == ZCASH:
        return {1: 48, 2: 96}.get(group, 0) if C.name == "BLS12381" else 0
    if enc == SEC1:
        return 1 + modbytes(C) if group == 1 else 0
    return 0


# ---- the three sign rules --------------------------------------------------------
def sign_parity(C, y):
    return y & 1


def sign_lex_g1(C, y):
    return int(y > (C.p - 1) // 2)


def sign_lex_g2(C, y):
    return sign_lex_g1(C, y[1]) if y[1] != 0 else sign_lex_g1(C, y[0])


# ---- G1 --------------------------------------------------------------------------
def g1_compress_raw(C, x, y, enc, inf=False):
    """no validation: the sign of y as given (the device compress kernel's contract)"""
    nb = modbytes(C)
    if enc == ZCASH:
        assert C.name == "BLS12381"
        if inf:
            return bytes([0xC0]) + bytes(nb - 1)
        b = bytearray((x % (1 << 381)).to_bytes(nb, "big"))
        b[0] = (b[0] & 0x1F) | 0x80 | (sign_lex_g1(C, y) << 5)
        return bytes(b)
    assert enc == SEC1
    if inf:
        return bytes(1 + nb)
    return bytes([2 | sign_parity(C, y)]) + x.to_bytes(nb, "big")


def g1_compress(C, P, enc):
    if P is None:
        return g1_compress_raw(C, 0, 0, enc, inf=True)
    return g1_compress_raw(C, P[0], P[1], enc)


def g1_decompress(C, rec, enc):
    nb = modbytes(C)
    assert len(rec) == point_bytes(C, 1, enc)
    if enc == ZCASH:
        c, i, s = rec[0] >> 7 & 1, rec[0] >> 6 & 1, rec[0] >> 5 & 1
        x = int.from_bytes(bytes([rec[0] & 0x1F]) + rec[1:], "big")
        if not c:
            return INVALID
        if i:
            return None if (s == 0 and x == 0) else INVALID
        sign, want = sign_lex_g1, s
    else:
        x = int.from_bytes(rec[1:], "big")
        if rec[0] == 0:
            return None if x == 0 else INVALID
        if rec[0] not in (2, 3):
            return INVALID
        sign, want = sign_parity, rec[0] & 1
    if x >= C.p:
        return INVALID
    a = (x * x * x + C.b) % C.p
    y = pow(a, (C.p + 1) // 4, C.p)
    if y * y % C.p != a:
        return INVALID
    if sign(C, y) != want:
        if y == 0:
            return INVALID
        y = C.p - y
    return (x, y)


# ---- G2 (ZCash) ------------------------------------------------------------------
def g2_compress_raw(C, x, y, inf=False):
    assert C.name == "BLS12381"
    if inf:
        return bytes([0xC0]) + bytes(95)
    b = bytearray((x[1] % (1 << 381)).to_bytes(48, "big") + x[0].to_bytes(48, "big"))
    b[0] = (b[0] & 0x1F) | 0x80 | (sign_lex_g2(C, y) << 5)
    return bytes(b)


def g2_compress(C, Q):
    return g2_compress_raw(C, None, None, inf=True) if Q is None else g2_compress_raw(C, Q[0], Q[1])


def g2_decompress(C, rec):
    assert len(rec) == 96 and C.name == "BLS12381"
    p = C.p
    c, i, s = rec[0] >> 7 & 1, rec[0] >> 6 & 1, rec[0] >> 5 & 1
    xim = int.from_bytes(bytes([rec[0] & 0x1F]) + rec[1:48], "big")
    xre = int.from_bytes(rec[48:], "big")
    if not c:
        return INVALID
    if i:
        return None if (s == 0 and xim == 0 and xre == 0) else INVALID
    if xim >= p or xre >= p:
        return INVALID
    x = (xre, xim)
    a = PR.f2add(p, PR.f2mul(p, PR.f2mul(p, x, x), x), PR.twist(C).b2)
    y = PR.f2sqrt(p, a)
    if y is None:
        return INVALID
    if sign_lex_g2(C, y) != s:
        if y == (0, 0):
            return INVALID
        y = PR.f2neg(p, y)
    return (x, y)
