// The Fiat-Shamir message of a blob proof, walked block by block on the host and
// on the device by the same code (include/kzg_gpu.h "blob proofs" has the layout):
//
//   M = "FSBLOBVERIFY_V1_" (16 B) || n as 16-byte big-endian || element 0 .. n - 1,
//       32 bytes big-endian each, in the order given || the 48-byte commitment record
//   z = int_be(SHA-256(M)) mod r
//
// Every part is a whole number of 32-bit words, so the walk never touches a byte:
// block 0 is the 8 header words and element 0, each following block two elements,
// the last element shares a block with the record's first 8 words, and the final
// block holds its last 4 words, the 0x80 marker and the bit length (n = 1: the whole
// record, the marker and the length fit the second block).  (80 + 32 n) / 64 + 1
// compressions in all.
//
// `load(i, e)` hands element i as 8 words, most significant first, and the walk
// compares each against r on the way (words in registers either way).
#pragma once
#include "sha256.hpp"

namespace kzgx {

// e (8 words, most significant first) < r, with r's little-endian words rp
KZGX_HD bool blob_words_lt(const uint32_t e[8], const uint32_t* rp) {
  int cmp = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const uint32_t m = rp[7 - j];
    const int c = e[j] > m ? 1 : (e[j] < m ? -1 : 0);
    cmp = cmp == 0 ? c : cmp;
  }
  return cmp < 0;
}

// The digest of (n = 2^log2n elements, record) as 8 state words; returns false iff
// some element is >= r.  rec: the record's 12 big-endian words.  rp: r's words.
template <class Load>
KZGX_HD bool blob_digest(unsigned log2n, Load load, const uint32_t rec[12], const uint32_t* rp, uint32_t h[8]) {
  const uint64_t n = (uint64_t)1 << log2n;
  uint32_t w[16], e[8];
  bool ok = true;
  sha256_init(h);
  // "FSBLOBVERIFY_V1_", then n in 128 bits
  w[0] = 0x4653424cu;
  w[1] = 0x4f425645u;
  w[2] = 0x52494659u;
  w[3] = 0x5f56315fu;
  w[4] = 0;
  w[5] = 0;
  w[6] = (uint32_t)(n >> 32);
  w[7] = (uint32_t)n;
  load(0, e);
  ok = blob_words_lt(e, rp) && ok;
#pragma unroll
  for (int j = 0; j < 8; j++) w[8 + j] = e[j];
  sha256_block(h, w);
  const uint64_t bits = (80 + 32 * n) * 8;
  if (n == 1) {
#pragma unroll
    for (int j = 0; j < 12; j++) w[j] = rec[j];
    w[12] = 0x80000000u;
    w[13] = 0;
    w[14] = (uint32_t)(bits >> 32);
    w[15] = (uint32_t)bits;
    sha256_block(h, w);
    return ok;
  }
  for (uint64_t i = 1; i + 1 < n; i += 2) {
    load(i, e);
    ok = blob_words_lt(e, rp) && ok;
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = e[j];
    load(i + 1, e);
    ok = blob_words_lt(e, rp) && ok;
#pragma unroll
    for (int j = 0; j < 8; j++) w[8 + j] = e[j];
    sha256_block(h, w);
  }
  load(n - 1, e);
  ok = blob_words_lt(e, rp) && ok;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    w[j] = e[j];
    w[8 + j] = rec[j];
  }
  sha256_block(h, w);
#pragma unroll
  for (int j = 0; j < 4; j++) w[j] = rec[8 + j];
  w[4] = 0x80000000u;
#pragma unroll
  for (int j = 5; j < 14; j++) w[j] = 0;
  w[14] = (uint32_t)(bits >> 32);
  w[15] = (uint32_t)bits;
  sha256_block(h, w);
  return ok;
}

// digest words (h[0] most significant) -> z = digest mod r as 8 little-endian words:
// 2^256 div r = 2 on BLS12-381, so r is subtracted zero, one or two times
KZGX_HD void blob_reduce(const uint32_t h[8], const uint32_t* rp, uint32_t z[8]) {
#pragma unroll
  for (int j = 0; j < 8; j++) z[j] = h[7 - j];
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
    uint32_t d[8];
    uint32_t borrow = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint64_t t = (uint64_t)z[j] - rp[j] - borrow;
      d[j] = (uint32_t)t;
      borrow = (uint32_t)(t >> 63);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) z[j] = borrow ? z[j] : d[j];  // no borrow: z >= r
  }
}

}  // namespace kzgx
