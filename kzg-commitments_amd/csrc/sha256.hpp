// SHA-256 (FIPS 180-4) in plain C++ for host and device: the one implementation
// behind kzgx_sha256, the host challenge helper and k_blob_challenge (blob.hip).
//
//   sha256_init(h)            the initial state
//   sha256_block(h, w)        one compression of the 16 message words w (each the
//                             big-endian reading of 4 message bytes); w is consumed
//                             as the rolling message schedule
//   sha256_finish(h, ...)     the padding blocks of a byte tail, then the digest bytes
//
// Everything is indexed by compile-time constants once unrolled, so on the device
// the state and the schedule stay in registers.  The blob messages are word-aligned
// and are fed to sha256_block directly (blob_msg.hpp); only kzgx_sha256 takes the
// general byte path of sha256_finish.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KZGX_HD __host__ __device__ inline
#else
#define KZGX_HD inline
#endif

namespace kzgx {

KZGX_HD uint32_t sha256_rotr(uint32_t x, int s) { return (x >> s) | (x << (32 - s)); }

KZGX_HD uint32_t sha256_k(int i) {
  // the round constants: the first 32 bits of the fractional parts of the cube
  // roots of the first 64 primes
  constexpr uint32_t K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
      0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
      0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
      0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
      0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
      0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
      0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
      0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  return K[i];
}

KZGX_HD void sha256_init(uint32_t h[8]) {
  h[0] = 0x6a09e667u;
  h[1] = 0xbb67ae85u;
  h[2] = 0x3c6ef372u;
  h[3] = 0xa54ff53au;
  h[4] = 0x510e527fu;
  h[5] = 0x9b05688cu;
  h[6] = 0x1f83d9abu;
  h[7] = 0x5be0cd19u;
}

KZGX_HD void sha256_block(uint32_t h[8], uint32_t w[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], k = h[7];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    if (i >= 16) {  // w[i] in the 16-word ring
      const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
      const uint32_t s0 = sha256_rotr(w15, 7) ^ sha256_rotr(w15, 18) ^ (w15 >> 3);
      const uint32_t s1 = sha256_rotr(w2, 17) ^ sha256_rotr(w2, 19) ^ (w2 >> 10);
      w[i & 15] += s0 + w[(i + 9) & 15] + s1;
    }
    const uint32_t S1 = sha256_rotr(e, 6) ^ sha256_rotr(e, 11) ^ sha256_rotr(e, 25);
    const uint32_t ch = (e & f) ^ (~e & g);
    const uint32_t t1 = k + S1 + ch + sha256_k(i) + w[i & 15];
    const uint32_t S0 = sha256_rotr(a, 2) ^ sha256_rotr(a, 13) ^ sha256_rotr(a, 22);
    const uint32_t maj = (a & b) ^ (a & c) ^ (b & c);
    const uint32_t t2 = S0 + maj;
    k = g;
    g = f;
    f = e;
    e = d + t1;
    d = c;
    c = b;
    b = a;
    a = t1 + t2;
  }
  h[0] += a;
  h[1] += b;
  h[2] += c;
  h[3] += d;
  h[4] += e;
  h[5] += f;
  h[6] += g;
  h[7] += k;
}

// 64 message bytes -> the 16 words of a block
KZGX_HD void sha256_words(const uint8_t* p, uint32_t w[16]) {
  for (int i = 0; i < 16; i++)
    w[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) | ((uint32_t)p[4 * i + 2] << 8) |
           (uint32_t)p[4 * i + 3];
}

// the last tail_len < 64 bytes of a message of total_len bytes whose whole blocks
// went through sha256_block: 0x80, zeros, the bit length (one block, or two when
// tail_len > 55), then the digest
KZGX_HD void sha256_finish(uint32_t h[8], const uint8_t* tail, size_t tail_len, uint64_t total_len, uint8_t out[32]) {
  uint8_t buf[128];
  for (size_t i = 0; i < 128; i++) buf[i] = 0;
  for (size_t i = 0; i < tail_len; i++) buf[i] = tail[i];
  buf[tail_len] = 0x80;
  const size_t end = tail_len > 55 ? 128 : 64;
  const uint64_t bits = total_len * 8;
  for (int i = 0; i < 8; i++) buf[end - 1 - i] = (uint8_t)(bits >> (8 * i));
  uint32_t w[16];
  for (size_t o = 0; o < end; o += 64) {
    sha256_words(buf + o, w);
    sha256_block(h, w);
  }
  for (int i = 0; i < 8; i++) {
    out[4 * i] = (uint8_t)(h[i] >> 24);
    out[4 * i + 1] = (uint8_t)(h[i] >> 16);
    out[4 * i + 2] = (uint8_t)(h[i] >> 8);
    out[4 * i + 3] = (uint8_t)h[i];
  }
}

// the whole digest of len bytes
KZGX_HD void sha256_bytes(const uint8_t* msg, size_t len, uint8_t out[32]) {
  uint32_t h[8], w[16];
  sha256_init(h);
  size_t o = 0;
  for (; o + 64 <= len; o += 64) {
    sha256_words(msg + o, w);
    sha256_block(h, w);
  }
  sha256_finish(h, msg + o, len - o, (uint64_t)len, out);
}

}  // namespace kzgx
