// Compressed point encodings for gfx950: batched decompression (a square root
// per record) and compression, one lane per record, any count, one launch.
//
// Encodings (include/kzg_gpu.h has the byte-level rules):
//   KZGX_ENC_ZCASH  BLS12-381.  G1: 48 bytes, x big-endian, byte 0 carries
//                   C (0x80, must be 1), I (0x40, infinity), S (0x20, the sign:
//                   y > (p - 1) / 2).  G2: 96 bytes, x.im || x.re, S by y.im,
//                   or by y.re when y.im = 0.
//   KZGX_ENC_SEC1   both curves, G1: 0x02 | (y mod 2), then x big-endian;
//                   0x00 || 0 is infinity.
//
// k_g1_decompress: a = x^3 + b, y = a^((p + 1) / 4) (p = 3 mod 4 on both
// curves) by f29_inv's width-3 sliding window (f29_pow) over the constant exponent
// C::SQRT_EXP, accepted iff y^2 = a -- which is also the residue test.  The
// exponent is a compile-time constant, so every lane of a wave walks the same
// squarings and products.  A lane whose record is malformed, non-canonical
// or infinite runs the chain on the generator's x and has its result masked;
// with the subgroup test (BLS12-381) a lane without a root hands the
// generator to k_g1_check's chain (point_check.hpp), so the group law only
// ever sees curve points.  E(Fp) has odd order on both curves: y = 0 never
// occurs for a valid x, and a record that would need the other sign of y = 0
// is refused.
//
// k_g2_decompress: the complex method in Fp2 = Fp[i] for p = 3 mod 4
// (Adj and Rodriguez-Henriquez, "Square root computation over even extension
// fields", algorithm 9): a1 = a^((p - 3) / 4), alpha = a1^2 a, x0 = a1 a; the
// root is i x0 when alpha = -1, else (1 + alpha)^((p - 1) / 2) x0; accepted
// iff it squares to a.  Cold path (a setup's G2 half): the lanes may diverge
// on alpha, and an invalid lane takes the generator's x through the root and
// the generator through [r]Q.
//
// The sign rules are ONE device function each -- g1 parity, g1
// lexicographic, g2 lexicographic -- shared by both directions.
#include <hip/hip_runtime.h>

#include "kzgx_internal.hpp"
#include "point_check.hpp"

namespace kzgx {

// ---- sign rules on canonical words ------------------------------------------
template <class C>
KZGX_DEV uint32_t sign_parity(const uint32_t* y) {
  return y[0] & 1u;
}
// y > (p - 1) / 2
template <class C>
KZGX_DEV uint32_t sign_lex_g1(const uint32_t* y) {
  constexpr int N = C::Fp::N;
  int cmp = 0;  // most significant word first
#pragma unroll
  for (int i = N - 1; i >= 0; i--) {
    const int c = y[i] > C::HALF[i] ? 1 : (y[i] < C::HALF[i] ? -1 : 0);
    cmp = cmp == 0 ? c : cmp;
  }
  return cmp > 0 ? 1u : 0u;
}
// y.im > (p - 1) / 2, or y.im = 0 and y.re > (p - 1) / 2
template <class C>
KZGX_DEV uint32_t sign_lex_g2(const uint32_t* re, const uint32_t* im) {
  constexpr int N = C::Fp::N;
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < N; i++) o |= im[i];
  return o == 0 ? sign_lex_g1<C>(re) : sign_lex_g1<C>(im);
}

// ---- bytes <-> canonical words -----------------------------------------------
// 4 N big-endian bytes -> N little-endian words
template <int N>
KZGX_DEV void words_from_be(const uint8_t* __restrict__ b, uint32_t* w) {
#pragma unroll
  for (int i = 0; i < N; i++) {
    const uint8_t* q = b + 4 * (N - 1 - i);
    w[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3];
  }
}
template <int N>
KZGX_DEV void words_to_be(const uint32_t* w, uint8_t* __restrict__ b) {
#pragma unroll
  for (int i = 0; i < N; i++) {
    uint8_t* q = b + 4 * (N - 1 - i);
    q[0] = (uint8_t)(w[i] >> 24);
    q[1] = (uint8_t)(w[i] >> 16);
    q[2] = (uint8_t)(w[i] >> 8);
    q[3] = (uint8_t)w[i];
  }
}
// w < p, no early exit (w stays in registers)
template <class C>
KZGX_DEV bool words_lt_p(const uint32_t* w) {
  constexpr int N = C::Fp::N;
  int cmp = 0;
#pragma unroll
  for (int i = N - 1; i >= 0; i--) {
    const int c = w[i] > C::Fp::P[i] ? 1 : (w[i] < C::Fp::P[i] ? -1 : 0);
    cmp = cmp == 0 ? c : cmp;
  }
  return cmp < 0;
}
template <int N>
KZGX_DEV uint32_t words_or(const uint32_t* w) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < N; i++) o |= w[i];
  return o;
}
// w <- p - w for 0 < w < p
template <class C>
KZGX_DEV void words_neg(uint32_t* w) {
  constexpr int N = C::Fp::N;
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    const uint64_t d = (uint64_t)C::Fp::P[i] - w[i] - borrow;
    w[i] = (uint32_t)d;
    borrow = (uint32_t)(d >> 63);
  }
}

// a^e for a constant exponent e > 0: f29_inv is a plain fixed-exponent power (a width-3 sliding
// window over the words it is handed), here with (p + 1) / 4 in place of p - 2
template <class F, int NW>
KZGX_DEV F29<F> f29_pow(const F29<F>& a, const uint32_t (&e)[NW]) {
  return f29_inv<F, NW>(a, e);
}

// the head of a record: whether it is well formed, the identity, and the sign it asks for
struct RecHead {
  bool fmt_ok, identity;
  uint32_t want;
};
// ZCash flags in `head` (byte 0); rest_zero: every other bit of the record is zero
KZGX_DEV RecHead head_zcash(uint32_t head, bool rest_zero) {
  const bool fc = (head & 0x80u) != 0, fi = (head & 0x40u) != 0, fs = (head & 0x20u) != 0;
  RecHead h;
  h.fmt_ok = fc && (!fi || (!fs && rest_zero));
  h.identity = h.fmt_ok && fi;
  h.want = fs ? 1u : 0u;
  return h;
}
KZGX_DEV RecHead head_sec1(uint32_t head, bool rest_zero) {
  RecHead h;
  h.identity = head == 0u && rest_zero;
  h.fmt_ok = head == 2u || head == 3u || h.identity;
  h.want = head & 1u;
  return h;
}

// Two record arrays in one launch (count1 may be 0), as k_g1_check: lane k
// decodes record k of the first array for k < count0, else record k - count0
// of the second; the outputs hold count0 + count1 entries in that order.
template <class C>
__global__ __launch_bounds__(64) void k_g1_decompress(const uint8_t* __restrict__ b0, uint32_t count0,
                                                      const uint8_t* __restrict__ b1, uint32_t count1, uint32_t enc,
                                                      uint32_t subgroup, uint32_t* __restrict__ out_xy,
                                                      uint32_t* __restrict__ out_inf, uint32_t* __restrict__ ok) {
  using F = typename C::Fp29;
  constexpr int N = C::Fp::N;
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count0 + count1) return;
  const bool second = k >= count0;
  const uint32_t j = second ? k - count0 : k;
  const bool zc = enc == KZGX_ENC_ZCASH;  // uniform: a kernel argument
  const size_t rb = zc ? 4 * N : 4 * N + 1;
  const uint8_t* rec = (second ? b1 : b0) + (size_t)j * rb;
  uint32_t xw[N];
  words_from_be<N>(rec + (zc ? 0 : 1), xw);
  const uint32_t head = rec[0];
  if (zc) xw[N - 1] &= 0x1fffffffu;
  const bool x_zero = words_or<N>(xw) == 0;
  const RecHead h = zc ? head_zcash(head, x_zero) : head_sec1(head, x_zero);
  const bool run = h.fmt_ok && !h.identity && words_lt_p<C>(xw);
  // a = x^3 + b, on the generator's x for a masked lane
  F29<F> x = f29_reduce<F>(f29_to_mont<F>(f29_from_words<F, N>(xw)));
  const F29<F> gx = f29_const<F>(C::GX29);
#pragma unroll
  for (int i = 0; i < F::L; i++) x.v[i] = run ? x.v[i] : gx.v[i];
  uint32_t bw[N];
#pragma unroll
  for (int i = 0; i < N; i++) bw[i] = i == 0 ? C::BSMALL : 0u;
  const F29<F> b = f29_to_mont<F>(f29_from_words<F, N>(bw));
  const F29<F> a = f29_reduce<F>(f29_add<F>(f29_mul<F>(f29_sqr<F>(x), x), b));  // < 4m -> < m
  const F29<F> y = f29_reduce<F>(f29_pow<F, N>(a, C::SQRT_EXP));                // a^((p + 1) / 4)
  const bool is_sq = f29_is_zero<F>(f29_sub<F>(f29_sqr<F>(y), a, F::P2));       // < 4m
  uint32_t yw[N];
  f29_to_words<F, N>(f29_from_mont<F>(y), yw);
  const uint32_t s = zc ? sign_lex_g1<C>(yw) : sign_parity<C>(yw);
  const bool flip = s != h.want, y_zero = words_or<N>(yw) == 0;
  if (flip && !y_zero) words_neg<C>(yw);
  const bool valid = run && is_sq && !(flip && y_zero);
  bool member = true;
  if constexpr (!C::COFACTOR_ONE) {
    if (subgroup) {  // uniform: a kernel argument
      Affine<C> p;
      p.x = x;
      p.y = flip ? f29_sub<F>(f29_zero<F>(), y, F::P) : y;  // m - y
      if (!valid) {
        p.x = gx;
        p.y = f29_const<F>(C::GY29);
      }
      member = g1_in_subgroup<C>(p);
    }
  }
  const bool good = valid && member;
  uint32_t* o = out_xy + (size_t)k * 2 * N;
#pragma unroll
  for (int i = 0; i < N; i++) {
    o[i] = good ? xw[i] : 0u;
    o[N + i] = good ? yw[i] : 0u;
  }
  if (out_inf) out_inf[k] = good ? 0u : 1u;
  ok[k] = (h.identity || good) ? 1u : 0u;
}

// Canonical limbs (+ an optional infinity flag; all-zero limbs are infinity
// too) -> records.  Validates nothing: the sign is that of y as given.
template <class C>
__global__ __launch_bounds__(64) void k_g1_compress(const uint32_t* __restrict__ xy, const uint32_t* __restrict__ inf,
                                                    uint32_t count, uint32_t enc, uint8_t* __restrict__ out) {
  constexpr int N = C::Fp::N;
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const bool zc = enc == KZGX_ENC_ZCASH;
  const size_t rb = zc ? 4 * N : 4 * N + 1;
  const uint32_t* w = xy + (size_t)k * 2 * N;
  uint32_t xw[N], yw[N];
#pragma unroll
  for (int i = 0; i < N; i++) {
    xw[i] = w[i];
    yw[i] = w[N + i];
  }
  const bool is_inf = (inf && inf[k]) || (words_or<N>(xw) | words_or<N>(yw)) == 0;
  if (is_inf) {
#pragma unroll
    for (int i = 0; i < N; i++) xw[i] = 0;
  }
  uint8_t* rec = out + (size_t)k * rb;
  if (zc) {
    const uint32_t fl = is_inf ? 0xc0u : (0x80u | (sign_lex_g1<C>(yw) << 5));
    xw[N - 1] = (xw[N - 1] & 0x1fffffffu) | (fl << 24);
    words_to_be<N>(xw, rec);
  } else {
    rec[0] = is_inf ? 0u : (uint8_t)(2u | sign_parity<C>(yw));
    words_to_be<N>(xw, rec + 1);
  }
}

// a^e over the constant bits of e, most significant first (e > 0)
template <class C>
__device__ __noinline__ Fp2<C> f2_pow(const Fp2<C>& a, const uint32_t (&e)[C::Fp::N]) {
  constexpr int N = C::Fp::N;
  int i = 32 * N - 1;
  while (!((e[i >> 5] >> (i & 31)) & 1u)) i--;
  Fp2<C> r = a;
  for (i--; i >= 0; i--) {
    r = f2_sqr<C>(r);
    if ((e[i >> 5] >> (i & 31)) & 1u) r = f2_mul<C>(r, a);
  }
  return r;
}

// a root of a in Fp2 (header comment); false when a is not a square
template <class C>
__device__ __noinline__ bool f2_sqrt(const Fp2<C>& a, Fp2<C>& y) {
  const Fp2<C> a1 = f2_pow<C>(a, C::SQRT2_EXP);
  const Fp2<C> alpha = f2_mul<C>(f2_sqr<C>(a1), a);
  const Fp2<C> x0 = f2_mul<C>(a1, a);
  const Fp2<C> t = f2_add<C>(alpha, f2_one<C>());
  if (f2_is_zero<C>(t))
    y = Fp2<C>{fp_neg<typename C::Fp29>(x0.b), x0.a};  // i x0
  else
    y = f2_mul<C>(f2_pow<C>(t, C::HALF), x0);
  return f2_is_zero<C>(f2_sub<C>(f2_sqr<C>(y), a));
}

// G2, KZGX_ENC_ZCASH: records x.im || x.re -> canonical (x.re, x.im, y.re, y.im)
template <class C>
__global__ __launch_bounds__(64) void k_g2_decompress(const uint8_t* __restrict__ bytes, uint32_t count,
                                                      uint32_t subgroup, uint32_t* __restrict__ out_xy,
                                                      uint32_t* __restrict__ out_inf, uint32_t* __restrict__ ok) {
  using P = typename PairOf<C>::T;
  constexpr int N = C::Fp::N;
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const uint8_t* rec = bytes + (size_t)k * 8 * N;
  uint32_t xw[2 * N];  // re | im
  words_from_be<N>(rec, xw + N);
  words_from_be<N>(rec + 4 * N, xw);
  const uint32_t head = rec[0];
  xw[2 * N - 1] &= 0x1fffffffu;
  const RecHead h = head_zcash(head, words_or<2 * N>(xw) == 0);
  const bool run = h.fmt_ok && !h.identity && words_lt_p<C>(xw) && words_lt_p<C>(xw + N);
  G2A<C> q;
  q.x = run ? f2_from_canon<C>(xw) : f2_const<C>(P::G2X);
  const Fp2<C> a = f2_add<C>(f2_mul<C>(f2_sqr<C>(q.x), q.x), f2_const<C>(P::B2));
  const bool is_sq = f2_sqrt<C>(a, q.y);
  uint32_t yw[2 * N];  // re | im
  f2_to_canon<C>(q.y, yw);
  const bool flip = sign_lex_g2<C>(yw, yw + N) != h.want, y_zero = words_or<2 * N>(yw) == 0;
  if (flip) {  // -y, component-wise (a zero component stays zero)
    if (words_or<N>(yw)) words_neg<C>(yw);
    if (words_or<N>(yw + N)) words_neg<C>(yw + N);
    q.y = f2_neg<C>(q.y);
  }
  const bool valid = run && is_sq && !(flip && y_zero);
  bool member = true;
  if (subgroup) {  // uniform: a kernel argument
    if (!valid) {
      q.x = f2_const<C>(P::G2X);
      q.y = f2_const<C>(P::G2Y);
    }
    member = g2_in_subgroup<C>(q);
  }
  const bool good = valid && member;
  uint32_t* o = out_xy + (size_t)k * 4 * N;
  for (int i = 0; i < 2 * N; i++) {
    o[i] = good ? xw[i] : 0u;
    o[2 * N + i] = good ? yw[i] : 0u;
  }
  if (out_inf) out_inf[k] = good ? 0u : 1u;
  ok[k] = (h.identity || good) ? 1u : 0u;
}

template <class C>
__global__ __launch_bounds__(64) void k_g2_compress(const uint32_t* __restrict__ xy, const uint32_t* __restrict__ inf,
                                                    uint32_t count, uint8_t* __restrict__ out) {
  constexpr int N = C::Fp::N;
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const uint32_t* w = xy + (size_t)k * 4 * N;
  uint32_t xw[2 * N], yw[2 * N];  // re | im
  for (int i = 0; i < 2 * N; i++) {
    xw[i] = w[i];
    yw[i] = w[2 * N + i];
  }
  const bool is_inf = (inf && inf[k]) || (words_or<2 * N>(xw) | words_or<2 * N>(yw)) == 0;
  if (is_inf)
    for (int i = 0; i < 2 * N; i++) xw[i] = 0;
  const uint32_t fl = is_inf ? 0xc0u : (0x80u | (sign_lex_g2<C>(yw, yw + N) << 5));
  xw[2 * N - 1] = (xw[2 * N - 1] & 0x1fffffffu) | (fl << 24);
  uint8_t* rec = out + (size_t)k * 8 * N;
  words_to_be<N>(xw + N, rec);
  words_to_be<N>(xw, rec + 4 * N);
}

size_t point_bytes(int curve, int group, int encoding) {
  const bool bn = curve == KZGX_CURVE_BN254, bls = curve == KZGX_CURVE_BLS12381;
  if (!bn && !bls) return 0;
  if (encoding == KZGX_ENC_ZCASH) return !bls ? 0 : (group == 1 ? 48 : (group == 2 ? 96 : 0));
  if (encoding == KZGX_ENC_SEC1) return group != 1 ? 0 : (bn ? 33 : 49);
  return 0;
}

int g1_decompress2(Ctx* ctx, const uint8_t* d_b0, size_t count0, const uint8_t* d_b1, size_t count1, int encoding,
                   int subgroup, uint32_t* d_xy, uint32_t* d_inf, uint32_t* d_ok, hipStream_t st) {
  if (point_bytes(ctx->curve, 1, encoding) == 0) return KZGX_ERR_ARG;
  const size_t count = count0 + count1;
  if (count == 0) return KZGX_OK;
  if (count0 > 0x7fffffffu || count1 > 0x7fffffffu || !d_xy || !d_ok) return KZGX_ERR_ARG;
  const dim3 blk(64), grd((unsigned)((count + 63) / 64));
  const uint32_t sg = subgroup ? 1u : 0u, enc = (uint32_t)encoding;
  if (ctx->curve == KZGX_CURVE_BN254)
    hipLaunchKernelGGL(k_g1_decompress<BN254G1>, grd, blk, 0, st, d_b0, (uint32_t)count0, d_b1, (uint32_t)count1, enc,
                       sg, d_xy, d_inf, d_ok);
  else
    hipLaunchKernelGGL(k_g1_decompress<BLS12381G1>, grd, blk, 0, st, d_b0, (uint32_t)count0, d_b1, (uint32_t)count1,
                       enc, sg, d_xy, d_inf, d_ok);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int g1_compress(Ctx* ctx, const uint32_t* d_xy, const uint32_t* d_inf, size_t count, int encoding, uint8_t* d_out,
                hipStream_t st) {
  if (point_bytes(ctx->curve, 1, encoding) == 0) return KZGX_ERR_ARG;
  if (count == 0) return KZGX_OK;
  if (count > 0xffffffffu || !d_xy || !d_out) return KZGX_ERR_ARG;
  const dim3 blk(64), grd((unsigned)((count + 63) / 64));
  if (ctx->curve == KZGX_CURVE_BN254)
    hipLaunchKernelGGL(k_g1_compress<BN254G1>, grd, blk, 0, st, d_xy, d_inf, (uint32_t)count, (uint32_t)encoding,
                       d_out);
  else
    hipLaunchKernelGGL(k_g1_compress<BLS12381G1>, grd, blk, 0, st, d_xy, d_inf, (uint32_t)count, (uint32_t)encoding,
                       d_out);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int g2_decompress(Ctx* ctx, const uint8_t* d_b, size_t count, int subgroup, uint32_t* d_xy, uint32_t* d_inf,
                  uint32_t* d_ok, hipStream_t st) {
  if (point_bytes(ctx->curve, 2, KZGX_ENC_ZCASH) == 0) return KZGX_ERR_ARG;
  if (count == 0) return KZGX_OK;
  if (count > 0xffffffffu || !d_b || !d_xy || !d_ok) return KZGX_ERR_ARG;
  const dim3 blk(64), grd((unsigned)((count + 63) / 64));
  hipLaunchKernelGGL(k_g2_decompress<BLS12381G1>, grd, blk, 0, st, d_b, (uint32_t)count, subgroup ? 1u : 0u, d_xy,
                     d_inf, d_ok);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int g2_compress(Ctx* ctx, const uint32_t* d_xy, const uint32_t* d_inf, size_t count, uint8_t* d_out, hipStream_t st) {
  if (point_bytes(ctx->curve, 2, KZGX_ENC_ZCASH) == 0) return KZGX_ERR_ARG;
  if (count == 0) return KZGX_OK;
  if (count > 0xffffffffu || !d_xy || !d_out) return KZGX_ERR_ARG;
  const dim3 blk(64), grd((unsigned)((count + 63) / 64));
  hipLaunchKernelGGL(k_g2_compress<BLS12381G1>, grd, blk, 0, st, d_xy, d_inf, (uint32_t)count, d_out);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

}  // namespace kzgx
