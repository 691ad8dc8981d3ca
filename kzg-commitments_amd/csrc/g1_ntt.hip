// Batched radix-2 discrete Fourier transform over G1 points for gfx950, and the
// all-domain openings (Feist-Khovratovich, "FK20") built on it (DESIGN.md
// "All-domain openings and the G1 NTT"), then its multi-point form, one
// opening per coset (DESIGN.md "Coset openings (multi-point FK20)").
//
//   forward: out[i] = sum_j [w^(i j)] in[j]          w = FrNtt::ROOT[log2 n]
//   inverse: out[j] = [n^-1] sum_i [w^(-i j)] in[i]
//
// the domains and index conventions of ntt.hip: the coefficient side in natural
// order, with bitrev the evaluation side indexed by the bit reversal of i.
//
// Points live as XYZZ records in the stream's workspace for the length of a
// transform.  One launch per radix-2 stage, one lane per butterfly and
// transform; a stage works in place:
//   decimation in frequency  (a, b) -> (a + b, [w^j](a - b))   natural in, bit-reversed out
//   decimation in time       (a, b) -> (a + [w^j] b, a - [w^j] b)   bit-reversed in, natural out
// The twiddle w^j comes from the context's Fr twiddle table (Montgomery values,
// converted to canonical bits in the lane) and costs one scalar multiplication:
// plain double-and-add over the 256 bits of the scalar words, a fixed trip
// count.  Butterfly index j is the same for every transform of the batch, and
// lanes are numbered transform-fastest, so from 64 transforms on a wave shares
// its twiddle and the additions of the zero bits are skipped by the whole wave.
// j = 0 takes no multiplication.  Every addition is the complete xyzz_add_impl
// (equal operands double, opposite operands and infinite operands are exact),
// so the result is the exact group element whatever the input.
//
// FK20, for n = 2^k coefficients f and the SRS s_j = [tau^j]G:
//   X = G1-DFT_2n(s_(n-2), ..., s_0, O x (n + 1))                    once per (k, SRS)
//   v = DFT_2n(f_(n-1), 0 x (n + 1), f_1, ..., f_(n-2)) / 2n          Fr, ntt.hip
//   u_i = [v_i] X_i                                                   k_fk_pointwise
//   h = the first n of the unscaled inverse G1-DFT_2n(u)              DIF: h_m lands at record 2 brev_k(m)
//   proofs = G1-DFT_n(h)                                              DIT over the even records: proof i at record 2 i
// so the two transforms chain in place with no permutation pass.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "curve.hpp"
#include "fixed_msm.hpp"  // xyzz_shfl_xor_add
#include "kzgx_internal.hpp"

namespace kzgx {

template <class C>
struct G1NttOf;
template <>
struct G1NttOf<BN254G1> {
  using T = BN254FrNtt;
};
template <>
struct G1NttOf<BLS12381G1> {
  using T = BLS12381FrNtt;
};

constexpr int G1N_BLOCK = 128;  // lanes per workgroup of the point kernels

// min waves per SIMD asked of the two kernels that multiply (VGPR budget).  At 1
// the BLS12-381 stage kernel holds its two points and the addition's temporaries
// in 256 VGPRs + 45 AGPRs with no scratch; at 2 (256 registers in all) it spills
// 192 B per lane (DESIGN.md "All-domain openings and the G1 NTT").
#ifndef KZGX_G1N_WAVES
#define KZGX_G1N_WAVES 1
#endif

struct alignas(16) G1NttScalar {
  uint32_t v[8];  // Montgomery
};

KZGX_DEV uint32_t g1n_brev(uint32_t x, uint32_t bits) { return bits ? __brev(x) >> (32 - bits) : 0u; }

// word w of e, w a runtime index: a select chain, so e stays in registers
template <class FR>
KZGX_DEV uint32_t g1n_word(const Fe<FR>& e, int w) {
  uint32_t r = 0;
#pragma unroll
  for (int i = 0; i < FR::N; i++) r = i == w ? e.v[i] : r;
  return r;
}

// [e] p, e canonical: 32 FR::N doublings, an addition per set bit
template <class C>
KZGX_DEV Xyzz<C> g1n_mul(const Xyzz<C>& p, const Fe<typename C::Fr>& e) {
  using FR = typename C::Fr;
  Xyzz<C> acc = xyzz_inf<C>();
#pragma unroll 1
  for (int w = FR::N - 1; w >= 0; w--) {
    const uint32_t word = g1n_word<FR>(e, w);
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      acc = xyzz_dbl_impl<C>(acc);
      if ((word >> b) & 1u) acc = xyzz_add_impl<C>(acc, p);
    }
  }
  return acc;
}

// the same for an affine (finite) base: mixed additions
template <class C>
KZGX_DEV Xyzz<C> g1n_mul_affine(const Affine<C>& a, const Fe<typename C::Fr>& e) {
  using FR = typename C::Fr;
  Xyzz<C> acc = xyzz_inf<C>();
#pragma unroll 1
  for (int w = FR::N - 1; w >= 0; w--) {
    const uint32_t word = g1n_word<FR>(e, w);
#pragma unroll 1
    for (int b = 31; b >= 0; b--) {
      acc = xyzz_dbl_impl<C>(acc);
      if ((word >> b) & 1u) acc = xyzz_add_affine_impl<C>(acc, a);
    }
  }
  return acc;
}

// ---- canonical affine points -> records ------------------------------------------
// record (b, pos) = in[b n + q], pos = q or its bit reversal
template <class C>
__global__ __launch_bounds__(G1N_BLOCK) void k_g1ntt_load(const uint32_t* __restrict__ in_xy,
                                                          const uint32_t* __restrict__ in_inf, uint32_t k,
                                                          uint32_t total, uint32_t in_brev,
                                                          uint32_t* __restrict__ rec) {
  constexpr int XW = xyzz_words<C>();
  const uint32_t t = blockIdx.x * G1N_BLOCK + threadIdx.x;
  if (t >= total) return;
  const uint32_t q = t & ((1u << k) - 1), pos = in_brev ? g1n_brev(q, k) : q;
  Affine<C> a;
  const bool fin = affine_from_canonical<C>(in_xy + (size_t)t * 2 * C::Fp::N, a) && !(in_inf && in_inf[t]);
  xyzz_store<C>(rec + ((size_t)(t - q) + pos) * XW, fin ? xyzz_from_affine<C>(a) : xyzz_inf<C>());
}

// ---- one radix-2 stage, in place ------------------------------------------------------
struct G1NttStage {
  uint32_t* rec;
  const uint32_t* table;  // w^j of the 2^K-th root, j <= 2^(K-1), Montgomery
  uint32_t K;
  uint32_t k;        // log2 of the transform
  uint32_t lh;       // log2 of the butterfly span
  uint32_t batch;    // transforms
  uint32_t tstride;  // records between transforms
  uint32_t pstride;  // records between a transform's positions
  uint32_t inverse, dit, scale;
  G1NttScalar ninv;  // scale: both outputs are also multiplied by it
};

template <class C>
__global__ __launch_bounds__(G1N_BLOCK, KZGX_G1N_WAVES) void k_g1ntt_stage(G1NttStage A) {
  using FR = typename C::Fr;
  constexpr int XW = xyzz_words<C>();
  const uint32_t t = blockIdx.x * G1N_BLOCK + threadIdx.x;
  if (t >= (A.batch << (A.k - 1))) return;
  const uint32_t b = t % A.batch, bf = t / A.batch;  // transform-fastest: bf is wave-uniform from 64 transforms on
  const uint32_t half = 1u << A.lh;
  const uint32_t jj = bf & (half - 1), a = ((bf >> A.lh) << (A.lh + 1)) | jj;
  uint32_t* pa = A.rec + ((size_t)b * A.tstride + (size_t)a * A.pstride) * XW;
  uint32_t* pb = pa + (size_t)half * A.pstride * XW;
  const bool mul = jj != 0 || A.scale;
  Fe<FR> e = fe_zero<FR>();
  if (mul) {
    // w_(2 half)^(+-jj) = table[jj << sh]; inverse: w^-i = -w^(N/2 - i), table[N/2] = -1 covers i = 0
    const uint32_t idx = jj << (A.K - 1 - A.lh);
    Fe<FR> w = fe_load<FR>(A.table + (size_t)(A.inverse ? (1u << (A.K - 1)) - idx : idx) * FR::N);
    if (A.inverse) w = fe_neg<FR>(w);
    if (A.scale) w = fe_mul<FR>(w, fe_const<FR>(A.ninv.v));
    e = fe_from_mont<FR>(w);
  }
  // frequency: the butterfly (round 0), then the twiddle on its difference;
  // time: the twiddle on b, then the butterfly (round 1); scale: round 2 takes
  // the stored sum through the multiplication once more, by n^-1 (w carries
  // it already).  Rounds of one body, so the kernel holds one copy of the
  // butterfly and one of the multiplication, and the multiplication runs with
  // nothing but its base and its accumulator live: a sits in memory meanwhile.
  Xyzz<C> v = xyzz_load<C>(pb);
  uint32_t* pv = pb;
#pragma unroll 1
  for (uint32_t round = 0; round < 2 + A.scale; round++) {
    if (round == 2) {
      xyzz_store<C>(pv, v);
      pv = pa;
      v = xyzz_load<C>(pa);
      e = fe_from_mont<FR>(fe_const<FR>(A.ninv.v));
    } else if (round == A.dit) {
      const Xyzz<C> u = xyzz_load<C>(pa);
      xyzz_store<C>(pa, xyzz_add_impl<C>(u, v));
      v = xyzz_add_impl<C>(u, xyzz_neg<C>(v));
    }
    if (round != 1 && mul) v = g1n_mul<C>(v, e);
  }
  xyzz_store<C>(pv, v);
}

// ---- records -> canonical affine points and flags ------------------------------------
// out[b n + d] = value i of transform b, i = d or its bit reversal (out_brev), read from
// position i (natural results) or brev(i) (pos_brev: a decimation-in-frequency result)
template <class C>
__global__ __launch_bounds__(G1N_BLOCK) void k_g1ntt_store(const uint32_t* __restrict__ rec, uint32_t k,
                                                           uint32_t total, uint32_t tstride, uint32_t pstride,
                                                           uint32_t pos_brev, uint32_t out_brev,
                                                           uint32_t* __restrict__ out_xy,
                                                           uint32_t* __restrict__ out_inf) {
  constexpr int XW = xyzz_words<C>();
  const uint32_t t = blockIdx.x * G1N_BLOCK + threadIdx.x;
  if (t >= total) return;
  const uint32_t b = t >> k, d = t & ((1u << k) - 1);
  const uint32_t pos = (pos_brev != 0) != (out_brev != 0) ? g1n_brev(d, k) : d;
  Affine<C> a;
  const bool fin = xyzz_to_affine_impl<C>(xyzz_load<C>(rec + ((size_t)b * tstride + (size_t)pos * pstride) * XW), a);
  affine_to_canonical<C>(out_xy + (size_t)t * 2 * C::Fp::N, a, fin);
  out_inf[t] = fin ? 0u : 1u;
}

// ---- FK20 --------------------------------------------------------------------------------
// record j of the setup's input: s_(n-2-j) for j <= n - 2, infinity above
template <class C>
__global__ __launch_bounds__(G1N_BLOCK) void k_fk_load_srs(const uint32_t* __restrict__ srs, uint32_t n,
                                                           uint32_t* __restrict__ rec) {
  constexpr int XW = xyzz_words<C>();
  const uint32_t j = blockIdx.x * G1N_BLOCK + threadIdx.x;
  if (j >= 2 * n) return;
  Xyzz<C> p = xyzz_inf<C>();
  if (j + 2 <= n) {
    Affine<C> a;
    if (affine_from_canonical<C>(srs + (size_t)(n - 2 - j) * 2 * C::Fp::N, a)) p = xyzz_from_affine<C>(a);
  }
  xyzz_store<C>(rec + (size_t)j * XW, p);
}

// X_i (record brev(i) of the decimation-in-frequency result) -> packed affine Montgomery, flag
template <class C>
__global__ __launch_bounds__(G1N_BLOCK) void k_fk_store_x(const uint32_t* __restrict__ rec, uint32_t k1,
                                                          uint32_t* __restrict__ x, uint32_t* __restrict__ xinf) {
  constexpr int XW = xyzz_words<C>(), AW = affine_words<C>();
  const uint32_t i = blockIdx.x * G1N_BLOCK + threadIdx.x;
  if (i >= (1u << k1)) return;
  Affine<C> a;
  const bool fin = xyzz_to_affine_impl<C>(xyzz_load<C>(rec + (size_t)g1n_brev(i, k1) * XW), a);
  affine_store<C>(x + (size_t)i * AW, a);
  xinf[i] = fin ? 0u : 1u;
}

// c = (f_(n-1), 0 x (n + 1), f_1, ..., f_(n-2)) / 2n per polynomial (canonical x Montgomery = canonical)
template <class FR>
__global__ __launch_bounds__(256) void k_fk_build_c(const uint32_t* __restrict__ f, size_t stride, uint32_t k,
                                                    uint32_t total, G1NttScalar ninv, uint32_t* __restrict__ c) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const uint32_t n = 1u << k, b = t >> (k + 1), j = t & (2 * n - 1);
  Fe<FR> v = fe_zero<FR>();
  if (j == 0 || j >= n + 2) {
    const uint32_t src = j == 0 ? n - 1 : j - n - 1;
    v = fe_mul<FR>(fe_load<FR>(f + ((size_t)b * stride + src) * FR::N), fe_const<FR>(ninv.v));
  }
  fe_store<FR>(c + (size_t)t * FR::N, v);
}

// record (b, i) = [v_(b, i)] X_i, i < 2n
template <class C>
__global__ __launch_bounds__(G1N_BLOCK, KZGX_G1N_WAVES) void k_fk_pointwise(const uint32_t* __restrict__ x,
                                                            const uint32_t* __restrict__ xinf,
                                                            const uint32_t* __restrict__ v, uint32_t k1,
                                                            uint32_t total, uint32_t* __restrict__ rec) {
  using FR = typename C::Fr;
  constexpr int XW = xyzz_words<C>(), AW = affine_words<C>();
  const uint32_t t = blockIdx.x * G1N_BLOCK + threadIdx.x;
  if (t >= total) return;
  const uint32_t i = t & ((1u << k1) - 1);
  Xyzz<C> p = xyzz_inf<C>();
  if (!xinf[i]) p = g1n_mul_affine<C>(affine_load<C>(x + (size_t)i * AW), fe_load<FR>(v + (size_t)t * FR::N));
  xyzz_store<C>(rec + (size_t)t * XW, p);
}

__global__ void k_g1n_fill(uint32_t* __restrict__ p, uint32_t count, uint32_t value) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t < count) p[t] = value;
}

// --------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------
static unsigned g1n_blocks(size_t lanes) { return (unsigned)((lanes + G1N_BLOCK - 1) / G1N_BLOCK); }

// the stages of `batch` transforms of 2^k records: decimation in frequency
// (spans n/2 .. 1) or in time (1 .. n/2); scale: the first stage also multiplies by n^-1
template <class C>
static int g1n_stages(Ctx* ctx, uint32_t* rec, uint32_t k, size_t batch, size_t tstride, uint32_t pstride,
                      bool inverse, bool dit, bool scale, hipStream_t st) {
  using T = typename G1NttOf<C>::T;
  if (k == 0) return KZGX_OK;
  G1NttStage a{};
  a.rec = rec;
  a.table = ctx->d_ntt_tw;
  a.K = (uint32_t)ctx->ntt_log2;
  a.k = k;
  a.batch = (uint32_t)batch;
  a.tstride = (uint32_t)tstride;
  a.pstride = pstride;
  a.inverse = inverse;
  a.dit = dit;
  for (int w = 0; w < 8; w++) a.ninv.v[w] = T::NINV_M[k][w];
  const unsigned blocks = g1n_blocks(batch << (k - 1));
  for (uint32_t s = 0; s < k; s++) {
    a.lh = dit ? s : k - 1 - s;
    a.scale = scale && s == 0;
    hipLaunchKernelGGL(k_g1ntt_stage<C>, dim3(blocks), dim3(G1N_BLOCK), 0, st, a);
  }
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

// transforms per chunk: at most G1_NTT_CHUNK_RECORDS records, one transform at least
static size_t g1n_chunk(uint32_t k) { return std::max<size_t>(1, G1_NTT_CHUNK_RECORDS >> k); }

template <class C>
static int g1_ntt_impl(Ctx* ctx, MsmWs& ws, const uint32_t* d_in_xy, const uint32_t* d_in_inf, uint32_t* d_out_xy,
                       uint32_t* d_out_inf, uint32_t k, size_t batch, bool inverse, bool bitrev, hipStream_t st) {
  constexpr int XW = xyzz_words<C>();
  constexpr size_t PW = 2 * C::Fp::N;
  const size_t n = (size_t)1 << k, chunk = g1n_chunk(k);
  KZGX_TRY(ntt_twiddles(ctx, k, st));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.g1n_rec, (std::min(batch, chunk) << k) * XW * sizeof(uint32_t), &ws.g1n_rec_b));
  for (size_t b0 = 0; b0 < batch; b0 += chunk) {
    const size_t cb = std::min(chunk, batch - b0), lanes = cb << k;
    hipLaunchKernelGGL(k_g1ntt_load<C>, dim3(g1n_blocks(lanes)), dim3(G1N_BLOCK), 0, st, d_in_xy + b0 * n * PW,
                       d_in_inf ? d_in_inf + b0 * n : nullptr, k, (uint32_t)lanes, (uint32_t)(inverse && bitrev),
                       ws.g1n_rec);
    KZGX_TRY(g1n_stages<C>(ctx, ws.g1n_rec, k, cb, n, 1, inverse, false, inverse, st));
    hipLaunchKernelGGL(k_g1ntt_store<C>, dim3(g1n_blocks(lanes)), dim3(G1N_BLOCK), 0, st, ws.g1n_rec, k,
                       (uint32_t)lanes, (uint32_t)n, 1u, 1u, (uint32_t)(!inverse && bitrev), d_out_xy + b0 * n * PW,
                       d_out_inf + b0 * n);
    KZGX_TRY_HIP(hipGetLastError());
  }
  return KZGX_OK;
}

int g1_ntt(Ctx* ctx, MsmWs& ws, const uint32_t* d_in_xy, const uint32_t* d_in_inf, uint32_t* d_out_xy,
           uint32_t* d_out_inf, unsigned log2n, size_t batch, bool inverse, bool bitrev, hipStream_t st) {
  if ((int)log2n > ntt_max_log2(ctx->curve)) return KZGX_ERR_ARG;
  if (batch == 0) return KZGX_OK;
  return ctx->curve == KZGX_CURVE_BN254
             ? g1_ntt_impl<BN254G1>(ctx, ws, d_in_xy, d_in_inf, d_out_xy, d_out_inf, log2n, batch, inverse, bitrev, st)
             : g1_ntt_impl<BLS12381G1>(ctx, ws, d_in_xy, d_in_inf, d_out_xy, d_out_inf, log2n, batch, inverse, bitrev,
                                       st);
}

template <class C>
static int prove_all_setup_impl(Ctx* ctx, MsmWs& ws, const uint32_t* d_srs, uint32_t k, hipStream_t st) {
  constexpr int XW = xyzz_words<C>(), AW = affine_words<C>();
  FkSetup& s = ctx->fk[k];
  if (s.ready) {
    // built on another stream, perhaps: order this one behind the build
    KZGX_TRY_HIP(hipStreamWaitEvent(st, s.ev, 0));
    return KZGX_OK;
  }
  const size_t m = (size_t)2 << k;
  if (!s.ev) KZGX_TRY_HIP(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
  KZGX_TRY(dev_alloc(ctx, (void**)&s.x, m * AW * sizeof(uint32_t), &s.x_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&s.inf, m * sizeof(uint32_t), &s.inf_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.g1n_rec, m * XW * sizeof(uint32_t), &ws.g1n_rec_b));
  KZGX_TRY(ntt_twiddles(ctx, k + 1, st));
  hipLaunchKernelGGL(k_fk_load_srs<C>, dim3(g1n_blocks(m)), dim3(G1N_BLOCK), 0, st, d_srs, (uint32_t)(m / 2),
                     ws.g1n_rec);
  KZGX_TRY(g1n_stages<C>(ctx, ws.g1n_rec, k + 1, 1, m, 1, false, false, false, st));
  hipLaunchKernelGGL(k_fk_store_x<C>, dim3(g1n_blocks(m)), dim3(G1N_BLOCK), 0, st, ws.g1n_rec, k + 1, s.x, s.inf);
  KZGX_TRY_HIP(hipGetLastError());
  KZGX_TRY_HIP(hipEventRecord(s.ev, st));
  s.ready = true;
  return KZGX_OK;
}

int prove_all_setup(Ctx* ctx, MsmWs& ws, const uint32_t* d_srs_canon, unsigned log2n, hipStream_t st) {
  if (log2n == 0) return KZGX_OK;  // one proof, infinity: no setup
  if ((int)log2n + 1 > ntt_max_log2(ctx->curve)) return KZGX_ERR_ARG;
  return ctx->curve == KZGX_CURVE_BN254 ? prove_all_setup_impl<BN254G1>(ctx, ws, d_srs_canon, log2n, st)
                                        : prove_all_setup_impl<BLS12381G1>(ctx, ws, d_srs_canon, log2n, st);
}

void prove_all_drop(Ctx* ctx) {
  for (auto& s : ctx->fk) s.ready = false;
  for (auto& row : ctx->fkm)
    for (auto& s : row) s.ready = false;
}

template <class C>
static int prove_all_impl(Ctx* ctx, MsmWs& ws, const uint32_t* d_srs, const uint32_t* d_coeffs, size_t stride,
                          uint32_t k, size_t batch, bool bitrev, uint32_t* d_out_xy, uint32_t* d_out_inf,
                          hipStream_t st) {
  using FR = typename C::Fr;
  using T = typename G1NttOf<C>::T;
  constexpr int XW = xyzz_words<C>();
  constexpr size_t PW = 2 * C::Fp::N;
  const size_t n = (size_t)1 << k, m = 2 * n;
  if (k == 0) {  // a constant's quotient is zero: one proof per polynomial, infinity
    for (size_t b0 = 0; b0 < batch; b0 += (size_t)1 << 30) {
      const size_t cb = std::min<size_t>((size_t)1 << 30, batch - b0);
      KZGX_TRY_HIP(hipMemsetAsync(d_out_xy + b0 * PW, 0, cb * PW * sizeof(uint32_t), st));
      hipLaunchKernelGGL(k_g1n_fill, dim3((unsigned)((cb + 255) / 256)), dim3(256), 0, st, d_out_inf + b0,
                         (uint32_t)cb, 1u);
    }
    KZGX_TRY_HIP(hipGetLastError());
    return KZGX_OK;
  }
  KZGX_TRY(prove_all_setup_impl<C>(ctx, ws, d_srs, k, st));
  const FkSetup& s = ctx->fk[k];
  const size_t chunk = g1n_chunk(k + 1), cmax = std::min(batch, chunk);
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.g1n_rec, cmax * m * XW * sizeof(uint32_t), &ws.g1n_rec_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.fk_c, cmax * m * FR::N * sizeof(uint32_t), &ws.fk_c_b));
  KZGX_TRY(ntt_twiddles(ctx, k + 1, st));
  G1NttScalar ninv;
  for (int w = 0; w < 8; w++) ninv.v[w] = T::NINV_M[k + 1][w];
  for (size_t b0 = 0; b0 < batch; b0 += chunk) {
    const size_t cb = std::min(chunk, batch - b0), lanes = cb * m;
    hipLaunchKernelGGL(k_fk_build_c<FR>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st,
                       d_coeffs + b0 * stride * FR::N, stride, k, (uint32_t)lanes, ninv, ws.fk_c);
    KZGX_TRY_HIP(hipGetLastError());
    KZGX_TRY(ntt(ctx, ws.fk_c, m, ws.fk_c, m, k + 1, cb, false, false, st));
    hipLaunchKernelGGL(k_fk_pointwise<C>, dim3(g1n_blocks(lanes)), dim3(G1N_BLOCK), 0, st, s.x, s.inf, ws.fk_c, k + 1,
                       (uint32_t)lanes, ws.g1n_rec);
    // h: the unscaled inverse transform of the 2n records (the scale sits in v); h_m at record 2 brev_k(m)
    KZGX_TRY(g1n_stages<C>(ctx, ws.g1n_rec, k + 1, cb, m, 1, true, false, false, st));
    // proofs: the forward transform of h over the even records, bit-reversed in, natural out
    KZGX_TRY(g1n_stages<C>(ctx, ws.g1n_rec, k, cb, m, 2, false, true, false, st));
    hipLaunchKernelGGL(k_g1ntt_store<C>, dim3(g1n_blocks(cb * n)), dim3(G1N_BLOCK), 0, st, ws.g1n_rec, k,
                       (uint32_t)(cb * n), (uint32_t)m, 2u, 0u, (uint32_t)bitrev, d_out_xy + b0 * n * PW,
                       d_out_inf + b0 * n);
    KZGX_TRY_HIP(hipGetLastError());
  }
  return KZGX_OK;
}

int prove_all(Ctx* ctx, MsmWs& ws, const uint32_t* d_srs_canon, const uint32_t* d_coeffs, size_t stride,
              unsigned log2n, size_t batch, bool bitrev, uint32_t* d_out_xy, uint32_t* d_out_inf, hipStream_t st) {
  if ((int)log2n + 1 > ntt_max_log2(ctx->curve)) return KZGX_ERR_ARG;
  if (batch == 0) return KZGX_OK;
  return ctx->curve == KZGX_CURVE_BN254
             ? prove_all_impl<BN254G1>(ctx, ws, d_srs_canon, d_coeffs, stride, log2n, batch, bitrev, d_out_xy,
                                       d_out_inf, st)
             : prove_all_impl<BLS12381G1>(ctx, ws, d_srs_canon, d_coeffs, stride, log2n, batch, bitrev, d_out_xy,
                                          d_out_inf, st);
}

// ---- coset openings: the multi-point FK20 -------------------------------------------------
// n = 2^k coefficients f, cosets of l = 2^kl points, m = n / l = 2^km.  Proof i is
// [q(tau)]G, q = f div (X^l - a_i), a_i = w_R^i:  q(tau) = sum_e a_i^e h_e with
//   h_e = sum_(t < l) sum_u F_t[u + e + 1] S_t[u],  F_t[q] = f[t + l q], S_t[u] = s[t + l u],
// l Toeplitz products of size m, each the FK20 of prove_all with n -> m:
//   X_t = G1-DFT_2m(S_t[m-2], ..., S_t[0], O x (m + 1))                 once per (k, kl, SRS), x[i][t]
//   v_t = DFT_2m(F_t[m-1], 0 x (m + 1), F_t[1], ..., F_t[m-2]) / 2m       batch l transforms, ntt.hip
//   u_i = sum_t [v_t,i] X_t,i                                            k_fkm_pointwise_sum
//   h = the first m of the unscaled inverse G1-DFT_2m(u)                 DIF: h_e at record 2 brev_km(e)
//   proofs = G1-DFT_R(h, O x (R - m))                                    DIT: R = m over the even records,
//                                                                        R = 2m over all, the odd ones cleared
// record (t, j) of the setup's input, j < 2m: S_t[m - 2 - j] for j <= m - 2, infinity above
template <class C>
__global__ __launch_bounds__(G1N_BLOCK) void k_fkm_load_srs(const uint32_t* __restrict__ srs, uint32_t km,
                                                            uint32_t kl, uint32_t* __restrict__ rec) {
  constexpr int XW = xyzz_words<C>();
  const uint32_t g = blockIdx.x * G1N_BLOCK + threadIdx.x;
  if (g >= (2u << (km + kl))) return;
  const uint32_t m = 1u << km, t = g >> (km + 1), j = g & (2 * m - 1);
  Xyzz<C> p = xyzz_inf<C>();
  if (j + 2 <= m) {
    Affine<C> a;
    if (affine_from_canonical<C>(srs + ((size_t)t + ((size_t)(m - 2 - j) << kl)) * 2 * C::Fp::N, a))
      p = xyzz_from_affine<C>(a);
  }
  xyzz_store<C>(rec + (size_t)g * XW, p);
}

// x[i][t] = value i of transform t (record brev(i) of its decimation-in-frequency result)
template <class C>
__global__ __launch_bounds__(G1N_BLOCK) void k_fkm_store_x(const uint32_t* __restrict__ rec, uint32_t km1,
                                                           uint32_t kl, uint32_t* __restrict__ x,
                                                           uint32_t* __restrict__ xinf) {
  constexpr int XW = xyzz_words<C>(), AW = affine_words<C>();
  const uint32_t g = blockIdx.x * G1N_BLOCK + threadIdx.x;
  if (g >= (1u << (km1 + kl))) return;
  const uint32_t i = g >> kl, t = g & ((1u << kl) - 1);
  Affine<C> a;
  const bool fin = xyzz_to_affine_impl<C>(xyzz_load<C>(rec + (((size_t)t << km1) + g1n_brev(i, km1)) * XW), a);
  affine_store<C>(x + (size_t)g * AW, a);
  xinf[g] = fin ? 0u : 1u;
}

// k_fk_build_c with a stride: c[(b, t)] = (F_t[m-1], 0 x (m + 1), F_t[1], ..., F_t[m-2]) / 2m
template <class FR>
__global__ __launch_bounds__(256) void k_fkm_build_c(const uint32_t* __restrict__ f, size_t stride, uint32_t km,
                                                     uint32_t kl, uint32_t total, G1NttScalar ninv,
                                                     uint32_t* __restrict__ c) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const uint32_t m = 1u << km, j = g & (2 * m - 1), t = (g >> (km + 1)) & ((1u << kl) - 1), b = g >> (km + 1 + kl);
  Fe<FR> v = fe_zero<FR>();
  if (j == 0 || j >= m + 2) {
    const uint32_t q = j == 0 ? m - 1 : j - m - 1;
    v = fe_mul<FR>(fe_load<FR>(f + ((size_t)b * stride + t + ((size_t)q << kl)) * FR::N), fe_const<FR>(ninv.v));
  }
  fe_store<FR>(c + (size_t)g * FR::N, v);
}

// record (b, i) = sum_(t < l) [v_(b, t, i)] x[i][t], i < 2m.  Lanes are numbered
// (b, i, t), t fastest over g = min(l, 64) of them: a lane multiplies its base by
// its scalar (l > 64: the terms t, t + 64, ... one after the other into one
// accumulator), then the g adjacent lanes fold with log2 g shuffle additions, the
// complete addition, and the lane of t = 0 stores.  Lanes past the last output
// carry infinity through the fold: no lane leaves before it.
template <class C>
__global__ __launch_bounds__(G1N_BLOCK, KZGX_G1N_WAVES) void k_fkm_pointwise_sum(
    const uint32_t* __restrict__ x, const uint32_t* __restrict__ xinf, const uint32_t* __restrict__ v, uint32_t km1,
    uint32_t kl, uint32_t outputs, uint32_t* __restrict__ rec) {
  using FR = typename C::Fr;
  constexpr int XW = xyzz_words<C>(), AW = affine_words<C>();
  const uint32_t lg = kl < 6 ? kl : 6, l = 1u << kl;
  const uint32_t lane = blockIdx.x * G1N_BLOCK + threadIdx.x;
  const uint32_t o = lane >> lg, t0 = lane & ((1u << lg) - 1);
  const uint32_t i = o & ((1u << km1) - 1), b = o >> km1;
  Xyzz<C> acc = xyzz_inf<C>();
  if (o < outputs) {
#pragma unroll 1
    for (uint32_t t = t0; t < l; t += 64) {
      const size_t xi = ((size_t)i << kl) + t;
      Xyzz<C> p = xyzz_inf<C>();
      if (!xinf[xi])
        p = g1n_mul_affine<C>(affine_load<C>(x + xi * AW), fe_load<FR>(v + ((((size_t)b << kl) + t) << km1 | i) * FR::N));
      acc = t == t0 ? p : xyzz_add_impl<C>(acc, p);
    }
  }
#pragma unroll 1
  for (int off = (1 << lg) >> 1; off >= 1; off >>= 1) acc = xyzz_shfl_xor_add<C>(acc, off);
  if (o < outputs && t0 == 0) xyzz_store<C>(rec + (size_t)o * XW, acc);
}

// the odd records of every transform (the outputs m .. 2m - 1 of the inverse transform) := infinity
template <class C>
__global__ __launch_bounds__(G1N_BLOCK) void k_fkm_clear_odd(uint32_t* __restrict__ rec, uint32_t total) {
  constexpr int XW = xyzz_words<C>();
  const uint32_t g = blockIdx.x * G1N_BLOCK + threadIdx.x;
  if (g < total) xyzz_store<C>(rec + ((size_t)2 * g + 1) * XW, xyzz_inf<C>());
}

// y: out[b D + q] = q < n ? in[b stride + q] : 0, the coefficients padded to the opened domain
template <class FR>
__global__ __launch_bounds__(256) void k_fkm_pad(const uint32_t* __restrict__ in, size_t stride, uint32_t k,
                                                 uint32_t kd, uint32_t total, uint32_t* __restrict__ out) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const uint32_t b = g >> kd, q = g & ((1u << kd) - 1);
  fe_store<FR>(out + (size_t)g * FR::N,
               q >> k ? fe_zero<FR>() : fe_load<FR>(in + ((size_t)b * stride + q) * FR::N));
}

// y: natural evaluation order -> coset order, out[b D + i l + j] = in[b D + i + R j]
template <class FR>
__global__ __launch_bounds__(256) void k_fkm_gather(const uint32_t* __restrict__ in, uint32_t kr, uint32_t kl,
                                                    uint32_t total, uint32_t* __restrict__ out) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const uint32_t c = g & ((1u << (kr + kl)) - 1), i = c >> kl, j = c & ((1u << kl) - 1);
  fe_store<FR>(out + (size_t)g * FR::N, fe_load<FR>(in + ((size_t)(g - c) + i + ((size_t)j << kr)) * FR::N));
}

template <class C>
static int prove_cosets_setup_impl(Ctx* ctx, MsmWs& ws, const uint32_t* d_srs, uint32_t k, uint32_t kl,
                                   hipStream_t st) {
  constexpr int XW = xyzz_words<C>(), AW = affine_words<C>();
  FkSetup& s = ctx->fkm[k][kl];
  if (s.ready) {
    KZGX_TRY_HIP(hipStreamWaitEvent(st, s.ev, 0));
    return KZGX_OK;
  }
  const uint32_t km = k - kl;
  const size_t pts = (size_t)2 << k;  // l transforms of 2m points
  if (!s.ev) KZGX_TRY_HIP(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
  KZGX_TRY(dev_alloc(ctx, (void**)&s.x, pts * AW * sizeof(uint32_t), &s.x_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&s.inf, pts * sizeof(uint32_t), &s.inf_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.g1n_rec, pts * XW * sizeof(uint32_t), &ws.g1n_rec_b));
  KZGX_TRY(ntt_twiddles(ctx, km + 1, st));
  hipLaunchKernelGGL(k_fkm_load_srs<C>, dim3(g1n_blocks(pts)), dim3(G1N_BLOCK), 0, st, d_srs, km, kl, ws.g1n_rec);
  KZGX_TRY(g1n_stages<C>(ctx, ws.g1n_rec, km + 1, (size_t)1 << kl, (size_t)2 << km, 1, false, false, false, st));
  hipLaunchKernelGGL(k_fkm_store_x<C>, dim3(g1n_blocks(pts)), dim3(G1N_BLOCK), 0, st, ws.g1n_rec, km + 1, kl, s.x,
                     s.inf);
  KZGX_TRY_HIP(hipGetLastError());
  KZGX_TRY_HIP(hipEventRecord(s.ev, st));
  s.ready = true;
  return KZGX_OK;
}

// the shapes the coset entries take: the size-2m and the size-D domains must exist
static bool prove_cosets_shape_ok(const Ctx* ctx, unsigned log2n, unsigned log2l, bool ext) {
  const int mx = ntt_max_log2(ctx->curve);
  return log2l <= log2n && (int)(log2n - log2l) + 1 <= mx && (int)log2n + (ext ? 1 : 0) <= mx;
}

int prove_cosets_setup(Ctx* ctx, MsmWs& ws, const uint32_t* d_srs_canon, unsigned log2n, unsigned log2l,
                       hipStream_t st) {
  if (!prove_cosets_shape_ok(ctx, log2n, log2l, false)) return KZGX_ERR_ARG;
  if (log2n == log2l) return KZGX_OK;  // m = 1: every proof is infinity, no setup
  return ctx->curve == KZGX_CURVE_BN254 ? prove_cosets_setup_impl<BN254G1>(ctx, ws, d_srs_canon, log2n, log2l, st)
                                        : prove_cosets_setup_impl<BLS12381G1>(ctx, ws, d_srs_canon, log2n, log2l, st);
}

template <class C>
static int prove_cosets_impl(Ctx* ctx, MsmWs& ws, const uint32_t* d_srs, const uint32_t* d_coeffs, size_t stride,
                             uint32_t k, uint32_t kl, size_t batch, bool ext, bool bitrev, uint32_t* d_out_xy,
                             uint32_t* d_out_inf, uint32_t* d_y, hipStream_t st) {
  using FR = typename C::Fr;
  using T = typename G1NttOf<C>::T;
  constexpr int XW = xyzz_words<C>();
  constexpr size_t PW = 2 * C::Fp::N;
  const uint32_t km = k - kl, kr = km + (ext ? 1 : 0), kd = kr + kl;
  const size_t n = (size_t)1 << k, m = (size_t)1 << km, R = (size_t)1 << kr, D = (size_t)1 << kd;
  const size_t chunk = g1n_chunk(k + 1), cmax = std::min(batch, chunk);
  if (d_y) {
    // one forward transform of size D of the zero-padded coefficients; naturally, regrouped by coset
    if (ext || !bitrev) KZGX_TRY(dev_alloc(ctx, (void**)&ws.fkm_y, cmax * D * FR::N * sizeof(uint32_t), &ws.fkm_y_b));
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
      const size_t cb = std::min(chunk, batch - b0);
      const uint32_t total = (uint32_t)(cb * D), blocks = (total + 255) / 256;
      const uint32_t* src = d_coeffs + b0 * stride * FR::N;
      size_t sstride = stride;
      uint32_t* dst = d_y + b0 * D * FR::N;
      if (ext) {
        hipLaunchKernelGGL(k_fkm_pad<FR>, dim3(blocks), dim3(256), 0, st, src, stride, k, kd, total, ws.fkm_y);
        KZGX_TRY_HIP(hipGetLastError());
        src = ws.fkm_y;
        sstride = D;
      }
      KZGX_TRY(ntt(ctx, src, sstride, bitrev ? dst : ws.fkm_y, D, kd, cb, false, bitrev, st));
      if (!bitrev) {
        hipLaunchKernelGGL(k_fkm_gather<FR>, dim3(blocks), dim3(256), 0, st, ws.fkm_y, kr, kl, total, dst);
        KZGX_TRY_HIP(hipGetLastError());
      }
    }
  }
  if (km == 0) {  // l = n: every quotient is zero, every proof infinity
    const size_t cnt = batch * R;
    for (size_t b0 = 0; b0 < cnt; b0 += (size_t)1 << 30) {
      const size_t cb = std::min<size_t>((size_t)1 << 30, cnt - b0);
      KZGX_TRY_HIP(hipMemsetAsync(d_out_xy + b0 * PW, 0, cb * PW * sizeof(uint32_t), st));
      hipLaunchKernelGGL(k_g1n_fill, dim3((unsigned)((cb + 255) / 256)), dim3(256), 0, st, d_out_inf + b0,
                         (uint32_t)cb, 1u);
    }
    KZGX_TRY_HIP(hipGetLastError());
    return KZGX_OK;
  }
  KZGX_TRY(prove_cosets_setup_impl<C>(ctx, ws, d_srs, k, kl, st));
  const FkSetup& s = ctx->fkm[k][kl];
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.g1n_rec, cmax * 2 * m * XW * sizeof(uint32_t), &ws.g1n_rec_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.fk_c, cmax * 2 * n * FR::N * sizeof(uint32_t), &ws.fk_c_b));
  KZGX_TRY(ntt_twiddles(ctx, km + 1, st));
  G1NttScalar ninv;
  for (int w = 0; w < 8; w++) ninv.v[w] = T::NINV_M[km + 1][w];
  const uint32_t lg = std::min<uint32_t>(kl, 6);
  for (size_t b0 = 0; b0 < batch; b0 += chunk) {
    const size_t cb = std::min(chunk, batch - b0), scal = cb * 2 * n, outs = cb * 2 * m;
    hipLaunchKernelGGL(k_fkm_build_c<FR>, dim3((unsigned)((scal + 255) / 256)), dim3(256), 0, st,
                       d_coeffs + b0 * stride * FR::N, stride, km, kl, (uint32_t)scal, ninv, ws.fk_c);
    KZGX_TRY_HIP(hipGetLastError());
    KZGX_TRY(ntt(ctx, ws.fk_c, 2 * m, ws.fk_c, 2 * m, km + 1, cb << kl, false, false, st));
    hipLaunchKernelGGL(k_fkm_pointwise_sum<C>, dim3(g1n_blocks(outs << lg)), dim3(G1N_BLOCK), 0, st, s.x, s.inf,
                       ws.fk_c, km + 1, kl, (uint32_t)outs, ws.g1n_rec);
    // h: the unscaled inverse transform of the 2m records; h_e at record 2 brev_km(e)
    KZGX_TRY(g1n_stages<C>(ctx, ws.g1n_rec, km + 1, cb, 2 * m, 1, true, false, false, st));
    if (ext) {
      // the size-2m transform of (h, O x m): bit-reversed in over all the records, the odd ones infinity
      hipLaunchKernelGGL(k_fkm_clear_odd<C>, dim3(g1n_blocks(cb * m)), dim3(G1N_BLOCK), 0, st, ws.g1n_rec,
                         (uint32_t)(cb * m));
      KZGX_TRY(g1n_stages<C>(ctx, ws.g1n_rec, km + 1, cb, 2 * m, 1, false, true, false, st));
    } else {
      KZGX_TRY(g1n_stages<C>(ctx, ws.g1n_rec, km, cb, 2 * m, 2, false, true, false, st));
    }
    hipLaunchKernelGGL(k_g1ntt_store<C>, dim3(g1n_blocks(cb * R)), dim3(G1N_BLOCK), 0, st, ws.g1n_rec, kr,
                       (uint32_t)(cb * R), (uint32_t)(2 * m), ext ? 1u : 2u, 0u, (uint32_t)bitrev,
                       d_out_xy + b0 * R * PW, d_out_inf + b0 * R);
    KZGX_TRY_HIP(hipGetLastError());
  }
  return KZGX_OK;
}

int prove_cosets(Ctx* ctx, MsmWs& ws, const uint32_t* d_srs_canon, const uint32_t* d_coeffs, size_t stride,
                 unsigned log2n, unsigned log2l, size_t batch, bool ext, bool bitrev, uint32_t* d_out_xy,
                 uint32_t* d_out_inf, uint32_t* d_y, hipStream_t st) {
  if (!prove_cosets_shape_ok(ctx, log2n, log2l, ext)) return KZGX_ERR_ARG;
  if (batch == 0) return KZGX_OK;
  return ctx->curve == KZGX_CURVE_BN254
             ? prove_cosets_impl<BN254G1>(ctx, ws, d_srs_canon, d_coeffs, stride, log2n, log2l, batch, ext, bitrev,
                                          d_out_xy, d_out_inf, d_y, st)
             : prove_cosets_impl<BLS12381G1>(ctx, ws, d_srs_canon, d_coeffs, stride, log2n, log2l, batch, ext,
                                             bitrev, d_out_xy, d_out_inf, d_y, st);
}

}  // namespace kzgx
