// Setup ceremony on gfx950: one powers-of-tau contribution over an installed
// SRS, and the challenge powers of its structure test ("Setup
// ceremony").
//
// A contribution with the secret s maps G1[i] -> [s^(start + i)] G1[i] and
// G2[j] -> [s^(start + j)] G2[j]: a setup for tau becomes one for tau s.  It
// is the variable-base twin of k_gen_srs (srs.hip) and k_gen_srs_g2
// (pairing.hip): every lane derives its own exponent by the same 64-bit
// square-and-multiply, then runs a 256-bit double-and-add over its own point
// instead of the generator.  Canonical affine in, canonical affine out, so
// the result does not depend on the addition chain.
//
// The conditional addition is a select.  The lanes of a wave hold unrelated
// 255-bit exponents, so at nearly every bit some lane adds: the wave runs
// the addition anyway, and a branch would only add the divergence
// bookkeeping (and, for G2, a second call site of the non-inlined addition).
#include <hip/hip_runtime.h>

#include "curve.hpp"
#include "kzgx_internal.hpp"
#include "kzgx_setup.hpp"
#include "pairing_common.hpp"

namespace kzgx {

// e = s^ex mod r, canonical words (the exponent loop of k_gen_srs)
template <class FR>
KZGX_DEV void fr_pow_u64(const uint32_t* __restrict__ s_canon, uint64_t ex, uint32_t (&ew)[8]) {
  static_assert(FR::N == 8, "256-bit scalars");
  const Fe<FR> sm = fe_to_mont<FR>(fe_load<FR>(s_canon));
  Fe<FR> e = fe_one<FR>();
  for (int b = 63; b >= 0; b--) {
    e = fe_sqr<FR>(e);
    if ((ex >> b) & 1ull) e = fe_mul<FR>(e, sm);
  }
  e = fe_from_mont<FR>(e);
#pragma unroll
  for (int k = 0; k < 8; k++) ew[k] = e.v[k];
}

template <class F>
KZGX_DEV F29<F> f29_select(bool take, const F29<F>& a, const F29<F>& b) {
  F29<F> r;
#pragma unroll
  for (int k = 0; k < F::L; k++) r.v[k] = take ? a.v[k] : b.v[k];
  return r;
}

// G1[i] <- [s^(start + i)] G1[i]; in == out is allowed (a lane reads and
// writes its own point only)
template <class C>
__global__ __launch_bounds__(256) void k_srs_update_g1(const uint32_t* __restrict__ s_canon, uint64_t start, uint32_t n,
                                                       const uint32_t* in, uint32_t* out) {
  using F = typename C::Fp29;
  using FR = typename C::Fr;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t ew[8];
  fr_pow_u64<FR>(s_canon, start + i, ew);
  Affine<C> p;
  const bool fin = affine_from_canonical<C>(in + (size_t)i * 2 * C::Fp::N, p);
  Xyzz<C> acc = xyzz_inf<C>();
  for (int b = 255; b >= 0; b--) {
    acc = xyzz_dbl<C>(acc);
    const Xyzz<C> t = xyzz_add_affine<C>(acc, p);
    const bool bit = (ew[b >> 5] >> (b & 31)) & 1u;
    acc.X = f29_select<F>(bit, t.X, acc.X);
    acc.Y = f29_select<F>(bit, t.Y, acc.Y);
    acc.ZZ = f29_select<F>(bit, t.ZZ, acc.ZZ);
    acc.ZZZ = f29_select<F>(bit, t.ZZZ, acc.ZZZ);
  }
  Affine<C> a;
  const bool rfin = xyzz_to_affine<C>(acc, a);
  // an infinite entry (all zero) stays all zero, whatever its coordinates fed the chain
  affine_to_canonical<C>(out + (size_t)i * 2 * C::Fp::N, a, fin && rfin);
}

template <class C>
KZGX_DEV Fp2<C> f2_select(bool take, const Fp2<C>& a, const Fp2<C>& b) {
  using F = typename C::Fp29;
  return Fp2<C>{f29_select<F>(take, a.a, b.a), f29_select<F>(take, a.b, b.b)};
}

// g2_mul_words (pairing.hip) with the addition selected, not branched to
template <class C>
KZGX_TW G2J<C> g2_mul_words_select(const G2A<C>& q, const uint32_t (&e)[8]) {
  G2J<C> acc = g2_inf<C>();
  for (int b = 255; b >= 0; b--) {
    acc = g2_dbl<C>(acc);
    const G2J<C> t = g2_add_mixed<C>(acc, q);
    const bool bit = (e[b >> 5] >> (b & 31)) & 1u;
    acc.X = f2_select<C>(bit, t.X, acc.X);
    acc.Y = f2_select<C>(bit, t.Y, acc.Y);
    acc.Z = f2_select<C>(bit, t.Z, acc.Z);
  }
  return acc;
}

// G2[j] <- [s^(start + j)] G2[j]; in == out is allowed.  With `witness`, one
// more lane (index n) writes [s] times the curve's G2 generator there: the
// contribution's witness rides in the same launch (a lone G2 lane takes as
// long as a full wave of them).
template <class C>
__global__ __launch_bounds__(64) void k_srs_update_g2(const uint32_t* __restrict__ s_canon, uint64_t start, uint32_t n,
                                                      const uint32_t* in, uint32_t* out, uint32_t* witness) {
  using P = typename PairOf<C>::T;
  using FR = typename C::Fr;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool wit = witness && i == n;
  if (i >= n && !wit) return;
  uint32_t ew[8];
  fr_pow_u64<FR>(s_canon, wit ? 1 : start + i, ew);
  G2A<C> q;
  bool fin = true;
  if (wit) {
    q.x = f2_const<C>(P::G2X);
    q.y = f2_const<C>(P::G2Y);
  } else {
    fin = g2_from_canon<C>(in + (size_t)i * 4 * C::Fp::N, q);
  }
  G2A<C> a;
  const bool rfin = g2_to_affine<C>(g2_mul_words_select<C>(q, ew), a);
  g2_to_canon<C>(a, fin && rfin, wit ? witness : out + (size_t)i * 4 * C::Fp::N);
}

// the curve's generators, canonical affine: G1 (x, y), then G2 (x.re, x.im, y.re, y.im)
template <class C>
__global__ void k_generators(uint32_t* __restrict__ out) {
  using F = typename C::Fp29;
  using P = typename PairOf<C>::T;
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  Affine<C> g;
  g.x = f29_const<F>(C::GX29);
  g.y = f29_const<F>(C::GY29);
  affine_to_canonical<C>(out, g, true);
  G2A<C> g2;
  g2.x = f2_const<C>(P::G2X);
  g2.y = f2_const<C>(P::G2Y);
  g2_to_canon<C>(g2, true, out + 2 * C::Fp::N);
}

// row0[i] = rho^i for i < count, canonical, each lane by its own
// square-and-multiply.  With row1 (the structure test's second row, one
// element to the right): row1[i + 1] = rho^i, and the two free ends
// row0[count] and row1[0] are zero, so both rows hold count + 1 scalars.
template <class FR>
__global__ __launch_bounds__(256) void k_fr_powers(const uint32_t* __restrict__ rho_canon, uint32_t count,
                                                   uint32_t* __restrict__ row0, uint32_t* __restrict__ row1) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  uint32_t ew[8];
  fr_pow_u64<FR>(rho_canon, i, ew);
#pragma unroll
  for (int k = 0; k < 8; k++) row0[(size_t)i * 8 + k] = ew[k];
  if (!row1) return;
#pragma unroll
  for (int k = 0; k < 8; k++) row1[(size_t)(i + 1) * 8 + k] = ew[k];
  if (i == 0) {
#pragma unroll
    for (int k = 0; k < 8; k++) {
      row0[(size_t)count * 8 + k] = 0u;
      row1[k] = 0u;
    }
  }
}

int srs_update_g1(int curve, const uint32_t* d_s, size_t start, size_t n, const uint32_t* d_in, uint32_t* d_out,
                  hipStream_t st) {
  if (n == 0) return KZGX_OK;
  dim3 blk(256), grd((unsigned)((n + 255) / 256));
  if (curve == KZGX_CURVE_BN254)
    hipLaunchKernelGGL(k_srs_update_g1<BN254G1>, grd, blk, 0, st, d_s, (uint64_t)start, (uint32_t)n, d_in, d_out);
  else
    hipLaunchKernelGGL(k_srs_update_g1<BLS12381G1>, grd, blk, 0, st, d_s, (uint64_t)start, (uint32_t)n, d_in, d_out);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int srs_update_g2(int curve, const uint32_t* d_s, size_t start, size_t n, const uint32_t* d_in, uint32_t* d_out,
                  uint32_t* d_witness, hipStream_t st) {
  const size_t lanes = n + (d_witness ? 1 : 0);
  if (lanes == 0) return KZGX_OK;
  dim3 blk(64), grd((unsigned)((lanes + 63) / 64));
  if (curve == KZGX_CURVE_BN254)
    hipLaunchKernelGGL(k_srs_update_g2<BN254G1>, grd, blk, 0, st, d_s, (uint64_t)start, (uint32_t)n, d_in, d_out,
                       d_witness);
  else
    hipLaunchKernelGGL(k_srs_update_g2<BLS12381G1>, grd, blk, 0, st, d_s, (uint64_t)start, (uint32_t)n, d_in, d_out,
                       d_witness);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int curve_generators(int curve, uint32_t* d_out, hipStream_t st) {
  if (curve == KZGX_CURVE_BN254)
    hipLaunchKernelGGL(k_generators<BN254G1>, dim3(1), dim3(64), 0, st, d_out);
  else
    hipLaunchKernelGGL(k_generators<BLS12381G1>, dim3(1), dim3(64), 0, st, d_out);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int fr_powers(int curve, const uint32_t* d_rho, size_t count, uint32_t* d_row0, uint32_t* d_row1, hipStream_t st) {
  if (count == 0) return KZGX_OK;
  dim3 blk(256), grd((unsigned)((count + 255) / 256));
  if (curve == KZGX_CURVE_BN254)
    hipLaunchKernelGGL(k_fr_powers<BN254G1::Fr>, grd, blk, 0, st, d_rho, (uint32_t)count, d_row0, d_row1);
  else
    hipLaunchKernelGGL(k_fr_powers<BLS12381G1::Fr>, grd, blk, 0, st, d_rho, (uint32_t)count, d_row0, d_row1);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

// device bring-up (kzgx_setup.hpp): one launch loads this code object
__global__ void k_warm_srs_update() {}
int warm_srs_update(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_srs_update, dim3(1), dim3(64), 0, st);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

}  // namespace kzgx
