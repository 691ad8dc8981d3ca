// Batched point validation with an optional prime-order subgroup test, for
// gfx950: one lane per point, any count, one launch.
//
// k_g1_check: canonical coordinates and y^2 = x^3 + b by k_g1_validate's rules
// (srs.hip), then, on a curve with a cofactor (BLS12-381) and when asked,
// membership in the order-r subgroup by the endomorphism test
//   P != O  and  [x^2]P = (beta x, -y),
// beta the primitive cube root of 1 in Fp with phi(x, y) = (beta x, y) acting
// as -x^2 on the subgroup (gen_consts.py derives it).  phi^2 + phi + 1 = 0 on
// all of E(Fp), so phi(P) = -[x^2]P gives [x^4 - x^2 + 1]P = [r]P = O, and a
// point of order r satisfies it by the choice of beta: the test is exactly
// membership.  [x^2]P is ONE double-and-add over the 128 constant bits of x^2
// with mixed additions of P: 127 doublings + 16 mixed additions (x^2 has 17
// set bits), against ~255 + ~127 for the definitional [r]P.  The comparison is
// projective (X = beta x ZZ, Y = -y ZZZ, ZZ != 0): no inversion.
//
// The exponent is a compile-time constant, so every lane of a wave walks the
// same doublings and additions.  A lane whose entry is infinite, non-canonical
// or off the curve runs the chain on the generator instead and has its result
// masked: it never decides the wave's path, and the group law only ever sees
// curve points.  E(Fp) has odd order on both curves (no y = 0), and a
// small-order input reaches xyzz_add_affine's equal-x branch ([2]T = -T for
// an order-3 T), which doubles or cancels exactly.
//
// k_g2_check: k_g2_validate's rules (pairing.hip), then the definitional
// [r]Q = O with g2_dbl / g2_add_mixed over the constant bits of r.  Cold path
// (a setup's G2 half).  g2_add_mixed is complete: accumulator = Q doubles,
// accumulator = -Q gives infinity, accumulator = O restarts from Q, and
// g2_dbl keeps infinity, so a point of order 13 walks through O exactly.
#include <hip/hip_runtime.h>

#include "kzgx_internal.hpp"
#include "kzgx_setup.hpp"
#include "point_check.hpp"

namespace kzgx {

// Two arrays in one launch (count1 may be 0): lane k checks point k of the
// first array for k < count0, else point k - count0 of the second; ok holds
// count0 + count1 flags in that order.  The checked aggregate validates its
// commits and proofs side by side this way: the subgroup chain is latency
// bound (one lane per point), so the second array rides along for free until
// the GPU is full.
template <class C>
__global__ __launch_bounds__(64) void k_g1_check(const uint32_t* __restrict__ xy0, const uint32_t* __restrict__ inf0,
                                                 uint32_t count0, const uint32_t* __restrict__ xy1,
                                                 const uint32_t* __restrict__ inf1, uint32_t count1, uint32_t subgroup,
                                                 uint32_t* __restrict__ ok) {
  using F = typename C::Fp29;
  constexpr int N = C::Fp::N;
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count0 + count1) return;
  const bool second = k >= count0;
  const uint32_t j = second ? k - count0 : k;
  const uint32_t* w = (second ? xy1 : xy0) + (size_t)j * 2 * N;
  const uint32_t* inf = second ? inf1 : inf0;
  uint32_t any = 0;
  for (int i = 0; i < 2 * N; i++) any |= w[i];
  const bool is_inf = (inf && inf[j]) || any == 0;
  Affine<C> a;
  const bool on = g1_canonical_on_curve<C>(w, a);
  bool member = true;
  if constexpr (!C::COFACTOR_ONE) {
    if (subgroup) {  // uniform: a kernel argument
      const bool run = on && !is_inf;
      if (!run) {
        a.x = f29_const<F>(C::GX29);
        a.y = f29_const<F>(C::GY29);
      }
      member = g1_in_subgroup<C>(a);
    }
  }
  ok[k] = (is_inf || (on && member)) ? 1u : 0u;
}

template <class C>
__global__ __launch_bounds__(64) void k_g2_check(const uint32_t* __restrict__ xy, const uint32_t* __restrict__ inf,
                                                 uint32_t count, uint32_t subgroup, uint32_t* __restrict__ ok) {
  using P = typename PairOf<C>::T;
  constexpr int N = C::Fp::N;
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const uint32_t* w = xy + (size_t)k * 4 * N;
  bool lt = true;
  for (int c = 0; c < 4; c++) lt = lt && canon_lt_m<C>(w + c * N);
  G2A<C> q;
  const bool fin = g2_from_canon<C>(w, q);
  const bool is_inf = (inf && inf[k]) || !fin;
  const Fp2<C> d = f2_sub<C>(f2_sqr<C>(q.y), f2_add<C>(f2_mul<C>(f2_sqr<C>(q.x), q.x), f2_const<C>(P::B2)));
  const bool on = lt && fin && f2_is_zero<C>(d);
  bool member = true;
  if (subgroup) {  // uniform: a kernel argument
    if (!on || is_inf) {
      q.x = f2_const<C>(P::G2X);
      q.y = f2_const<C>(P::G2Y);
    }
    member = g2_in_subgroup<C>(q);
  }
  ok[k] = (is_inf || (on && member)) ? 1u : 0u;
}

// *all = AND of count flags (1 for count == 0): one block, strided reads, a
// tree in LDS.  AND is order-free, so the result does not depend on timing.
__global__ __launch_bounds__(1024) void k_flags_and(const uint32_t* __restrict__ flags, uint32_t count,
                                                    uint32_t* __restrict__ all) {
  __shared__ uint32_t s[1024];
  uint32_t v = 1u;
  for (uint32_t i = threadIdx.x; i < count; i += 1024) v &= flags[i] != 0u ? 1u : 0u;
  s[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t h = 512; h > 0; h >>= 1) {
    if (threadIdx.x < h) s[threadIdx.x] &= s[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) *all = s[0];
}

// *ok = *ok && *gate (the checked aggregate: the pairing's answer behind the point checks)
__global__ void k_flag_gate(uint32_t* __restrict__ ok, const uint32_t* __restrict__ gate) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *ok = (*ok != 0u && *gate != 0u) ? 1u : 0u;
}

int g1_check2(Ctx* ctx, const uint32_t* d_xy0, const uint32_t* d_inf0, size_t count0, const uint32_t* d_xy1,
              const uint32_t* d_inf1, size_t count1, int subgroup, uint32_t* d_ok, hipStream_t st) {
  const size_t count = count0 + count1;
  if (count == 0) return KZGX_OK;
  if (count0 > 0x7fffffffu || count1 > 0x7fffffffu) return KZGX_ERR_ARG;
  const dim3 blk(64), grd((unsigned)((count + 63) / 64));
  const uint32_t sg = subgroup ? 1u : 0u;
  if (ctx->curve == KZGX_CURVE_BN254)
    hipLaunchKernelGGL(k_g1_check<BN254G1>, grd, blk, 0, st, d_xy0, d_inf0, (uint32_t)count0, d_xy1, d_inf1,
                       (uint32_t)count1, sg, d_ok);
  else
    hipLaunchKernelGGL(k_g1_check<BLS12381G1>, grd, blk, 0, st, d_xy0, d_inf0, (uint32_t)count0, d_xy1, d_inf1,
                       (uint32_t)count1, sg, d_ok);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int g1_check(Ctx* ctx, const uint32_t* d_xy, const uint32_t* d_inf, size_t count, int subgroup, uint32_t* d_ok,
             hipStream_t st) {
  return g1_check2(ctx, d_xy, d_inf, count, nullptr, nullptr, 0, subgroup, d_ok, st);
}

int g2_check(Ctx* ctx, const uint32_t* d_xy, const uint32_t* d_inf, size_t count, int subgroup, uint32_t* d_ok,
             hipStream_t st) {
  if (count == 0) return KZGX_OK;
  if (count > 0xffffffffu) return KZGX_ERR_ARG;
  const dim3 blk(64), grd((unsigned)((count + 63) / 64));
  const uint32_t sg = subgroup ? 1u : 0u;
  if (ctx->curve == KZGX_CURVE_BN254)
    hipLaunchKernelGGL(k_g2_check<BN254G1>, grd, blk, 0, st, d_xy, d_inf, (uint32_t)count, sg, d_ok);
  else
    hipLaunchKernelGGL(k_g2_check<BLS12381G1>, grd, blk, 0, st, d_xy, d_inf, (uint32_t)count, sg, d_ok);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int flags_and(const uint32_t* d_flags, size_t count, uint32_t* d_all, hipStream_t st) {
  if (count > 0xffffffffu) return KZGX_ERR_ARG;
  hipLaunchKernelGGL(k_flags_and, dim3(1), dim3(1024), 0, st, d_flags, (uint32_t)count, d_all);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int flag_gate(uint32_t* d_ok, const uint32_t* d_gate, hipStream_t st) {
  hipLaunchKernelGGL(k_flag_gate, dim3(1), dim3(64), 0, st, d_ok, d_gate);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

// device bring-up (kzgx_setup.hpp): one launch loads this code object
__global__ void k_warm_subgroup() {}
int warm_subgroup(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_subgroup, dim3(1), dim3(64), 0, st);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

}  // namespace kzgx
