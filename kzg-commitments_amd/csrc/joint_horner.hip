// Horner pass of the block-table MSM (msm_joint.hip): the 254 / 255 plane
// sums A_w of each MSM (and block range) folded into sum_w 2^w A_w.
//
// The pass is under 2% of a call's point operations and all of its
// dependent chain: bits(r) - 1 doublings per MSM that no lane mapping
// removes.  What the mapping decides is what one link of the chain costs: a
// lone lane issues a doubling's 9 products one after another (~5 us in a
// wavefront with nothing else to run), an aligned group of 8 lanes
// (coop.hpp) runs them in 3 rounds.  So
//   stage 1  one lane per (MSM, range, segment of JOINT_SEG planes), many
//            short independent chains: S = sum_t 2^t A_{SEG seg + t};
//   stage 2  one 8-lane group per MSM walks the segments from the top:
//            JOINT_SEG cooperative doublings, then one cooperative addition
//            per range: sum_seg 2^(SEG seg) sum_rho S.
// The sum over planes is linear, so the ranges fold apart in stage 1 and
// meet in stage 2.  k_fixed_finish converts the sums (its lone-lane
// inversion inside stage 2 would run in 8 of a wavefront's 64 lanes and only
// lengthen the chain).
//
// Under the endomorphism split (msm_joint.hip) the 256 planes are two halves
// of 128, each with its own chain: stage 1 as above on inlined operations,
// stage 2 one 8-lane group per (MSM, half) over 8 segments -- 127 doublings
// deep, not 253 -- and k_joint_finish_glv adds S_1 + phi(S_2) in the lane
// that converts the result.
//
// Compiled with memory clauses off, as latency.hip and for its reason: the
// cooperative operations inlined next to clause-formed loads (DESIGN.md
// section 7).
#ifndef KZGX_MEMCLAUSE_OFF
#error "joint_horner.hip needs -mllvm -amdgpu-max-memory-clause=1 -DKZGX_MEMCLAUSE_OFF (see the Makefile)"
#endif
#include <hip/hip_runtime.h>

#include "coop.hpp"
#include "curve.hpp"
#include "kzgx_internal.hpp"
#include "kzgx_setup.hpp"

namespace kzgx {

// stage 1: lane (b, rho, seg) folds the planes [SEG seg, min(SEG seg + SEG,
// bits)) of range rho of MSM b, highest plane first.  Lanes hold independent
// segments, so a lane's SEG - 1 doublings and additions are not a
// wavefront's.  The next plane's partial is loaded ahead of the doubling it
// follows.  Layouts: part[b][rho][plane], segs[b][rho][seg].
// GLV (the endomorphism split): every plane is live and a segment lies inside
// one half (planes [0, 128) half 0, [128, 256) half 1).
template <class C, bool GLV = false>
__global__ __launch_bounds__(64) void k_joint_horner1(const uint32_t* __restrict__ part, uint64_t lanes,
                                                      uint32_t* __restrict__ segs) {
  constexpr int XW = xyzz_words<C>();
  constexpr uint32_t BITS = GLV ? JOINT_PL : C::SCALAR_BITS;
  __builtin_amdgcn_s_setprio(3);  // a tail pass: issue ahead of a co-resident accumulation (msm_joint.hip "Tail priority")
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= lanes) return;  // lanes = batch R JOINT_NSEG
  const uint64_t br = t / JOINT_NSEG;
  const uint32_t seg = (uint32_t)(t % JOINT_NSEG);
  const uint32_t lo = JOINT_SEG * seg, hi = lo + JOINT_SEG < BITS ? lo + JOINT_SEG : BITS;
  const uint32_t* p = part + br * JOINT_PL * XW;
  Xyzz<C> acc = xyzz_load<C>(p + (size_t)(hi - 1) * XW);
  for (uint32_t w = hi - 1; w-- > lo;) {
    const Xyzz<C> a = xyzz_load<C>(p + (size_t)w * XW);
    if constexpr (GLV) {
      // inlined: no call frames (the calls below cost 448 / 696 B of scratch per
      // lane and 226 / 248 VGPRs; inlined 144 / 224 VGPRs and no scratch)
      acc = xyzz_dbl_impl<C>(acc);
      acc = xyzz_add_impl<C>(acc, a);
    } else {
      acc = xyzz_dbl<C>(acc);
      acc = xyzz_add<C>(acc, a);
    }
  }
  xyzz_store<C>(segs + t * XW, acc);
}

// stage 2: the aligned 8-lane group (b) folds its R x JOINT_NSEG segment
// sums, 8 groups per workgroup.  Every lane of a group loads the same
// records and runs the same branches, so coop.hpp's contract holds: a group
// past the batch leaves before it touches LDS, and the infinity, doubling
// and cancel returns of the cooperative operations depend on the group's
// point alone.  Fixed trip counts; the first range's sum of the next segment
// is loaded ahead of the doublings it follows.
template <class C>
__global__ __launch_bounds__(64) void k_joint_horner2(const uint32_t* __restrict__ segs, uint32_t batch, uint32_t R,
                                                      uint32_t* __restrict__ sums) {
  constexpr int XW = xyzz_words<C>();
  constexpr int L = C::Fp29::L;
  __shared__ uint32_t sc[(64 / COOP_G) * COOP_SLOTS * L];
  const uint32_t grp = threadIdx.x / COOP_G;
  const int j = (int)(threadIdx.x % COOP_G);
  const uint32_t b = blockIdx.x * (64 / COOP_G) + grp;
  if (b >= batch) return;
  uint32_t* my = sc + grp * COOP_SLOTS * L;
  const uint32_t* p = segs + (size_t)b * R * JOINT_NSEG * XW;
  auto seg_sum = [&](uint32_t r, uint32_t seg) __attribute__((always_inline)) {
    return xyzz_load<C>(p + ((size_t)r * JOINT_NSEG + seg) * XW);
  };
  Xyzz<C> acc = seg_sum(0, JOINT_NSEG - 1);
#pragma unroll 1
  for (uint32_t r = 1; r < R; r++) acc = coop_add<C>(acc, seg_sum(r, JOINT_NSEG - 1), my, j);
#pragma unroll 1
  for (uint32_t seg = JOINT_NSEG - 1; seg-- > 0;) {
    const Xyzz<C> nxt = seg_sum(0, seg);
#pragma unroll 1
    for (uint32_t k = 0; k < JOINT_SEG; k++) acc = coop_dbl<C>(acc, my, j);
    acc = coop_add<C>(acc, nxt, my, j);
#pragma unroll 1
    for (uint32_t r = 1; r < R; r++) acc = coop_add<C>(acc, seg_sum(r, seg), my, j);
  }
  if (j == 0) xyzz_store<C>(sums + (size_t)b * XW, acc);
}

// stage 2 of the endomorphism split: two adjacent 8-lane groups per MSM, group
// (b, h) folds half h's JOINT_NSEG / 2 segment sums of every range: 127
// cooperative doublings, not 253.  sums[b][h].  GPW groups per workgroup
// (block size GPW COOP_G): 8 fill the wavefront; 4 halve the workgroup's LDS
// (BN254 5760 B, not 11 520 B), which is what a CU has left beside an
// accumulation that runs with a residency reserve (msm_joint.hip).
template <class C, int GPW>
__global__ __launch_bounds__(64) void k_joint_horner2_glv(const uint32_t* __restrict__ segs, uint32_t batch, uint32_t R,
                                                          uint32_t* __restrict__ sums) {
  constexpr int XW = xyzz_words<C>();
  constexpr int L = C::Fp29::L;
  constexpr uint32_t HSEG = JOINT_NSEG / 2;
  static_assert(GPW * COOP_G <= 64, "one wavefront");
  __shared__ uint32_t sc[GPW * COOP_SLOTS * L];
  __builtin_amdgcn_s_setprio(3);  // a tail pass: issue ahead of a co-resident accumulation (msm_joint.hip "Tail priority")
  const uint32_t grp = threadIdx.x / COOP_G;
  const int j = (int)(threadIdx.x % COOP_G);
  const uint32_t gid = blockIdx.x * GPW + grp;
  const uint32_t b = gid >> 1, h = gid & 1u;
  if (b >= batch) return;
  uint32_t* my = sc + grp * COOP_SLOTS * L;
  const uint32_t* p = segs + ((size_t)b * R * JOINT_NSEG + h * HSEG) * XW;
  auto seg_sum = [&](uint32_t r, uint32_t seg) __attribute__((always_inline)) {
    return xyzz_load<C>(p + ((size_t)r * JOINT_NSEG + seg) * XW);
  };
  Xyzz<C> acc = seg_sum(0, HSEG - 1);
#pragma unroll 1
  for (uint32_t r = 1; r < R; r++) acc = coop_add<C>(acc, seg_sum(r, HSEG - 1), my, j);
#pragma unroll 1
  for (uint32_t seg = HSEG - 1; seg-- > 0;) {
    const Xyzz<C> nxt = seg_sum(0, seg);
#pragma unroll 1
    for (uint32_t k = 0; k < JOINT_SEG; k++) acc = coop_dbl<C>(acc, my, j);
    acc = coop_add<C>(acc, nxt, my, j);
#pragma unroll 1
    for (uint32_t r = 1; r < R; r++) acc = coop_add<C>(acc, seg_sum(r, seg), my, j);
  }
  if (j == 0) xyzz_store<C>(sums + (size_t)gid * XW, acc);
}

// the split's finish, thread per MSM: S_1 + phi(S_2) with phi(X, Y, ZZ, ZZZ) =
// (beta X, Y, ZZ, ZZZ), by the complete addition (either sum at infinity and
// S_1 = +-phi(S_2) all occur: scalar 0 alone gives the last), then
// k_fixed_finish's conversion
template <class C>
__global__ __launch_bounds__(64) void k_joint_finish_glv(const uint32_t* __restrict__ sums, uint32_t batch,
                                                         uint32_t* __restrict__ out, uint32_t* __restrict__ out_inf) {
  using F = typename C::Fp29;
  constexpr int XW = xyzz_words<C>();
  __builtin_amdgcn_s_setprio(3);  // a tail pass: issue ahead of a co-resident accumulation (msm_joint.hip "Tail priority")
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  const Xyzz<C> s1 = xyzz_load<C>(sums + (size_t)(2 * b) * XW);
  Xyzz<C> s2 = xyzz_load<C>(sums + (size_t)(2 * b + 1) * XW);
  s2.X = f29_mul<F>(s2.X, f29_const<F>(C::Glv::BETA29));  // < 2m
  // inlined: the call's frame made this kernel 226 / 248 VGPRs with 568 / 892 B
  // of scratch; inlined 162 / 248 with 280 / 444 B, so that on BN254 it fits
  // beside two of the accumulation's wavefronts per SIMD (msm_joint.hip
  // "Residency reserve")
  const Xyzz<C> p = xyzz_add_impl<C>(s1, s2);
  Affine<C> a;
  const bool fin = xyzz_to_affine<C>(p, a);
  affine_to_canonical<C>(out + (size_t)b * 2 * C::Fp::N, a, fin);
  out_inf[b] = fin ? 0u : 1u;
}

template <class C>
int joint_horner_glv_launch(const uint32_t* part, uint32_t batch, uint32_t R, uint32_t* segs, uint32_t* sums,
                            uint32_t* out, uint32_t* out_inf, bool narrow, hipStream_t st) {
  static_assert(JOINT_PL == 256 && (JOINT_NSEG & 1u) == 0, "two halves of 128 planes, whole segments each");
  const uint64_t lanes = (uint64_t)batch * R * JOINT_NSEG;
  if (batch == 0 || batch > 0x3fffffffu || R == 0 || (lanes + 63) / 64 > 0x7fffffffull) return KZGX_ERR_ARG;
  hipLaunchKernelGGL((k_joint_horner1<C, true>), dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, st, part, lanes,
                     segs);
  constexpr uint32_t GPW = 64 / COOP_G;  // groups per workgroup; half of them beside a reserved residency
  if (narrow)
    hipLaunchKernelGGL((k_joint_horner2_glv<C, GPW / 2>), dim3((2 * batch + GPW / 2 - 1) / (GPW / 2)),
                       dim3(COOP_G * GPW / 2), 0, st, segs, batch, R, sums);
  else
    hipLaunchKernelGGL((k_joint_horner2_glv<C, GPW>), dim3((2 * batch + GPW - 1) / GPW), dim3(64), 0, st, segs, batch,
                       R, sums);
  hipLaunchKernelGGL(k_joint_finish_glv<C>, dim3((batch + 63) / 64), dim3(64), 0, st, sums, batch, out, out_inf);
  return KZGX_OK;
}
template int joint_horner_glv_launch<BN254G1>(const uint32_t*, uint32_t, uint32_t, uint32_t*, uint32_t*, uint32_t*,
                                              uint32_t*, bool, hipStream_t);
template int joint_horner_glv_launch<BLS12381G1>(const uint32_t*, uint32_t, uint32_t, uint32_t*, uint32_t*, uint32_t*,
                                                 uint32_t*, bool, hipStream_t);

template <class C>
int joint_horner_launch(const uint32_t* part, uint32_t batch, uint32_t R, uint32_t* segs, uint32_t* sums,
                        hipStream_t st) {
  static_assert(C::SCALAR_BITS <= (int)JOINT_PL && C::SCALAR_BITS > (int)(JOINT_PL - JOINT_SEG),
                "the top segment holds at least one plane");
  const uint64_t lanes = (uint64_t)batch * R * JOINT_NSEG;
  if (batch == 0 || R == 0 || (lanes + 63) / 64 > 0x7fffffffull) return KZGX_ERR_ARG;
  hipLaunchKernelGGL((k_joint_horner1<C, false>), dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, st, part, lanes, segs);
  constexpr uint32_t GPW = 64 / COOP_G;  // groups per workgroup
  hipLaunchKernelGGL(k_joint_horner2<C>, dim3((batch + GPW - 1) / GPW), dim3(64), 0, st, segs, batch, R, sums);
  return KZGX_OK;
}
template int joint_horner_launch<BN254G1>(const uint32_t*, uint32_t, uint32_t, uint32_t*, uint32_t*, hipStream_t);
template int joint_horner_launch<BLS12381G1>(const uint32_t*, uint32_t, uint32_t, uint32_t*, uint32_t*, hipStream_t);

// device bring-up (kzgx_setup.hpp): one launch loads this code object
__global__ void k_warm_joint_horner() {}
int warm_joint_horner(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_joint_horner, dim3(1), dim3(64), 0, st);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

}  // namespace kzgx
