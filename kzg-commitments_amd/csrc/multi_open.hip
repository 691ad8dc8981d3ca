// Batch openings for gfx950: many committed polynomials opened at shared
// points, one proof per point (kzgx_prove_multi_batch / kzgx_verify_multi_batch,
// include/kzg_gpu.h).  KZG is additively homomorphic, so the t openings of a
// group at z_g are one opening of F_g = sum_k w_k P_(poly_index[k]):
//
//  * k_multi_fold: F_g, one lane per (group, coefficient), FOLD_CPL
//    coefficients per lane so the per-claim weight work (its Montgomery form,
//    or the running power of gamma_g) is shared by FOLD_CPL products.  A wave
//    reads 64 consecutive scalars of a polynomial per load.
//  * k_multi_eval_wave / k_multi_eval_slice + k_multi_eval_combine: the
//    claimed values y_k = P(z_g), by k_quotient_single's local Horner and
//    wavefront suffix scan without its replay -- a wavefront per claim for
//    small n, a workgroup per (claim, slice) and a wavefront per claim over
//    the slice partials for large n.
//  * k_multi_rw + k_multi_gather: the verifier's scalars s_c, r_g z_g and -t
//    by a per-commitment gather over r_g(k) w_k -- field sums in a fixed order,
//    no atomics.
//  * k_multi_check: the index and group_start validation of the device entries.
//
// Canonical inputs are multiplied by Montgomery-form weights with fe_mul,
// which yields canonical results, as in poly.hip.  Every index read from
// device memory is range-checked before it addresses anything: group ranges
// are clamped to [0, count], polynomial and commitment indices are compared
// before use.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "field.hpp"
#include "multi_open.hpp"

namespace kzgx {
namespace {

template <class FR>
KZGX_DEV Fe<FR> mo_shfl_down(const Fe<FR>& a, int d) {
  Fe<FR> r;
#pragma unroll
  for (int i = 0; i < FR::N; i++) r.v[i] = __shfl_down(a.v[i], d, 64);
  return r;
}

template <class FR>
KZGX_DEV Fe<FR> mo_wave_sum(Fe<FR> a) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    Fe<FR> o;
#pragma unroll
    for (int i = 0; i < FR::N; i++) o.v[i] = __shfl_xor(a.v[i], m, 64);
    a = fe_add<FR>(a, o);
  }
  return a;
}

// the sum over a 256-thread workgroup, valid in thread 0 (lds: 4 scalars)
template <class FR>
KZGX_DEV Fe<FR> mo_block_sum(Fe<FR> acc, uint32_t* lds) {
  constexpr int N = FR::N;
  acc = mo_wave_sum<FR>(acc);
  if ((threadIdx.x & 63) == 0) fe_store<FR>(lds + (threadIdx.x >> 6) * N, acc);
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < 4; w++) acc = fe_add<FR>(acc, fe_load<FR>(lds + w * N));
  return acc;
}

// left-to-right square-and-multiply from the exponent's top set bit
template <class FR>
KZGX_DEV Fe<FR> mo_pow_u32(const Fe<FR>& base_m, uint32_t e) {
  if (e == 0) return fe_one<FR>();
  Fe<FR> acc = base_m;
  for (int b = 30 - __builtin_clz(e); b >= 0; b--) {
    acc = fe_sqr<FR>(acc);
    if ((e >> b) & 1u) acc = fe_mul<FR>(acc, base_m);
  }
  return acc;
}

// group g's claims [lo, hi), clamped to [0, count] (a decreasing pair is empty)
KZGX_DEV void group_range(const uint32_t* __restrict__ gs, uint32_t g, uint32_t count, uint32_t& lo, uint32_t& hi) {
  lo = min(gs[g], count);
  hi = min(gs[g + 1], count);
  if (hi < lo) hi = lo;
}

// the last group g < n_groups with group_start[g] <= k (0 when there is none): claim k's group
// for a well-formed group_start, empty groups included; always < n_groups (n_groups >= 1)
KZGX_DEV uint32_t claim_group(const uint32_t* __restrict__ gs, uint32_t n_groups, uint32_t k) {
  uint32_t lo = 0, hi = n_groups;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (gs[mid] <= k)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// sum_{i < n} P[i] z^i over one wavefront, valid in lane 0: lane-local Horner over a chunk of
// ceil(n / 64) coefficients, then the 6-step suffix scan of k_quotient_single (poly.hip)
template <class FR>
KZGX_DEV Fe<FR> wave_horner(const uint32_t* __restrict__ P, uint32_t n, const Fe<FR>& zm, uint32_t lane) {
  constexpr int N = FR::N;
  const uint32_t L = (n + 63) / 64;
  const uint32_t lo = min(lane * L, n), hi = min(lo + L, n);
  Fe<FR> h = fe_zero<FR>();
  for (uint32_t k = hi; k-- > lo;) h = fe_add<FR>(fe_load<FR>(P + (size_t)k * N), fe_mul<FR>(h, zm));
  Fe<FR> zp = mo_pow_u32<FR>(zm, L);
#pragma unroll
  for (int s = 0; s < 6; s++) {
    const Fe<FR> o = mo_shfl_down<FR>(h, 1 << s);
    if (lane + (1u << s) < 64) h = fe_add<FR>(h, fe_mul<FR>(o, zp));  // canonical * Montgomery = canonical
    zp = fe_sqr<FR>(zp);
  }
  return h;
}

__global__ __launch_bounds__(256) void k_multi_check(const uint32_t* __restrict__ index, uint32_t n_index,
                                                     const uint32_t* __restrict__ gs, uint32_t n_groups,
                                                     uint32_t count, uint32_t* __restrict__ ok) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (t < count) bad = index[t] >= n_index;
  if (t < n_groups) bad |= gs[t] > gs[t + 1];
  if (t == 0) bad |= gs[0] != 0u || gs[n_groups] != count;
  if (bad) *ok = 0u;  // every failing lane stores the same word
}

constexpr int FOLD_CPL = 4;  // coefficients per lane: 5 products per 4 coefficients and claim

template <class FR>
__global__ __launch_bounds__(256) void k_multi_fold(const uint32_t* __restrict__ coeffs, uint32_t n, size_t cstride,
                                                    uint32_t n_polys, const uint32_t* __restrict__ poly_index,
                                                    const uint32_t* __restrict__ gs, uint32_t g0, uint32_t count,
                                                    const uint32_t* __restrict__ weights, uint32_t powers,
                                                    uint32_t* __restrict__ F) {
  constexpr int N = FR::N;
  const uint32_t g = g0 + blockIdx.y;
  const size_t i0 = (size_t)blockIdx.x * (256 * FOLD_CPL) + threadIdx.x;
  uint32_t lo, hi;
  group_range(gs, g, count, lo, hi);
  Fe<FR> acc[FOLD_CPL];
#pragma unroll
  for (int c = 0; c < FOLD_CPL; c++) acc[c] = fe_zero<FR>();
  Fe<FR> gm = fe_zero<FR>(), wm = fe_one<FR>();
  if (powers) gm = fe_to_mont<FR>(fe_load<FR>(weights + (size_t)g * N));
  for (uint32_t k = lo; k < hi; k++) {
    if (!powers) wm = fe_to_mont<FR>(fe_load<FR>(weights + (size_t)k * N));
    const uint32_t p = poly_index[k];
    if (p < n_polys) {  // the same in every lane
      const uint32_t* P = coeffs + (size_t)p * cstride;
#pragma unroll
      for (int c = 0; c < FOLD_CPL; c++) {
        const size_t i = i0 + (size_t)c * 256;
        if (i < n) acc[c] = fe_add<FR>(acc[c], fe_mul<FR>(fe_load<FR>(P + i * N), wm));
      }
    }
    if (powers) wm = fe_mul<FR>(wm, gm);
  }
#pragma unroll
  for (int c = 0; c < FOLD_CPL; c++) {
    const size_t i = i0 + (size_t)c * 256;
    if (i < n) fe_store<FR>(F + ((size_t)blockIdx.y * n + i) * N, acc[c]);
  }
}

// one wavefront per claim, four claims per workgroup
template <class FR>
__global__ __launch_bounds__(256) void k_multi_eval_wave(const uint32_t* __restrict__ coeffs, uint32_t n,
                                                         size_t cstride, uint32_t n_polys,
                                                         const uint32_t* __restrict__ poly_index,
                                                         const uint32_t* __restrict__ gs, uint32_t n_groups,
                                                         const uint32_t* __restrict__ zs, uint32_t k0, uint32_t nk,
                                                         uint32_t* __restrict__ y) {
  constexpr int N = FR::N;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t kl = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (kl >= nk) return;  // whole wavefront
  const uint32_t k = k0 + kl;
  const uint32_t p = poly_index[k];
  Fe<FR> c = fe_zero<FR>();
  if (p < n_polys) {
    const uint32_t g = claim_group(gs, n_groups, k);
    const Fe<FR> zm = fe_to_mont<FR>(fe_load<FR>(zs + (size_t)g * N));
    c = wave_horner<FR>(coeffs + (size_t)p * cstride, n, zm, lane);
  }
  if (lane == 0) fe_store<FR>(y + (size_t)k * N, c);
}

// workgroup b = (claim k0 + b / nslices, slice b % nslices): part[b] = sum_{i in slice} P[i] z^(i - slice start),
// each wavefront a quarter of the slice
template <class FR>
__global__ __launch_bounds__(256) void k_multi_eval_slice(const uint32_t* __restrict__ coeffs, uint32_t n,
                                                          size_t cstride, uint32_t n_polys,
                                                          const uint32_t* __restrict__ poly_index,
                                                          const uint32_t* __restrict__ gs, uint32_t n_groups,
                                                          const uint32_t* __restrict__ zs, uint32_t k0,
                                                          uint32_t nslices, uint32_t slice,
                                                          uint32_t* __restrict__ part) {
  constexpr int N = FR::N;
  __shared__ uint32_t sh[4 * N];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t s = blockIdx.x % nslices, k = k0 + blockIdx.x / nslices;
  const uint32_t Q = slice / 4;
  const uint32_t p = poly_index[k];
  Fe<FR> c = fe_zero<FR>(), zm = fe_zero<FR>();
  if (p < n_polys) {  // the same in every lane of the workgroup
    const uint32_t g = claim_group(gs, n_groups, k);
    zm = fe_to_mont<FR>(fe_load<FR>(zs + (size_t)g * N));
    const uint64_t base = (uint64_t)s * slice + (uint64_t)wv * Q;
    const uint32_t len = base >= n ? 0u : (n - base < Q ? (uint32_t)(n - base) : Q);
    c = wave_horner<FR>(coeffs + (size_t)p * cstride + base * N, len, zm, lane);
  }
  if (lane == 0) fe_store<FR>(sh + wv * N, c);
  __syncthreads();
  if (threadIdx.x == 0) {
    const Fe<FR> zq = mo_pow_u32<FR>(zm, Q);
    Fe<FR> h = fe_load<FR>(sh + 3 * N);
    for (int w = 2; w >= 0; w--) h = fe_add<FR>(fe_load<FR>(sh + w * N), fe_mul<FR>(h, zq));
    fe_store<FR>(part + (size_t)blockIdx.x * N, h);
  }
}

// y_k = sum_s part[k][s] (z^slice)^s, one wavefront per claim
template <class FR>
__global__ __launch_bounds__(256) void k_multi_eval_combine(const uint32_t* __restrict__ part, uint32_t nslices,
                                                            uint32_t slice, const uint32_t* __restrict__ gs,
                                                            uint32_t n_groups, const uint32_t* __restrict__ zs,
                                                            uint32_t k0, uint32_t nk, uint32_t* __restrict__ y) {
  constexpr int N = FR::N;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t kl = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (kl >= nk) return;  // whole wavefront
  const uint32_t k = k0 + kl;
  const uint32_t g = claim_group(gs, n_groups, k);
  const Fe<FR> zs_m = mo_pow_u32<FR>(fe_to_mont<FR>(fe_load<FR>(zs + (size_t)g * N)), slice);
  const Fe<FR> c = wave_horner<FR>(part + (size_t)kl * nslices * N, nslices, zs_m, lane);
  if (lane == 0) fe_store<FR>(y + (size_t)k * N, c);
}

// workgroup g: rw[k] = r_g w_k over the group's claims, rz[g] = r_g z_g, tpart[g] = sum_k rw[k] y_k
template <class FR>
__global__ __launch_bounds__(256) void k_multi_rw(const uint32_t* __restrict__ gs, uint32_t count,
                                                  const uint32_t* __restrict__ zs, const uint32_t* __restrict__ ys,
                                                  const uint32_t* __restrict__ weights, uint32_t powers,
                                                  const uint32_t* __restrict__ r, uint32_t* __restrict__ rw,
                                                  uint32_t* __restrict__ rz, uint32_t* __restrict__ tpart) {
  constexpr int N = FR::N;
  __shared__ uint32_t lds[4 * N];
  const uint32_t g = blockIdx.x;
  uint32_t lo, hi;
  group_range(gs, g, count, lo, hi);
  const Fe<FR> rc = fe_load<FR>(r + (size_t)g * N);
  const Fe<FR> rm = fe_to_mont<FR>(rc);
  if (threadIdx.x == 0) fe_store<FR>(rz + (size_t)g * N, fe_mul<FR>(fe_load<FR>(zs + (size_t)g * N), rm));
  Fe<FR> wm = fe_one<FR>(), step = fe_one<FR>();
  if (powers) {
    const Fe<FR> gm = fe_to_mont<FR>(fe_load<FR>(weights + (size_t)g * N));
    wm = mo_pow_u32<FR>(gm, threadIdx.x);
    step = mo_pow_u32<FR>(gm, 256);
  }
  Fe<FR> acc = fe_zero<FR>();
  for (uint64_t k = (uint64_t)lo + threadIdx.x; k < hi; k += 256) {
    if (!powers) wm = fe_to_mont<FR>(fe_load<FR>(weights + (size_t)k * N));
    fe_store<FR>(rw + (size_t)k * N, fe_mul<FR>(rc, wm));
    acc = fe_add<FR>(acc, fe_mul<FR>(fe_mul<FR>(fe_load<FR>(ys + (size_t)k * N), wm), rm));
    if (powers) wm = fe_mul<FR>(wm, step);
  }
  acc = mo_block_sum<FR>(acc, lds);
  if (threadIdx.x == 0) fe_store<FR>(tpart + (size_t)g * N, acc);
}

// workgroup c < n_commits: s_c = sum_{k : commit_index[k] = c} rw[k] (count x n_commits comparisons, no
// sort: as k_cells_commit_weights); workgroup n_commits: -t = -sum_g tpart[g]
template <class FR>
__global__ __launch_bounds__(256) void k_multi_gather(const uint32_t* __restrict__ rw,
                                                      const uint32_t* __restrict__ commit_index, uint32_t count,
                                                      uint32_t n_commits, const uint32_t* __restrict__ tpart,
                                                      uint32_t n_groups, uint32_t* __restrict__ s,
                                                      uint32_t* __restrict__ neg_t) {
  constexpr int N = FR::N;
  __shared__ uint32_t lds[4 * N];
  const uint32_t c = blockIdx.x;
  Fe<FR> acc = fe_zero<FR>();
  if (c < n_commits) {
    for (uint64_t k = threadIdx.x; k < count; k += 256)
      if (commit_index[k] == c) acc = fe_add<FR>(acc, fe_load<FR>(rw + (size_t)k * N));
  } else {
    for (uint64_t g = threadIdx.x; g < n_groups; g += 256) acc = fe_add<FR>(acc, fe_load<FR>(tpart + (size_t)g * N));
  }
  acc = mo_block_sum<FR>(acc, lds);
  if (threadIdx.x == 0) {
    if (c < n_commits)
      fe_store<FR>(s + (size_t)c * N, acc);
    else
      fe_store<FR>(neg_t, fe_neg<FR>(acc));
  }
}

template <class FR>
int fold_impl(const uint32_t* d_coeffs, size_t n, size_t cstride, size_t n_polys, const uint32_t* d_poly_index,
              const uint32_t* d_group_start, size_t g0, size_t ng, size_t count, const uint32_t* d_weights,
              bool powers, uint32_t* d_F, hipStream_t st) {
  const size_t tile = 256 * FOLD_CPL;
  hipLaunchKernelGGL(k_multi_fold<FR>, dim3((unsigned)((n + tile - 1) / tile), (unsigned)ng), dim3(256), 0, st,
                     d_coeffs, (uint32_t)n, cstride, (uint32_t)n_polys, d_poly_index, d_group_start, (uint32_t)g0,
                     (uint32_t)count, d_weights, powers ? 1u : 0u, d_F);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

template <class FR>
int eval_impl(const uint32_t* d_coeffs, size_t n, size_t cstride, size_t n_polys, const uint32_t* d_poly_index,
              const uint32_t* d_group_start, size_t n_groups, const uint32_t* d_zs, size_t k0, size_t nk,
              uint32_t* d_y, uint32_t* d_part, uint32_t slice, hipStream_t st) {
  const unsigned waves = (unsigned)((nk + 3) / 4);
  if (n <= slice) {
    hipLaunchKernelGGL(k_multi_eval_wave<FR>, dim3(waves), dim3(256), 0, st, d_coeffs, (uint32_t)n, cstride,
                       (uint32_t)n_polys, d_poly_index, d_group_start, (uint32_t)n_groups, d_zs, (uint32_t)k0,
                       (uint32_t)nk, d_y);
  } else {
    const size_t nslices = (n + slice - 1) / slice;
    hipLaunchKernelGGL(k_multi_eval_slice<FR>, dim3((unsigned)(nk * nslices)), dim3(256), 0, st, d_coeffs,
                       (uint32_t)n, cstride, (uint32_t)n_polys, d_poly_index, d_group_start, (uint32_t)n_groups, d_zs,
                       (uint32_t)k0, (uint32_t)nslices, slice, d_part);
    hipLaunchKernelGGL(k_multi_eval_combine<FR>, dim3(waves), dim3(256), 0, st, d_part, (uint32_t)nslices, slice,
                       d_group_start, (uint32_t)n_groups, d_zs, (uint32_t)k0, (uint32_t)nk, d_y);
  }
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

template <class FR>
int scalars_impl(const uint32_t* d_commit_index, const uint32_t* d_group_start, size_t n_groups, const uint32_t* d_zs,
                 const uint32_t* d_ys, const uint32_t* d_weights, bool powers, const uint32_t* d_r, size_t count,
                 size_t n_commits, uint32_t* d_out, hipStream_t st) {
  constexpr int N = FR::N;
  uint32_t* s = d_out;
  uint32_t* rz = s + n_commits * N;
  uint32_t* neg_t = rz + n_groups * N;
  uint32_t* rw = neg_t + N;
  uint32_t* tpart = rw + count * N;
  // a claim no group covers (malformed group_start) gathers zero
  if (count) KZGX_TRY_HIP(hipMemsetAsync(rw, 0, count * N * sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_multi_rw<FR>, dim3((unsigned)n_groups), dim3(256), 0, st, d_group_start, (uint32_t)count, d_zs,
                     d_ys, d_weights, powers ? 1u : 0u, d_r, rw, rz, tpart);
  hipLaunchKernelGGL(k_multi_gather<FR>, dim3((unsigned)(n_commits + 1)), dim3(256), 0, st, rw, d_commit_index,
                     (uint32_t)count, (uint32_t)n_commits, tpart, (uint32_t)n_groups, s, neg_t);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

}  // namespace

int multi_check(Ctx* ctx, const uint32_t* d_index, size_t n_index, const uint32_t* d_group_start, size_t n_groups,
                size_t count, uint32_t* d_ok, hipStream_t st) {
  (void)ctx;
  if (n_groups == 0 || n_groups > 0x7fffffffu || count > 0x7fffffffu || n_index > 0xffffffffu) return KZGX_ERR_ARG;
  KZGX_TRY_HIP(hipMemsetD32Async((hipDeviceptr_t)d_ok, 1, 1, st));
  const size_t lanes = std::max(count, n_groups);
  hipLaunchKernelGGL(k_multi_check, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, d_index,
                     (uint32_t)n_index, d_group_start, (uint32_t)n_groups, (uint32_t)count, d_ok);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int multi_fold(Ctx* ctx, const uint32_t* d_coeffs, size_t n, size_t cstride_words, size_t n_polys,
               const uint32_t* d_poly_index, const uint32_t* d_group_start, size_t g0, size_t ng, size_t count,
               const uint32_t* d_weights, bool powers, uint32_t* d_F, hipStream_t st) {
  if (ng == 0) return KZGX_OK;
  if (n == 0 || n > 0xffffffffu || ng > 65535 || g0 + ng > 0x7fffffffu || count > 0x7fffffffu ||
      n_polys > 0xffffffffu)
    return KZGX_ERR_ARG;
  ProfScope prof(ctx, st, "multi_fold");
  return ctx->curve == KZGX_CURVE_BN254
             ? fold_impl<BN254Fr>(d_coeffs, n, cstride_words, n_polys, d_poly_index, d_group_start, g0, ng, count,
                                  d_weights, powers, d_F, st)
             : fold_impl<BLS12381Fr>(d_coeffs, n, cstride_words, n_polys, d_poly_index, d_group_start, g0, ng, count,
                                     d_weights, powers, d_F, st);
}

size_t multi_eval_part_scalars(size_t nk, size_t n, uint32_t slice) {
  return n <= slice ? 0 : nk * ((n + slice - 1) / slice);
}

int multi_eval(Ctx* ctx, const uint32_t* d_coeffs, size_t n, size_t cstride_words, size_t n_polys,
               const uint32_t* d_poly_index, const uint32_t* d_group_start, size_t n_groups, const uint32_t* d_zs,
               size_t k0, size_t nk, uint32_t* d_y, uint32_t* d_part, uint32_t slice, hipStream_t st) {
  if (nk == 0) return KZGX_OK;
  if (n == 0 || n > 0xffffffffu || n_groups == 0 || n_groups > 0x7fffffffu || k0 + nk > 0x7fffffffu ||
      n_polys > 0xffffffffu || slice == 0 || slice % 256 != 0 ||
      multi_eval_part_scalars(nk, n, slice) > 0x7fffffffu || (n > slice && !d_part))
    return KZGX_ERR_ARG;
  ProfScope prof(ctx, st, "multi_eval");
  return ctx->curve == KZGX_CURVE_BN254
             ? eval_impl<BN254Fr>(d_coeffs, n, cstride_words, n_polys, d_poly_index, d_group_start, n_groups, d_zs,
                                  k0, nk, d_y, d_part, slice, st)
             : eval_impl<BLS12381Fr>(d_coeffs, n, cstride_words, n_polys, d_poly_index, d_group_start, n_groups, d_zs,
                                     k0, nk, d_y, d_part, slice, st);
}

size_t multi_scalars_words(size_t n_commits, size_t n_groups, size_t count) {
  return (n_commits + n_groups + 1 + count + n_groups) * 8;
}

int multi_scalars(Ctx* ctx, const uint32_t* d_commit_index, const uint32_t* d_group_start, size_t n_groups,
                  const uint32_t* d_zs, const uint32_t* d_ys, const uint32_t* d_weights, bool powers,
                  const uint32_t* d_r, size_t count, size_t n_commits, uint32_t* d_out, hipStream_t st) {
  if (n_groups == 0 || n_groups > 0x7fffffffu || count > 0x7fffffffu || n_commits > 0x7fffffffu) return KZGX_ERR_ARG;
  ProfScope prof(ctx, st, "multi_scalars");
  return ctx->curve == KZGX_CURVE_BN254
             ? scalars_impl<BN254Fr>(d_commit_index, d_group_start, n_groups, d_zs, d_ys, d_weights, powers, d_r,
                                     count, n_commits, d_out, st)
             : scalars_impl<BLS12381Fr>(d_commit_index, d_group_start, n_groups, d_zs, d_ys, d_weights, powers, d_r,
                                        count, n_commits, d_out, st);
}

}  // namespace kzgx
