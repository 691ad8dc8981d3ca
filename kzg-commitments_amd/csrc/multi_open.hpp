// Batch openings (multi_open.hip): many polynomials opened at shared points,
// one proof per point.  Host-side declarations; include/kzg_gpu.h has the
// definitions (groups, claims, weights) these arguments follow.
#pragma once
#include "kzgx_internal.hpp"

namespace kzgx {

constexpr size_t MULTI_CHUNK_SCALARS = KZGX_MULTI_CHUNK_SCALARS;
constexpr uint32_t MULTI_EVAL_SLICE = KZGX_MULTI_EVAL_SLICE;

// *d_ok = 1 iff group_start runs non-decreasing from 0 to count over its n_groups + 1 entries and
// every index[k] < n_index.  Asynchronous; no atomics (every failing lane stores the same 0).
int multi_check(Ctx* ctx, const uint32_t* d_index, size_t n_index, const uint32_t* d_group_start, size_t n_groups,
                size_t count, uint32_t* d_ok, hipStream_t st);

// d_F[(g - g0) n + i] = sum_{k in group g} w_k P_(poly_index[k])[i] for the ng groups from g0 (canonical).
// d_weights: one scalar per claim, or one per group with powers (w_k = gamma_g^(k - group_start[g])).
// Group ranges are clamped to [0, count] and a claim naming a polynomial >= n_polys adds nothing.
int multi_fold(Ctx* ctx, const uint32_t* d_coeffs, size_t n, size_t cstride_words, size_t n_polys,
               const uint32_t* d_poly_index, const uint32_t* d_group_start, size_t g0, size_t ng, size_t count,
               const uint32_t* d_weights, bool powers, uint32_t* d_F, hipStream_t st);

// d_y[k] = P_(poly_index[k])(z_g(k)) for the claims k0 <= k < k0 + nk (d_y points at claim 0), g(k) the
// last group with group_start[g] <= k; 0 for a polynomial index >= n_polys.  n <= MULTI_EVAL_SLICE: one
// wavefront per claim.  Larger n: one workgroup per (claim, slice of `slice` coefficients) into d_part
// (multi_eval_part_scalars(nk, n, slice) scalars), then one wavefront per claim over its partials.
// slice: a multiple of 256 (MULTI_EVAL_SLICE outside tests).
size_t multi_eval_part_scalars(size_t nk, size_t n, uint32_t slice);
int multi_eval(Ctx* ctx, const uint32_t* d_coeffs, size_t n, size_t cstride_words, size_t n_polys,
               const uint32_t* d_poly_index, const uint32_t* d_group_start, size_t n_groups, const uint32_t* d_zs,
               size_t k0, size_t nk, uint32_t* d_y, uint32_t* d_part, uint32_t slice, hipStream_t st);

// The verifier's scalars.  d_out = s_c (n_commits) | r_g z_g (n_groups) | -t (1), all canonical, followed by
// count scalars (r_g(k) w_k, zeroed first) and n_groups scalars (the groups' shares of t) of scratch:
// multi_scalars_words(...) words in all.  Group ranges clamped as in multi_fold; a claim naming a
// commitment >= n_commits matches no gather.
size_t multi_scalars_words(size_t n_commits, size_t n_groups, size_t count);
int multi_scalars(Ctx* ctx, const uint32_t* d_commit_index, const uint32_t* d_group_start, size_t n_groups,
                  const uint32_t* d_zs, const uint32_t* d_ys, const uint32_t* d_weights, bool powers,
                  const uint32_t* d_r, size_t count, size_t n_commits, uint32_t* d_out, hipStream_t st);

}  // namespace kzgx
