// Shplonk openings (shplonk.hip): many polynomials opened at different point
// sets under one two-point proof (BDFG20 section 4).  Host-side declarations;
// include/kzg_gpu.h has the definitions (points, sets, claims, weights, value
// layout) these arguments follow.
#pragma once
#include "kzgx_internal.hpp"

namespace kzgx {

constexpr uint32_t SHP_SET_MAX = KZGX_SHPLONK_SET_MAX;
constexpr uint32_t SHP_TILE = KZGX_SHPLONK_TILE;  // coefficients per workgroup of the fused quotient
constexpr size_t SHP_CHUNK_SCALARS = KZGX_SHPLONK_CHUNK_SCALARS;

// a call's table, all device pointers: the points T, the sets' point indices (set s names
// set_points[set_point_start[s] .. set_point_start[s+1])) and the sets' claim ranges
struct ShpTable {
  const uint32_t* points;
  const uint32_t* set_point_start;
  const uint32_t* set_points;
  const uint32_t* claim_start;
  uint32_t n_points, n_set_points, n_sets, count;
};

// *d_ok &= both start arrays run non-decreasing from 0 to their totals, 1 <= d_s <= SHP_SET_MAX, every
// set_points entry < n_points and every index[k] < n_index.  The caller sets *d_ok = 1 first.
int shp_check(const ShpTable& t, const uint32_t* d_index, size_t n_index, uint32_t* d_ok, hipStream_t st);

// per (set, point) pair p = position in set_points: d_c[p] = c_(s,i) = 1 / prod_(j != i)(t_i - t_j) and, with
// d_z, d_l[p] = l_(s,i)(z), both in Montgomery form.  A zero denominator stores 0 and clears *d_ok.
int shp_pairs(Ctx* ctx, const ShpTable& t, const uint32_t* d_z, uint32_t* d_c, uint32_t* d_l, uint32_t* d_ok,
              hipStream_t st);

// d_zeta[s] = prod_(i in T \ S_s)(z - t_i) for s < n_sets and d_zeta[n_sets] = Z_T(z), canonical
int shp_zeta(Ctx* ctx, const ShpTable& t, const uint32_t* d_z, uint32_t* d_zeta, hipStream_t st);

// d_voff[s] = sum_(s' < s) d_s' m_s' (n_sets + 1 uint64 entries); a total != n_values clears *d_ok
int shp_offsets(const ShpTable& t, uint64_t* d_voff, size_t n_values, uint32_t* d_ok, hipStream_t st);

// d_w[k] = gamma^k for k < count, canonical
int shp_weight_powers(Ctx* ctx, const uint32_t* d_gamma, size_t count, uint32_t* d_w, hipStream_t st);

// the (claim, point) list of the values for multi_eval: value v names polynomial d_epoly[v] (0xffffffff where
// nothing covers v) at the point d_ezs[v], as a group of its own (d_egs[v] = v, n_values + 1 entries)
int shp_expand(Ctx* ctx, const ShpTable& t, const uint64_t* d_voff, const uint32_t* d_poly_index, size_t n_values,
               uint32_t* d_epoly, uint32_t* d_ezs, uint32_t* d_egs, hipStream_t st);

// h (n scalars, h[n-1] = 0) (+)= sum over the ns sets from s0 and their points of c_p (F_s - F_s(t_p)) / (X - t_p),
// F_s at d_F + (s - s0) n scalars.  d_tot: ns * SHP_SET_MAX * shp_tiles(n) * 2 scalars of scratch when
// shp_tiles(n) > 1 (the tile totals and their scan), unused otherwise.  accumulate: add to what d_h holds.
size_t shp_tiles(size_t n);
int shp_quotient(Ctx* ctx, const ShpTable& t, const uint32_t* d_F, size_t n, size_t s0, size_t ns,
                 const uint32_t* d_c, uint32_t* d_tot, uint32_t* d_h, bool accumulate, hipStream_t st);

// d_cw[k] = zeta_(s(k)) w_k (0 for a claim no set covers), canonical; d_gs2 = {0, count}
int shp_claim_weights(Ctx* ctx, const ShpTable& t, const uint32_t* d_zeta, const uint32_t* d_w, uint32_t* d_cw,
                      uint32_t* d_gs2, hipStream_t st);

// d_G[i] -= zt * d_h[i] for i < n
int shp_axpy(Ctx* ctx, uint32_t* d_G, const uint32_t* d_h, const uint32_t* d_zt, size_t n, hipStream_t st);

// d_rk[k] = r_k(z) = sum_i y_(k,i) l_(s,i)(z), canonical (values past n_values count as 0)
int shp_interp(Ctx* ctx, const ShpTable& t, const uint64_t* d_voff, const uint32_t* d_ys, size_t n_values,
               const uint32_t* d_l, uint32_t* d_rk, hipStream_t st);

// the verifier's MSM scalars: d_out = s_c (n_commits) | -t | -Z_T(z) | z | 1 from multi_scalars' output d_ms
int shp_pack(Ctx* ctx, const uint32_t* d_ms, size_t n_commits, size_t n_sets, const uint32_t* d_zeta,
             const uint32_t* d_z, uint32_t* d_out, hipStream_t st);

}  // namespace kzgx
