// Shplonk openings for gfx950: many committed polynomials opened at different
// point sets under one two-point proof (kzgx_shplonk_commit / _open / _verify,
// include/kzg_gpu.h; BDFG20 section 4).  The hot path is the fused multi-point
// quotient h = sum_s F_s div Z_s, through the partial-fraction identity
//
//   F div Z_s = sum_(i in S_s) c_(s,i) q_(F,t_i),   q_(F,t) = (F - F(t)) / (X - t),
//   c_(s,i) = 1 / prod_(j != i)(t_i - t_j)
//
// (the interpolant's share cancels), so h is a weighted sum of independent
// single-point quotients instead of d_s dependent division passes per set.
// With g_j = f_(j+1) (g_(n-1) = 0) a single-point quotient is the suffix
// recurrence q_j = g_j + t q_(j+1) over n entries, q_(n-1) = 0, which is
// k_qbig_local / k_qbig_scan / k_qbig_replay's recurrence (poly.hip).  Lane l
// of workgroup b owns the SHP_L entries from (256 b + l) SHP_L:
//
//  * k_shp_local (grid: tile x set): the lane's entries of F_s are loaded once
//    into registers; per point of the set a local Horner, the wavefront suffix
//    scan and the four wavefront totals give the tile's total.
//  * k_shp_scan (grid: pair): k_qbig_scan's scheme over a pair's tile totals
//    gives the carry entering each tile from above.
//  * k_shp_replay (grid: tile): the lane owns SHP_L entries of h.  Per set of
//    the chunk it reloads its entries of F_s, and per point it rebuilds the
//    lane carries (local Horner, wavefront scan, the tile's four wavefront
//    totals and the tile carry), replays the chunk and adds c_p q_j into
//    register accumulators.  h is stored once per chunk of sets.
//    The lane carries are recomputed, not stored by k_shp_local: that costs
//    one more Horner pass per (coefficient, point) and saves a workspace of
//    SHP_SET_MAX n / SHP_L scalars per set of the chunk.
//  Up to SHP_TILE coefficients there is one tile, its carry is zero and the
//  first two kernels are not launched.  Field sums run in a fixed order and
//  there are no atomics: results are bit-reproducible.
//
// The rest is small: structure checks, the pair constants c_(s,i) and
// l_(s,i)(z) (one lane per pair, Fermat inverse), zeta_s and Z_T(z) (one
// wavefront per set), value offsets, weight expansion, the (claim, point)
// list of the claimed values for multi_eval, the per-claim weights and the
// axpy of step 2, and the verifier's r_k(z) and scalar packing.
//
// Canonical inputs are multiplied by Montgomery-form constants with fe_mul,
// which yields canonical results, as in poly.hip.  Every index read from
// device memory is range-checked before it addresses anything: start ranges
// are clamped to their totals and to SHP_SET_MAX, point, polynomial and value
// indices are compared before use.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "field.hpp"
#include "shplonk.hpp"

namespace kzgx {
namespace {

constexpr int SHP_L = 8;  // entries per lane: 2 x 64 VGPRs of chunk and accumulators
static_assert(SHP_TILE == 256 * SHP_L, "KZGX_SHPLONK_TILE is one workgroup's span");
// The per-entry steps are written out with constant indices (X(u) for u = 0 .. SHP_L - 1, or downwards): left
// to the loop unroller, one of these loops kept a run-time index and the lane's chunk went to scratch memory.
#define SHP_EACH_UP(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
#define SHP_EACH_DOWN(X) X(7) X(6) X(5) X(4) X(3) X(2) X(1) X(0)
static_assert(SHP_L == 8, "SHP_EACH_UP / SHP_EACH_DOWN list SHP_L entries");

template <class FR>
KZGX_DEV Fe<FR> sh_shfl_down(const Fe<FR>& a, int d) {
  Fe<FR> r;
#pragma unroll
  for (int i = 0; i < FR::N; i++) r.v[i] = __shfl_down(a.v[i], d, 64);
  return r;
}

template <class FR>
KZGX_DEV Fe<FR> sh_shfl(const Fe<FR>& a, uint32_t src) {
  Fe<FR> r;
#pragma unroll
  for (int i = 0; i < FR::N; i++) r.v[i] = __shfl(a.v[i], (int)src, 64);
  return r;
}

template <class FR>
KZGX_DEV Fe<FR> sh_wave_prod(Fe<FR> a) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    Fe<FR> o;
#pragma unroll
    for (int i = 0; i < FR::N; i++) o.v[i] = __shfl_xor(a.v[i], m, 64);
    a = fe_mul<FR>(a, o);
  }
  return a;
}

// left-to-right square-and-multiply from the exponent's top set bit
template <class FR>
KZGX_DEV Fe<FR> sh_pow_u32(const Fe<FR>& base_m, uint32_t e) {
  if (e == 0) return fe_one<FR>();
  Fe<FR> acc = base_m;
  for (int b = 30 - __builtin_clz(e); b >= 0; b--) {
    acc = fe_sqr<FR>(acc);
    if ((e >> b) & 1u) acc = fe_mul<FR>(acc, base_m);
  }
  return acc;
}

// entries [lo, lo + len) of a start array, clamped to [0, total] and to cap entries
KZGX_DEV void sh_range(const uint32_t* __restrict__ start, uint32_t s, uint32_t total, uint32_t cap, uint32_t& lo,
                       uint32_t& len) {
  lo = min(start[s], total);
  uint32_t hi = min(start[s + 1], total);
  if (hi < lo) hi = lo;
  len = min(hi - lo, cap);
}

// the last set s < n_sets with claim_start[s] <= k (0 when there is none); always < n_sets
KZGX_DEV uint32_t sh_claim_set(const uint32_t* __restrict__ cs, uint32_t n_sets, uint32_t k) {
  uint32_t lo = 0, hi = n_sets;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (cs[mid] <= k)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// claim k's set, its point range and its first value; false when no set covers k
KZGX_DEV bool sh_claim(const ShpTable& t, uint32_t k, uint32_t& s, uint32_t& plo, uint32_t& d, uint32_t& kin) {
  s = sh_claim_set(t.claim_start, t.n_sets, k);
  uint32_t clo, m;
  sh_range(t.claim_start, s, t.count, 0xffffffffu, clo, m);
  if (k < clo || k - clo >= m) return false;
  kin = k - clo;
  sh_range(t.set_point_start, s, t.n_set_points, SHP_SET_MAX, plo, d);
  return true;
}

__global__ __launch_bounds__(256) void k_shp_check(ShpTable t, const uint32_t* __restrict__ index, uint32_t n_index,
                                                   uint32_t* __restrict__ ok) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (i < t.count) bad = index[i] >= n_index;
  if (i < t.n_set_points) bad |= t.set_points[i] >= t.n_points;
  if (i < t.n_sets) {
    const uint32_t a = t.set_point_start[i], b = t.set_point_start[i + 1];
    bad |= a >= b || b - a > SHP_SET_MAX;
    bad |= t.claim_start[i] > t.claim_start[i + 1];
  }
  if (i == 0)
    bad |= t.set_point_start[0] != 0u || t.set_point_start[t.n_sets] != t.n_set_points || t.claim_start[0] != 0u ||
           t.claim_start[t.n_sets] != t.count;
  if (bad) *ok = 0u;  // every failing lane stores the same word
}

// one lane per (set, point of the set)
template <class FR>
__global__ __launch_bounds__(256) void k_shp_pairs(ShpTable t, const uint32_t* __restrict__ z,
                                                   uint32_t* __restrict__ pc, uint32_t* __restrict__ pl,
                                                   uint32_t* __restrict__ ok) {
  constexpr int N = FR::N;
  const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t s = (uint32_t)(gid / SHP_SET_MAX), i = (uint32_t)(gid % SHP_SET_MAX);
  if (s >= t.n_sets) return;
  uint32_t lo, d;
  sh_range(t.set_point_start, s, t.n_set_points, SHP_SET_MAX, lo, d);
  if (i >= d) return;
  const uint32_t ii = t.set_points[lo + i];
  Fe<FR> den = fe_one<FR>(), num = fe_one<FR>();
  if (ii < t.n_points) {
    const Fe<FR> ti = fe_load<FR>(t.points + (size_t)ii * N);
    Fe<FR> zc = fe_zero<FR>();
    if (z) zc = fe_load<FR>(z);
    for (uint32_t j = 0; j < d; j++) {
      const uint32_t jj = t.set_points[lo + j];
      if (j == i || jj >= t.n_points) continue;
      const Fe<FR> tj = fe_load<FR>(t.points + (size_t)jj * N);
      den = fe_mul<FR>(den, fe_to_mont<FR>(fe_sub<FR>(ti, tj)));
      if (z) num = fe_mul<FR>(num, fe_to_mont<FR>(fe_sub<FR>(zc, tj)));
    }
  } else {
    den = fe_zero<FR>();
  }
  if (fe_is_zero<FR>(den)) *ok = 0u;  // every failing lane stores the same word
  const Fe<FR> c = fe_inv<FR>(den);   // inv(0) = 0
  fe_store<FR>(pc + (size_t)(lo + i) * N, c);
  if (z) fe_store<FR>(pl + (size_t)(lo + i) * N, fe_mul<FR>(c, num));
}

// one wavefront per set, four per workgroup; set n_sets: all of T
template <class FR>
__global__ __launch_bounds__(256) void k_shp_zeta(ShpTable t, const uint32_t* __restrict__ z,
                                                  uint32_t* __restrict__ zeta) {
  constexpr int N = FR::N;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s > t.n_sets) return;  // whole wavefront
  uint32_t lo = 0, d = 0;
  if (s < t.n_sets) sh_range(t.set_point_start, s, t.n_set_points, SHP_SET_MAX, lo, d);
  const Fe<FR> zc = fe_load<FR>(z);
  Fe<FR> acc = fe_one<FR>();
  for (uint32_t i = lane; i < t.n_points; i += 64) {
    bool in = false;
    for (uint32_t j = 0; j < d; j++) in |= t.set_points[lo + j] == i;
    if (!in) acc = fe_mul<FR>(acc, fe_to_mont<FR>(fe_sub<FR>(zc, fe_load<FR>(t.points + (size_t)i * N))));
  }
  acc = sh_wave_prod<FR>(acc);
  if (lane == 0) fe_store<FR>(zeta + (size_t)s * N, fe_from_mont<FR>(acc));
}

// one workgroup: exclusive prefix sums of d_s m_s over the sets
__global__ __launch_bounds__(256) void k_shp_offsets(ShpTable t, uint64_t* __restrict__ voff, uint64_t n_values,
                                                     uint32_t* __restrict__ ok) {
  __shared__ uint64_t part[256];
  const uint32_t th = threadIdx.x;
  const uint32_t per = (t.n_sets + 255) / 256;
  const uint32_t s0 = min(th * per, t.n_sets), s1 = min(s0 + per, t.n_sets);
  uint64_t sum = 0;
  for (uint32_t s = s0; s < s1; s++) {
    uint32_t lo, d, m;
    sh_range(t.set_point_start, s, t.n_set_points, SHP_SET_MAX, lo, d);
    sh_range(t.claim_start, s, t.count, 0xffffffffu, lo, m);
    sum += (uint64_t)d * m;
  }
  part[th] = sum;
  __syncthreads();
  uint64_t base = 0;
  for (uint32_t u = 0; u < th; u++) base += part[u];
  for (uint32_t s = s0; s < s1; s++) {
    uint32_t lo, d, m;
    sh_range(t.set_point_start, s, t.n_set_points, SHP_SET_MAX, lo, d);
    sh_range(t.claim_start, s, t.count, 0xffffffffu, lo, m);
    voff[s] = base;
    base += (uint64_t)d * m;
  }
  if (th == 255) {  // the last thread's running sum is the total
    voff[t.n_sets] = base;
    if (base != n_values) *ok = 0u;
  }
}

template <class FR>
__global__ __launch_bounds__(256) void k_shp_weight_powers(const uint32_t* __restrict__ gamma, uint32_t count,
                                                           uint32_t* __restrict__ w) {
  constexpr int N = FR::N;
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= count) return;
  const Fe<FR> gm = fe_to_mont<FR>(fe_load<FR>(gamma));
  fe_store<FR>(w + (size_t)k * N, fe_from_mont<FR>(sh_pow_u32<FR>(gm, k)));
}

// one lane per (claim, point slot); the first n_values + 1 lanes also write d_egs
template <class FR>
__global__ __launch_bounds__(256) void k_shp_expand(ShpTable t, const uint64_t* __restrict__ voff,
                                                    const uint32_t* __restrict__ poly_index, uint64_t n_values,
                                                    uint32_t* __restrict__ epoly, uint32_t* __restrict__ ezs,
                                                    uint32_t* __restrict__ egs) {
  constexpr int N = FR::N;
  const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid <= n_values) egs[gid] = (uint32_t)gid;
  const uint64_t k64 = gid / SHP_SET_MAX;
  const uint32_t i = (uint32_t)(gid % SHP_SET_MAX);
  if (k64 >= t.count) return;
  const uint32_t k = (uint32_t)k64;
  uint32_t s, plo, d, kin;
  if (!sh_claim(t, k, s, plo, d, kin) || i >= d) return;
  const uint64_t v = voff[s] + (uint64_t)kin * d + i;
  const uint32_t ii = t.set_points[plo + i];
  if (v >= n_values || ii >= t.n_points) return;
  epoly[v] = poly_index[k];
  fe_store<FR>(ezs + (size_t)v * N, fe_load<FR>(t.points + (size_t)ii * N));
}

// ---- the fused multi-point quotient ---------------------------------------------------------------

// the lane's SHP_L entries g_j = f_(j+1) from entry j0 (zero from n - 1 on)
template <class FR>
KZGX_DEV void shp_load_chunk(const uint32_t* __restrict__ F, uint32_t n, uint64_t j0, Fe<FR> (&g)[SHP_L]) {
#define SHP_STEP(u) g[u] = j0 + u + 1 < n ? fe_load<FR>(F + (size_t)(j0 + u + 1) * FR::N) : fe_zero<FR>();
  SHP_EACH_UP(SHP_STEP)
#undef SHP_STEP
}

// local Horner sum_u g_u t^u, then k_quotient_wg's wavefront suffix scan (poly.hip): c = the wavefront-local
// suffix sum at the lane's first entry, pw = t^(SHP_L (63 - lane)) (when PW), Z = t^(64 SHP_L)
template <class FR, bool PW>
KZGX_DEV void shp_wave_scan(const Fe<FR> (&g)[SHP_L], const Fe<FR>& tm, uint32_t lane, Fe<FR>& c, Fe<FR>& pw,
                            Fe<FR>& Z) {
  Fe<FR> a = g[SHP_L - 1];
#define SHP_STEP(u) a = fe_add<FR>(g[u], fe_mul<FR>(a, tm));
  SHP_STEP(6) SHP_STEP(5) SHP_STEP(4) SHP_STEP(3) SHP_STEP(2) SHP_STEP(1) SHP_STEP(0)
#undef SHP_STEP
  const Fe<FR> tL = sh_pow_u32<FR>(tm, SHP_L);
  Fe<FR> zp = tL;
  c = a;
  pw = lane < 63 ? tL : fe_one<FR>();
#pragma unroll
  for (int s = 0; s < 6; s++) {
    const Fe<FR> o = sh_shfl_down<FR>(c, 1 << s);
    Fe<FR> po;
    if (PW) po = sh_shfl_down<FR>(pw, 1 << s);
    if (lane + (1u << s) < 64) {
      c = fe_add<FR>(c, fe_mul<FR>(o, zp));  // canonical * Montgomery = canonical
      if (PW) pw = fe_mul<FR>(pw, po);
    }
    zp = fe_sqr<FR>(zp);
  }
  Z = zp;
}

// workgroup (tile, set of the chunk): tot[(set slot * SHP_SET_MAX + i) * NT + tile] = sum_(j in tile) g_j t_i^(j - tile start)
template <class FR>
__global__ __launch_bounds__(256) void k_shp_local(const uint32_t* __restrict__ F, uint32_t n, ShpTable t, uint32_t s0,
                                                   uint32_t NT, uint32_t* __restrict__ tot) {
  constexpr int N = FR::N;
  __shared__ uint32_t sh[2][4 * N];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t tile = blockIdx.x, sl = blockIdx.y;
  uint32_t lo, d;
  sh_range(t.set_point_start, s0 + sl, t.n_set_points, SHP_SET_MAX, lo, d);
  Fe<FR> g[SHP_L];
  shp_load_chunk<FR>(F + (size_t)sl * n * N, n, ((uint64_t)tile * 256 + threadIdx.x) * SHP_L, g);
  for (uint32_t i = 0; i < d; i++) {  // d, and every branch below, is the same in every lane of the workgroup
    const uint32_t ii = t.set_points[lo + i];
    Fe<FR> tm = fe_zero<FR>();
    if (ii < t.n_points) tm = fe_to_mont<FR>(fe_load<FR>(t.points + (size_t)ii * N));
    Fe<FR> c, pw, Z;
    shp_wave_scan<FR, false>(g, tm, lane, c, pw, Z);
    uint32_t* buf = sh[i & 1];  // two buffers: one barrier per point
    if (lane == 0) fe_store<FR>(buf + wv * N, c);
    __syncthreads();
    if (threadIdx.x == 0) {
      Fe<FR> H = fe_load<FR>(buf + 3 * N);
      for (int w = 2; w >= 0; w--) H = fe_add<FR>(fe_load<FR>(buf + w * N), fe_mul<FR>(H, Z));
      fe_store<FR>(tot + (((size_t)sl * SHP_SET_MAX + i) * NT + tile) * N, H);
    }
  }
}

// workgroup (set slot * SHP_SET_MAX + i): k_qbig_scan's scheme over the pair's NT tile totals H:
// Ct[g] = sum_(g' > g) H_g' Z^(g' - g - 1), Z = t^SHP_TILE -- the carry entering tile g from above
template <class FR>
__global__ __launch_bounds__(256) void k_shp_scan(ShpTable t, uint32_t s0, uint32_t NT,
                                                  const uint32_t* __restrict__ tot, uint32_t* __restrict__ Ct) {
  constexpr int N = FR::N;
  __shared__ uint32_t sh[256 * N];
  const uint32_t th = threadIdx.x;
  const uint32_t sl = blockIdx.x / SHP_SET_MAX, i = blockIdx.x % SHP_SET_MAX;
  uint32_t lo, d;
  sh_range(t.set_point_start, s0 + sl, t.n_set_points, SHP_SET_MAX, lo, d);
  if (i >= d) return;  // whole workgroup
  const uint32_t ii = t.set_points[lo + i];
  Fe<FR> tm = fe_zero<FR>();
  if (ii < t.n_points) tm = fe_to_mont<FR>(fe_load<FR>(t.points + (size_t)ii * N));
  const uint32_t* H = tot + (size_t)blockIdx.x * NT * N;
  uint32_t* C = Ct + (size_t)blockIdx.x * NT * N;
  const Fe<FR> Z = sh_pow_u32<FR>(tm, SHP_TILE);
  const uint32_t per = (NT + 255) / 256;
  const uint32_t g0 = min(th * per, NT), g1 = min(g0 + per, NT);
  Fe<FR> u = fe_zero<FR>();
  for (uint32_t g = g1; g-- > g0;) u = fe_add<FR>(fe_load<FR>(H + (size_t)g * N), fe_mul<FR>(u, Z));
  // S_t = sum_{t' >= t} u_t' Z^(per (t' - t)), Hillis-Steele over LDS
  Fe<FR> S = u;
  Fe<FR> Zp = sh_pow_u32<FR>(Z, per);
  for (uint32_t dd = 1; dd < 256; dd <<= 1) {
    fe_store<FR>(sh + th * N, S);
    __syncthreads();
    if (th + dd < 256) S = fe_add<FR>(S, fe_mul<FR>(fe_load<FR>(sh + (th + dd) * N), Zp));
    __syncthreads();
    Zp = fe_sqr<FR>(Zp);
  }
  fe_store<FR>(sh + th * N, S);
  __syncthreads();
  Fe<FR> K = th + 1 < 256 ? fe_load<FR>(sh + (th + 1) * N) : fe_zero<FR>();
  // K = the carry at the top of this thread's range (ranges start at multiples of per; only the last
  // non-empty one can be short, and it has no successor)
  for (uint32_t g = g1; g-- > g0;) {
    fe_store<FR>(C + (size_t)g * N, K);
    K = fe_add<FR>(fe_load<FR>(H + (size_t)g * N), fe_mul<FR>(K, Z));
  }
}

// workgroup (tile): h[tile's entries] (+)= sum over the chunk's ns sets and their points of c_p q_(F_s,t_p)
template <class FR>
__global__ __launch_bounds__(256) void k_shp_replay(const uint32_t* __restrict__ F, uint32_t n, ShpTable t,
                                                    uint32_t s0, uint32_t ns, const uint32_t* __restrict__ pc,
                                                    const uint32_t* __restrict__ Ct, uint32_t NT,
                                                    uint32_t* __restrict__ h, uint32_t accumulate) {
  constexpr int N = FR::N;
  __shared__ uint32_t sh[2][4 * N];
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t tile = blockIdx.x;
  const uint64_t j0 = ((uint64_t)tile * 256 + threadIdx.x) * SHP_L;
  Fe<FR> acc[SHP_L];
#define SHP_STEP(u) acc[u] = fe_zero<FR>();
  SHP_EACH_UP(SHP_STEP)
#undef SHP_STEP
  uint32_t it = 0;  // points done: the LDS buffer's parity
  for (uint32_t sl = 0; sl < ns; sl++) {
    uint32_t lo, d;
    sh_range(t.set_point_start, s0 + sl, t.n_set_points, SHP_SET_MAX, lo, d);
    Fe<FR> g[SHP_L];
    shp_load_chunk<FR>(F + (size_t)sl * n * N, n, j0, g);
    for (uint32_t i = 0; i < d; i++) {  // the same trip count and branches in every lane of the workgroup
      const uint32_t ii = t.set_points[lo + i];
      if (ii >= t.n_points) continue;
      const Fe<FR> tm = fe_to_mont<FR>(fe_load<FR>(t.points + (size_t)ii * N));
      const Fe<FR> cm = fe_load<FR>(pc + (size_t)(lo + i) * N);
      Fe<FR> c, pw, Z;
      shp_wave_scan<FR, true>(g, tm, lane, c, pw, Z);
      uint32_t* buf = sh[it & 1];  // two buffers: one barrier per point
      it++;
      if (lane == 0) fe_store<FR>(buf + wv * N, c);
      __syncthreads();
      // lanes 0..3: the wavefront totals; lane 4: the carry entering the tile; S_v = sum_(u >= v) S_u Z^(u - v)
      Fe<FR> S = fe_zero<FR>();
      if (lane < 4) S = fe_load<FR>(buf + lane * N);
      if (lane == 4 && Ct) S = fe_load<FR>(Ct + (((size_t)sl * SHP_SET_MAX + i) * NT + tile) * N);
      Fe<FR> Zp = Z;
#pragma unroll
      for (int st = 0; st < 3; st++) {
        const Fe<FR> o = sh_shfl_down<FR>(S, 1 << st);
        if (lane + (1u << st) < 5) S = fe_add<FR>(S, fe_mul<FR>(o, Zp));
        Zp = fe_sqr<FR>(Zp);
      }
      const Fe<FR> Cw = sh_shfl<FR>(S, wv + 1);  // the carry entering this wavefront's span
      const Fe<FR> cn = sh_shfl_down<FR>(c, 1);
      Fe<FR> q = fe_mul<FR>(Cw, pw);
      if (lane < 63) q = fe_add<FR>(q, cn);
#define SHP_STEP(u)                        \
  q = fe_add<FR>(g[u], fe_mul<FR>(q, tm)); \
  acc[u] = fe_add<FR>(acc[u], fe_mul<FR>(q, cm));
      SHP_EACH_DOWN(SHP_STEP)
#undef SHP_STEP
    }
  }
#define SHP_STEP(u)                                                                      \
  if (j0 + u < n) {                                                                      \
    if (accumulate) acc[u] = fe_add<FR>(acc[u], fe_load<FR>(h + (size_t)(j0 + u) * N)); \
    fe_store<FR>(h + (size_t)(j0 + u) * N, acc[u]);                                      \
  }
  SHP_EACH_UP(SHP_STEP)
#undef SHP_STEP
}

// ---- step 2 and the verifier ----------------------------------------------------------------------

template <class FR>
__global__ __launch_bounds__(256) void k_shp_claim_weights(ShpTable t, const uint32_t* __restrict__ zeta,
                                                           const uint32_t* __restrict__ w, uint32_t* __restrict__ cw,
                                                           uint32_t* __restrict__ gs2) {
  constexpr int N = FR::N;
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k == 0) {
    gs2[0] = 0u;
    gs2[1] = t.count;
  }
  if (k >= t.count) return;
  uint32_t s, plo, d, kin;
  Fe<FR> v = fe_zero<FR>();
  if (sh_claim(t, k, s, plo, d, kin))
    v = fe_mul<FR>(fe_load<FR>(w + (size_t)k * N), fe_to_mont<FR>(fe_load<FR>(zeta + (size_t)s * N)));
  fe_store<FR>(cw + (size_t)k * N, v);
}

template <class FR>
__global__ __launch_bounds__(256) void k_shp_axpy(uint32_t* __restrict__ G, const uint32_t* __restrict__ h,
                                                  const uint32_t* __restrict__ zt, uint32_t n) {
  constexpr int N = FR::N;
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Fe<FR> zm = fe_to_mont<FR>(fe_load<FR>(zt));
  fe_store<FR>(G + (size_t)i * N,
               fe_sub<FR>(fe_load<FR>(G + (size_t)i * N), fe_mul<FR>(fe_load<FR>(h + (size_t)i * N), zm)));
}

template <class FR>
__global__ __launch_bounds__(256) void k_shp_interp(ShpTable t, const uint64_t* __restrict__ voff,
                                                    const uint32_t* __restrict__ ys, uint64_t n_values,
                                                    const uint32_t* __restrict__ pl, uint32_t* __restrict__ rk) {
  constexpr int N = FR::N;
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= t.count) return;
  uint32_t s, plo, d, kin;
  Fe<FR> acc = fe_zero<FR>();
  if (sh_claim(t, k, s, plo, d, kin)) {
    const uint64_t v0 = voff[s] + (uint64_t)kin * d;
    for (uint32_t i = 0; i < d; i++)
      if (v0 + i < n_values)
        acc = fe_add<FR>(acc, fe_mul<FR>(fe_load<FR>(ys + (size_t)(v0 + i) * N), fe_load<FR>(pl + (size_t)(plo + i) * N)));
  }
  fe_store<FR>(rk + (size_t)k * N, acc);
}

template <class FR>
__global__ __launch_bounds__(256) void k_shp_pack(const uint32_t* __restrict__ ms, uint32_t n_commits, uint32_t n_sets,
                                                  const uint32_t* __restrict__ zeta, const uint32_t* __restrict__ z,
                                                  uint32_t* __restrict__ out) {
  constexpr int N = FR::N;
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_commits + 4) return;
  Fe<FR> v;
  if (j < n_commits)
    v = fe_load<FR>(ms + (size_t)j * N);
  else if (j == n_commits)
    v = fe_load<FR>(ms + (size_t)(n_commits + n_sets) * N);  // -t
  else if (j == n_commits + 1)
    v = fe_neg<FR>(fe_load<FR>(zeta + (size_t)n_sets * N));
  else if (j == n_commits + 2)
    v = fe_load<FR>(z);
  else
    v = fe_from_mont<FR>(fe_one<FR>());
  fe_store<FR>(out + (size_t)j * N, v);
}

unsigned blocks256(size_t lanes) { return (unsigned)std::max<size_t>(1, (lanes + 255) / 256); }

template <class FR>
int quotient_impl(const ShpTable& t, const uint32_t* d_F, size_t n, size_t s0, size_t ns, const uint32_t* d_c,
                  uint32_t* d_tot, uint32_t* d_h, bool accumulate, hipStream_t st) {
  const size_t NT = shp_tiles(n);
  uint32_t* Ct = nullptr;
  if (NT > 1) {
    Ct = d_tot + ns * SHP_SET_MAX * NT * FR::N;
    hipLaunchKernelGGL(k_shp_local<FR>, dim3((unsigned)NT, (unsigned)ns), dim3(256), 0, st, d_F, (uint32_t)n, t,
                       (uint32_t)s0, (uint32_t)NT, d_tot);
    hipLaunchKernelGGL(k_shp_scan<FR>, dim3((unsigned)(ns * SHP_SET_MAX)), dim3(256), 0, st, t, (uint32_t)s0,
                       (uint32_t)NT, d_tot, Ct);
  }
  hipLaunchKernelGGL(k_shp_replay<FR>, dim3((unsigned)NT), dim3(256), 0, st, d_F, (uint32_t)n, t, (uint32_t)s0,
                     (uint32_t)ns, d_c, Ct, (uint32_t)NT, d_h, accumulate ? 1u : 0u);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

}  // namespace

#define SHP_DISPATCH(ctx, call)             \
  do {                                      \
    if ((ctx)->curve == KZGX_CURVE_BN254) { \
      call(BN254Fr);                        \
    } else {                                \
      call(BLS12381Fr);                     \
    }                                       \
  } while (0)

int shp_check(const ShpTable& t, const uint32_t* d_index, size_t n_index, uint32_t* d_ok, hipStream_t st) {
  if (n_index > 0xffffffffu) return KZGX_ERR_ARG;
  const size_t lanes = std::max<size_t>({t.count, t.n_set_points, t.n_sets});
  hipLaunchKernelGGL(k_shp_check, dim3(blocks256(lanes)), dim3(256), 0, st, t, d_index, (uint32_t)n_index, d_ok);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int shp_pairs(Ctx* ctx, const ShpTable& t, const uint32_t* d_z, uint32_t* d_c, uint32_t* d_l, uint32_t* d_ok,
              hipStream_t st) {
  ProfScope prof(ctx, st, "shplonk_pairs");
  const dim3 grid(blocks256((size_t)t.n_sets * SHP_SET_MAX));
#define SHP_CALL(FR) hipLaunchKernelGGL(k_shp_pairs<FR>, grid, dim3(256), 0, st, t, d_z, d_c, d_l, d_ok)
  SHP_DISPATCH(ctx, SHP_CALL);
#undef SHP_CALL
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int shp_zeta(Ctx* ctx, const ShpTable& t, const uint32_t* d_z, uint32_t* d_zeta, hipStream_t st) {
  ProfScope prof(ctx, st, "shplonk_zeta");
  const dim3 grid((t.n_sets + 1 + 3) / 4);
#define SHP_CALL(FR) hipLaunchKernelGGL(k_shp_zeta<FR>, grid, dim3(256), 0, st, t, d_z, d_zeta)
  SHP_DISPATCH(ctx, SHP_CALL);
#undef SHP_CALL
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int shp_offsets(const ShpTable& t, uint64_t* d_voff, size_t n_values, uint32_t* d_ok, hipStream_t st) {
  hipLaunchKernelGGL(k_shp_offsets, dim3(1), dim3(256), 0, st, t, d_voff, (uint64_t)n_values, d_ok);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int shp_weight_powers(Ctx* ctx, const uint32_t* d_gamma, size_t count, uint32_t* d_w, hipStream_t st) {
  if (count == 0) return KZGX_OK;
  if (count > 0x7fffffffu) return KZGX_ERR_ARG;
#define SHP_CALL(FR) \
  hipLaunchKernelGGL(k_shp_weight_powers<FR>, dim3(blocks256(count)), dim3(256), 0, st, d_gamma, (uint32_t)count, d_w)
  SHP_DISPATCH(ctx, SHP_CALL);
#undef SHP_CALL
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int shp_expand(Ctx* ctx, const ShpTable& t, const uint64_t* d_voff, const uint32_t* d_poly_index, size_t n_values,
               uint32_t* d_epoly, uint32_t* d_ezs, uint32_t* d_egs, hipStream_t st) {
  if (n_values > 0x7fffffffu) return KZGX_ERR_ARG;
  if (n_values) {
    KZGX_TRY_HIP(hipMemsetAsync(d_epoly, 0xff, n_values * 4, st));
    KZGX_TRY_HIP(hipMemsetAsync(d_ezs, 0, n_values * 32, st));
  }
  const dim3 grid(blocks256(std::max<size_t>((size_t)t.count * SHP_SET_MAX, n_values + 1)));
#define SHP_CALL(FR)                                                                                         \
  hipLaunchKernelGGL(k_shp_expand<FR>, grid, dim3(256), 0, st, t, d_voff, d_poly_index, (uint64_t)n_values, \
                     d_epoly, d_ezs, d_egs)
  SHP_DISPATCH(ctx, SHP_CALL);
#undef SHP_CALL
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

size_t shp_tiles(size_t n) { return std::max<size_t>(1, (n + SHP_TILE - 1) / SHP_TILE); }

int shp_quotient(Ctx* ctx, const ShpTable& t, const uint32_t* d_F, size_t n, size_t s0, size_t ns,
                 const uint32_t* d_c, uint32_t* d_tot, uint32_t* d_h, bool accumulate, hipStream_t st) {
  if (n == 0 || n > 0xffffffffu || ns == 0 || ns > 65535 || s0 + ns > t.n_sets) return KZGX_ERR_ARG;
  ProfScope prof(ctx, st, "shplonk_quotient");
  return ctx->curve == KZGX_CURVE_BN254
             ? quotient_impl<BN254Fr>(t, d_F, n, s0, ns, d_c, d_tot, d_h, accumulate, st)
             : quotient_impl<BLS12381Fr>(t, d_F, n, s0, ns, d_c, d_tot, d_h, accumulate, st);
}

int shp_claim_weights(Ctx* ctx, const ShpTable& t, const uint32_t* d_zeta, const uint32_t* d_w, uint32_t* d_cw,
                      uint32_t* d_gs2, hipStream_t st) {
#define SHP_CALL(FR) \
  hipLaunchKernelGGL(k_shp_claim_weights<FR>, dim3(blocks256(t.count)), dim3(256), 0, st, t, d_zeta, d_w, d_cw, d_gs2)
  SHP_DISPATCH(ctx, SHP_CALL);
#undef SHP_CALL
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int shp_axpy(Ctx* ctx, uint32_t* d_G, const uint32_t* d_h, const uint32_t* d_zt, size_t n, hipStream_t st) {
  if (n > 0xffffffffu) return KZGX_ERR_ARG;
#define SHP_CALL(FR) \
  hipLaunchKernelGGL(k_shp_axpy<FR>, dim3(blocks256(n)), dim3(256), 0, st, d_G, d_h, d_zt, (uint32_t)n)
  SHP_DISPATCH(ctx, SHP_CALL);
#undef SHP_CALL
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int shp_interp(Ctx* ctx, const ShpTable& t, const uint64_t* d_voff, const uint32_t* d_ys, size_t n_values,
               const uint32_t* d_l, uint32_t* d_rk, hipStream_t st) {
  if (t.count == 0) return KZGX_OK;
#define SHP_CALL(FR)                                                                                      \
  hipLaunchKernelGGL(k_shp_interp<FR>, dim3(blocks256(t.count)), dim3(256), 0, st, t, d_voff, d_ys, \
                     (uint64_t)n_values, d_l, d_rk)
  SHP_DISPATCH(ctx, SHP_CALL);
#undef SHP_CALL
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int shp_pack(Ctx* ctx, const uint32_t* d_ms, size_t n_commits, size_t n_sets, const uint32_t* d_zeta,
             const uint32_t* d_z, uint32_t* d_out, hipStream_t st) {
#define SHP_CALL(FR)                                                                                           \
  hipLaunchKernelGGL(k_shp_pack<FR>, dim3(blocks256(n_commits + 4)), dim3(256), 0, st, d_ms, (uint32_t)n_commits, \
                     (uint32_t)n_sets, d_zeta, d_z, d_out)
  SHP_DISPATCH(ctx, SHP_CALL);
#undef SHP_CALL
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

}  // namespace kzgx
