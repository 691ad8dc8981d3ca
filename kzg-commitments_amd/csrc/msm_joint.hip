// Cross-point subset-sum ("block") table for the batched fixed-base G1 MSM.
//
// The window table of msm_fixed.hip replicates every SRS point at W window
// positions so that one scalar never needs a doubling: n W mixed additions
// per MSM.  An MSM of n points can share its doublings instead (bits(r) per
// MSM, not per point), and a table that is not replicated per bit position
// affords a much wider index:
//
//   * the n_t tabled points are cut into blocks of g consecutive points;
//     block b holds points [b g, min((b + 1) g, n_t)), g_b of them;
//   * entry j < 2^(g_b - 1) of a block is
//       P_top + sum_{i < g_b - 1} (2 j_i - 1) P_i
//     (P_top the block's last point, j_i bit i of j): every signed subset sum
//     with sigma_i = +-1, halved by the sign symmetry.  Entries are stored as
//     the window table's (packed_store); the point at infinity as x = y = 0.
//     Block stride 2^(g - 1) entries;
//   * every scalar is recoded in regular +-1 digits (Joye-Tunstall at c = 1,
//     fixed_accum.hpp's recoding): an odd k with u = k >> 1 has
//     d_w = 2 u_w - 1 (w < bits - 1), d_{bits-1} = +1; an even k runs as
//     r - k with every sign flipped, k = 0 as r.  Points [n, blocks g) of a
//     shorter MSM run as scalar 0; whole blocks beyond n are skipped;
//   * MSM = sum_w 2^w A_w, A_w = sum_blocks +- entry[block][signs of plane w]:
//     one gather and one mixed addition per (block, bit plane), then one
//     Horner pass of bits(r) doublings per MSM.
//
// ceil(n / g) bits(r) mixed additions per MSM: 164 x 254 = 41 656 at g = 25
// over 4097 BN254 points against the c = 17 window table's 61 455.
//
// With the endomorphism split (JointTable::glv, KZGX_FIXED_JOINT_GLV; see
// k_joint_index) the same table serves two 128-plane sums per MSM, S_1 and
// S_2 with MSM = S_1 + phi(S_2): ceil(n / g) x 256 mixed additions (against
// 254 / 255) and two Horner chains of 127 doublings side by side, not one of
// 253 / 254.
//
// Passes of one call (profiler scopes):
//   k_joint_index   (msm_scatter)  one 32-bit word per (block, plane)
//   k_joint_accum   (msm_accum)    lane (MSM, plane) sums its plane's entries
//   k_joint_horner1/2 (joint_horner.hip) + k_fixed_finish (msm_reduce);
//   split: k_joint_horner1, k_joint_horner2_glv, k_joint_finish_glv
#include <hip/hip_runtime.h>

#include <algorithm>

#include "curve.hpp"
#include "fixed_accum.hpp"
#include "fixed_msm.hpp"
#include "kzgx_internal.hpp"
#include "kzgx_setup.hpp"

namespace kzgx {

constexpr uint32_t JOINT_NEG = 1u << 31;  // index word: negate the entry

// low / high split of a block's m = g_b - 1 non-top points for the build:
// entry j = HB[j >> a] + LA[j & (2^a - 1)].  a >= 4 whenever m >= 4, so the
// batched builder's 16 consecutive entries share one HB operand; both a(m)
// and m - a(m) are non-decreasing, so a short last block fits the full
// block's half-table slots
__host__ __device__ static inline int joint_split(int m) { return m < 4 ? m : (m / 2 > 4 ? m / 2 : 4); }

// a field element's limbs as they are, into / from a table slot
template <class F>
KZGX_DEV void f29_store_words(uint32_t* p, const F29<F>& a) {
#pragma unroll
  for (int i = 0; i < F::L; i++) p[i] = a.v[i];
}
template <class F>
KZGX_DEV F29<F> f29_load_words(const uint32_t* p) {
  F29<F> r;
#pragma unroll
  for (int i = 0; i < F::L; i++) r.v[i] = p[i];
  return r;
}

size_t joint_table_bytes(int curve, int g, size_t n) {
  if (g < 2 || n == 0) return 0;
  const size_t pb = curve == KZGX_CURVE_BN254 ? packed_words<BN254G1>() * 4 : packed_words<BLS12381G1>() * 4;
  return (n + g - 1) / g * ((size_t)1 << (g - 1)) * pb;
}

// --------------------------------------------------------------------------
// table construction
// --------------------------------------------------------------------------
// entry slot e of block b's half tables (stride hs affine entries):
//   e < la_max:  LA[e]  = sum_{i < a} (2 e_i - 1) P_i
//   e >= la_max: HB[jb] = P_top + sum_{i < m - a} (2 jb_i - 1) P_{a + i}, jb = e - la_max
// An infinite SRS point contributes nothing; a sum at infinity is stored as
// x = y = 0 (not on the curve).
template <class C>
__global__ __launch_bounds__(64) void k_joint_halves(const uint32_t* __restrict__ canon, uint32_t n_t, uint32_t g,
                                                     uint32_t blocks, uint32_t la_max, uint32_t hs,
                                                     uint32_t* __restrict__ half) {
  constexpr int AW = affine_words<C>();
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint64_t)blocks * hs) return;
  const uint32_t b = (uint32_t)(t / hs), e = (uint32_t)(t % hs);
  const uint32_t p0 = b * g;
  const uint32_t gb = n_t - p0 < g ? n_t - p0 : g;
  const int m = (int)gb - 1, a = joint_split(m);
  const bool hi = e >= la_max;
  const uint32_t j = hi ? e - la_max : e;
  const int cnt = hi ? m - a : a;
  if (j >= (1u << cnt)) return;  // a short block's unused slots
  Xyzz<C> acc = xyzz_inf<C>();
  Affine<C> p;
  if (hi && affine_from_canonical<C>(canon + (size_t)(p0 + m) * 2 * C::Fp::N, p)) acc = xyzz_from_affine<C>(p);
  const uint32_t first = p0 + (hi ? (uint32_t)a : 0u);
  for (int i = 0; i < cnt; i++) {
    if (!affine_from_canonical<C>(canon + (size_t)(first + i) * 2 * C::Fp::N, p)) continue;
    if (!((j >> i) & 1u)) p = affine_neg<C>(p);
    acc = xyzz_add_affine<C>(acc, p);
  }
  xyzz_to_affine<C>(acc, p);  // zeros for infinity
  affine_store<C>(half + ((size_t)b * hs + e) * AW, p);
}

template <class C>
KZGX_DEV bool affine_is_inf(const Affine<C>& a) {
  using F = typename C::Fp29;
  return f29_is_zero_exact<F>(a.x) && f29_is_zero_exact<F>(a.y);
}

// HB + LA by the projective route (exact for equal, opposite and infinite
// operands); returns false, and zeros, for a sum at infinity
template <class C>
KZGX_PT bool joint_entry_exact(const Affine<C>& hb, const Affine<C>& la, Affine<C>& out) {
  Xyzz<C> s = affine_is_inf<C>(hb) ? xyzz_inf<C>() : xyzz_from_affine<C>(hb);
  if (!affine_is_inf<C>(la)) s = xyzz_add_affine<C>(s, la);
  return xyzz_to_affine<C>(s, out);
}

// blocks of fewer than 16 entries (m < 4), and any block when asked: one
// thread per entry, projective
template <class C>
__global__ __launch_bounds__(64) void k_joint_entries_small(const uint32_t* __restrict__ half, uint32_t b0,
                                                            uint32_t nb, int m, uint32_t la_max, uint32_t hs,
                                                            size_t bstride, uint32_t* __restrict__ tab,
                                                            unsigned long long* __restrict__ n_inf) {
  constexpr int AW = affine_words<C>();
  constexpr int PW = packed_words<C>();
  const int a = joint_split(m);
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ((uint64_t)nb << m)) return;
  const uint32_t b = b0 + (uint32_t)(t >> m), j = (uint32_t)(t & ((1u << m) - 1u));
  const uint32_t* H = half + (size_t)b * hs * AW;
  Affine<C> r;
  const bool fin = joint_entry_exact<C>(affine_load<C>(H + (size_t)(la_max + (j >> a)) * AW),
                                        affine_load<C>(H + (size_t)(j & ((1u << a) - 1u)) * AW), r);
  if (!fin) atomicAdd(n_inf, 1ull);
  packed_store<C>(tab + (size_t)b * bstride + (size_t)j * PW, r);
}

// Blocks of >= 16 entries: task (block, 16 consecutive entries j0 .. j0 + 15),
// which share HB[j0 >> a].  One affine + affine addition per entry,
//   lambda = (HB.y - LA.y) / (HB.x - LA.x), x' = lambda^2 - LA.x - HB.x,
//   y' = lambda (LA.x - x') - LA.y,
// the 16 inversions batched into one (prefix products kept in the entries'
// own, still empty, table slots: k_fixed_multiples_batch's scheme).  A lane
// with an infinite operand or equal x (equal or opposite points: they do
// occur on a degenerate SRS, tau = 0, +-1) puts 1 into the product and takes
// the projective route.
template <class C>
__global__ __launch_bounds__(64) void k_joint_entries(const uint32_t* __restrict__ half, uint32_t b0, uint32_t nb,
                                                      int m, uint32_t la_max, uint32_t hs, size_t bstride,
                                                      uint64_t t0, uint64_t cnt, uint32_t* __restrict__ tab,
                                                      unsigned long long* __restrict__ n_inf) {
  using F = typename C::Fp29;
  constexpr int AW = affine_words<C>();
  constexpr int PW = packed_words<C>();
  constexpr int K = 16;
  static_assert(PW >= F::L, "a prefix product fits an entry slot");
  const uint64_t gl = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gl >= cnt) return;
  const uint64_t t = t0 + gl;  // < nb 2^(m - 4)
  const int a = joint_split(m);
  const uint32_t b = b0 + (uint32_t)(t >> (m - 4)), j0 = (uint32_t)(t & ((1u << (m - 4)) - 1u)) * K;
  const uint32_t* H = half + (size_t)b * hs * AW;
  const uint32_t* LA = H + (size_t)(j0 & ((1u << a) - 1u)) * AW;
  const Affine<C> B = affine_load<C>(H + (size_t)(la_max + (j0 >> a)) * AW);
  const bool binf = affine_is_inf<C>(B);
  uint32_t* out = tab + (size_t)b * bstride + (size_t)j0 * PW;
  uint32_t deg = 0;  // lanes on the projective route
  F29<F> pre;
  static_for<0, K>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    const Affine<C> A = affine_load<C>(LA + k * AW);
    F29<F> d = f29_sub<F>(B.x, A.x, F::P2);  // B.x + 2m - x in (m, 3m)
    if (binf || affine_is_inf<C>(A) || f29_is_zero<F>(d)) {
      deg |= 1u << k;
      d = f29_one<F>();
    }
    if constexpr (k == 0) pre = d;
    else pre = f29_mul<F>(pre, d);
    if constexpr (k + 1 < K) f29_store_words<F>(out + (size_t)k * PW, pre);
  });
  F29<F> inv = f29_inv_fast<F, C::Fp::N>(pre, C::Fp::P, C::Fp::PM2);
  uint32_t ninf = 0;
  static_for<0, K>([&](auto kc) {
    constexpr int k = K - 1 - decltype(kc)::value;
    const Affine<C> A = affine_load<C>(LA + k * AW);
    const bool dg = (deg >> k) & 1u;
    F29<F> ik = inv;
    if constexpr (k > 0) {
      ik = f29_mul<F>(inv, f29_load_words<F>(out + (size_t)(k - 1) * PW));
      inv = f29_mul<F>(inv, dg ? f29_one<F>() : f29_sub<F>(B.x, A.x, F::P2));
    }
    Affine<C> r;
    if (dg) {
      if (!joint_entry_exact<C>(B, A, r)) ninf++;
    } else {
      const F29<F> lam = f29_mul<F>(f29_sub<F>(B.y, A.y, F::P2), ik);             // (< 3m)(< 2m) -> < 2m
      const F29<F> x3 = f29_sub<F>(f29_sqr<F>(lam), f29_add<F>(A.x, B.x), F::P4);  // < 6m
      const F29<F> tt = f29_mul<F>(lam, f29_sub<F>(A.x, x3, F::P8));               // (< 2m)(< 9m) -> < 2m
      r.x = f29_reduce<F>(x3);
      r.y = f29_reduce<F>(f29_sub<F>(tt, A.y, F::P2));  // < 4m
    }
    packed_store<C>(out + (size_t)k * PW, r);  // slot k's prefix was consumed by step k + 1
  });
  if (ninf) atomicAdd(n_inf, (unsigned long long)ninf);
}

template <class C>
static int joint_build_impl(Ctx* ctx, JointTable& jt, const uint32_t* d_canon, size_t n, int g) {
  constexpr size_t PW = packed_words<C>();
  constexpr size_t AW = affine_words<C>();
  const uint32_t blocks = (uint32_t)((n + g - 1) / g);
  const size_t bstride = ((size_t)1 << (g - 1)) * PW;  // words
  const size_t bytes = (size_t)blocks * bstride * 4;
  const int m_full = g - 1, a_full = joint_split(m_full);
  const uint32_t la_max = 1u << a_full, hs = la_max + (1u << (m_full - a_full));
  hipStream_t st = ctx->stream;
  struct Guard {
    JointTable& jt;
    uint32_t* half = nullptr;
    unsigned long long* cnt = nullptr;
    bool ok = false;
    ~Guard() {
      if (half) (void)hipFree(half);
      if (cnt) (void)hipFree(cnt);
      if (!ok) joint_free(jt);
    }
  } gd{jt};
  KZGX_TRY_HIP(table_malloc((void**)&jt.d, bytes));
  jt.bytes = bytes;
  KZGX_TRY_HIP(hipMalloc((void**)&gd.half, (size_t)blocks * hs * AW * 4));
  KZGX_TRY_HIP(hipMalloc((void**)&gd.cnt, 8));
  KZGX_TRY_HIP(hipMemsetAsync(gd.cnt, 0, 8, st));
  ProfScope p(ctx, st, "fixed_build");
  {
    const uint64_t th = (uint64_t)blocks * hs;
    hipLaunchKernelGGL(k_joint_halves<C>, dim3((unsigned)((th + 63) / 64)), dim3(64), 0, st, d_canon, (uint32_t)n,
                       (uint32_t)g, blocks, la_max, hs, gd.half);
    KZGX_TRY_HIP(hipGetLastError());
  }
  // the full blocks, then the short last block (if any) with its own m
  const uint32_t g_last = (uint32_t)(n - (size_t)(blocks - 1) * g);
  const uint32_t nfull = g_last == (uint32_t)g ? blocks : blocks - 1;
  auto entries = [&](uint32_t b0, uint32_t nb, int m) -> int {
    if (nb == 0) return KZGX_OK;
    if (m < 4) {
      const uint64_t th = (uint64_t)nb << m;
      hipLaunchKernelGGL(k_joint_entries_small<C>, dim3((unsigned)((th + 63) / 64)), dim3(64), 0, st, gd.half, b0, nb,
                         m, la_max, hs, bstride, jt.d, gd.cnt);
      KZGX_TRY_HIP(hipGetLastError());
      return KZGX_OK;
    }
    // bounded launches, synchronised per slice (fixed_multiples_batch)
    const uint64_t tasks = (uint64_t)nb << (m - 4), slice = 1ull << 21;
    for (uint64_t s0 = 0; s0 < tasks; s0 += slice) {
      const uint64_t cnt = tasks - s0 < slice ? tasks - s0 : slice;
      hipLaunchKernelGGL(k_joint_entries<C>, dim3((unsigned)((cnt + 63) / 64)), dim3(64), 0, st, gd.half, b0, nb, m,
                         la_max, hs, bstride, s0, cnt, jt.d, gd.cnt);
      KZGX_TRY_HIP(hipGetLastError());
      KZGX_TRY_HIP(hipStreamSynchronize(st));
    }
    return KZGX_OK;
  };
  KZGX_TRY(entries(0, nfull, m_full));
  if (nfull < blocks) KZGX_TRY(entries(nfull, 1, (int)g_last - 1));
  unsigned long long n_inf = 0;
  KZGX_TRY_HIP(hipMemcpyAsync(&n_inf, gd.cnt, 8, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  jt.n_inf = n_inf;
  jt.g = g;
  jt.blocks = blocks;
  jt.n_t = n;
  gd.ok = true;
  return KZGX_OK;
}

int joint_build(Ctx* ctx, JointTable& jt, const uint32_t* d_canon, size_t n, int g) {
  if (g < 2 || g > 25 || n == 0) return KZGX_ERR_ARG;
  return ctx->curve == KZGX_CURVE_BN254 ? joint_build_impl<BN254G1>(ctx, jt, d_canon, n, g)
                                        : joint_build_impl<BLS12381G1>(ctx, jt, d_canon, n, g);
}

void joint_free(JointTable& jt) {
  if (jt.d) table_free(jt.d, jt.bytes);
  jt.d = nullptr;
  jt.bytes = 0;
  jt.g = 0;
  jt.blocks = 0;
  jt.n_t = 0;
  jt.n_inf = 0;
}

// The split of set_fixed_base(c, n)'s footprint fixed_table_bytes(c, n):
// *g = the block size (0: no block table), *c_win = the window table's bits.
// Automatic (g_req = -1): for 1024 .. 16384 tabled points, the widest g <= 25
// that leaves room for a window table of at least c - 3 bits, and the widest
// such window table.  (Below 1024 points the table is small and nothing
// changes; a table over more than 2^14 points serves few large MSMs -- the
// flat kernel, sharded commits -- which read the window table only, so
// narrowing it for a block table would only cost them.)  Forced (g_req >=
// 2): that g with the widest window table that still fits (KZGX_ERR_ARG when
// none does).
int joint_plan(int curve, int c, size_t n, int g_req, int* g, int* c_win) {
  *g = 0;
  *c_win = c;
  if (g_req == 0 || c == 0 || n == 0) return KZGX_OK;
  if (g_req < 0 && (n < 1024 || n > 16384)) return KZGX_OK;
  const size_t budget = fixed_table_bytes(curve, c, n);
  auto widest = [&](size_t room, int c_min) {
    for (int cw = c; cw >= c_min; cw--)
      if (fixed_bits_supported(cw) && cw != 0 && fixed_table_bytes(curve, cw, n) <= room) return cw;
    return 0;
  };
  if (g_req >= 2) {
    const size_t jb = joint_table_bytes(curve, g_req, n);
    const int cw = jb < budget ? widest(budget - jb, 4) : 0;
    if (!cw) return KZGX_ERR_ARG;
    *g = g_req;
    *c_win = cw;
    return KZGX_OK;
  }
  for (int gg = 25; gg >= 2; gg--) {
    const size_t jb = joint_table_bytes(curve, gg, n);
    if (jb >= budget) continue;
    const int cw = widest(budget - jb, std::max(4, c - 3));
    if (!cw) continue;
    *g = gg;
    *c_win = cw;
    return KZGX_OK;
  }
  return KZGX_OK;  // no split fits: the window table alone, as before
}

// --------------------------------------------------------------------------
// MSM
// --------------------------------------------------------------------------
// Index pass.  A wavefront takes two blocks (lanes 0..31 block 2 q, lanes
// 32..63 block 2 q + 1; lane l & 31 < g_b holds that point's recoded scalar).
// Plane w's sign word of a block is bit w of its <= 32 scalars: a 32 x 32
// bit transpose per scalar word inside each half (five shuffle steps, ~8
// instructions each, for 32 planes of two blocks; a ballot per plane, three
// to four instructions for one plane of two blocks, measured 0.57 ms per
// 2048-MSM launch, 9% of the accumulation), after which lane t holds the
// word of plane 32 k + t.  Bit = 1: plus.  The
// word is normalised to the stored half -- a top point's bit of 0 complements
// it and sets JOINT_NEG -- and masked to g_b - 1 bits: idx < 2^(g_b - 1),
// whatever the scalars.  Layout idx[b][block][plane], plane fastest.
//
// GLV (the endomorphism split, gen_consts.py "Endomorphism split"): the scalar
// is written k = k1 + lambda k2 mod r with both halves odd and below 2^128 in
// magnitude, and each half is recoded as above at 128 planes: u = |k_i| >> 1,
// top digit +1, every sign flipped for a negative half.  Planes 0..127 are
// half 0's (k1), 128..255 half 1's (k2): the MSM is S_1 + phi(S_2), each S
// the half's own block-table sum.  Odd halves need no "even k runs as r - k" step; scalar 0
// (and the padding lanes) splits like any other, into an odd pair that sums
// to 0 mod r.
template <int NA, int NB, int NO>
KZGX_DEV void glv_mul_add(const uint32_t (&a)[NA], const uint32_t (&b)[NB], uint32_t (&acc)[NO]) {
  // acc += a b mod 2^(32 NO)
#pragma unroll
  for (int i = 0; i < NA; i++) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < NB; j++) {
      if (i + j < NO) {
        const uint64_t v = (uint64_t)a[i] * b[j] + acc[i + j] + carry;
        acc[i + j] = (uint32_t)v;
        carry = v >> 32;
      }
    }
#pragma unroll
    for (int t = i + NB; t < NO; t++) {
      const uint64_t v = (uint64_t)acc[t] + carry;
      acc[t] = (uint32_t)v;
      carry = v >> 32;
    }
  }
}

// canonical k < r -> h[0..3] = |k1|, h[4..7] = |k2| (both odd, < 2^128); bit i
// of the return value: half i is negative
template <class C>
KZGX_DEV uint32_t glv_split(const uint32_t (&k)[8], uint32_t (&h)[8]) {
  using G = typename C::Glv;
  static_assert(G::SHIFT == 288, "f_i = words 9..13 of the 14-word product");
  const uint32_t kp = (k[0] & 1u) ^ 1u;  // k + 1 mod 2
  uint32_t c[2][5];
#pragma unroll
  for (int i = 0; i < 2; i++) {
    uint32_t t[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    glv_mul_add<8, 6, 14>(k, G::G[i], t);
    // c_i = f_i or f_i + 1, whichever has the parity that makes both halves odd
    const uint32_t PB = (G::PAR >> (2 * i)) & 1u, PA = (G::PAR >> (2 * i + 1)) & 1u;  // b2, a2 / b1, a1
    const uint32_t want = (PB & kp) ^ PA;
    uint64_t carry = (t[9] ^ want) & 1u;
#pragma unroll
    for (int j = 0; j < 5; j++) {
      const uint64_t v = (uint64_t)t[9 + j] + carry;
      c[i][j] = (uint32_t)v;
      carry = v >> 32;
    }
  }
  uint32_t neg = 0;
#pragma unroll
  for (int half = 0; half < 2; half++) {
    // k1 = k - c1 a1 - c2 a2, k2 = -c1 b1 - c2 b2, mod 2^160 (|k_i| < 2^128)
    uint32_t v[5] = {0, 0, 0, 0, 0};
    if (half == 0) {
#pragma unroll
      for (int j = 0; j < 5; j++) v[j] = k[j];
    }
    glv_mul_add<5, 5, 5>(c[0], G::NEG[2 * half], v);
    glv_mul_add<5, 5, 5>(c[1], G::NEG[2 * half + 1], v);
    const uint32_t sg = v[4] >> 31;
    neg |= sg << half;
    const uint32_t m = 0u - sg;  // |v| = (v ^ m) + sg
    uint64_t carry = sg;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint64_t x = (uint64_t)(v[j] ^ m) + carry;
      h[4 * half + j] = (uint32_t)x;
      carry = x >> 32;
    }
  }
  return neg;
}

template <class C, bool GLV>
__global__ __launch_bounds__(64) void k_joint_index(const uint32_t* __restrict__ scalars, uint32_t n,
                                                    size_t stride_words, uint32_t n_t, uint32_t g, uint32_t nb,
                                                    uint32_t* __restrict__ idx) {
  constexpr int BITS = C::SCALAR_BITS;
  __builtin_amdgcn_s_setprio(3);  // a tail pass: issue ahead of a co-resident accumulation (msm_joint.hip "Tail priority")
  const uint32_t b = blockIdx.y, lane = threadIdx.x;
  const uint32_t hi = lane >> 5, li = lane & 31u;
  const uint32_t blk = 2 * blockIdx.x + hi;
  uint32_t gb = 0;
  if (blk < nb) gb = n_t - blk * g < g ? n_t - blk * g : g;
  const uint32_t i = blk * g + li;
  uint32_t s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (li < gb && i < n) scalar_load(scalars + (size_t)b * stride_words + (size_t)i * 8, s);
  scalar_reduce<C>(s);
  const uint32_t keep = li < gb ? ~0u : 0u;   // lanes past the block offer 0 bits
  if constexpr (GLV) {
    uint32_t h[8];
    const uint32_t neg = glv_split<C>(s, h);
#pragma unroll
    for (int half = 0; half < 2; half++) {
      const uint32_t fl = 0u - ((neg >> half) & 1u);
#pragma unroll
      for (int k = 0; k < 3; k++)
        s[4 * half + k] = (__builtin_amdgcn_alignbit(h[4 * half + k + 1], h[4 * half + k], 1) ^ fl) & keep;
      s[4 * half + 3] = (((h[4 * half + 3] >> 1) | 0x80000000u) ^ fl) & keep;  // u = |k_i| >> 1, d_127 = +1
    }
  } else {
    const uint32_t flip = odd_prepare<C>(s);    // s = u = k' >> 1 < 2^(BITS - 1); scalar 0 runs as r
    s[(BITS - 1) >> 5] |= 1u << ((BITS - 1) & 31);  // d_{BITS-1} = +1
#pragma unroll
    for (int k = 0; k < 8; k++) s[k] = (s[k] ^ (0u - flip)) & keep;
  }
  const uint32_t low = gb ? (1u << (gb - 1)) - 1u : 0u;
  uint32_t* out = idx + ((size_t)b * nb + blk) * JOINT_PL + li;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    // the 32 lanes x 32 bits of word k, transposed in five butterfly steps:
    // step j swaps the (row bit j = 0, column bit j = 1) blocks with their
    // mirror images, rows being lanes (__shfl_xor stays inside the half)
    uint32_t mine = s[k];
    auto swap = [&](int j, uint32_t m) __attribute__((always_inline)) {  // m: the columns with bit j clear
      const uint32_t p = __shfl_xor(mine, j, 64);
      mine = (li & (uint32_t)j) ? (((p >> j) & m) | (mine & ~m)) : ((mine & m) | ((p & m) << j));
    };
    swap(16, 0x0000ffffu);
    swap(8, 0x00ff00ffu);
    swap(4, 0x0f0f0f0fu);
    swap(2, 0x33333333u);
    swap(1, 0x55555555u);
    if (gb) {
      const uint32_t top = (mine >> (gb - 1)) & 1u;
      out[32 * k] = ((top ? mine : ~mine) & low) | (top ? 0u : JOINT_NEG);
    }
  }
}

// Accumulation.  Lane (b, rho, w): plane w of MSM b over block range rho
// (blocks [rho per, min(nb, (rho + 1) per))), one index word, one gathered
// entry and one mixed addition per block; the entry of the next block is in
// flight during each addition and the index word one block further ahead.
// The trip count is uniform: the loop body is straight-line code.  INF (the
// builder counted entries at infinity): the sum with such an entry, x = y =
// 0, is dropped by per-limb selects, no branch; the kernel without it tests
// nothing.
template <class C, bool INF, bool GLV = false, int V = madd_variant<C>()>
__global__ __launch_bounds__(64, fixed_accum_waves<C>()) void k_joint_accum(
    const uint32_t* __restrict__ idx, uint32_t nb, uint32_t per, const uint32_t* __restrict__ tab, size_t bstride,
    uint32_t R, uint32_t* __restrict__ part) {
  constexpr int XW = xyzz_words<C>();
  constexpr int PW = packed_words<C>();
  const uint32_t b = blockIdx.y, rho = blockIdx.x >> 2;
  const uint32_t w = (blockIdx.x & 3u) * 64 + threadIdx.x;
  if constexpr (!GLV) {  // the split's 2 x 128 planes are all live
    if (w >= (uint32_t)C::SCALAR_BITS) return;
  }
  const uint32_t b0 = rho * per, b1 = b0 + per < nb ? b0 + per : nb;
  Xyzz<C> acc = xyzz_inf<C>();
  if (b0 < b1) {
    const uint32_t last = b1 - 1;
    const uint32_t* ip = idx + (size_t)b * nb * JOINT_PL + w;
    auto fetch = [&](uint32_t blk, uint32_t word) __attribute__((always_inline)) {
      return packed_fetch<C>(tab + (size_t)blk * bstride + (size_t)(word & ~JOINT_NEG) * PW);
    };
    uint32_t wq = ip[(size_t)b0 * JOINT_PL];
    PackedPt<C> pq = fetch(b0, wq);
    uint32_t wn = ip[(size_t)(b0 + 1 < last ? b0 + 1 : last) * JOINT_PL];
#pragma unroll 1
    for (uint32_t blk = b0; blk < b1; blk++) {
      Affine<C> cur = packed_unpack<C>(pq);
      const uint32_t neg = wq >> 31;
      const uint32_t nx = blk + 1 < last ? blk + 1 : last;
      wq = wn;
      pq = fetch(nx, wq);
      wn = ip[(size_t)(blk + 2 < last ? blk + 2 : last) * JOINT_PL];
      const bool skip = INF && affine_is_inf<C>(cur);
      affine_cond_neg<C>(cur, neg);
      const Xyzz<C> sum = xyzz_add_affine_v<C, V>(acc, cur);
      if constexpr (INF) {
#pragma unroll
        for (int k = 0; k < C::Fp29::L; k++) {
          acc.X.v[k] = skip ? acc.X.v[k] : sum.X.v[k];
          acc.Y.v[k] = skip ? acc.Y.v[k] : sum.Y.v[k];
          acc.ZZ.v[k] = skip ? acc.ZZ.v[k] : sum.ZZ.v[k];
          acc.ZZZ.v[k] = skip ? acc.ZZZ.v[k] : sum.ZZZ.v[k];
        }
      } else {
        acc = sum;
      }
    }
  }
  xyzz_store<C>(part + (((size_t)b * R + rho) * JOINT_PL + w) * XW, acc);
}

// The Horner pass over the partials (part[b][rho][plane]) is joint_horner.hip's.

// The endomorphism split's default per curve (KZGX_FIXED_JOINT_GLV overrides
// it at context creation): on for both, each measured faster in alternated
// runs (BN254 cfg2 +3.0%, cfg3 +3.0%; BLS12-381 cfg4 +3.7%; DESIGN.md "Block
// table").
bool joint_glv_default(int curve) { return curve == KZGX_CURVE_BN254 || curve == KZGX_CURVE_BLS12381; }

// Residency reserve.  The accumulation's one-wave workgroups fill every wave
// slot their registers allow and free them only at residency boundaries, so
// the other stream's tail passes (stage 1, stage 2, finish, the quotient)
// wait a whole residency each for registers.  A launch with r > 0 asks for
// an unused dynamic LDS size under which a CU admits r workgroups fewer: the
// kernel's code is the same, r wave slots per CU with their registers stay
// free, and the tails run beside the accumulation (DESIGN.md "Block table").
// The size is the smallest for which the occupancy query answers full - r,
// found by bisection (the answer does not rise with the size); r is clamped
// to what a launch's 64 KiB of dynamic LDS can hold back, which leaves at
// least one workgroup per CU.  (The query divides the CU's 160 KiB by the
// byte size; the hardware hands LDS out in granules of 1280 B.  For the
// smallest size of a given answer both agree: profiles/accum_reserve_probe.txt.)
//
// Measured (DESIGN.md "Tail priority and the residency reserve"): the
// accumulation is issue-bound, so the reserve costs no throughput, but a
// launch on its own gets longer and the two-stream line did not win that
// back.  The default is 0 on both curves; the setter stays for A/B runs.
// Only the endomorphism split's tail is fitted to the room a reserve leaves.
//
// Tail priority.  What does make room for the tails is issue priority: the
// index pass, the Horner stages, the finish and the quotient raise their
// wavefronts' priority (s_setprio 3) as they start.  They are short dependent
// chains that need few issue slots, so the accumulation beside them loses
// little, and a tail that no longer crawls behind three accumulation
// wavefronts per SIMD hands its stream's next accumulation to the queue
// while the other stream's is still resident (figures: DESIGN.md).
constexpr size_t JOINT_RESERVE_LDS_MAX = 65536;

int joint_reserve_default(int curve) {
  (void)curve;  // 0 on both curves: see above
  return 0;
}

template <class C>
static int joint_reserve_resolve_impl(JointTable& jt, int req) {
  int rs[4] = {0, 0, 0, 0};  // committed to jt only when every query went through
  uint32_t ls[4] = {0, 0, 0, 0};
  for (int v = 0; v < 4; v++) {
    if (req == 0) continue;
    auto occ = [&](size_t lds, int* out) {
      switch (v) {
        case 0: return hipOccupancyMaxActiveBlocksPerMultiprocessor(out, k_joint_accum<C, false, false>, 64, lds);
        case 1: return hipOccupancyMaxActiveBlocksPerMultiprocessor(out, k_joint_accum<C, true, false>, 64, lds);
        case 2: return hipOccupancyMaxActiveBlocksPerMultiprocessor(out, k_joint_accum<C, false, true>, 64, lds);
        default: return hipOccupancyMaxActiveBlocksPerMultiprocessor(out, k_joint_accum<C, true, true>, 64, lds);
      }
    };
    int full = 0, least = 0;
    KZGX_TRY_HIP(occ(0, &full));
    KZGX_TRY_HIP(occ(JOINT_RESERVE_LDS_MAX, &least));
    if (full < 1) return KZGX_ERR_HIP;
    const int target = std::max(full - std::min(req, full), std::max(least, 1));
    if (target >= full) continue;
    size_t lo = 0, hi = JOINT_RESERVE_LDS_MAX;  // occ(lo) > target >= occ(hi)
    while (hi - lo > 1) {
      const size_t mid = lo + (hi - lo) / 2;
      int o = 0;
      KZGX_TRY_HIP(occ(mid, &o));
      if (o > target) lo = mid;
      else hi = mid;
    }
    int got = 0;
    KZGX_TRY_HIP(occ(hi, &got));
    if (got < 1 || got >= full) return KZGX_ERR_HIP;
    rs[v] = full - got;
    ls[v] = (uint32_t)hi;
  }
  for (int v = 0; v < 4; v++) {
    jt.reserve[v] = rs[v];
    jt.reserve_lds[v] = ls[v];
  }
  return KZGX_OK;
}

int joint_reserve_resolve(int curve, JointTable& jt) {
  const int req = jt.reserve_req < 0 ? joint_reserve_default(curve) : jt.reserve_req;
  return curve == KZGX_CURVE_BN254 ? joint_reserve_resolve_impl<BN254G1>(jt, req)
                                   : joint_reserve_resolve_impl<BLS12381G1>(jt, req);
}

bool joint_serves(const FixedTable& ft, size_t n, size_t batch, bool xyzz_out) {
  const JointTable& jt = ft.joint;
  if (!jt.d || xyzz_out || n == 0 || n > jt.n_t) return false;
  return jt.g_req >= 2 ? batch >= 1 : batch >= 64;
}

template <class C>
static int joint_msm_impl(Ctx* ctx, FixedTable& ft, const uint32_t* d_scalars, size_t n, size_t batch,
                          size_t stride_words, uint32_t* d_out, uint32_t* d_out_inf, hipStream_t st) {
  const JointTable& jt = ft.joint;
  const bool glv = jt.glv;
  constexpr size_t XB = xyzz_words<C>() * sizeof(uint32_t);
  static_assert(C::SCALAR_BITS <= (int)JOINT_PL && C::SCALAR_BITS > 192, "4 wavefronts of planes");
  const uint32_t nb = (uint32_t)((n + jt.g - 1) / jt.g);  // whole blocks beyond n sum to r (...) = O: skipped
  // block ranges per MSM: 1 unless set (2 halves the last residency's tail
  // but doubles the partials; 2048 MSMs of 4097 points measured 272.1k with 2
  // against 276.1k commits + proofs per second with 1, inside the run-to-run
  // spread); never more than blocks
  uint32_t R = jt.ranges ? jt.ranges : 1u;
  R = std::min(R, nb);
  const uint32_t per = (nb + R - 1) / R;
  if (batch > 65535 || 4 * (size_t)R > 65535) return KZGX_ERR_ARG;
  WsLease wsp = ctx->ws_for(st);
  if (!wsp) return KZGX_ERR_ARG;
  MsmWs& ws = *wsp;
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.jidx, batch * (size_t)nb * JOINT_PL * 4, &ws.jidx_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.fpart, batch * (size_t)R * JOINT_PL * XB, &ws.fpart_b));
  // the Horner pass's segment sums [batch][R][JOINT_NSEG], then its [batch] results (one per half under the split)
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.fsum, batch * ((size_t)R * JOINT_NSEG + 2) * XB, &ws.fsum_b));
  {
    ProfScope p(ctx, st, "msm_scatter");
    if (glv)
      hipLaunchKernelGGL((k_joint_index<C, true>), dim3((nb + 1) / 2, (unsigned)batch), dim3(64), 0, st, d_scalars,
                         (uint32_t)n, stride_words, (uint32_t)jt.n_t, (uint32_t)jt.g, nb, ws.jidx);
    else
      hipLaunchKernelGGL((k_joint_index<C, false>), dim3((nb + 1) / 2, (unsigned)batch), dim3(64), 0, st, d_scalars,
                         (uint32_t)n, stride_words, (uint32_t)jt.n_t, (uint32_t)jt.g, nb, ws.jidx);
  }
  {
    ProfScope p(ctx, st, "msm_accum");
    const size_t bstride = ((size_t)1 << (jt.g - 1)) * packed_words<C>();
    // the residency reserve's unused dynamic LDS (0 without one: the plain launch)
    const uint32_t lds = jt.reserve_lds[(glv ? 2 : 0) + (jt.n_inf ? 1 : 0)];
    if (glv && jt.n_inf)
      hipLaunchKernelGGL((k_joint_accum<C, true, true>), dim3(4 * R, (unsigned)batch), dim3(64), lds, st, ws.jidx, nb,
                         per, jt.d, bstride, R, ws.fpart);
    else if (glv)
      hipLaunchKernelGGL((k_joint_accum<C, false, true>), dim3(4 * R, (unsigned)batch), dim3(64), lds, st, ws.jidx,
                         nb, per, jt.d, bstride, R, ws.fpart);
    else if (jt.n_inf)
      hipLaunchKernelGGL((k_joint_accum<C, true>), dim3(4 * R, (unsigned)batch), dim3(64), lds, st, ws.jidx, nb, per,
                         jt.d, bstride, R, ws.fpart);
    else
      hipLaunchKernelGGL((k_joint_accum<C, false>), dim3(4 * R, (unsigned)batch), dim3(64), lds, st, ws.jidx, nb, per,
                         jt.d, bstride, R, ws.fpart);
  }
  {
    ProfScope p(ctx, st, "msm_reduce");
    uint32_t* sums = ws.fsum + batch * (size_t)R * JOINT_NSEG * xyzz_words<C>();
    if (glv) {
      const bool narrow = jt.reserve_lds[2 + (jt.n_inf ? 1 : 0)] != 0;
      KZGX_TRY(joint_horner_glv_launch<C>(ws.fpart, (uint32_t)batch, R, ws.fsum, sums, d_out, d_out_inf, narrow, st));
    } else {
      KZGX_TRY(joint_horner_launch<C>(ws.fpart, (uint32_t)batch, R, ws.fsum, sums, st));
      fixed_finish_launch<C>(sums, (uint32_t)batch, d_out, d_out_inf, nullptr, st);
    }
  }
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int joint_msm(Ctx* ctx, FixedTable& ft, const uint32_t* d_scalars, size_t n, size_t batch, size_t stride_words,
              uint32_t* d_out, uint32_t* d_out_inf, hipStream_t st) {
  return ctx->curve == KZGX_CURVE_BN254
             ? joint_msm_impl<BN254G1>(ctx, ft, d_scalars, n, batch, stride_words, d_out, d_out_inf, st)
             : joint_msm_impl<BLS12381G1>(ctx, ft, d_scalars, n, batch, stride_words, d_out, d_out_inf, st);
}

// debug: the split of count scalars as the index pass forms it; 9 words per
// scalar: |k1| (4), |k2| (4), the sign bits
template <class C>
__global__ __launch_bounds__(64) void k_joint_glv_debug(const uint32_t* __restrict__ scalars, uint32_t count,
                                                        uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  uint32_t s[8], h[8];
  scalar_load(scalars + (size_t)i * 8, s);
  scalar_reduce<C>(s);
  const uint32_t neg = glv_split<C>(s, h);
#pragma unroll
  for (int k = 0; k < 8; k++) out[(size_t)i * 9 + k] = h[k];
  out[(size_t)i * 9 + 8] = neg;
}

int joint_glv_debug(Ctx* ctx, const uint32_t* scalars, size_t count, uint32_t* out) {
  if (!scalars || !out || count == 0 || count > (1u << 24)) return KZGX_ERR_ARG;
  hipStream_t st = ctx->stream;
  uint32_t *d_in = nullptr, *d_out = nullptr;
  KZGX_TRY_HIP(hipMalloc((void**)&d_in, count * 32));
  int rc = hipMalloc((void**)&d_out, count * 36) == hipSuccess ? KZGX_OK : KZGX_ERR_HIP;
  if (rc == KZGX_OK && hipMemcpyAsync(d_in, scalars, count * 32, hipMemcpyHostToDevice, st) != hipSuccess) rc = KZGX_ERR_HIP;
  if (rc == KZGX_OK) {
    const dim3 grid((unsigned)((count + 63) / 64));
    if (ctx->curve == KZGX_CURVE_BN254)
      hipLaunchKernelGGL(k_joint_glv_debug<BN254G1>, grid, dim3(64), 0, st, d_in, (uint32_t)count, d_out);
    else
      hipLaunchKernelGGL(k_joint_glv_debug<BLS12381G1>, grid, dim3(64), 0, st, d_in, (uint32_t)count, d_out);
    if (hipGetLastError() != hipSuccess) rc = KZGX_ERR_HIP;
  }
  if (rc == KZGX_OK && hipMemcpyAsync(out, d_out, count * 36, hipMemcpyDeviceToHost, st) != hipSuccess) rc = KZGX_ERR_HIP;
  if (rc == KZGX_OK && hipStreamSynchronize(st) != hipSuccess) rc = KZGX_ERR_HIP;
  (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  return rc;
}

// device bring-up (kzgx_setup.hpp): one launch loads this code object
__global__ void k_warm_msm_joint() {}
int warm_msm_joint(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_msm_joint, dim3(1), dim3(64), 0, st);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

}  // namespace kzgx
