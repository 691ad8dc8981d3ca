// Fixed-base G1 MSM with a precomputed table of signed-digit multiples
// (Brickell-Gordon-McCurley-Wilson style) for gfx950 -- the fast path behind
// kzg::trusted_setup::create_commit / create_proof / verify_commit when the
// SRS prefix is small enough to precompute
// (reference: trusted_setup::polyeval_G1, src/trusted_setup.cpp:149-174, a
// naive per-term PAIR_G1mul + ECP_add loop).
//
// The SRS is fixed for the lifetime of a trusted_setup, so the work that
// does not depend on the scalars is paid once, at setup time:
//
//   M[w][i][j] = (j + 1) 2^(c w) P_i      w < W, i < n_t, j < H = 2^(c-1)
// stored window-major, or point-major for small c (TabStrides, fixed_accum.hpp)
//
// stored affine, Montgomery form (64-B packed words on BN254, 112-B radix-2^29
// limbs on BLS12-381, see fixed_l29).  A scalar s_i with signed c-bit digits
// d_w (|d_w| <= H) then
// contributes sum_w sign(d_w) M[w][i][|d_w| - 1], so an MSM is a plain sum
// of n W table points: no bucket sort, no bucket reduction, no doublings.
// Each thread sums the W terms of ~P points into one XYZZ accumulator with
// mixed additions (the only heavy instruction stream: 8M + 2S per term, the
// table lookup for the next term in flight underneath), one wavefront per
// MSM folds the partials, and one thread per MSM converts to affine.
//
// Size: W n_t H points; BN254 c = 17 (W = 15) for the 4097-point prefix of
// the degree-4096 benchmark is 257.8 GB -- sized for the 288 GB of HBM3E.
// Every step is an exact group operation, so the affine output is bit-exact
// with any other correct evaluation of sum c_i [tau^i]G1.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "curve.hpp"
#include "fixed_accum.hpp"
#include "fixed_msm.hpp"
#include "kzgx_internal.hpp"
#include "kzgx_setup.hpp"

namespace kzgx {

int fixed_windows(int curve, int c) {  // FixedWin<C, c>::W (regular odd digits)
  const int bits = curve == KZGX_CURVE_BN254 ? BN254G1::SCALAR_BITS : BLS12381G1::SCALAR_BITS;
  return (bits + c - 1) / c;
}

// --------------------------------------------------------------------------
// table construction (setup time)
// --------------------------------------------------------------------------
// window bases B[w][i] = 2^(c w) P_i, packed; thread per SRS point
template <class C>
__global__ __launch_bounds__(64) void k_fixed_bases(const uint32_t* __restrict__ canon, uint32_t n, int W, int c,
                                                    uint32_t* __restrict__ bases, uint8_t* __restrict__ inf) {
  constexpr int PW = packed_words<C>();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Affine<C> a;
  const bool finite = affine_from_canonical<C>(canon + (size_t)i * 2 * C::Fp::N, a);
  inf[i] = finite ? 0 : 1;
  for (int w = 0; w < W; w++) {
    packed_store<C>(bases + ((size_t)w * n + i) * PW, a);
    if (finite && w + 1 < W) {
      Xyzz<C> p = xyzz_from_affine<C>(a);
      for (int s = 0; s < c; s++) p = xyzz_dbl<C>(p);
      xyzz_to_affine<C>(p, a);  // 2^(cw) P_i != O: P_i has order r > 2^(cw)
    }
  }
}

// the same bases from the Pippenger window table when it has the fixed
// table's window (T[w][i] = 2^(c w) P_i, msm.hip k_table_build): a copy into
// the packed layout instead of each point's chain of c (W - 1) doublings and
// W - 1 inversions (2.4 ms for any SRS size, latency-bound)
template <class C>
__global__ __launch_bounds__(256) void k_fixed_bases_from_table(const uint32_t* __restrict__ table,
                                                                const uint8_t* __restrict__ inf_src, uint32_t n,
                                                                uint32_t n_rows, int W, uint32_t* __restrict__ bases,
                                                                uint8_t* __restrict__ inf) {
  constexpr int PW = packed_words<C>();
  constexpr int AW = affine_words<C>();
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (uint64_t)W * n) return;
  const uint32_t w = (uint32_t)(g / n), i = (uint32_t)(g % n);
  packed_store<C>(bases + g * PW, affine_load<C>(table + ((size_t)w * n_rows + i) * AW));
  if (w == 0) inf[i] = inf_src[i];
}

// one wavefront per MSM: strided sums of the T partials, then a shuffle tree
template <class C>
__global__ __launch_bounds__(256) void k_fixed_reduce(const uint32_t* __restrict__ part, uint32_t T, uint32_t batch,
                                                      uint32_t* __restrict__ sums) {
  constexpr int XW = xyzz_words<C>();
  constexpr int L = C::Fp29::L;
  const uint32_t b = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
  const uint32_t lane = threadIdx.x & 63;
  if (b >= batch) return;  // whole wavefronts
  Xyzz<C> acc = xyzz_inf<C>();
  for (uint32_t k = lane; k < T; k += 64) acc = xyzz_add_impl<C>(acc, xyzz_load<C>(part + ((size_t)b * T + k) * XW));
  for (int off = 32; off >= 1; off >>= 1) {
    Xyzz<C> o;
#pragma unroll
    for (int k = 0; k < L; k++) {
      o.X.v[k] = __shfl_down(acc.X.v[k], off, 64);
      o.Y.v[k] = __shfl_down(acc.Y.v[k], off, 64);
      o.ZZ.v[k] = __shfl_down(acc.ZZ.v[k], off, 64);
      o.ZZZ.v[k] = __shfl_down(acc.ZZZ.v[k], off, 64);
    }
    acc = xyzz_add_impl<C>(acc, o);
  }
  if (lane == 0) xyzz_store<C>(sums + (size_t)b * XW, acc);
}

// thread per MSM: XYZZ -> canonical affine + infinity flag, or copy the XYZZ
// point out (chunked callers sum partials themselves)
template <class C>
__global__ __launch_bounds__(64) void k_fixed_finish(const uint32_t* __restrict__ sums, uint32_t batch,
                                                     uint32_t* __restrict__ out, uint32_t* __restrict__ out_inf,
                                                     uint32_t* __restrict__ xyzz_out) {
  constexpr int XW = xyzz_words<C>();
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  const Xyzz<C> p = xyzz_load<C>(sums + (size_t)b * XW);
  if (xyzz_out) {
    xyzz_store<C>(xyzz_out + (size_t)b * XW, p);
    return;
  }
  Affine<C> a;
  const bool fin = xyzz_to_affine<C>(p, a);
  affine_to_canonical<C>(out + (size_t)b * 2 * C::Fp::N, a, fin);
  out_inf[b] = fin ? 0u : 1u;
}


template <class C>
void fixed_reduce_launch(const uint32_t* part, uint32_t T, uint32_t batch, uint32_t* sums, hipStream_t st) {
  // one wavefront per workgroup: a 131 073-point shard's 64:1 level over 48
  // wavefronts took 77 us against 116 us as 4-wave workgroups (r06
  // profiles; the waves of a workgroup do land on 4 different SIMDs,
  // scripts/probe_simd.hip)
  hipLaunchKernelGGL(k_fixed_reduce<C>, dim3(batch), dim3(64), 0, st, part, T, batch, sums);
}
template <class C>
void fixed_finish_launch(const uint32_t* sums, uint32_t batch, uint32_t* out, uint32_t* out_inf, uint32_t* xyzz_out,
                         hipStream_t st) {
  hipLaunchKernelGGL(k_fixed_finish<C>, dim3((batch + 63) / 64), dim3(64), 0, st, sums, batch, out, out_inf, xyzz_out);
}
template void fixed_reduce_launch<BN254G1>(const uint32_t*, uint32_t, uint32_t, uint32_t*, hipStream_t);
template void fixed_reduce_launch<BLS12381G1>(const uint32_t*, uint32_t, uint32_t, uint32_t*, hipStream_t);
template void fixed_finish_launch<BN254G1>(const uint32_t*, uint32_t, uint32_t*, uint32_t*, uint32_t*, hipStream_t);
template void fixed_finish_launch<BLS12381G1>(const uint32_t*, uint32_t, uint32_t*, uint32_t*, uint32_t*, hipStream_t);

// --------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------
// Table layout (TabStrides): point-major for c <= KZGX_FIXED_PM_MAX_C (the
// few-large-MSM tables, walked point by point by k_fixed_accum_flat),
// window-major above (profiles/r03_cfg5_table_layout.json,
// r03_ab_point_major_cfg2.json).  kzgx_set_fixed_base_layout forces one.
#ifndef KZGX_FIXED_PM_MAX_C
#define KZGX_FIXED_PM_MAX_C 12
#endif
static bool fixed_point_major(int c, int layout_req) {
  if (layout_req >= 0) return layout_req != 0;  // kzgx_set_fixed_base_layout(0/1)
  return c <= KZGX_FIXED_PM_MAX_C;
}


template <class C>
static int fixed_build_impl(Ctx* ctx, FixedTable& ft, const uint32_t* d_canon, size_t n) {
  // the request's footprint, fixed_table_bytes(c_req, n), holds the block
  // table (msm_joint.hip; g = 0: none) and a window table at c <= c_req
  int g = 0, c = ft.c_req;
  KZGX_TRY(joint_plan(ctx->curve, ft.c_req, n, ft.joint.g_req, &g, &c));
  const int W = fixed_windows(ctx->curve, c);
  const uint64_t H = 1ull << (c - 1);
  const size_t PB = packed_words<C>() * sizeof(uint32_t);
  const size_t bytes = (size_t)W * n * H * PB;
  // drop the old tables (and the infinity flags) first: the new ones may need
  // most of the device
  if (ft.d || ft.inf || ft.joint.d) {
    KZGX_TRY_HIP(hipDeviceSynchronize());
    fixed_free_table(ft);
  }
  // any failure below leaves no table (and no half-built allocation) behind
  struct Guard {
    FixedTable& ft;
    uint32_t* bases = nullptr;
    uint8_t* inf = nullptr;
    bool ok = false;
    ~Guard() {
      if (bases) (void)hipFree(bases);
      if (!ok) {
        if (inf) (void)hipFree(inf);
        fixed_free_table(ft);
      }
    }
  } gd{ft};
  if (g) KZGX_TRY(joint_build(ctx, ft.joint, d_canon, n, g));
  KZGX_TRY_HIP(table_malloc((void**)&ft.d, bytes));
  ft.bytes = bytes;
  KZGX_TRY_HIP(hipMalloc((void**)&gd.bases, (size_t)W * n * PB));
  KZGX_TRY_HIP(hipMalloc((void**)&gd.inf, n));
  uint32_t* d_bases = gd.bases;
  uint8_t* d_inf = gd.inf;
  hipStream_t st = ctx->stream;
  if (ctx->d_table && ctx->c == c && W <= ctx->W && n <= ctx->n_srs)
    hipLaunchKernelGGL(k_fixed_bases_from_table<C>, dim3((unsigned)(((uint64_t)W * n + 255) / 256)), dim3(256), 0, st,
                       ctx->d_table, ctx->d_inf, (uint32_t)n, (uint32_t)ctx->n_srs, W, d_bases, d_inf);
  else
    hipLaunchKernelGGL(k_fixed_bases<C>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, d_canon, (uint32_t)n, W, c,
                       d_bases, d_inf);
  ft.point_major = fixed_point_major(ft.c_req, ft.layout_req);  // by the request, whatever the split
  const TabStrides ts = fixed_strides<C>(ft.point_major, W, n, H);
  // the batch-affine builder (setup.hip): one inversion per 16 entries
  {
    ProfScope p(ctx, st, "fixed_build");
    KZGX_TRY(fixed_multiples_batch(ctx->curve, d_bases, d_inf, (uint32_t)n, W, (uint32_t)H, ts.is, ts.ws, ft.d, st));
  }
  // whether any SRS point of the prefix is infinite: when none is (every SRS
  // but a degenerate tau = 0 one), the accumulation kernels get no flag array
  // and read no flag per point
  {
    std::vector<uint8_t> h(n);
    KZGX_TRY_HIP(hipMemcpyAsync(h.data(), d_inf, n, hipMemcpyDeviceToHost, st));
    KZGX_TRY_HIP(hipStreamSynchronize(st));
    ft.any_inf = std::any_of(h.begin(), h.end(), [](uint8_t v) { return v != 0; });
    const auto f = std::find(h.begin(), h.end(), (uint8_t)0);
    ft.fin0 = f == h.end() ? UINT32_MAX : (uint32_t)(f - h.begin());
  }
  gd.ok = true;
  ft.inf = d_inf;
  ft.c = c;
  ft.W = W;
  ft.n_t = n;
  return KZGX_OK;
}

int fixed_build_table(Ctx* ctx, FixedTable& ft, const uint32_t* d_canon, size_t n_srs) {
  if (ft.c_req == 0 || ft.n_req == 0) return KZGX_OK;
  const size_t n = ft.n_req < n_srs ? ft.n_req : n_srs;
  return ctx->curve == KZGX_CURVE_BN254 ? fixed_build_impl<BN254G1>(ctx, ft, d_canon, n)
                                        : fixed_build_impl<BLS12381G1>(ctx, ft, d_canon, n);
}

// the default table: a fixed window, or (c_req < 0) the widest c <= 12 whose
// table fits KZGX_DEFAULT_TABLE_PERMILLE of the device memory and the free
// memory less 4 GiB; none if even c = 7 does not.  A context whose device
// already holds a default table over the same SRS prefix (and, for a fixed
// c_req, the same window) shares it instead of building its own.
static int fixed_build_default(Ctx* ctx, const uint32_t* d_canon, size_t n_srs) {
  FixedTable& ft = ctx->fixed_def;
  if (ft.c_req == 0 || ft.n_req == 0) return KZGX_OK;
  fixed_free_table(ft);  // its memory counts as free for the choice
  const size_t n = ft.n_req < n_srs ? ft.n_req : n_srs;
  // the SRS prefix, word for word, is the sharing key (kept and compared on
  // the device)
  const size_t kw = (size_t)n * 2 * ctx->base_words();
  if (table_share_attach(ctx->device, ctx->curve, ft.c_req, d_canon, kw, ctx->stream, ft)) return KZGX_OK;
  auto build = [&](int c) {
    const int keep = ft.c_req;
    ft.c_req = c;
    const int rc = fixed_build_table(ctx, ft, d_canon, n_srs);
    ft.c_req = keep;  // -1: the next SRS picks again
    if (rc == KZGX_OK && ft.d) table_share_register(ctx->device, ctx->curve, d_canon, kw, ctx->stream, ft);
    return rc;
  };
  if (ft.c_req > 0) return build(ft.c_req);
  size_t free_b = 0, total_b = 0;
  KZGX_TRY_HIP(hipMemGetInfo(&free_b, &total_b));
  free_b += table_cache_bytes();  // the cached block is reused or released by table_malloc
  const size_t margin = (size_t)4 << 30;
  size_t budget = total_b / 1000 * KZGX_DEFAULT_TABLE_PERMILLE;
  if (free_b < margin) return KZGX_OK;
  if (budget > free_b - margin) budget = free_b - margin;
  for (int c = 12; c >= 7; c--) {
    if (fixed_table_bytes(ctx->curve, c, n) > budget) continue;
    const int rc = build(c);
    return rc == KZGX_ERR_OOM ? KZGX_OK : rc;  // no room after all: no default table
  }
  return KZGX_OK;
}

int fixed_build(Ctx* ctx, const uint32_t* d_canon, size_t n_srs) {
  KZGX_TRY(fixed_build_table(ctx, ctx->fixed, d_canon, n_srs));
  // the default table is an acceleration cache: if it cannot be built (any
  // status) the SRS stays loaded and the MSMs take Pippenger
  if (fixed_build_default(ctx, d_canon, n_srs) != KZGX_OK) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(ctx->stream);
    fixed_free_table(ctx->fixed_def);
  }
  return KZGX_OK;
}

int fixed_rebuild_default(Ctx* ctx, const uint32_t* d_canon, size_t n_srs) {
  return fixed_build_default(ctx, d_canon, n_srs);
}

void fixed_free(Ctx* ctx) { fixed_free_table(ctx->fixed); }

void fixed_free_table(FixedTable& ft) {
  if (ft.shared) {
    table_share_release(ft);  // the last holder frees it
    ft.shared = 0;
  } else {
    if (ft.d) table_free(ft.d, ft.bytes);
    if (ft.inf) (void)hipFree(ft.inf);
  }
  joint_free(ft.joint);  // the request (g_req, ranges) stays
  ft.d = nullptr;
  ft.inf = nullptr;
  ft.bytes = 0;
  ft.n_t = 0;
  ft.c = 0;
  ft.fin0 = UINT32_MAX;
}

template <class C>
static int fixed_msm_c(Ctx* ctx, FixedTable& ft, const uint32_t* d_scalars, size_t n, size_t batch,
                       size_t stride_words, uint32_t* d_out, uint32_t* d_out_inf, hipStream_t st, uint32_t* xyzz_out) {
  switch (ft.c) {
#define KZGX_FIXED_CASE(cb) \
  case cb: return fixed_msm_win<C, cb>(ctx, ft, d_scalars, n, batch, stride_words, d_out, d_out_inf, st, xyzz_out);
    KZGX_FIXED_CASE(4)
    KZGX_FIXED_CASE(7)
    KZGX_FIXED_CASE(8)
    KZGX_FIXED_CASE(9)
    KZGX_FIXED_CASE(10)
    KZGX_FIXED_CASE(11)
    KZGX_FIXED_CASE(12)
    KZGX_FIXED_CASE(13)
    KZGX_FIXED_CASE(14)
    KZGX_FIXED_CASE(15)
    KZGX_FIXED_CASE(16)
    KZGX_FIXED_CASE(17)
#undef KZGX_FIXED_CASE
    default: return KZGX_ERR_INTERNAL;
  }
}

size_t fixed_table_bytes(int curve, int c, size_t n) {
  if (c <= 0) return 0;
  const size_t pb = curve == KZGX_CURVE_BN254 ? packed_words<BN254G1>() * 4 : packed_words<BLS12381G1>() * 4;
  return (size_t)fixed_windows(curve, c) * n * ((size_t)1 << (c - 1)) * pb;
}

bool fixed_bits_supported(int c) {
  return c == 0 || c == 4 || (c >= 7 && c <= 17);
}

// (a prefix of infinite points only -- a loaded all-infinity SRS -- has no
// finite point to carry the identity terms of k_fixed_accum: Pippenger)
bool fixed_table_usable(const FixedTable& ft, size_t n) {
  return ft.d && ft.n_t > 0 && n <= ft.n_t && ft.fin0 != UINT32_MAX;
}
bool fixed_usable(const Ctx* ctx, size_t n) { return fixed_table_usable(ctx->fixed, n); }

int fixed_msm_table(Ctx* ctx, FixedTable& ft, const uint32_t* d_scalars, size_t n, size_t batch, size_t stride_words,
                    uint32_t* d_out, uint32_t* d_out_inf, hipStream_t st, uint32_t* xyzz_out) {
  // batched calls take the block table when there is one; the window table
  // keeps the latency kernel, the XYZZ partial records and the flat path
  if (joint_serves(ft, n, batch, xyzz_out != nullptr))
    return joint_msm(ctx, ft, d_scalars, n, batch, stride_words, d_out, d_out_inf, st);
  return ctx->curve == KZGX_CURVE_BN254
             ? fixed_msm_c<BN254G1>(ctx, ft, d_scalars, n, batch, stride_words, d_out, d_out_inf, st, xyzz_out)
             : fixed_msm_c<BLS12381G1>(ctx, ft, d_scalars, n, batch, stride_words, d_out, d_out_inf, st, xyzz_out);
}

int fixed_msm(Ctx* ctx, const uint32_t* d_scalars, size_t n, size_t batch, size_t stride_words, uint32_t* d_out,
              uint32_t* d_out_inf, hipStream_t st, uint32_t* xyzz_out) {
  return fixed_msm_table(ctx, ctx->fixed, d_scalars, n, batch, stride_words, d_out, d_out_inf, st, xyzz_out);
}

// --------------------------------------------------------------------------
// measured VALU peak of the accumulation loop (the denominator of the bench's
// valu_roofline): k_fixed_accum's inlined XYZZ mixed addition, with the same
// launch bounds (waves per SIMD), over operands that stay in L1 (a 64-point
// table: no HBM stream, no digit logic), whole GPU, ITER additions per thread
// --------------------------------------------------------------------------
template <class C>
__global__ __launch_bounds__(64, fixed_accum_waves<C>()) void k_microbench_madd(const uint32_t* __restrict__ pts,
                                                                                uint32_t iters,
                                                                                uint32_t* __restrict__ sink) {
  constexpr int PW = affine_words<C>();
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  Xyzz<C> acc = xyzz_from_affine<C>(affine_load<C>(pts + (size_t)(t & 63) * PW));
#pragma unroll 1
  for (uint32_t k = 0; k < iters; k++) {
    Affine<C> a = affine_load<C>(pts + (size_t)((t + 1 + k) & 63) * PW);
    acc = xyzz_add_affine_impl<C>(acc, a);
  }
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < C::Fp29::L; i++) o ^= acc.X.v[i] ^ acc.ZZ.v[i];
  if (o == 0x9e3779b9u) sink[t] = o;  // keeps the chain live; practically never stores
}

// mixed additions per second: 64 distinct multiples of the SRS's first point
// (built with the table kernels' own arithmetic), then a timed launch
template <class C>
static int microbench_madd_impl(Ctx* ctx, double* rate) {
  if (ctx->n_srs == 0) return KZGX_ERR_NO_SRS;
  constexpr int PW = affine_words<C>();
  hipStream_t st = ctx->stream;
  uint32_t *d_pts = nullptr, *d_sink = nullptr;
  const uint32_t waves = 256 * 4 * fixed_accum_waves<C>() * 4;  // four full residencies
  const uint32_t iters = 192;
  KZGX_TRY_HIP(hipMalloc((void**)&d_pts, 64 * PW * 4));
  struct Free {
    uint32_t** a;
    uint32_t** b;
    ~Free() {
      if (*a) (void)hipFree(*a);
      if (*b) (void)hipFree(*b);
    }
  } fr{&d_pts, &d_sink};
  KZGX_TRY_HIP(hipMalloc((void**)&d_sink, (size_t)waves * 64 * 4));
  // T[0][i] holds the SRS points in the 80 / 112 B radix-2^29 layout; the
  // first 64 points (or repeats of them) are distinct curve points
  for (uint32_t i = 0; i < 64; i++)
    KZGX_TRY_HIP(hipMemcpyAsync(d_pts + (size_t)i * PW, ctx->d_table + (size_t)(i % ctx->n_srs) * PW, PW * 4,
                                hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(k_microbench_madd<C>, dim3(waves), dim3(64), 0, st, d_pts, 8u, d_sink);  // warm
  hipEvent_t a, b;
  KZGX_TRY_HIP(hipEventCreate(&a));
  KZGX_TRY_HIP(hipEventCreate(&b));
  KZGX_TRY_HIP(hipEventRecord(a, st));
  hipLaunchKernelGGL(k_microbench_madd<C>, dim3(waves), dim3(64), 0, st, d_pts, iters, d_sink);
  KZGX_TRY_HIP(hipEventRecord(b, st));
  KZGX_TRY_HIP(hipEventSynchronize(b));
  float ms = 0;
  hipError_t e = hipEventElapsedTime(&ms, a, b);
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  KZGX_TRY_HIP(e);
  KZGX_TRY_HIP(hipGetLastError());
  *rate = (double)waves * 64 * iters / (ms * 1e-3);
  return KZGX_OK;
}

// v_mad_u64_u32 issue ceiling: 8 independent accumulator chains per lane,
// 256 mads per chain per iteration, 8 waves per SIMD (the instruction
// exactly, in asm; scripts/micro_valu.hip, profiles/r01_micro_valu.txt)
__global__ __launch_bounds__(256) void k_microbench_mad64(uint32_t iters, uint32_t* __restrict__ sink,
                                                          uint64_t* __restrict__ stamp) {
  // block 0's first lane counts core clocks against the constant-rate wall
  // clock over its run: every block is resident at once, so that is the
  // clock the ceiling was measured at
  uint64_t w0 = 0, c0 = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    w0 = wall_clock64();
    c0 = clock64();
  }
  uint64_t acc[8];
  const uint32_t a = threadIdx.x + 1, b = blockIdx.x + 3;
#pragma unroll
  for (int k = 0; k < 8; k++) acc[k] = k;
#pragma unroll 1
  for (uint32_t it = 0; it < iters; it++) {
#pragma unroll
    for (int r = 0; r < 32; r++) {
#pragma unroll
      for (int k = 0; k < 8; k++) {
        uint64_t sc;
        asm volatile("v_mad_u64_u32 %0, %1, %2, %3, %0" : "+v"(acc[k]), "=s"(sc) : "v"(a), "v"(b));
      }
    }
  }
  uint64_t o = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) o ^= acc[k];
  if ((uint32_t)o == 0x9e3779b9u) sink[blockIdx.x * blockDim.x + threadIdx.x] = (uint32_t)o;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t c1 = clock64(), w1 = wall_clock64();
    stamp[0] = c1 - c0;
    stamp[1] = w1 - w0;
  }
}

int microbench_mad_u64(Ctx* ctx, double* rate, double* ghz) {
  hipStream_t st = ctx->stream;
  const uint32_t blocks = 256 * 8, iters = 64;
  uint32_t* d_sink = nullptr;
  KZGX_TRY_HIP(hipMalloc((void**)&d_sink, (size_t)blocks * 256 * 4 + 16));
  uint64_t* d_stamp = reinterpret_cast<uint64_t*>(d_sink + (size_t)blocks * 256);
  hipLaunchKernelGGL(k_microbench_mad64, dim3(blocks), dim3(256), 0, st, 2u, d_sink, d_stamp);  // warm
  hipEvent_t a, b;
  KZGX_TRY_HIP(hipEventCreate(&a));
  KZGX_TRY_HIP(hipEventCreate(&b));
  KZGX_TRY_HIP(hipEventRecord(a, st));
  hipLaunchKernelGGL(k_microbench_mad64, dim3(blocks), dim3(256), 0, st, iters, d_sink, d_stamp);
  KZGX_TRY_HIP(hipEventRecord(b, st));
  KZGX_TRY_HIP(hipEventSynchronize(b));
  float ms = 0;
  hipError_t e = hipEventElapsedTime(&ms, a, b);
  uint64_t h[2] = {0, 0};
  if (e == hipSuccess) e = hipMemcpy(h, d_stamp, sizeof h, hipMemcpyDeviceToHost);
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  (void)hipFree(d_sink);
  KZGX_TRY_HIP(e);
  KZGX_TRY_HIP(hipGetLastError());
  *rate = (double)blocks * 256 * iters * 256 / (ms * 1e-3);
  if (ghz) {
    int khz = 0;
    KZGX_TRY_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
    *ghz = h[1] ? (double)h[0] / (double)h[1] * khz * 1e-6 : 0.0;
  }
  return KZGX_OK;
}

// The core clock while other work runs: one lane spins for spin_us of the
// constant-rate wall clock and counts core clocks meanwhile.  The DVFS clock
// is one per device (MI355X_MICROARCH.md, DVFS give-back), so a probe
// resident beside a kernel reads that kernel's clock; it holds one wave slot.
// out: core clocks, wall ticks, wall clock rate in kHz.
__global__ __launch_bounds__(64) void k_clock_probe(uint64_t ticks, uint32_t khz, uint64_t* __restrict__ out) {
  if (threadIdx.x != 0) return;
  const uint64_t w0 = wall_clock64(), c0 = clock64();
  uint64_t w = w0;
  while (w - w0 < ticks) w = wall_clock64();
  const uint64_t c1 = clock64();
  out[0] = c1 - c0;
  out[1] = w - w0;
  out[2] = khz;
}

int clock_probe(Ctx* ctx, hipStream_t st, uint32_t spin_us, uint64_t* d_out) {
  int khz = 0;
  KZGX_TRY_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
  const uint64_t ticks = (uint64_t)spin_us * (uint64_t)khz / 1000;
  hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, st ? st : ctx->stream, ticks, (uint32_t)khz, d_out);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int microbench_mixed_add(Ctx* ctx, double* rate) {
  return ctx->curve == KZGX_CURVE_BN254 ? microbench_madd_impl<BN254G1>(ctx, rate)
                                        : microbench_madd_impl<BLS12381G1>(ctx, rate);
}

// --------------------------------------------------------------------------
// single-lane latency of the primitives on the latency-bound tails (the
// finish kernels and the last reduction levels of one MSM): a dependent chain
// of ITER operations in one lane of one wavefront, timed with the shader's
// constant-rate wall clock and its core-clock counter inside the kernel
// (no launch overhead).  op: 0 Montgomery product, 1 Fermat inversion,
// 2 binary-Euclid inversion, 3 XYZZ addition, 4 mixed addition, 5 XYZZ ->
// affine conversion, 6 / 7 the same as 2 / 5 on the scalar ALU (one lane's
// value made wave-uniform), 8 / 9 the same with the whole wavefront active
// (the linear combinations one per lane).
// --------------------------------------------------------------------------
template <class C>
__global__ __launch_bounds__(64) void k_debug_latency(const uint32_t* __restrict__ pts, int op, uint32_t iters,
                                                      uint64_t* __restrict__ out) {
  using F = typename C::Fp29;
  constexpr int PW = affine_words<C>();
  if (threadIdx.x != 0 && op < 8) return;  // 8, 9: the whole wavefront on one value
  const Affine<C> p = affine_load<C>(pts), q = affine_load<C>(pts + PW);
  F29<F> a = p.x;
  Xyzz<C> acc = xyzz_from_affine<C>(p);
  const Xyzz<C> qx = xyzz_add_affine_impl<C>(xyzz_from_affine<C>(q), q);  // 2q, Z != 1
  const uint64_t w0 = wall_clock64(), c0 = clock64();
#pragma unroll 1
  for (uint32_t k = 0; k < iters; k++) {
    if (op == 0) a = f29_mul<F>(a, p.y);
    else if (op == 1) a = f29_inv<F, C::Fp::N>(a, C::Fp::PM2);
    else if (op == 2) a = f29_inv_vt<F, C::Fp::N>(a, C::Fp::P);
    else if (op == 3) acc = xyzz_add_impl<C>(acc, qx);
    else if (op == 4) acc = xyzz_add_affine_impl<C>(acc, q);
    else if (op == 6 || op == 8) a = f29_inv_uniform<F, C::Fp::N>(a, C::Fp::P);
    else if (op == 7 || op == 9) {
      Affine<C> r;
      (void)xyzz_to_affine_impl<C, true>(acc, r);
      acc.X = r.y;
    } else {
      Affine<C> r;
      (void)xyzz_to_affine_impl<C>(acc, r);
      acc.X = r.y;  // next input depends on this output
    }
  }
  const uint64_t w1 = wall_clock64(), c1 = clock64();
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < F::L; i++) o ^= a.v[i] ^ acc.X.v[i] ^ acc.ZZ.v[i];
  if (threadIdx.x != 0) return;
  out[0] = w1 - w0;
  out[1] = c1 - c0;
  out[2] = o;
}

template <class C>
static int debug_latency_impl(Ctx* ctx, int op, uint32_t iters, double* res) {
  if (ctx->n_srs < 2) return KZGX_ERR_NO_SRS;
  constexpr int PW = affine_words<C>();
  hipStream_t st = ctx->stream;
  uint32_t* d_pts = nullptr;
  uint64_t* d_out = nullptr;
  KZGX_TRY_HIP(hipMalloc((void**)&d_pts, 2 * PW * 4));
  if (hipMalloc((void**)&d_out, 3 * 8) != hipSuccess) {
    (void)hipFree(d_pts);
    return KZGX_ERR_HIP;
  }
  (void)hipMemcpyAsync(d_pts, ctx->d_table, 2 * PW * 4, hipMemcpyDeviceToDevice, st);
  hipLaunchKernelGGL(k_debug_latency<C>, dim3(1), dim3(64), 0, st, d_pts, op, 1u, d_out);  // warm
  hipLaunchKernelGGL(k_debug_latency<C>, dim3(1), dim3(64), 0, st, d_pts, op, iters, d_out);
  uint64_t h[3] = {0, 0, 0};
  hipError_t e = hipMemcpyAsync(h, d_out, sizeof h, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(d_pts);
  (void)hipFree(d_out);
  KZGX_TRY_HIP(e);
  int khz = 0;
  KZGX_TRY_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
  res[0] = (double)h[0] / iters / (khz * 1e3) * 1e9;  // ns per operation
  res[1] = (double)h[1] / iters;                      // core clocks per operation
  return KZGX_OK;
}

int debug_latency(Ctx* ctx, int op, uint32_t iters, double* res) {
  if (op < 0 || op > 9 || iters == 0) return KZGX_ERR_ARG;
  return ctx->curve == KZGX_CURVE_BN254 ? debug_latency_impl<BN254G1>(ctx, op, iters, res)
                                        : debug_latency_impl<BLS12381G1>(ctx, op, iters, res);
}

}  // namespace kzgx

namespace kzgx {
// device bring-up (kzgx_setup.hpp): one launch loads this code object
__global__ void k_warm_msm_fixed() {}
int warm_msm_fixed(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_msm_fixed, dim3(1), dim3(64), 0, st);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}
}  // namespace kzgx
