// Cell recovery for gfx950: rebuilds polynomials of n coefficients from any half
// of the R cells of their size-D = 2n evaluation domain (DESIGN.md "Cell
// recovery"), the inverse of the extended coset openings of g1_ntt.hip.
//
// Notation of include/kzg_gpu.h: l = 2^kl values per cell, R = 2^kR = D / l cosets,
// w = w_D, w_R = w^l, coset i = {w^(i + R j)} = the roots of X^l - w_R^i.  Per blob,
// M = the cosets no cell names:
//   Zs(Y) = prod_{i in M} (Y - w_R^i),  Z(X) = Zs(X^l)      (constant on a coset)
//   E = y Z on the domain (0 on M)        -> Q = INTT_D(E) = the coefficients of P Z
//   Q'[j] = g^j Q[j], NTT_D, / Zs(g^l w_R^(e mod R)), INTT_D, * g^-j  -> P, n coefficients
//   V = NTT_D(P zero-extended), compared with every supplied value    -> ok
// The four transforms are ntt.hip's, in place on the chunk's workspace; the
// kernels here are the steps between them:
//   k_rec_map      slot[b][i] = k + 1 for the cell k that names coset i of blob b
//                  (compare-and-swap: a second cell of the same coset marks the blob),
//                  the blobs' cell counts, cell indices >= R, blob indices >= n_blobs
//   k_rec_locator  one lane per (blob, p): Zs(w_R^p) and 1 / Zs(g^l w_R^p); the roots of
//                  the missing cosets come from the Fr NTT's twiddle table, gathered
//                  through LDS once per workgroup; a Fermat inverse per lane; lane 0 of
//                  a blob settles its gate (enough cells, no duplicate)
//   k_rec_mask     E in the transform's input order (a cell is one contiguous chunk of
//                  the bit-reversed array)
//   k_rec_shift    Q'[j] = g^j Q[j], and with TRUNC the way back: P[j] = g^-j S[j] for
//                  j < n, zero above (the zero extension of the last transform).  One
//                  lane per j computes g^(+-j) from the squarings passed by value and
//                  uses it for every blob of its slice of the chunk
//   k_rec_scale    the division by Z on the shifted coset (bit-reversed positions)
//   k_rec_check    clears the blob's gate on the first supplied value that differs
//   k_rec_finish   out_y in the caller's layout, ok, and zeros for a failed blob
// Scalars are canonical in and out; locator values and powers of g are Montgomery
// values, so fe_mul(canonical, Montgomery) is canonical and no conversion pass runs
// (ntt.hip's convention).  A blob the device form cannot recover (too few cells, a
// duplicate) still runs through every step on whatever its map holds: every index
// is in range by construction and its gate is already 0.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "field.hpp"
#include "fr_host.hpp"
#include "kzgx_internal.hpp"

namespace kzgx {

// the quadratic non-residue whose powers are the domain roots (gen_consts.py NTT_GEN)
template <class FR>
struct RecGen;
template <>
struct RecGen<BN254Fr> {
  static constexpr uint32_t G = 2;
};
template <>
struct RecGen<BLS12381Fr> {
  static constexpr uint32_t G = 7;
};

// g^(2^b) (or g^-(2^b)) for b <= NTT_MAX_LOG2, Montgomery, by value to the kernels
struct alignas(16) RecPows {
  uint32_t p[NTT_MAX_LOG2 + 1][8];
};

template <class FR>
struct RecConsts {
  RecPows fwd, inv;
  RecConsts() {
    uint32_t g[8] = {RecGen<FR>::G, 0, 0, 0, 0, 0, 0, 0}, gi[8];
    fr_host_mmul<FR>(g, FR::R2, g);
    fr_host_minv<FR>(g, gi);
    for (int b = 0; b <= NTT_MAX_LOG2; b++) {
      std::copy(g, g + 8, fwd.p[b]);
      std::copy(gi, gi + 8, inv.p[b]);
      fr_host_mmul<FR>(g, g, g);
      fr_host_mmul<FR>(gi, gi, gi);
    }
  }
};

KZGX_DEV uint32_t rec_brev(uint32_t x, uint32_t bits) { return bits ? __brev(x) >> (32 - bits) : 0u; }

// the coset and the offset inside its cell of position e of a size-D array in the
// caller's evaluation order: bit-reversed, chunk p = e >> kl is coset brev_R(p) and
// the cell's values lie as they come; natural, e = i + R j
KZGX_DEV void rec_split(uint32_t e, uint32_t kR, uint32_t kl, uint32_t bitrev, uint32_t* i, uint32_t* q) {
  if (bitrev) {
    *i = rec_brev(e >> kl, kR);
    *q = e & ((1u << kl) - 1);
  } else {
    *i = e & ((1u << kR) - 1);
    *q = e >> kR;
  }
}

// aux (zeroed before): slot[cb][R] | cnt[cb] | bad[cb] | gbad
__global__ __launch_bounds__(256) void k_rec_map(const uint32_t* __restrict__ blob_index,
                                                 const uint32_t* __restrict__ cell_index, uint32_t count,
                                                 uint32_t n_blobs, uint32_t b0, uint32_t cb, uint32_t kR,
                                                 uint32_t bitrev, uint32_t* __restrict__ slot,
                                                 uint32_t* __restrict__ cnt, uint32_t* __restrict__ bad,
                                                 uint32_t* __restrict__ gbad) {
  for (uint32_t k = blockIdx.x * 256 + threadIdx.x; k < count; k += gridDim.x * 256) {
    const uint32_t bg = blob_index[k];
    if (bg >= n_blobs) {
      atomicOr(gbad, 1u);
      continue;
    }
    if (bg < b0 || bg - b0 >= cb) continue;  // another chunk's
    const uint32_t b = bg - b0, p = cell_index[k];
    if (p >> kR) {
      atomicOr(bad + b, 1u);
      continue;
    }
    const uint32_t i = bitrev ? rec_brev(p, kR) : p;
    if (atomicCAS(slot + ((size_t)b << kR) + i, 0u, k + 1) != 0u)
      atomicOr(bad + b, 1u);
    else
      atomicAdd(cnt + b, 1u);
  }
}

constexpr uint32_t REC_TILE = 512;  // 16 KiB of LDS

template <class FR>
__global__ __launch_bounds__(256) void k_rec_locator(const uint32_t* __restrict__ slot,
                                                     const uint32_t* __restrict__ cnt,
                                                     const uint32_t* __restrict__ bad,
                                                     const uint32_t* __restrict__ gbad, uint32_t kR, RecPows pw,
                                                     uint32_t kl, const uint32_t* __restrict__ table, uint32_t K,
                                                     uint32_t* __restrict__ zs, uint32_t* __restrict__ izs,
                                                     uint32_t* __restrict__ gate) {
  constexpr int N = FR::N;
  // the roots w_R^i of the missing cosets, REC_TILE cosets at a time, gathered once per
  // workgroup (in any order: the products are exact) so that the lanes' loop reads LDS,
  // not one dependent global load per coset
  __shared__ uint32_t roots[REC_TILE * N];
  __shared__ uint32_t nroots;
  const uint32_t R = 1u << kR, b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p == 0) gate[b] = (cnt[b] >= R / 2 && !bad[b] && !*gbad) ? 1u : 0u;
  const bool live = p < R;
  const uint32_t* sl = slot + ((size_t)b << kR);
  const Fe<FR> x = ntt_tw<FR>(table, K, kR, live ? p : 0u, false);  // w_R^p
  const Fe<FR> xs = fe_mul<FR>(x, fe_const<FR>(pw.p[kl]));          // g^l w_R^p
  Fe<FR> a = fe_one<FR>(), c = fe_one<FR>();
  for (uint32_t base = 0; base < R; base += REC_TILE) {
    if (threadIdx.x == 0) nroots = 0;
    __syncthreads();
    for (uint32_t i = base + threadIdx.x; i < R && i < base + REC_TILE; i += 256)
      if (!sl[i]) fe_store<FR>(roots + atomicAdd(&nroots, 1u) * N, ntt_tw<FR>(table, K, kR, i, false));
    __syncthreads();
    const uint32_t m = nroots;  // <= REC_TILE
    for (uint32_t t = 0; t < m; t++) {
      const Fe<FR> wi = fe_load<FR>(roots + t * N);
      a = fe_mul<FR>(a, fe_sub<FR>(x, wi));
      c = fe_mul<FR>(c, fe_sub<FR>(xs, wi));
    }
    __syncthreads();
  }
  if (!live) return;
  fe_store<FR>(zs + (((size_t)b << kR) + p) * N, a);
  fe_store<FR>(izs + (((size_t)b << kR) + p) * N, fe_inv<FR>(c));  // c != 0: g^D != 1
}

template <class FR>
__global__ __launch_bounds__(256) void k_rec_mask(const uint32_t* __restrict__ ys,
                                                  const uint32_t* __restrict__ slot,
                                                  const uint32_t* __restrict__ zs, uint32_t kR, uint32_t kl,
                                                  uint32_t bitrev, uint32_t total, uint32_t* __restrict__ W) {
  constexpr int N = FR::N;
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const uint32_t kD = kR + kl, b = t >> kD;
  uint32_t i, q;
  rec_split(t & ((1u << kD) - 1), kR, kl, bitrev, &i, &q);
  const size_t c = ((size_t)b << kR) + i;
  const uint32_t s = slot[c];
  Fe<FR> v = fe_zero<FR>();
  if (s) v = fe_mul<FR>(fe_load<FR>(ys + ((((size_t)s - 1) << kl) + q) * N), fe_load<FR>(zs + c * N));
  fe_store<FR>(W + (size_t)t * N, v);
}

// W[b][j] *= g^(+-j) for the blobs b = blockIdx.y, + gridDim.y, ... < cb; TRUNC: only
// below n = D / 2 (also written to coef, packed, when given), zero above
template <class FR, bool TRUNC>
__global__ __launch_bounds__(256) void k_rec_shift(uint32_t* __restrict__ W, uint32_t kD, uint32_t cb, RecPows pw,
                                                   uint32_t* __restrict__ coef) {
  constexpr int N = FR::N;
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >> kD) return;
  const bool low = !TRUNC || j < (1u << (kD - 1));
  Fe<FR> gj = fe_one<FR>();
  if (low)
    for (uint32_t t = 0; t < kD; t++)
      if ((j >> t) & 1u) gj = fe_mul<FR>(gj, fe_const<FR>(pw.p[t]));
  for (uint32_t b = blockIdx.y; b < cb; b += gridDim.y) {
    uint32_t* w = W + (((size_t)b << kD) + j) * N;
    const Fe<FR> v = low ? fe_mul<FR>(fe_load<FR>(w), gj) : fe_zero<FR>();
    fe_store<FR>(w, v);
    if (TRUNC && low && coef) fe_store<FR>(coef + (((size_t)b << (kD - 1)) + j) * N, v);
  }
}

// position x of the bit-reversed array holds the value at g w^e, e = brev_D(x):
// e mod R = brev_R(x >> kl)
template <class FR>
__global__ __launch_bounds__(256) void k_rec_scale(uint32_t* __restrict__ W, const uint32_t* __restrict__ izs,
                                                   uint32_t kR, uint32_t kl, uint32_t total) {
  constexpr int N = FR::N;
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const uint32_t kD = kR + kl, b = t >> kD, i = rec_brev((t & ((1u << kD) - 1)) >> kl, kR);
  uint32_t* w = W + (size_t)t * N;
  fe_store<FR>(w, fe_mul<FR>(fe_load<FR>(w), fe_load<FR>(izs + (((size_t)b << kR) + i) * N)));
}

template <class FR>
__global__ __launch_bounds__(256) void k_rec_check(const uint32_t* __restrict__ W, const uint32_t* __restrict__ ys,
                                                   const uint32_t* __restrict__ slot, uint32_t kR, uint32_t kl,
                                                   uint32_t bitrev, uint32_t total, uint32_t* __restrict__ gate) {
  constexpr int N = FR::N;
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const uint32_t kD = kR + kl, b = t >> kD;
  uint32_t i, q;
  rec_split(t & ((1u << kD) - 1), kR, kl, bitrev, &i, &q);
  const uint32_t s = slot[((size_t)b << kR) + i];
  if (!s) return;
  if (!fe_eq<FR>(fe_load<FR>(W + (size_t)t * N), fe_load<FR>(ys + ((((size_t)s - 1) << kl) + q) * N)))
    atomicAnd(gate + b, 0u);
}

// out_y[b][o]: bit-reversed, the array as it lies; natural, coset order: o = i l + j
// is the value at w^(i + R j).  out_y / coef may be null
template <class FR>
__global__ __launch_bounds__(256) void k_rec_finish(const uint32_t* __restrict__ W, const uint32_t* __restrict__ gate,
                                                    uint32_t kR, uint32_t kl, uint32_t bitrev, uint32_t total,
                                                    uint32_t* __restrict__ out_y, uint32_t* __restrict__ coef,
                                                    uint32_t* __restrict__ ok) {
  constexpr int N = FR::N;
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const uint32_t kD = kR + kl, b = t >> kD, o = t & ((1u << kD) - 1);
  const bool good = gate[b] != 0;
  if (o == 0) ok[b] = good ? 1u : 0u;
  if (out_y) {
    const uint32_t src = bitrev ? o : (o >> kl) + ((o & ((1u << kl) - 1)) << kR);
    fe_store<FR>(out_y + (size_t)t * N, good ? fe_load<FR>(W + (((size_t)b << kD) + src) * N) : fe_zero<FR>());
  }
  if (coef && !good && o < (1u << (kD - 1))) fe_store<FR>(coef + (((size_t)b << (kD - 1)) + o) * N, fe_zero<FR>());
}

template <class FR>
static int recover_impl(Ctx* ctx, MsmWs& ws, const uint32_t* d_blob_index, const uint32_t* d_cell_index,
                        const uint32_t* d_ys, size_t count, size_t n_blobs, size_t b0, size_t cb, unsigned kn,
                        unsigned kl, bool bitrev, bool want_coef, uint32_t* d_out_y, uint32_t* d_out_coeffs,
                        uint32_t* d_ok, hipStream_t st) {
  constexpr int N = FR::N;
  static const RecConsts<FR> consts;
  const unsigned kD = kn + 1, kR = kD - kl;
  const size_t D = (size_t)1 << kD, R = (size_t)1 << kR, n = D / 2;
  const uint32_t total = (uint32_t)(cb * D), blocks = (total + 255) / 256, br = bitrev ? 1u : 0u;
  // zs | izs | slot | cnt | bad | gbad | gate
  const size_t fe_words = 2 * cb * R * N, map_words = cb * R + 2 * cb + 1;
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.rec_aux, (fe_words + map_words + cb) * sizeof(uint32_t), &ws.rec_aux_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.rec_w, cb * D * N * sizeof(uint32_t), &ws.rec_w_b));
  uint32_t* coef = d_out_coeffs;
  if (!coef && want_coef) {
    KZGX_TRY(dev_alloc(ctx, (void**)&ws.rec_coef, cb * n * N * sizeof(uint32_t), &ws.rec_coef_b));
    coef = ws.rec_coef;
  }
  uint32_t* zs = ws.rec_aux;
  uint32_t* izs = zs + cb * R * N;
  uint32_t* slot = izs + cb * R * N;
  uint32_t* cnt = slot + cb * R;
  uint32_t* bad = cnt + cb;
  uint32_t* gbad = bad + cb;
  uint32_t* gate = gbad + 1;
  uint32_t* W = ws.rec_w;
  KZGX_TRY(ntt_twiddles(ctx, kD, st));
  const uint32_t K = (uint32_t)ctx->ntt_log2;
  {
    ProfScope p(ctx, st, "rec_locator");
    KZGX_TRY_HIP(hipMemsetAsync(slot, 0, map_words * sizeof(uint32_t), st));
    if (count)
      hipLaunchKernelGGL(k_rec_map, dim3((unsigned)std::min<size_t>((count + 255) / 256, 1024)), dim3(256), 0, st,
                         d_blob_index, d_cell_index, (uint32_t)count, (uint32_t)n_blobs, (uint32_t)b0, (uint32_t)cb,
                         kR, br, slot, cnt, bad, gbad);
    hipLaunchKernelGGL(k_rec_locator<FR>, dim3((unsigned)((R + 255) / 256), (unsigned)cb), dim3(256), 0, st, slot,
                       cnt, bad, gbad, kR, consts.fwd, kl, ctx->d_ntt_tw, K, zs, izs, gate);
    KZGX_TRY_HIP(hipGetLastError());
  }
  // a blob of the chunk per y row up to 16 rows: the lanes of a row reuse their power of g
  const dim3 sgrid((unsigned)((D + 255) / 256), (unsigned)std::min<size_t>(cb, 16));
  {
    ProfScope p(ctx, st, "rec_mask");
    hipLaunchKernelGGL(k_rec_mask<FR>, dim3(blocks), dim3(256), 0, st, d_ys, slot, zs, kR, kl, br, total, W);
    KZGX_TRY_HIP(hipGetLastError());
  }
  KZGX_TRY(ntt(ctx, W, D, W, D, kD, cb, true, bitrev, st));
  {
    ProfScope p(ctx, st, "rec_shift");
    hipLaunchKernelGGL((k_rec_shift<FR, false>), sgrid, dim3(256), 0, st, W, kD, (uint32_t)cb, consts.fwd,
                       (uint32_t*)nullptr);
    KZGX_TRY_HIP(hipGetLastError());
  }
  KZGX_TRY(ntt(ctx, W, D, W, D, kD, cb, false, true, st));
  {
    ProfScope p(ctx, st, "rec_scale");
    hipLaunchKernelGGL(k_rec_scale<FR>, dim3(blocks), dim3(256), 0, st, W, izs, kR, kl, total);
    KZGX_TRY_HIP(hipGetLastError());
  }
  KZGX_TRY(ntt(ctx, W, D, W, D, kD, cb, true, true, st));
  {
    ProfScope p(ctx, st, "rec_unshift");
    hipLaunchKernelGGL((k_rec_shift<FR, true>), sgrid, dim3(256), 0, st, W, kD, (uint32_t)cb, consts.inv, coef);
    KZGX_TRY_HIP(hipGetLastError());
  }
  KZGX_TRY(ntt(ctx, W, D, W, D, kD, cb, false, bitrev, st));
  {
    ProfScope p(ctx, st, "rec_finish");
    if (count)
      hipLaunchKernelGGL(k_rec_check<FR>, dim3(blocks), dim3(256), 0, st, W, d_ys, slot, kR, kl, br, total, gate);
    hipLaunchKernelGGL(k_rec_finish<FR>, dim3(blocks), dim3(256), 0, st, W, gate, kR, kl, br, total, d_out_y, coef,
                       d_ok);
    KZGX_TRY_HIP(hipGetLastError());
  }
  return KZGX_OK;
}

int recover_cells(Ctx* ctx, MsmWs& ws, const uint32_t* d_blob_index, const uint32_t* d_cell_index,
                  const uint32_t* d_ys, size_t count, size_t n_blobs, size_t b0, size_t cb, unsigned log2n,
                  unsigned log2l, bool bitrev, bool want_coef, uint32_t* d_out_y, uint32_t* d_out_coeffs,
                  uint32_t* d_ok, hipStream_t st) {
  const unsigned kD = log2n + 1;
  // every index of a chunk is counted in 32 bits; cell numbers are stored plus one
  if (cb == 0 || log2l > log2n || (int)kD > ntt_max_log2(ctx->curve) || kD - log2l > KZGX_RECOVER_MAX_LOG2_CELLS ||
      (cb << kD) > std::max<size_t>(RECOVER_CHUNK_SCALARS, (size_t)1 << kD) || count > 0xfffffffeu ||
      n_blobs > 0xffffffffu || b0 + cb > n_blobs)
    return KZGX_ERR_ARG;
  return ctx->curve == KZGX_CURVE_BN254
             ? recover_impl<BN254Fr>(ctx, ws, d_blob_index, d_cell_index, d_ys, count, n_blobs, b0, cb, log2n, log2l,
                                     bitrev, want_coef, d_out_y, d_out_coeffs, d_ok, st)
             : recover_impl<BLS12381Fr>(ctx, ws, d_blob_index, d_cell_index, d_ys, count, n_blobs, b0, cb, log2n,
                                        log2l, bitrev, want_coef, d_out_y, d_out_coeffs, d_ok, st);
}

}  // namespace kzgx
