// Batched radix-2 number-theoretic transform over the scalar field (Fr) for
// gfx950: the bridge between a polynomial's values on a power-of-two domain
// of roots of unity and its monomial coefficients (DESIGN.md "Evaluation form
// and the Fr NTT").
//
//   forward: out[i] = sum_j in[j] w^(i j)           w = FrNtt::ROOT[log2 n]
//   inverse: out[j] = n^-1 sum_i in[i] w^(-i j)
//
// The coefficient side is in natural order; with bitrev the evaluation side
// (forward output, inverse input) is indexed by the bit reversal of i.
//
// One kernel, k_ntt, does all the work on a tile of T = 2^LOGT scalars held in
// LDS: it loads the tile once, runs every butterfly stage of the tile's
// transforms between barriers (decimation in frequency: natural order in,
// bit-reversed order out, undone by the index map of the store), and stores
// the tile once.  Three tile shapes:
//   WHOLE  n <= T: the tile holds T / n whole transforms of consecutive batch
//          entries (one read and one write of the data in all);
//   COLS   n = n1 n2 > T, first pass: T / n1 adjacent columns (stride n2) of
//          one transform, each a length-n1 transform, times the inter-pass
//          twiddle w^(j2 i1), written to the workspace in place;
//   ROWS   second pass: T / n2 adjacent rows of the workspace, each a
//          length-n2 transform, stored transposed (natural order) or row by
//          row (bit-reversed order).
// with X[i1 + n1 i2] = sum_j2 w_n2^(j2 i2) [w^(j2 i1) sum_j1 x[j1 n2 + j2] w_n1^(j1 i1)].
//
// Scalars are canonical in and out; twiddles and n^-1 are Montgomery values,
// so fe_mul(canonical, Montgomery) is canonical and no conversion pass runs
// (the same trick as poly.hip).  The twiddle table w^j, j <= N / 2, is built
// on the device from the N-th root's squarings (curve_consts.h) on first use.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "field.hpp"
#include "kzgx_internal.hpp"

namespace kzgx {

template <class FR>
struct NttOf;
template <>
struct NttOf<BN254Fr> {
  using T = BN254FrNtt;
};
template <>
struct NttOf<BLS12381Fr> {
  using T = BLS12381FrNtt;
};

// w_k (Montgomery) for k = 0..NTT_MAX_LOG2, by value to the table kernel
struct alignas(16) NttRoots {
  uint32_t r[NTT_MAX_LOG2 + 1][8];
};
struct alignas(16) NttScale {
  uint32_t v[8];  // n^-1, Montgomery
};

KZGX_DEV uint32_t ntt_brev(uint32_t x, uint32_t bits) { return bits ? __brev(x) >> (32 - bits) : 0u; }

// LDS image of tile element a: the low three bits of the element index (the
// 8 x 32 B that span the 64 banks) XORed with the three-bit groups above, so
// the power-of-two strides of the transposed and bit-reversed accesses spread
// over the banks while consecutive elements stay conflict-free
KZGX_DEV uint32_t ntt_phys(uint32_t a) { return a ^ (((a >> 3) ^ (a >> 6) ^ (a >> 9)) & 7u); }

// table[j] = w^j for j <= half (w of order 2 half; table[half] = -1): the
// product of the root's squarings picked by the bits of j
template <class FR>
__global__ __launch_bounds__(256) void k_ntt_twiddles(NttRoots roots, uint32_t K, uint32_t half,
                                                      uint32_t* __restrict__ table) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j > half) return;
  Fe<FR> acc = fe_one<FR>();
  for (uint32_t b = 0; b < K; b++)
    if ((j >> b) & 1u) acc = fe_mul<FR>(acc, fe_const<FR>(roots.r[K - b]));  // w^(2^b) = w_(K-b)
  fe_store<FR>(table + (size_t)j * FR::N, acc);
}

// (ntt_tw, the table lookup w_m^(+-e), is in field.hpp: poly.hip's cell fold reads the table too)

enum NttMode : uint32_t { NTT_WHOLE = 0, NTT_COLS = 1, NTT_ROWS = 2 };

struct NttArgs {
  const uint32_t* in;
  uint32_t* out;
  size_t in_stride, out_stride;  // scalars between consecutive transforms
  const uint32_t* table;
  uint32_t K;       // table of the 2^K-th root
  uint32_t mode;
  uint32_t k;       // log2 n
  uint32_t k1, k2;  // COLS / ROWS: n = 2^k1 columns-length x 2^k2 row-length
  uint32_t batch;
  uint32_t inverse, in_brev, out_brev, scale;
  NttScale ninv;
};

template <class FR, int LOGT>
__global__ __launch_bounds__((1 << LOGT) / 4) void k_ntt(NttArgs A) {
  constexpr int N = FR::N;
  constexpr uint32_t T = 1u << LOGT, NT = T / 4;
  __shared__ uint32_t sh[T * N];
  const uint32_t tid = threadIdx.x;
  const bool inverse = A.inverse != 0;
  // lm: log2 of the transforms in this tile; g: batch entry; sub: tile within it
  uint32_t lm, g, sub;
  if (A.mode == NTT_WHOLE) {
    lm = A.k;
    g = blockIdx.x << (LOGT - A.k);  // first of the tile's T / n entries
    sub = 0;
  } else {
    lm = A.mode == NTT_COLS ? A.k1 : A.k2;
    const uint32_t ltpt = A.k - LOGT;  // tiles per transform
    g = blockIdx.x >> ltpt;
    sub = blockIdx.x & ((1u << ltpt) - 1);
  }
  const uint32_t n1 = 1u << A.k1, n2 = 1u << A.k2;

  // ---- load: consecutive threads read consecutive global scalars ----
  for (uint32_t e = tid; e < T; e += NT) {
    Fe<FR> v = fe_zero<FR>();
    uint32_t pos;
    if (A.mode == NTT_WHOLE) {
      const uint32_t t = e >> lm, q = e & ((1u << lm) - 1);
      pos = (t << lm) | (A.in_brev ? ntt_brev(q, lm) : q);
      if (g + t < A.batch) v = fe_load<FR>(A.in + ((size_t)(g + t) * A.in_stride + q) * N);
    } else if (A.mode == NTT_COLS) {
      const uint32_t lcw = LOGT - A.k1;  // columns per tile
      if (!A.in_brev) {
        const uint32_t t = e & ((1u << lcw) - 1), j1 = e >> lcw;
        pos = (t << A.k1) | j1;
        v = fe_load<FR>(A.in + ((size_t)g * A.in_stride + ((size_t)j1 << A.k2) + (sub << lcw) + t) * N);
      } else {  // x[j1 n2 + j2] lies at brev(j2) n1 + brev(j1): column j2 is a contiguous run
        const uint32_t q = e & (n1 - 1), t = e >> A.k1;
        const uint32_t row = ntt_brev((sub << lcw) + t, A.k2);
        pos = (t << A.k1) | ntt_brev(q, A.k1);
        v = fe_load<FR>(A.in + ((size_t)g * A.in_stride + ((size_t)row << A.k1) + q) * N);
      }
    } else {  // ROWS: T contiguous scalars of the workspace
      pos = e;
      v = fe_load<FR>(A.in + ((size_t)g * A.in_stride + ((size_t)sub << LOGT) + e) * N);
    }
    fe_store<FR>(sh + ntt_phys(pos) * N, v);
  }
  __syncthreads();

  // ---- decimation in frequency over the whole tile: natural in, bit-reversed out ----
  for (int lh = (int)lm - 1; lh >= 0; lh--) {
    const uint32_t half = 1u << lh;
    const uint32_t sh_tw = A.K - 1 - (uint32_t)lh;  // w_(2 half)^jj = table[jj << sh_tw]
    for (uint32_t bf = tid; bf < T / 2; bf += NT) {
      const uint32_t jj = bf & (half - 1), a = ((bf >> lh) << (lh + 1)) | jj;
      uint32_t* pa = sh + ntt_phys(a) * N;
      uint32_t* pb = sh + ntt_phys(a + half) * N;
      const Fe<FR> u = fe_load<FR>(pa), v = fe_load<FR>(pb);
      // inverse: w^-i = -w^(N/2 - i), and table[N/2] = -1 covers i = 0
      const uint32_t idx = jj << sh_tw;
      Fe<FR> w = fe_load<FR>(A.table + (size_t)(inverse ? (1u << (A.K - 1)) - idx : idx) * N);
      if (inverse) w = fe_neg<FR>(w);
      fe_store<FR>(pa, fe_add<FR>(u, v));
      fe_store<FR>(pb, fe_mul<FR>(fe_sub<FR>(u, v), w));  // canonical * Montgomery = canonical
    }
    __syncthreads();
  }

  // ---- store: consecutive threads write consecutive global scalars; result i of a
  // transform sits at tile position brev(i) ----
  const Fe<FR> ninv = fe_const<FR>(A.ninv.v);
  for (uint32_t e = tid; e < T; e += NT) {
    if (A.mode == NTT_WHOLE) {
      const uint32_t t = e >> lm, d = e & ((1u << lm) - 1);
      if (g + t >= A.batch) continue;
      Fe<FR> v = fe_load<FR>(sh + ntt_phys((t << lm) | (A.out_brev ? d : ntt_brev(d, lm))) * N);
      if (A.scale) v = fe_mul<FR>(v, ninv);
      fe_store<FR>(A.out + ((size_t)(g + t) * A.out_stride + d) * N, v);
    } else if (A.mode == NTT_COLS) {
      const uint32_t lcw = LOGT - A.k1;
      const uint32_t t = e & ((1u << lcw) - 1), i1 = e >> lcw, j2 = (sub << lcw) + t;
      Fe<FR> v = fe_load<FR>(sh + ntt_phys((t << A.k1) | ntt_brev(i1, A.k1)) * N);
      v = fe_mul<FR>(v, ntt_tw<FR>(A.table, A.K, A.k, j2 * i1, inverse));
      fe_store<FR>(A.out + ((size_t)g * A.out_stride + ((size_t)i1 << A.k2) + j2) * N, v);
    } else {
      const uint32_t lrw = LOGT - A.k2;  // rows per tile
      Fe<FR> v;
      size_t dst;
      if (!A.out_brev) {  // X[i1 + n1 i2]: the tile's rows are adjacent i1
        const uint32_t t = e & ((1u << lrw) - 1), i2 = e >> lrw;
        v = fe_load<FR>(sh + ntt_phys((t << A.k2) | ntt_brev(i2, A.k2)) * N);
        dst = ((size_t)i2 << A.k1) + (sub << lrw) + t;
      } else {  // brev(i1 + n1 i2) = brev(i1) n2 + brev(i2): a contiguous row as it lies in the tile
        const uint32_t t = e >> A.k2, d2 = e & (n2 - 1);
        v = fe_load<FR>(sh + ntt_phys(e) * N);
        dst = ((size_t)ntt_brev((sub << lrw) + t, A.k1) << A.k2) + d2;
      }
      if (A.scale) v = fe_mul<FR>(v, ninv);
      fe_store<FR>(A.out + ((size_t)g * A.out_stride + dst) * N, v);
    }
  }
}

// --------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------
template <class FR>
static int ntt_table_ensure(Ctx* ctx, uint32_t k, hipStream_t st) {
  using C = typename NttOf<FR>::T;
  constexpr uint32_t KMAX = C::TWO_ADICITY < NTT_MAX_LOG2 ? C::TWO_ADICITY : NTT_MAX_LOG2;
  if (ctx->ntt_log2 >= (int)k) {
    // built on another stream, perhaps: order this one behind the build
    KZGX_TRY_HIP(hipStreamWaitEvent(st, ctx->ntt_ev, 0));
    return KZGX_OK;
  }
  // at least the one-tile sizes at once (64 KiB), so the common sizes build once
  const uint32_t K = std::min(KMAX, std::max(k, (uint32_t)NTT_TILE_LOG2));
  const uint32_t half = 1u << (K - 1);
  if (!ctx->ntt_ev) KZGX_TRY_HIP(hipEventCreateWithFlags(&ctx->ntt_ev, hipEventDisableTiming));
  ctx->ntt_log2 = -1;
  // growing frees the smaller table behind a device synchronisation (dev_alloc)
  KZGX_TRY(dev_alloc(ctx, (void**)&ctx->d_ntt_tw, ((size_t)half + 1) * FR::N * sizeof(uint32_t), &ctx->ntt_tw_b));
  NttRoots roots;
  for (uint32_t i = 0; i <= (uint32_t)NTT_MAX_LOG2; i++)
    for (int w = 0; w < 8; w++) roots.r[i][w] = i <= KMAX ? C::ROOT_M[i][w] : 0u;
  hipLaunchKernelGGL(k_ntt_twiddles<FR>, dim3(half / 256 + 1), dim3(256), 0, st, roots, K, half, ctx->d_ntt_tw);
  KZGX_TRY_HIP(hipGetLastError());
  KZGX_TRY_HIP(hipEventRecord(ctx->ntt_ev, st));
  ctx->ntt_log2 = (int)K;
  return KZGX_OK;
}

template <class FR, int LOGT>
static void ntt_launch(const NttArgs& a, size_t blocks, hipStream_t st) {
  hipLaunchKernelGGL((k_ntt<FR, LOGT>), dim3((unsigned)blocks), dim3((1u << LOGT) / 4), 0, st, a);
}

template <class FR, bool BIG>
static int ntt_impl(Ctx* ctx, const uint32_t* d_in, size_t in_stride, uint32_t* d_out, size_t out_stride, uint32_t k,
                    size_t batch, bool inverse, bool bitrev, hipStream_t st) {
  using C = typename NttOf<FR>::T;
  constexpr int N = FR::N;
  if (batch == 0) return KZGX_OK;
  const size_t n = (size_t)1 << k;
  if (k == 0) {  // the identity
    if (d_in != d_out || in_stride != out_stride)
      KZGX_TRY_HIP(hipMemcpy2DAsync(d_out, out_stride * N * 4, d_in, in_stride * N * 4, N * 4, batch,
                                    hipMemcpyDeviceToDevice, st));
    return KZGX_OK;
  }
  KZGX_TRY(ntt_table_ensure<FR>(ctx, k, st));
  NttArgs a{};
  a.table = ctx->d_ntt_tw;
  a.K = (uint32_t)ctx->ntt_log2;
  a.k = k;
  a.batch = (uint32_t)batch;
  a.inverse = inverse;
  for (int w = 0; w < 8; w++) a.ninv.v[w] = C::NINV_M[k][w];
  if (k <= (uint32_t)NTT_TILE_LOG2) {
    a.mode = NTT_WHOLE;
    a.in = d_in;
    a.out = d_out;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.in_brev = inverse && bitrev;
    a.out_brev = !inverse && bitrev;
    a.scale = inverse;
    // small transforms in 32 KiB tiles of 256 threads (several workgroups per
    // CU), the two largest one-tile sizes in the 128 KiB tile
    if (!BIG || k <= (uint32_t)NTT_SMALL_TILE_LOG2) {
      const size_t per = (size_t)1 << (NTT_SMALL_TILE_LOG2 - k);
      ntt_launch<FR, NTT_SMALL_TILE_LOG2>(a, (batch + per - 1) / per, st);
    } else if constexpr (BIG) {
      const size_t per = (size_t)1 << (NTT_TILE_LOG2 - k);
      ntt_launch<FR, NTT_TILE_LOG2>(a, (batch + per - 1) / per, st);
    }
    KZGX_TRY_HIP(hipGetLastError());
    return KZGX_OK;
  }
  if constexpr (BIG) {
    // two passes through the stream's workspace (the second pass reads whole
    // rows and writes other tiles' rows, so it cannot run in place)
    WsLease ws = ctx->ws_for(st);
    if (!ws) return KZGX_ERR_ARG;
    KZGX_TRY(dev_alloc(ctx, (void**)&ws->ntt_tmp, batch * n * N * sizeof(uint32_t), &ws->ntt_tmp_b));
    const size_t blocks = batch << (k - NTT_TILE_LOG2);
    a.k1 = (k + 1) / 2;
    a.k2 = k - a.k1;
    a.mode = NTT_COLS;
    a.in = d_in;
    a.in_stride = in_stride;
    a.out = ws->ntt_tmp;
    a.out_stride = n;
    a.in_brev = inverse && bitrev;
    ntt_launch<FR, NTT_TILE_LOG2>(a, blocks, st);
    a.mode = NTT_ROWS;
    a.in = ws->ntt_tmp;
    a.in_stride = n;
    a.out = d_out;
    a.out_stride = out_stride;
    a.in_brev = 0;
    a.out_brev = !inverse && bitrev;
    a.scale = inverse;
    ntt_launch<FR, NTT_TILE_LOG2>(a, blocks, st);
    KZGX_TRY_HIP(hipGetLastError());
    return KZGX_OK;
  }
  return KZGX_ERR_ARG;
}

int ntt_max_log2(int curve) {
  if (curve == KZGX_CURVE_BN254) return std::min<int>(BN254FrNtt::TWO_ADICITY, NTT_MAX_LOG2);
  if (curve == KZGX_CURVE_BLS12381) return std::min<int>(BLS12381FrNtt::TWO_ADICITY, NTT_MAX_LOG2);
  return -1;
}

int ntt_twiddles(Ctx* ctx, unsigned log2n, hipStream_t st) {
  if ((int)log2n > ntt_max_log2(ctx->curve)) return KZGX_ERR_ARG;
  const uint32_t k = std::max(log2n, 1u);  // the table holds w^0 .. w^(N/2): N >= 2
  return ctx->curve == KZGX_CURVE_BN254 ? ntt_table_ensure<BN254Fr>(ctx, k, st)
                                        : ntt_table_ensure<BLS12381Fr>(ctx, k, st);
}

int ntt(Ctx* ctx, const uint32_t* d_in, size_t in_stride, uint32_t* d_out, size_t out_stride, unsigned log2n,
        size_t batch, bool inverse, bool bitrev, hipStream_t st) {
  if ((int)log2n > ntt_max_log2(ctx->curve)) return KZGX_ERR_ARG;
  const size_t n = (size_t)1 << log2n;
  // tiles are counted in 32 bits, and so are the batch entries
  if (batch > 0xffffffffu || (batch * n) >> NTT_SMALL_TILE_LOG2 > 0x7fffffffu) return KZGX_ERR_ARG;
  return ctx->curve == KZGX_CURVE_BN254
             ? ntt_impl<BN254Fr, false>(ctx, d_in, in_stride, d_out, out_stride, log2n, batch, inverse, bitrev, st)
             : ntt_impl<BLS12381Fr, true>(ctx, d_in, in_stride, d_out, out_stride, log2n, batch, inverse, bitrev, st);
}

}  // namespace kzgx
