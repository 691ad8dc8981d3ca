// Batched Pippenger G1 MSM for gfx950 -- the hot path behind
// kzg::trusted_setup::create_commit / create_proof / verify_commit
// (reference: trusted_setup::polyeval_G1, src/trusted_setup.cpp:149-174,
// a naive per-term PAIR_G1mul + ECP_add loop).
//
// Design (MI355X-first):
//  * fixed-base windows: at SRS load every point P_i is expanded into W
//    window copies T[w][i] = 2^(c w) P_i (affine, Montgomery, HBM resident),
//    so all windows of an MSM share ONE set of 2^(c-1) signed-digit buckets and
//    there is no per-window doubling chain;
//  * per MSM b: signed c-bit digits -> (point, sign) entries counting-sorted by
//    bucket: per-block LDS histograms, a 2-D scan into bucket offsets and
//    per-block write bases, and a scatter ranked by LDS atomics alone (no
//    global atomics anywhere in the sort);
//  * bucket accumulation is load balanced: every thread owns exactly K
//    consecutive sorted entries and does K mixed XYZZ additions; partials of
//    buckets that cross segment boundaries are staged in LDS and merged
//    inside the workgroup, only workgroup-crossing buckets go through HBM;
//  * the bucket running sum sum_k (k+1) B_k: per-thread running sums over
//    J = 8 buckets, then one wavefront per MSM folds the (R, T) pairs with a
//    __shfl_down suffix scan and a shuffle-tree reduction; a thread per MSM
//    converts to affine.
// Every step is an exact group operation, so the affine output is bit-exact
// with any other correct evaluation of sum c_i [tau^i]G1.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <optional>

#include "curve.hpp"
#include "msm_merge.hpp"
#include "kzgx_internal.hpp"
#include "kzgx_setup.hpp"

namespace kzgx {

// --------------------------------------------------------------------------
// SRS upload / fixed-base table
// --------------------------------------------------------------------------
// canonical affine (x||y, 2N words per point) -> Montgomery into T[0];
// all-zero input marks infinity.
template <class C>
__global__ void k_srs_to_mont(const uint32_t* __restrict__ canon, uint32_t* __restrict__ table, uint8_t* __restrict__ inf,
                              uint32_t n) {
  constexpr int AW = affine_words<C>();
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Affine<C> a;
  const bool finite = affine_from_canonical<C>(canon + (size_t)i * 2 * C::Fp::N, a);
  inf[i] = finite ? 0 : 1;
  affine_store<C>(table + (size_t)i * AW, a);
}

// T[w][i] = 2^c T[w-1][i] for w = 1..W-1
template <class C>
__global__ void k_table_build(uint32_t* __restrict__ table, const uint8_t* __restrict__ inf, uint32_t n, int W, int c) {
  using F = typename C::Fp29;
  constexpr int AW = affine_words<C>();
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Affine<C> a = affine_load<C>(table + (size_t)i * AW);
  const bool is_inf = inf[i] != 0;
  for (int w = 1; w < W; w++) {
    if (!is_inf) {
      Xyzz<C> p = xyzz_from_affine<C>(a);
      for (int s = 0; s < c; s++) p = xyzz_dbl<C>(p);
      if (!xyzz_to_affine<C>(p, a)) {
        a.x = f29_zero<F>();
        a.y = f29_zero<F>();
      }
    }
    affine_store<C>(table + ((size_t)w * n + i) * AW, a);
  }
}

// the same table with a thread per (point, window): window w's c w
// doublings from T[0][i] run beside the other windows' instead of after
// them -- c W^2 / 2 doublings per point against c W, so only for small SRSs,
// where the sequential chain (c (W - 1) doublings and W - 1 inversions,
// ~2.4 ms whatever n) is the setup's latency (table_build launcher)
template <class C>
__global__ __launch_bounds__(256) void k_table_build_par(uint32_t* __restrict__ table, const uint8_t* __restrict__ inf,
                                                         uint32_t n, int W, int c) {
  using F = typename C::Fp29;
  constexpr int AW = affine_words<C>();
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (uint64_t)(W - 1) * n) return;
  const uint32_t w = 1 + (uint32_t)(g / n), i = (uint32_t)(g % n);
  Affine<C> a = affine_load<C>(table + (size_t)i * AW);
  if (!inf[i]) {
    Xyzz<C> p = xyzz_from_affine<C>(a);
    const int steps = c * (int)w;
    for (int s = 0; s < steps; s++) p = xyzz_dbl<C>(p);
    if (!xyzz_to_affine<C>(p, a)) {
      a.x = f29_zero<F>();
      a.y = f29_zero<F>();
    }
  }
  affine_store<C>(table + ((size_t)w * n + i) * AW, a);
}

template <class C>
static void table_build(uint32_t* table, const uint8_t* inf, size_t n, int W, int c, hipStream_t st) {
  if (W < 2) return;
  if ((uint64_t)(W - 1) * n <= (1u << 17))
    hipLaunchKernelGGL(k_table_build_par<C>, dim3((unsigned)(((uint64_t)(W - 1) * n + 255) / 256)), dim3(256), 0, st,
                       table, inf, (uint32_t)n, W, c);
  else
    hipLaunchKernelGGL(k_table_build<C>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, table, inf, (uint32_t)n,
                       W, c);
}

// --------------------------------------------------------------------------
// signed-digit recoding
// --------------------------------------------------------------------------
template <int CB>
struct Win {
  static constexpr int W = (257 + CB - 1) / CB;  // covers any 256-bit integer
  static constexpr uint32_t NB = 1u << (CB - 1);
};

// digit w of the scalar (8 canonical LE words); returns signed digit, updates carry
template <int CB>
KZGX_DEV int digit_at(const uint32_t (&s)[8], int w, uint32_t& carry) {
  const int bit = CB * w;
  const int word = bit >> 5;
  const int sh = bit & 31;
  uint32_t raw = 0;
  if (word < 8) {
    raw = s[word] >> sh;
    if (sh + CB > 32 && word + 1 < 8) raw |= s[word + 1] << (32 - sh);
  }
  raw &= (1u << CB) - 1u;
  raw += carry;
  if (raw > Win<CB>::NB) {
    carry = 1;
    return (int)raw - (1 << CB);
  }
  carry = 0;
  return (int)raw;
}

KZGX_DEV void load_scalar(const uint32_t* p, uint32_t (&s)[8]) {
  uint4 a = reinterpret_cast<const uint4*>(p)[0];
  uint4 b = reinterpret_cast<const uint4*>(p)[1];
  s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w;
  s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
}

// Scalars are recoded per (bucket set, count block) of consecutive points.
// Each count block keeps its own bucket histogram, so the sort needs no
// global atomics: the scan turns the histograms into bucket offsets and
// per-block write bases, and the scatter ranks entries with LDS atomics only.
#ifndef KZGX_SORT_SPT
#define KZGX_SORT_SPT 2
#endif
constexpr uint32_t SORT_SPT = KZGX_SORT_SPT;  // scalars per thread in count / scatter
constexpr uint32_t SORT_BLK = 256 * SORT_SPT;  // scalars per count block

// The three sort kernels serve every batched Pippenger.  What a bucket set
// (blockIdx.y) sorts is its digit source, a small struct passed by value:
//   SPT                  points per thread, so 256 SPT points per count block;
//   digits_per_point(W)  entries a point can add to one bucket set (sizes the
//                        scatter's LDS stage);
//   entries_base(b)      the first entry word of bucket set b;
//   digits<CB>(.., b, i, emit)   emit(d, row) for every non-zero signed digit
//                        d of point i that belongs to bucket set b; row is
//                        the digit's table row, the entry is row | sign << 31.
// SrsSrc (msm_batch_impl): bucket set b is MSM b, every scalar adds all its W
// digits, the rows are those of a window table over the SRS.  PointSrc
// (msm_points_impl, with the variable-base section below) adds one digit.
struct SrsSrc {
  static constexpr uint32_t SPT = SORT_SPT;
  static constexpr uint32_t digits_per_point(int W) { return (uint32_t)W; }
  size_t stride_words;                // between the scalars of consecutive MSMs
  uint32_t point_base, point_stride;  // scalar i of MSM b multiplies SRS point point_base + b point_stride + i
  uint32_t n_rows;                    // points per window of the table
  size_t emax;
  KZGX_DEV size_t entries_base(uint32_t b) const { return b * emax; }
  template <int CB, class F>
  KZGX_DEV void digits(const uint32_t* __restrict__ scalars, const uint8_t* __restrict__ inf, uint32_t n, uint32_t b,
                       uint32_t i, F emit) const {
    const uint32_t ig = point_base + b * point_stride + i;  // SRS index of this scalar
    if (i < n && !inf[ig]) {
      uint32_t s[8];
      load_scalar(scalars + b * stride_words + (size_t)i * 8, s);
      uint32_t carry = 0;
#pragma unroll
      for (int w = 0; w < Win<CB>::W; w++) {
        const int d = digit_at<CB>(s, w, carry);
        if (d != 0) emit(d, (uint32_t)w * n_rows + ig);
      }
    }
  }
};

KZGX_DEV uint32_t digit_bucket(int d) { return (uint32_t)((d < 0 ? -d : d) - 1); }

// NB counters and the 256 threads of a block: dst[k] = src[k]
template <uint32_t NB>
KZGX_DEV void counters_copy(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src) {
  for (uint32_t k = threadIdx.x; k < NB; k += 256) dst[k] = src[k];
}

// Exclusive scan of NB LDS counters by the 256 threads of a block:
// excl[k] = sum of cnt[k' < k] (excl may be cnt).  Thread t reads and writes
// counters [t PER, t PER + PER) only, so it may have filled them itself just
// before; it returns the sum through its last counter (thread 255: the
// total).  part: 256 words of LDS.  No barrier after the last write.
template <uint32_t NB>
KZGX_DEV uint32_t counters_scan(const uint32_t* cnt, uint32_t* excl, uint32_t* part) {
  constexpr uint32_t PER = NB / 256;  // NB is a multiple of 256 (c >= 9)
  const uint32_t t = threadIdx.x;
  uint32_t local = 0;
#pragma unroll
  for (uint32_t j = 0; j < PER; j++) local += cnt[t * PER + j];
  part[t] = local;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {
    uint32_t v = (t >= d) ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t run = part[t] - local;  // exclusive prefix of this thread's counters
#pragma unroll
  for (uint32_t j = 0; j < PER; j++) {
    const uint32_t c = cnt[t * PER + j];
    excl[t * PER + j] = run;
    run += c;
  }
  return run;
}

// pass 1: bucket histogram of every (bucket set, count block), written in full
template <int CB, class Src>
__global__ __launch_bounds__(256) void k_msm_count(Src src, const uint32_t* __restrict__ scalars, uint32_t n,
                                                   const uint8_t* __restrict__ inf, uint32_t* __restrict__ bcount,
                                                   uint32_t nblk) {
  constexpr uint32_t NB = Win<CB>::NB;
  __shared__ uint32_t hist[NB];
  const uint32_t b = blockIdx.y;
  for (uint32_t k = threadIdx.x; k < NB; k += 256) hist[k] = 0;
  __syncthreads();
#pragma unroll 1
  for (uint32_t j = 0; j < Src::SPT; j++) {
    const uint32_t i = blockIdx.x * (256 * Src::SPT) + j * 256 + threadIdx.x;
    src.template digits<CB>(scalars, inf, n, b, i, [&](int d, uint32_t) { atomicAdd(&hist[digit_bucket(d)], 1u); });
  }
  __syncthreads();
  counters_copy<NB>(bcount + ((size_t)b * nblk + blockIdx.x) * NB, hist);
}

// pass 2, one workgroup per bucket set: bucket totals over the count blocks, an
// exclusive scan -> offsets[b][0..NB], and the write base of every
// (count block, bucket): bbase[b][blk][k] = offsets[k] + sum_{blk' < blk} count
template <int CB>
__global__ __launch_bounds__(256) void k_msm_scan(const uint32_t* __restrict__ bcount, uint32_t nblk,
                                                  uint32_t* __restrict__ offsets, uint32_t* __restrict__ bbase) {
  constexpr uint32_t NB = Win<CB>::NB;
  __shared__ uint32_t tot[NB];
  __shared__ uint32_t part[256];
  const uint32_t b = blockIdx.x;
  const uint32_t t = threadIdx.x;
  const uint32_t* bc = bcount + (size_t)b * nblk * NB;
  for (uint32_t k = t; k < NB; k += 256) {  // coalesced over k
    uint32_t s = 0;
    for (uint32_t blk = 0; blk < nblk; blk++) s += bc[(size_t)blk * NB + k];
    tot[k] = s;
  }
  __syncthreads();
  const uint32_t run = counters_scan<NB>(tot, tot, part);
  uint32_t* off = offsets + (size_t)b * (NB + 1);
  if (t == 255) off[NB] = run;
  __syncthreads();
  uint32_t* bb = bbase + (size_t)b * nblk * NB;
  for (uint32_t k = t; k < NB; k += 256) {
    uint32_t base = tot[k];
    off[k] = base;
    for (uint32_t blk = 0; blk < nblk; blk++) {
      bb[(size_t)blk * NB + k] = base;
      base += bc[(size_t)blk * NB + k];
    }
  }
}

// pass 3: scatter (table index | sign) entries into bucket order.  The block
// first sorts its own entries in LDS (local offsets from its histogram,
// ranks from LDS atomics), then writes them out in that order: lanes of a
// wavefront write consecutive positions of one bucket's run, so the stores
// coalesce instead of landing as scattered 4-byte writes.  No global atomics.
//
// The write-out: the block's lstart[NB] staged entries, bucket k's at
// stage[lstart[k] .. lstart[k + 1]), go to out[gbase[k] ..]
template <uint32_t NB>
KZGX_DEV void write_runs(const uint32_t* stage, const uint32_t* lstart, const uint32_t* gbase,
                         uint32_t* __restrict__ out) {
  const uint32_t total = lstart[NB];
  for (uint32_t j = threadIdx.x; j < total; j += 256) {
    uint32_t lo = 0, hi = NB;  // bucket of position j: lstart[lo] <= j < lstart[hi]
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (lstart[mid] <= j)
        lo = mid;
      else
        hi = mid;
    }
    out[gbase[lo] + (j - lstart[lo])] = stage[j];
  }
}

template <int CB, class Src>
__global__ __launch_bounds__(256) void k_msm_scatter(Src src, const uint32_t* __restrict__ scalars, uint32_t n,
                                                     const uint8_t* __restrict__ inf,
                                                     const uint32_t* __restrict__ bcount,
                                                     const uint32_t* __restrict__ bbase, uint32_t nblk,
                                                     uint32_t* __restrict__ entries) {
  constexpr uint32_t NB = Win<CB>::NB;
  constexpr uint32_t PER = NB / 256;
  __shared__ uint32_t stage[256 * Src::SPT * Src::digits_per_point(Win<CB>::W)];
  __shared__ uint32_t lstart[NB + 1];
  __shared__ uint32_t cur[NB];
  __shared__ uint32_t part[256];
  const uint32_t b = blockIdx.y;
  const uint32_t t = threadIdx.x;
  const size_t hb = ((size_t)b * nblk + blockIdx.x) * NB;
  // local exclusive scan of this block's histogram: the buckets' starts in
  // the stage, and the cursors the ranking advances from them
#pragma unroll
  for (uint32_t j = 0; j < PER; j++) cur[t * PER + j] = bcount[hb + t * PER + j];
  const uint32_t run = counters_scan<NB>(cur, lstart, part);
#pragma unroll
  for (uint32_t j = 0; j < PER; j++) cur[t * PER + j] = lstart[t * PER + j];
  if (t == 255) lstart[NB] = run;
  __syncthreads();
  // rank every digit into the block's LDS stage (pos < lstart[NB], the block's count of digits)
#pragma unroll 1
  for (uint32_t j = 0; j < Src::SPT; j++) {
    const uint32_t i = blockIdx.x * (256 * Src::SPT) + j * 256 + t;
    src.template digits<CB>(scalars, inf, n, b, i, [&](int d, uint32_t row) {
      const uint32_t pos = atomicAdd(&cur[digit_bucket(d)], 1u);
      stage[pos] = row | (d < 0 ? 0x80000000u : 0u);
    });
  }
  __syncthreads();
  counters_copy<NB>(cur, bbase + hb);  // global write bases
  __syncthreads();
  write_runs<NB>(stage, lstart, cur, entries + src.entries_base(b));
}

// pass 4: balanced bucket accumulation.  Thread s of an MSM owns the K
// consecutive sorted entries [s K, s K + K) and runs K mixed XYZZ additions
// from the L2-resident window table (the entry and table point of the next
// term in flight underneath).  Buckets that start and end inside the segment
// are written straight to bsum.  The partial of the bucket already open at the
// segment start (its "head", sstate HEAD; SPANS if that bucket also runs past
// the segment) and of a bucket that starts inside the segment and runs past
// its end (its "tail", tailk = bucket) go to per-segment slots for pass 4b.
// Keeping the merges out of this loop keeps it at 4 waves per SIMD.
// NO_TAIL, ACC_WG, HEAD, SPANS: msm_merge.hpp

// waves per SIMD the accumulation kernel is register-budgeted for (the
// 14-limb BLS12-381 field spills at 3)
template <class C>
constexpr int pip_accum_waves() {
  return C::Fp29::L <= 9 ? KZGX_ACCUM_WAVES : 2;
}

template <class C>
__global__ __launch_bounds__(256, pip_accum_waves<C>()) void k_msm_accum(
    const uint32_t* __restrict__ entries, size_t emax, const uint32_t* __restrict__ offsets, uint32_t nb,
    const uint32_t* __restrict__ table, uint32_t K, uint32_t smax, uint32_t* __restrict__ bsum,
    uint32_t* __restrict__ heads, uint32_t* __restrict__ tails, uint32_t* __restrict__ tailk,
    uint8_t* __restrict__ sstate) {
  constexpr int PW = affine_words<C>();
  constexpr int XW = xyzz_words<C>();
  const uint32_t b = blockIdx.y;
  const uint32_t seg = blockIdx.x * blockDim.x + threadIdx.x;
  if (seg >= smax) return;
  const size_t si = (size_t)b * smax + seg;
  const uint32_t* off = offsets + (size_t)b * (nb + 1);
  const uint32_t E = off[nb];
  const uint32_t start = seg * K;
  uint8_t state = 0;
  uint32_t tk = NO_TAIL;
  if (start < E) {
    const uint32_t end = min(start + K, E);
    // bucket k with off[k] <= start < off[k+1]
    uint32_t lo = 0, hi = nb;  // invariant off[lo] <= start < off[hi]
    while (hi - lo > 1) {
      uint32_t mid = (lo + hi) >> 1;
      if (off[mid] <= start)
        lo = mid;
      else
        hi = mid;
    }
    uint32_t k = lo;
    uint32_t next = off[k + 1];
    bool before = off[k] < start;
    Xyzz<C> acc = xyzz_inf<C>();
    const uint32_t* ent = entries + b * emax;
    // software pipeline: the entry and table point of p + 1 are in flight
    // during the mixed addition of p (the entry of p + 2 one step earlier)
#ifndef KZGX_NO_PREFETCH
    uint32_t e = ent[start];
    uint32_t e2 = start + 1 < end ? ent[start + 1] : 0u;
    Affine<C> nx = affine_load<C>(table + (size_t)(e & 0x7fffffffu) * PW);
#endif
    for (uint32_t p = start; p < end; ++p) {
#ifdef KZGX_NO_PREFETCH
      const uint32_t e = ent[p];
      Affine<C> a = affine_load<C>(table + (size_t)(e & 0x7fffffffu) * PW);
      const uint32_t neg = e >> 31;
#else
      Affine<C> a = nx;
      const uint32_t neg = e >> 31;
      if (p + 1 < end) {
        e = e2;
        if (p + 2 < end) e2 = ent[p + 2];
        nx = affine_load<C>(table + (size_t)(e & 0x7fffffffu) * PW);
      }
#endif
      if (p == next) {  // bucket k ended inside this segment
        if (before) {
          xyzz_store<C>(heads + si * XW, acc);
          state = HEAD;
          before = false;
        } else {
          xyzz_store<C>(bsum + ((size_t)b * nb + k) * XW, acc);
        }
        acc = xyzz_inf<C>();
        do {
          k++;
          next = off[k + 1];
        } while (next == p);
      }
      if (neg) a = affine_neg<C>(a);
      acc = xyzz_add_affine_impl<C>(acc, a);
    }
    if (before) {  // the whole segment is one head
      xyzz_store<C>(heads + si * XW, acc);
      state = HEAD | (next > end ? SPANS : 0);
    } else if (next > end) {
      xyzz_store<C>(tails + si * XW, acc);
      tk = k;
    } else {
      xyzz_store<C>(bsum + ((size_t)b * nb + k) * XW, acc);
    }
  }
  sstate[si] = state;
  tailk[si] = tk;
}

// pass 4b: buckets that cross workgroups.  The workgroup holding the start
// of such a bucket left its partial in gtail (gtailk = bucket); the later
// workgroups left their leading head chains in ghead.  Thread per workgroup.
template <class C>
__global__ __launch_bounds__(64) void k_msm_wg_fixup(uint32_t nb, uint32_t nwg, const uint32_t* __restrict__ ghead,
                                                     const uint32_t* __restrict__ gtail,
                                                     const uint32_t* __restrict__ gtailk,
                                                     const uint32_t* __restrict__ gflag, uint32_t* __restrict__ bsum) {
  constexpr int XW = xyzz_words<C>();
  const uint32_t b = blockIdx.y;
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= nwg) return;
  const size_t gi = (size_t)b * nwg + g;
  const uint32_t k = gtailk[gi];
  if (k == NO_TAIL) return;
  Xyzz<C> acc = xyzz_load<C>(gtail + gi * XW);
  for (uint32_t h = g + 1; h < nwg; h++) {
    const size_t hi = (size_t)b * nwg + h;
    acc = xyzz_add<C>(acc, xyzz_load<C>(ghead + hi * XW));
    if (!(gflag[hi] & SPANS)) break;
  }
  xyzz_store<C>(bsum + ((size_t)b * nb + k) * XW, acc);
}

// pass 5a: bucket running sums, J buckets per thread.  Thread t of
// MSM b owns buckets [t J, t J + J) and emits
//   R_t = sum_j (j + 1) B_{tJ+j}   and   T_t = sum_j B_{tJ+j}
// so that sum_k (k + 1) B_k = sum_t R_t + J sum_t t T_t.
// J = RED_J for batches; RED_J_SMALL for small batches, whose reduction is
// latency-bound: every lane is alone on its SIMD and issues its additions one
// after another, so the fewer per lane the sooner the call returns (the fold
// then runs as one workgroup with the affine conversion inline)
constexpr uint32_t RED_J = 8;
constexpr uint32_t RED_J_SMALL = 2;

template <class C, uint32_t J>
__global__ __launch_bounds__(256, KZGX_BS_WAVES) void k_msm_bucket_sums(const uint32_t* __restrict__ offsets, uint32_t nb,
                                                                        const uint32_t* __restrict__ bsum,
                                                                        uint32_t* __restrict__ rt) {
  constexpr int XW = xyzz_words<C>();
  const uint32_t b = blockIdx.y;
  const uint32_t T1 = nb / J;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T1) return;
  const uint32_t* off = offsets + (size_t)b * (nb + 1) + t * J;
  const uint32_t* src = bsum + ((size_t)b * nb + t * J) * XW;
  Xyzz<C> run = xyzz_inf<C>(), sum = xyzz_inf<C>();
  for (int j = (int)J - 1; j >= 0; j--) {
    if (off[j + 1] > off[j]) run = xyzz_add_impl<C>(run, xyzz_load<C>(src + (size_t)j * XW));  // empty buckets: never written
    sum = xyzz_add_impl<C>(sum, run);
  }
  uint32_t* dst = rt + ((size_t)b * T1 + t) * 2 * XW;
  xyzz_store<C>(dst, sum);
  xyzz_store<C>(dst + XW, run);
}

// XYZZ point moved down the wavefront by off lanes (lanes past the end keep
// their own value)
template <class C>
KZGX_DEV Xyzz<C> xyzz_shfl_down(const Xyzz<C>& p, int off) {
  constexpr int L = C::Fp29::L;
  Xyzz<C> o;
#pragma unroll
  for (int k = 0; k < L; k++) {
    o.X.v[k] = __shfl_down(p.X.v[k], off, 64);
    o.Y.v[k] = __shfl_down(p.Y.v[k], off, 64);
    o.ZZ.v[k] = __shfl_down(p.ZZ.v[k], off, 64);
    o.ZZZ.v[k] = __shfl_down(p.ZZZ.v[k], off, 64);
  }
  return o;
}

template <class C>
KZGX_DEV Xyzz<C> xyzz_dbl_n(Xyzz<C> p, uint32_t m) {  // 2^log2(m) p, m a power of two
#pragma unroll 1
  for (; m > 1; m >>= 1) p = xyzz_dbl_impl<C>(p);
  return p;
}

// pass 5b: one wavefront per MSM folds the T1 = NB / J pairs (R_t, T_t):
//   V = sum_t R_t + J sum_t t T_t.
// Lane l first folds its G = T1 / 64 consecutive pairs into
//   R'_l = sum_i R_{Gl+i} + J sum_i i T_{Gl+i},   T'_l = sum_i T_{Gl+i},
// so V = sum_l R'_l + J G sum_l l T'_l, and sum_l l T'_l = sum_{l >= 1} S_l
// with the suffix sums S_l = sum_{u >= l} T'_u: a 6-step __shfl_down scan.
// U_l = R'_l + J G S_l (l >= 1) is then summed by a 6-step shuffle tree, and
// lane 0 stores V as an XYZZ point (k_msm_finish converts it, or chunked
// callers sum it with k_xyzz_sum).  Four MSMs per 256-thread block.
template <class C, uint32_t RED_J>
__global__ __launch_bounds__(256) void k_msm_bucket_fold(const uint32_t* __restrict__ rt, uint32_t T1, uint32_t batch,
                                                         uint32_t* __restrict__ xyzz_out) {
  constexpr int XW = xyzz_words<C>();
  const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (b >= batch) return;  // whole wavefronts
  const uint32_t G = T1 / 64;
  const uint32_t* src = rt + ((size_t)b * T1 + (size_t)lane * G) * 2 * XW;
  Xyzz<C> R = xyzz_inf<C>(), run = xyzz_inf<C>(), acc = xyzz_inf<C>();
#pragma unroll 1
  for (int i = (int)G - 1; i >= 1; i--) {
    R = xyzz_add_impl<C>(R, xyzz_load<C>(src + (size_t)i * 2 * XW));
    run = xyzz_add_impl<C>(run, xyzz_load<C>(src + (size_t)i * 2 * XW + XW));
    acc = xyzz_add_impl<C>(acc, run);  // sum_i i T_i
  }
  R = xyzz_add_impl<C>(R, xyzz_load<C>(src));
  Xyzz<C> S = xyzz_add_impl<C>(run, xyzz_load<C>(src + XW));  // T'_l
  R = xyzz_add_impl<C>(R, xyzz_dbl_n<C>(acc, RED_J));           // R'_l
  // inclusive suffix scan of T' over the wavefront
#pragma unroll 1
  for (int o = 1; o < 64; o <<= 1) {
    const Xyzz<C> x = xyzz_shfl_down<C>(S, o);
    if (lane + o < 64) S = xyzz_add_impl<C>(S, x);
  }
  Xyzz<C> U = R;
  if (lane > 0) U = xyzz_add_impl<C>(U, xyzz_dbl_n<C>(S, RED_J * G));
#pragma unroll 1
  for (int o = 32; o >= 1; o >>= 1) U = xyzz_add_impl<C>(U, xyzz_shfl_down<C>(U, o));
  if (lane == 0) xyzz_store<C>(xyzz_out + (size_t)b * XW, U);
}

// pass 5b, workgroup form: one 256-thread workgroup per MSM folds the T1
// pairs, G = T1 / 256 per lane, with the same algebra as k_msm_bucket_fold:
//   V = sum_l R'_l + J G sum_{l >= 1} S_l,  S_l = sum_{u >= l} T'_u
// over l = 0..255.  The suffix scan is a wavefront scan plus the totals of
// the higher wavefronts (LDS), the final sum a wavefront tree plus the four
// wavefront sums.  Dependent chain: 3 (G - 1) + 2 + 6 + 3 + log2(J G)
// doublings + 1 + 6 + 2 additions, against 3 (G' - 1) + 2 + log2(J) + 1 + 6
// + log2(J G') + 1 + 6 (G' = T1 / 64) in the one-wavefront fold, and four
// wavefronts per MSM instead of one (a batch of 1024 MSMs keeps 4 waves per
// SIMD busy, not 1).  With out != nullptr lane 0 also converts to affine (no
// separate finish launch).
constexpr int FOLD_WG = 256;

template <class C, uint32_t RED_J>
__global__ __launch_bounds__(FOLD_WG) void k_msm_bucket_fold_wg(const uint32_t* __restrict__ rt, uint32_t T1,
                                                                uint32_t* __restrict__ xyzz_out,
                                                                uint32_t* __restrict__ out,
                                                                uint32_t* __restrict__ out_inf) {
  constexpr int XW = xyzz_words<C>();
  __shared__ uint32_t lds[4 * XW];
  const uint32_t b = blockIdx.x;
  const uint32_t l = threadIdx.x, lane = l & 63, wv = l >> 6;
  const uint32_t G = T1 / FOLD_WG;
  const uint32_t* src = rt + ((size_t)b * T1 + (size_t)l * G) * 2 * XW;
  Xyzz<C> R = xyzz_load<C>(src + (size_t)(G - 1) * 2 * XW);
  Xyzz<C> run = xyzz_load<C>(src + (size_t)(G - 1) * 2 * XW + XW);
  Xyzz<C> acc = xyzz_inf<C>();
#pragma unroll 1
  for (int i = (int)G - 2; i >= 0; i--) {
    acc = xyzz_add_impl<C>(acc, run);  // sum_i i T_i, one term per step
    R = xyzz_add_impl<C>(R, xyzz_load<C>(src + (size_t)i * 2 * XW));
    run = xyzz_add_impl<C>(run, xyzz_load<C>(src + (size_t)i * 2 * XW + XW));
  }
  if (G > 1) R = xyzz_add_impl<C>(R, xyzz_dbl_n<C>(acc, RED_J));  // R'_l
  Xyzz<C> S = run;                                                // T'_l
  // inclusive suffix scan of T' within the wavefront
#pragma unroll 1
  for (int o = 1; o < 64; o <<= 1) {
    const Xyzz<C> x = xyzz_shfl_down<C>(S, o);
    if (lane + o < 64) S = xyzz_add_impl<C>(S, x);
  }
  // + the totals of the higher wavefronts
  if (lane == 0) xyzz_store<C>(lds + wv * XW, S);
  __syncthreads();
#pragma unroll 1
  for (uint32_t w = wv + 1; w < 4; w++) S = xyzz_add_impl<C>(S, xyzz_load<C>(lds + w * XW));
  __syncthreads();  // lds is reused below
  Xyzz<C> U = R;
  if (l > 0) U = xyzz_add_impl<C>(U, xyzz_dbl_n<C>(S, RED_J * G));
#pragma unroll 1
  for (int o = 32; o >= 1; o >>= 1) U = xyzz_add_impl<C>(U, xyzz_shfl_down<C>(U, o));
  if (lane == 0) xyzz_store<C>(lds + wv * XW, U);
  __syncthreads();
  if (l < 2) U = xyzz_add_impl<C>(xyzz_load<C>(lds + l * XW), xyzz_load<C>(lds + (l + 2) * XW));
  U = xyzz_add_impl<C>(U, xyzz_shfl_down<C>(U, 1));
  if (wv != 0) return;  // wavefront 0 (the sum in its lane 0) converts
  if (xyzz_out) {
    if (l == 0) xyzz_store<C>(xyzz_out + (size_t)b * XW, U);
    return;
  }
  // the whole wavefront on lane 0's value: the inversion's loop on the scalar
  // ALU, its linear combinations one per lane (f29_inv_uniform)
  Xyzz<C> s;
#pragma unroll
  for (int k = 0; k < C::Fp29::L; k++) {
    s.X.v[k] = __builtin_amdgcn_readfirstlane(U.X.v[k]);
    s.Y.v[k] = __builtin_amdgcn_readfirstlane(U.Y.v[k]);
    s.ZZ.v[k] = __builtin_amdgcn_readfirstlane(U.ZZ.v[k]);
    s.ZZZ.v[k] = __builtin_amdgcn_readfirstlane(U.ZZZ.v[k]);
  }
  constexpr int N = C::Fp::N;
  uint32_t wx[N], wy[N];
  const bool fin = xyzz_to_canonical_lane<C>(s, wx, wy);
  if (l != 0) return;
#pragma unroll
  for (int k = 0; k < N; k++) {
    out[(size_t)b * 2 * N + k] = wx[k];
    out[(size_t)b * 2 * N + N + k] = wy[k];
  }
  out_inf[b] = fin ? 0u : 1u;
}

// pass 6: thread per MSM, XYZZ -> canonical affine (one inversion each), off
// the fold's single-lane critical path
template <class C>
__global__ __launch_bounds__(64) void k_msm_finish(const uint32_t* __restrict__ v, uint32_t batch,
                                                   uint32_t* __restrict__ out, uint32_t* __restrict__ out_inf) {
  constexpr int XW = xyzz_words<C>();
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  Affine<C> a;
  const bool fin = xyzz_to_affine<C>(xyzz_load<C>(v + (size_t)b * XW), a);
  affine_to_canonical<C>(out + (size_t)b * 2 * C::Fp::N, a, fin);
  out_inf[b] = fin ? 0u : 1u;
}

// sum of count XYZZ points -> canonical affine (one 256-thread workgroup:
// strided per-thread sums, then an LDS tree)
template <class C>
__global__ __launch_bounds__(256) void k_xyzz_sum(const uint32_t* __restrict__ pts, uint32_t count,
                                                  uint32_t* __restrict__ out, uint32_t* __restrict__ out_inf) {
  constexpr int XW = xyzz_words<C>();
  extern __shared__ uint32_t lds[];
  const uint32_t t = threadIdx.x;
  Xyzz<C> acc = xyzz_inf<C>();
  for (uint32_t i = t; i < count; i += blockDim.x) acc = xyzz_add_impl<C>(acc, xyzz_load<C>(pts + (size_t)i * XW));
  xyzz_store<C>(lds + t * XW, acc);
  __syncthreads();
  for (uint32_t h = blockDim.x / 2; h >= 1; h >>= 1) {
    if (t < h) {
      acc = xyzz_add_impl<C>(acc, xyzz_load<C>(lds + (t + h) * XW));
      xyzz_store<C>(lds + t * XW, acc);
    }
    __syncthreads();
  }
  if (t == 0) {
    constexpr int N = C::Fp::N;
    uint32_t wx[N], wy[N];
    const bool fin = xyzz_to_canonical_lane<C>(acc, wx, wy);
#pragma unroll
    for (int k = 0; k < N; k++) {
      out[k] = wx[k];
      out[N + k] = wy[k];
    }
    *out_inf = fin ? 0u : 1u;
  }
}

// --------------------------------------------------------------------------
// large single MSMs (n >= 2^16): wide windows, global counting sort
// --------------------------------------------------------------------------
// One MSM of n points at c = 14..16 (2^13..2^15 buckets) instead of n / 4096
// chunked c = 12 MSMs: n W additions (W = 17 at c = 16 against 22 at c = 12)
// and ONE bucket reduction instead of one per chunk.  The wide window's
// table T_big[w][i] = 2^(c w) P_i is built with the SRS (srs_upload).  The
// sort is a two-pass counting sort over blocks of `per` scalars: each block
// keeps its whole bucket histogram in LDS (2^(c-1) counters, up to 128 KB of
// gfx950's 160 KB), a scan turns the block histograms into per-(block,
// bucket) write bases, and the scatter ranks with LDS atomics that return
// global positions directly.  Accumulation and segment merges are the
// batched path's kernels; the bucket reduction runs in latency.hip.
constexpr uint32_t BIG_TPB = 1024;  // threads of a count / scatter block

template <int CB>
__global__ __launch_bounds__(BIG_TPB) void k_big_count(const uint32_t* __restrict__ scalars, uint32_t n,
                                                       const uint8_t* __restrict__ inf, uint32_t per,
                                                       uint32_t* __restrict__ counts) {
  constexpr int W = Win<CB>::W;
  constexpr uint32_t NB = Win<CB>::NB;
  __shared__ uint32_t hist[NB];
  for (uint32_t k = threadIdx.x; k < NB; k += BIG_TPB) hist[k] = 0;
  __syncthreads();
  const uint32_t i0 = blockIdx.x * per, i1 = min(n, i0 + per);
#pragma unroll 1
  for (uint32_t i = i0 + threadIdx.x; i < i1; i += BIG_TPB) {
    if (inf[i]) continue;
    uint32_t s[8];
    load_scalar(scalars + (size_t)i * 8, s);
    uint32_t carry = 0;
#pragma unroll
    for (int w = 0; w < W; w++) {
      const int d = digit_at<CB>(s, w, carry);
      if (d != 0) atomicAdd(&hist[(d < 0 ? -d : d) - 1], 1u);
    }
  }
  __syncthreads();
  uint32_t* out = counts + (size_t)blockIdx.x * NB;
  for (uint32_t k = threadIdx.x; k < NB; k += BIG_TPB) out[k] = hist[k];
}

// bucket totals over the blocks (thread per bucket, coalesced over k)
template <int CB>
__global__ __launch_bounds__(256) void k_big_tot(const uint32_t* __restrict__ counts, uint32_t nblk,
                                                 uint32_t* __restrict__ tot) {
  constexpr uint32_t NB = Win<CB>::NB;
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= NB) return;
  uint32_t s = 0;
  for (uint32_t b = 0; b < nblk; b++) s += counts[(size_t)b * NB + k];
  tot[k] = s;
}

// exclusive scan of the NB totals -> offsets[0..NB] (one workgroup)
template <int CB>
__global__ __launch_bounds__(1024) void k_big_scan(const uint32_t* __restrict__ tot, uint32_t* __restrict__ offsets) {
  constexpr uint32_t NB = Win<CB>::NB;
  constexpr uint32_t PER = NB / 1024;
  static_assert(PER >= 1 && NB % 1024 == 0, "k_big_scan: c >= 11");
  __shared__ uint32_t wsum[16];
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  uint32_t v[PER], local = 0;
#pragma unroll
  for (uint32_t j = 0; j < PER; j++) {
    v[j] = tot[t * PER + j];
    local += v[j];
  }
  uint32_t x = local;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= (uint32_t)o) x += y;
  }
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  if (t == 0) {
    uint32_t run = 0;
    for (int w = 0; w < 16; w++) {
      const uint32_t c = wsum[w];
      wsum[w] = run;
      run += c;
    }
    offsets[NB] = run;
  }
  __syncthreads();
  uint32_t excl = x - local + wsum[wv];
#pragma unroll
  for (uint32_t j = 0; j < PER; j++) {
    offsets[t * PER + j] = excl;
    excl += v[j];
  }
}

// write base of every (block, bucket): offsets[k] + the earlier blocks' counts
template <int CB>
__global__ __launch_bounds__(256) void k_big_bases(const uint32_t* __restrict__ counts, uint32_t nblk,
                                                   const uint32_t* __restrict__ offsets, uint32_t* __restrict__ bbase) {
  constexpr uint32_t NB = Win<CB>::NB;
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= NB) return;
  uint32_t base = offsets[k];
  for (uint32_t b = 0; b < nblk; b++) {
    bbase[(size_t)b * NB + k] = base;
    base += counts[(size_t)b * NB + k];
  }
}

// (table index | sign) entries into bucket order: LDS cursors start at the
// block's write bases, so an LDS atomic returns the entry's global position
template <int CB>
__global__ __launch_bounds__(BIG_TPB) void k_big_scatter(const uint32_t* __restrict__ scalars, uint32_t n,
                                                         const uint8_t* __restrict__ inf, uint32_t per,
                                                         const uint32_t* __restrict__ bbase,
                                                         uint32_t* __restrict__ entries, uint32_t n_rows) {
  constexpr int W = Win<CB>::W;
  constexpr uint32_t NB = Win<CB>::NB;
  __shared__ uint32_t cur[NB];
  const uint32_t* bb = bbase + (size_t)blockIdx.x * NB;
  for (uint32_t k = threadIdx.x; k < NB; k += BIG_TPB) cur[k] = bb[k];
  __syncthreads();
  const uint32_t i0 = blockIdx.x * per, i1 = min(n, i0 + per);
#pragma unroll 1
  for (uint32_t i = i0 + threadIdx.x; i < i1; i += BIG_TPB) {
    if (inf[i]) continue;
    uint32_t s[8];
    load_scalar(scalars + (size_t)i * 8, s);
    uint32_t carry = 0;
#pragma unroll
    for (int w = 0; w < W; w++) {
      const int d = digit_at<CB>(s, w, carry);
      if (d != 0) {
        const uint32_t pos = atomicAdd(&cur[(d < 0 ? -d : d) - 1], 1u);
        entries[pos] = ((uint32_t)w * n_rows + i) | (d < 0 ? 0x80000000u : 0u);
      }
    }
  }
}

// ---- two-pass sort and bucket-aligned segments (round 5) ----
// With 2^(c-1) = 8192..32768 buckets, a per-block bucket histogram is as
// large as the block's digits, so the one-pass sort above spends most of its
// time on its own count rows (the 2^20 + 1 MSM: 461 us of sort for 1.3 ms of
// accumulation, profiles/r05_big_msm_*).  Instead:
//   pass 1: BIG_NC = 1024 coarse bins (the high bits of the bucket): per-block
//           LDS histograms of 1024 counters, a per-bin scan over the blocks
//           (one workgroup per bin), a 1024-entry scan, and a scatter of
//           packed entries (table index | fine bits << 26 | sign << 31) in
//           runs of ~34 per (block, bin);
//   pass 2: one workgroup per coarse bin ranks its ~17k entries by the fine
//           bits in LDS and writes them in bucket order (bucket offsets too),
//           and cuts every bucket into ceil(len / K) accumulation segments
//           that never cross a bucket, so no merge of crossing partials is
//           needed: the reduction sums each bucket's few segment partials.
// Used when the table index fits 26 bits (W n_rows < 2^26: SRSs up to
// ~3.9M points at c = 16); larger SRSs keep the one-pass sort and merge.
constexpr uint32_t BIG_NC = 1024;
constexpr uint32_t BIG_IDX_BITS = 26;
constexpr uint32_t BIG_MAXSEG = 64;  // segment partials per bucket the reduction sums directly

template <int CB>
struct BigFine {
  static constexpr uint32_t NF = Win<CB>::NB / BIG_NC;  // buckets per coarse bin
  static constexpr int FB = CB - 1 - 10;
  static_assert(NF >= 2 && NF <= 64 && (1u << FB) == NF, "c = 12..17");
  // a pass-1 entry: table index (IDX bits) | fine bits << IDX | sign << 31:
  // 26 index bits up to c = 16, 25 at c = 17 (its 6 fine bits)
  static constexpr uint32_t IDX = FB <= 5 ? BIG_IDX_BITS : 31u - (uint32_t)FB;
};

template <int CB>
__global__ __launch_bounds__(BIG_TPB) void k_big2_count(const uint32_t* __restrict__ scalars, uint32_t n,
                                                        const uint8_t* __restrict__ inf, uint32_t per, uint32_t nblk,
                                                        uint32_t* __restrict__ counts_t) {
  constexpr int W = Win<CB>::W;
  constexpr int FB = BigFine<CB>::FB;
  __shared__ uint32_t hist[BIG_NC];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t i0 = blockIdx.x * per, i1 = min(n, i0 + per);
#pragma unroll 1
  for (uint32_t i = i0 + threadIdx.x; i < i1; i += BIG_TPB) {
    if (inf[i]) continue;
    uint32_t s[8];
    load_scalar(scalars + (size_t)i * 8, s);
    uint32_t carry = 0;
#pragma unroll
    for (int w = 0; w < W; w++) {
      const int d = digit_at<CB>(s, w, carry);
      if (d != 0) atomicAdd(&hist[((uint32_t)(d < 0 ? -d : d) - 1) >> FB], 1u);
    }
  }
  __syncthreads();
  counts_t[(size_t)threadIdx.x * nblk + blockIdx.x] = hist[threadIdx.x];  // bin-major
}

// workgroup per coarse bin: exclusive scan of its per-block counts (bases,
// relative to the bin start) and the bin total
static __global__ __launch_bounds__(256) void k_big2_binscan(const uint32_t* __restrict__ counts_t, uint32_t nblk,
                                                      uint32_t* __restrict__ bases_t, uint32_t* __restrict__ tot) {
  __shared__ uint32_t wsum[4];
  const uint32_t bin = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint32_t* src = counts_t + (size_t)bin * nblk;
  uint32_t* dst = bases_t + (size_t)bin * nblk;
  uint32_t run = 0;
  for (uint32_t b0 = 0; b0 < nblk; b0 += 256) {
    const uint32_t v = b0 + t < nblk ? src[b0 + t] : 0u;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(x, o, 64);
      if (lane >= (uint32_t)o) x += y;
    }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    uint32_t before = run;
    for (uint32_t w = 0; w < wv; w++) before += wsum[w];
    if (b0 + t < nblk) dst[b0 + t] = before + x - v;
    run += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  if (t == 0) tot[bin] = run;
}

// one workgroup: exclusive scan of 1024 values -> out[0..1024]
static __global__ __launch_bounds__(1024) void k_scan1024(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  __shared__ uint32_t wsum[16];
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint32_t v = in[t];
  uint32_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= (uint32_t)o) x += y;
  }
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (uint32_t w = 0; w < 16; w++) {
    before += w < wv ? wsum[w] : 0u;
    all += wsum[w];
  }
  out[t] = before + x - v;
  if (t == 1023) out[1024] = all;
}

// scalars per pass-1 block: the block's W per entries are staged in LDS
// (<= 37888 words with the 3 x 1024-word cursor arrays, gfx950's 160 KB)
template <int CB>
constexpr uint32_t big2_per() {
  return Win<CB>::W <= 18 ? 2048u : 1536u;
}

// pass-1 scatter: the block's entries are ranked into LDS by coarse bin
// (LDS atomics on local cursors), then written out in bin order -- runs of
// consecutive positions per bin, so a wave's stores cover a few lines
// instead of 64 scattered words (the direct scatter was write-request bound:
// 136 us for the 2^20 + 1 MSM)
template <int CB>
__global__ __launch_bounds__(BIG_TPB) void k_big2_scatter(const uint32_t* __restrict__ scalars, uint32_t n,
                                                          const uint8_t* __restrict__ inf, uint32_t nblk,
                                                          const uint32_t* __restrict__ counts_t,
                                                          const uint32_t* __restrict__ coff,
                                                          const uint32_t* __restrict__ bases_t,
                                                          uint32_t* __restrict__ tmp, uint32_t n_rows) {
  constexpr int W = Win<CB>::W;
  constexpr int FB = BigFine<CB>::FB;
  constexpr uint32_t FM = (1u << FB) - 1;
  constexpr uint32_t PER = big2_per<CB>();
  static_assert(BIG_TPB == BIG_NC, "thread per coarse bin");
  __shared__ uint32_t stage[PER * W];
  __shared__ uint32_t lstart[BIG_NC + 1], lcur[BIG_NC], gbase[BIG_NC];
  __shared__ uint32_t wsum[BIG_TPB / 64];
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  // local bin starts: exclusive scan of this block's counts (pass-1 count)
  const uint32_t h = counts_t[(size_t)t * nblk + blockIdx.x];
  uint32_t x = h;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= (uint32_t)o) x += y;
  }
  if (lane == 63) wsum[wv] = x;
  gbase[t] = coff[t] + bases_t[(size_t)t * nblk + blockIdx.x];
  __syncthreads();
  uint32_t before = 0, total = 0;
  for (uint32_t w = 0; w < BIG_TPB / 64; w++) {
    before += w < wv ? wsum[w] : 0u;
    total += wsum[w];
  }
  lstart[t] = before + x - h;
  lcur[t] = before + x - h;
  if (t == 0) lstart[BIG_NC] = total;
  __syncthreads();
  const uint32_t i0 = blockIdx.x * PER, i1 = min(n, i0 + PER);
#pragma unroll 1
  for (uint32_t i = i0 + t; i < i1; i += BIG_TPB) {
    if (inf[i]) continue;
    uint32_t s[8];
    load_scalar(scalars + (size_t)i * 8, s);
    uint32_t carry = 0;
#pragma unroll
    for (int w = 0; w < W; w++) {
      const int d = digit_at<CB>(s, w, carry);
      if (d != 0) {
        const uint32_t bk = (uint32_t)(d < 0 ? -d : d) - 1;
        const uint32_t pos = atomicAdd(&lcur[bk >> FB], 1u);
        stage[pos] = ((uint32_t)w * n_rows + i) | ((bk & FM) << BigFine<CB>::IDX) | (d < 0 ? 0x80000000u : 0u);
      }
    }
  }
  __syncthreads();
  for (uint32_t j = t; j < total; j += BIG_TPB) {
    uint32_t lo = 0, hi = BIG_NC;  // lstart[lo] <= j < lstart[hi]
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (lstart[mid] <= j)
        lo = mid;
      else
        hi = mid;
    }
    tmp[gbase[lo] + (j - lstart[lo])] = stage[j];
  }
}

// workgroup per coarse bin: a STABLE rank of its entries by the fine bits
// (rounds of 1024 entries in order, 4 per thread; a wave ranks equal keys
// with ballots, one thread per key prefixes the 16 (sub-round, wave)
// blocks), so every bucket keeps pass 1's block order -- ascending
// point index -- and the threads accumulating at the same moment gather from
// nearby table rows (an unordered rank measured the accumulation 35% slower
// on 2^20 + 1 points: the gathers lost their L2 / MALL locality).  Also the
// bucket offsets and each bucket's segment count ceil(len / K) (segl: the
// bin-local exclusive prefix, segn: the bin's total).
template <int CB>
__global__ __launch_bounds__(256) void k_big2_fine(const uint32_t* __restrict__ tmp, const uint32_t* __restrict__ coff,
                                                   uint32_t K, uint32_t* __restrict__ entries,
                                                   uint32_t* __restrict__ offsets, uint32_t* __restrict__ segl,
                                                   uint32_t* __restrict__ segn) {
  constexpr uint32_t NF = BigFine<CB>::NF;
  constexpr int FB = BigFine<CB>::FB;
  constexpr uint32_t NB = Win<CB>::NB;
  constexpr uint32_t FM = NF - 1;
  constexpr uint32_t IB = BigFine<CB>::IDX;
  constexpr uint32_t E = 4;  // entries per thread per round: (e, t) order, 1024 per round
  __shared__ uint32_t h[NF], cur[NF], pre[E * 4][NF], lbase[NF], gbase[NF], stage[256 * E];
  __shared__ uint32_t nround;
  const uint32_t bin = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const uint32_t b0 = coff[bin], b1 = coff[bin + 1];
  if (t < NF) h[t] = 0;
  __syncthreads();
  // the histogram sweep with 8 loads in flight per thread (one at a time it
  // waited ~68 global-load latencies per thread: 130 us of the 2^20 sort)
  uint32_t j = b0 + t;
  for (; j + 7 * 256 < b1; j += 8 * 256) {
    uint32_t v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = tmp[j + k * 256];
#pragma unroll
    for (int k = 0; k < 8; k++) atomicAdd(&h[(v[k] >> IB) & FM], 1u);
  }
  for (; j < b1; j += 256) atomicAdd(&h[(tmp[j] >> IB) & FM], 1u);
  __syncthreads();
  if (t == 0) {
    uint32_t run = b0, sr = 0;
    for (uint32_t f = 0; f < NF; f++) {
      const uint32_t len = h[f];
      offsets[bin * NF + f] = run;
      cur[f] = run;
      segl[bin * NF + f] = sr;
      run += len;
      sr += (len + K - 1) / K;
    }
    segn[bin] = sr;
    if (bin == BIG_NC - 1) offsets[NB] = run;
  }
  const uint64_t lt = (1ull << lane) - 1ull;
  // the next round's entries are loaded while this round ranks (its global
  // loads no longer sit between rounds)
  uint32_t vn[E];
#pragma unroll
  for (uint32_t e = 0; e < E; e++) vn[e] = b0 + e * 256 + t < b1 ? tmp[b0 + e * 256 + t] : 0u;
  for (uint32_t r0 = b0; r0 < b1; r0 += 256 * E) {
    uint32_t v[E], rank[E];
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
      v[e] = vn[e];
      const uint32_t jn = r0 + 256 * E + e * 256 + t;
      vn[e] = jn < b1 ? tmp[jn] : 0u;
    }
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
      const uint32_t j = r0 + e * 256 + t;
      const bool act = j < b1;
      const uint32_t f = (v[e] >> IB) & FM;
      // lanes of this wave with the same key: AND of the per-bit ballots
      uint64_t eq = __ballot(act);
#pragma unroll
      for (int b = 0; b < FB; b++) {
        const uint64_t m = __ballot((f >> b) & 1u);
        eq &= ((f >> b) & 1u) ? m : ~m;
      }
      rank[e] = act ? (uint32_t)__popcll(eq & lt) : ~0u;
      if (lane < NF) pre[e * 4 + wv][lane] = 0;  // this wave's counts (ordered before its own writes)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      if (act && (eq >> lane) == 1ull) pre[e * 4 + wv][f] = rank[e] + 1;  // the last lane of its key
    }
    __syncthreads();  // also orders this round's reads of cur after the previous update
    if (t < 64) {  // wave 0: per key, the 16 blocks' local prefix, the key's round total, then a
                   // scan over the keys -> each key's start in the round (sorted by key)
      uint32_t tot = 0;
      if (t < NF) {
#pragma unroll
        for (uint32_t q = 0; q < E * 4; q++) {
          const uint32_t c = pre[q][t];
          pre[q][t] = tot;
          tot += c;
        }
      }
      uint32_t x = tot;
#pragma unroll
      for (int o = 1; o < (int)NF; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= (uint32_t)o) x += y;
      }
      if (t < NF) {
        lbase[t] = x - tot;
        gbase[t] = cur[t];
        cur[t] += tot;
      }
      const uint32_t all = __shfl(x, (int)NF - 1, 64);
      if (t == 0) nround = all;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t e = 0; e < E; e++) {
      if (rank[e] == ~0u) continue;
      const uint32_t f = (v[e] >> IB) & FM;
      stage[lbase[f] + pre[e * 4 + wv][f] + rank[e]] = v[e];
    }
    __syncthreads();
    // write the round sorted by key: consecutive threads, consecutive
    // positions of each key's run (a wave's stores cover a few lines)
    for (uint32_t q = t; q < nround; q += 256) {
      const uint32_t w = stage[q];
      const uint32_t f = (w >> IB) & FM;
      entries[gbase[f] + (q - lbase[f])] = w & (0x80000000u | ((1u << IB) - 1u));
    }
    __syncthreads();  // pre, stage and the bases are rewritten by the next round
  }
}

// segment offsets: seg_off[k] = sum over buckets j < k of ceil(len_j / K);
// thread per coarse bin (one workgroup); *flag = some bucket has more than
// BIG_MAXSEG segments (the reduction then pre-sums them, big_reduce_seg)
template <int CB>
__global__ __launch_bounds__(1024) void k_big2_segscan(const uint32_t* __restrict__ segl,
                                                       const uint32_t* __restrict__ segn,
                                                       uint32_t* __restrict__ seg_off, uint32_t* __restrict__ flag) {
  constexpr uint32_t NF = BigFine<CB>::NF;
  constexpr uint32_t NB = Win<CB>::NB;
  __shared__ uint32_t wsum[16];
  __shared__ uint32_t any_long;
  const uint32_t t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t == 0) any_long = 0;
  const uint32_t v = segn[t];
  uint32_t x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= (uint32_t)o) x += y;
  }
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  uint32_t base = x - v;
  for (uint32_t w = 0; w < wv; w++) base += wsum[w];
  bool lng = false;
  for (uint32_t f = 0; f < NF; f++) {
    const uint32_t l = segl[t * NF + f];
    const uint32_t nx = f + 1 < NF ? segl[t * NF + f + 1] : v;
    lng |= nx - l > BIG_MAXSEG;
    seg_off[t * NF + f] = base + l;
  }
  if (t == BIG_NC - 1) seg_off[NB] = base + v;
  if (lng) atomicOr(&any_long, 1u);
  __syncthreads();
  if (t == 0) *flag = any_long;
}

// bucket k of segment j: seg_off[k] <= j < seg_off[k + 1]
KZGX_DEV uint32_t seg_bucket(const uint32_t* __restrict__ seg_off, uint32_t nb, uint32_t j) {
  uint32_t lo = 0, hi = nb;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (seg_off[mid] <= j)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// thread per segment: up to K entries of one bucket, summed into part[j]
template <class C>
__global__ __launch_bounds__(256, pip_accum_waves<C>()) void k_big_accum(
    const uint32_t* __restrict__ entries, const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ seg_off,
    uint32_t nb, const uint32_t* __restrict__ table, uint32_t K, uint32_t* __restrict__ part) {
  constexpr int PW = affine_words<C>();
  constexpr int XW = xyzz_words<C>();
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= seg_off[nb]) return;
  const uint32_t k = seg_bucket(seg_off, nb, j);
  // the bucket's len entries in s = ceil(len / K) equal parts (not K, K, ...,
  // rest: a wave waits for its longest thread, measured +35% on 2^20 points)
  const uint32_t o0 = offsets[k], len = offsets[k + 1] - o0, s = seg_off[k + 1] - seg_off[k], i = j - seg_off[k];
  const uint32_t start = o0 + (uint32_t)(((uint64_t)i * len) / s);
  const uint32_t end = o0 + (uint32_t)(((uint64_t)(i + 1) * len) / s);
  Xyzz<C> acc = xyzz_inf<C>();
  // the entry and table point of p + 1 in flight during the addition of p
  uint32_t e = entries[start];
  uint32_t e2 = start + 1 < end ? entries[start + 1] : 0u;
  Affine<C> nx = affine_load<C>(table + (size_t)(e & 0x7fffffffu) * PW);
  for (uint32_t p = start; p < end; ++p) {
    Affine<C> a = nx;
    const uint32_t neg = e >> 31;
    if (p + 1 < end) {
      e = e2;
      if (p + 2 < end) e2 = entries[p + 2];
      nx = affine_load<C>(table + (size_t)(e & 0x7fffffffu) * PW);
    }
    if (neg) a = affine_neg<C>(a);
    acc = xyzz_add_affine_impl<C>(acc, a);
  }
  xyzz_store<C>(part + (size_t)j * XW, acc);
}

// --------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------
// Small batches (a single create_commit / create_proof, the reference's own
// call pattern) are latency-bound: the bucket reduction of one MSM is a chain
// of dependent additions whose depth grows with the bucket count 2^(c-1).
// Measured single degree-4096 BN254 commits (host buffers,
// profiles/r03_latency_window.json): c = 10 0.545 ms, c = 11 0.587, c = 12
// 0.712, c = 13 0.679; batched throughput keeps c = 12.  So the context also
// keeps a c = 10 window table over the first SMALL_MAX_POINTS SRS points
// (8.5 MB for a 4097-point SRS, 136 MB at most), used for batches of at most
// Ctx::small_batch MSMs (kzgx_set_small_batch; 0 = never) inside that prefix.
#ifndef KZGX_SMALL_WINDOW_BITS
#define KZGX_SMALL_WINDOW_BITS 10
#endif
constexpr size_t SMALL_MAX_POINTS = 65536;
// batches of at most this many MSMs reduce their buckets RED_J_SMALL per thread
#ifndef KZGX_SMALL_BATCH_J
#define KZGX_SMALL_BATCH_J 16
#endif

// large single MSMs take the wide-window path from this many points
// (KZGX_BIG_MIN; 0 turns the path off: chunked c = 12 batches as in round 4)
static size_t big_min_points() {
  static const size_t v = std::getenv("KZGX_BIG_MIN") ? std::strtoull(std::getenv("KZGX_BIG_MIN"), nullptr, 10)
                                                      : (size_t)1 << 16;
  return v ? v : ~(size_t)0;
}
// its window for an SRS of n points: fewer additions per point (n W) against
// a deeper bucket reduction (log2 of 2^(c-1) buckets) -- and a top window
// that spreads.  Scalars are uniform below r (BN254 2^253.6, BLS12-381
// 2^254.9), so the top window's digit takes only the values r's top bits
// allow: at BN254 c = 14 (window 18 = bits 252..) a handful, which drops
// ~n/2 entries into 4 buckets (their pre-sum passes made a 131 073-point MSM
// 1.19 ms); c = 15 (bits 240..254, up to 12 388) and 16 (bits 240..255) spread
// them, and for BLS12-381 only c = 16 keeps the top digit below 2^(c-1) (no
// carry into a near-empty extra window).  Measured at 131 073 points,
// uniform scalars: c = 13 / 14 / 15 / 16 -> 0.79 / 1.19 / 0.65-0.68 /
// 0.76-0.83 ms (profiles/r06_shard8_window_ab.jsonl).  KZGX_BIG_WINDOW pins it.
// c = 17 (65 536 buckets, 15 digit windows) is built and pinnable: 6% fewer
// additions than c = 16 but a bucket reduction twice as wide, measured 2%
// slower at 2^19 + 1 and 2^20 + 1 points (profiles/r06_big_window17_ab.jsonl),
// so never chosen automatically.
static int big_window_bits(size_t n, int curve) {
  static const int pin = std::getenv("KZGX_BIG_WINDOW") ? std::atoi(std::getenv("KZGX_BIG_WINDOW")) : 0;
  if (pin >= 12 && pin <= 17) return pin;
  if (curve != KZGX_CURVE_BN254) return 16;
  return n >= ((size_t)1 << 18) ? 16 : 15;
}

template <class C>
int srs_upload_impl(Ctx* ctx, const uint32_t* d_canon, size_t n) {
  const int W = ctx->W;
  const size_t pw = affine_words<C>() * sizeof(uint32_t);
  KZGX_TRY(dev_alloc(ctx, (void**)&ctx->d_table, (size_t)W * n * pw, &ctx->table_bytes));
  KZGX_TRY(dev_alloc(ctx, (void**)&ctx->d_inf, n, &ctx->inf_bytes));
  dim3 blk(256), grd((unsigned)((n + 255) / 256));
  hipLaunchKernelGGL(k_srs_to_mont<C>, grd, blk, 0, ctx->stream, d_canon, ctx->d_table, ctx->d_inf, (uint32_t)n);
  table_build<C>(ctx->d_table, ctx->d_inf, n, W, ctx->c, ctx->stream);
  KZGX_TRY_HIP(hipGetLastError());
  // the small-batch window table is built on first use (small_table_ready):
  // only table-off single calls and small batches read it, and a setup whose
  // calls all take the default table never pays its ~2.6 ms latency-bound
  // build (the reference benchmark's 128-term setup)
  ctx->n_small = 0;
  // the wide-window table of the large single MSMs (window 0 = the
  // Montgomery SRS, window 0 of the main table) -- not when a requested main
  // fixed-base table will cover every MSM of this SRS (its ~1.3 GB at 2^20
  // points would only shrink that table's budget), and freed when the SRS
  // no longer qualifies
  ctx->c_big = 0;
  const bool fixed_covers = ctx->fixed.c_req > 0 && ctx->fixed.n_req >= n;
  if (n < big_min_points() || fixed_covers) {
    if (ctx->d_table_big) (void)hipFree(ctx->d_table_big);
    ctx->d_table_big = nullptr;
    ctx->table_big_bytes = 0;
  } else {
    const int cb = big_window_bits(n, ctx->curve);
    const int WB = (257 + cb - 1) / cb;
    KZGX_TRY(dev_alloc(ctx, (void**)&ctx->d_table_big, (size_t)WB * n * pw, &ctx->table_big_bytes));
    KZGX_TRY_HIP(hipMemcpyAsync(ctx->d_table_big, ctx->d_table, n * pw, hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(k_table_build<C>, grd, blk, 0, ctx->stream, ctx->d_table_big, ctx->d_inf, (uint32_t)n, WB, cb);
    KZGX_TRY_HIP(hipGetLastError());
    ctx->c_big = cb;
  }
  ctx->n_srs = n;
  return fixed_build(ctx, d_canon, n);
}

// bucket sums + fold (+ affine conversion) of a batch, J buckets per
// bucket-sum thread
template <class C, uint32_t NB, uint32_t J>
static int bucket_reduce(Ctx* ctx, MsmWs& ws, size_t batch, hipStream_t st, uint32_t* d_out, uint32_t* d_out_inf,
                         uint32_t* xyzz_out) {
  constexpr uint32_t T1 = NB / J;
  static_assert(T1 >= 64 && T1 % 64 == 0, "k_msm_bucket_fold: whole (R, T) pairs per lane");
  dim3 blk(256);
  hipLaunchKernelGGL((k_msm_bucket_sums<C, J>), dim3((T1 + 255) / 256, (unsigned)batch), blk, 0, st, ws.offsets, NB,
                     ws.bsum, ws.rt);
  // workgroup fold (affine conversion inline) for small batches, where four
  // wavefronts per MSM are what fills the chip; from 256 MSMs the
  // one-wavefront fold + thread-per-MSM finish is faster (measured, BN254
  // c = 12: B = 128 wg +2.4%; B = 512 wave +2.8%; B = 2048 wave +6.7%,
  // profiles/r02_s3_pip_fold_ab.json)
  if (T1 % FOLD_WG == 0 && batch < 256) {
    hipLaunchKernelGGL((k_msm_bucket_fold_wg<C, J>), dim3((unsigned)batch), dim3(FOLD_WG), 0, st, ws.rt, T1, xyzz_out,
                       d_out, d_out_inf);
    KZGX_TRY_HIP(hipGetLastError());
    return KZGX_OK;
  }
  // the fold's XYZZ results go to xyzz_out (chunked callers) or to the
  // start of bsum, which the fold no longer reads
  uint32_t* vx = xyzz_out ? xyzz_out : ws.bsum;
  hipLaunchKernelGGL((k_msm_bucket_fold<C, J>), dim3((unsigned)((batch + 3) / 4)), blk, 0, st, ws.rt, T1,
                     (uint32_t)batch, vx);
  if (!xyzz_out)
    hipLaunchKernelGGL(k_msm_finish<C>, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, st, vx, (uint32_t)batch,
                       d_out, d_out_inf);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

// entries per accumulation thread: the context's segment length, halved
// (down to 8) while the grid would hold fewer than ~128k threads, so a
// single or small batch of MSMs still spreads over the chip
static uint32_t segment_len(const Ctx* ctx, size_t total_entries) {
  uint32_t K = ctx->seg_k;
  while (K > 8 && total_entries / K < 131072) K >>= 1;
  return K;
}

// latency.hip: the segment merge with inlined additions (memory clauses off)
int big_merge_inline(int curve, const uint32_t* heads, const uint32_t* tails, const uint32_t* tailk,
                     const uint8_t* sstate, uint32_t smax, uint32_t nb, uint32_t nwg, uint32_t* bsum, uint32_t* ghead,
                     uint32_t* gtail, uint32_t* gtailk, uint32_t* gflag, hipStream_t st);

enum class Merge { Called, Inline };  // k_msm_merge | big_merge_inline (one bucket set)

// Passes 4 and 4b of every Pippenger whose sort left `batch` bucket sets of up
// to emax entries in ws.entries / ws.offsets: K entries per accumulation
// thread from the rows of `table` (span accum_span), then the merge of the
// bucket partials that cross segments and workgroups into ws.bsum.  The merge
// opens the caller's span `reduce` (named reduce_span), which the caller
// keeps open over its bucket reduction.
// heads / tails / tailk / sstate: per-segment partials; gpart (ghead | gtail
// points) and gmeta (gtailk | gflag): the workgroup-crossing ones.
template <class C>
static int accum_stage(Ctx* ctx, MsmWs& ws, size_t batch, size_t emax, uint32_t NB, const uint32_t* table, uint32_t K,
                       hipStream_t st, Merge merge, const char* accum_span, const char* reduce_span,
                       std::optional<ProfScope>& reduce) {
  constexpr size_t XW = xyzz_words<C>(), XB = XW * sizeof(uint32_t);
  const size_t smax = (emax + K - 1) / K;
  const size_t nwg = (smax + ACC_WG - 1) / ACC_WG;
  if (batch > 65535 || nwg > 65535) return KZGX_ERR_ARG;  // grid limits
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.bsum, batch * NB * XB, &ws.bsum_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.heads, batch * smax * XB, &ws.heads_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.tails, batch * smax * XB, &ws.tails_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.tailk, batch * smax * 4, &ws.tailk_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.sstate, batch * smax, &ws.sstate_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.gpart, batch * nwg * 2 * XB, &ws.gpart_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.gmeta, batch * nwg * 2 * 4, &ws.gmeta_b));
  uint32_t* ghead = ws.gpart;
  uint32_t* gtail = ws.gpart + batch * nwg * XW;
  uint32_t* gtailk = ws.gmeta;
  uint32_t* gflag = ws.gmeta + batch * nwg;
  {
    ProfScope p(ctx, st, accum_span);
    hipLaunchKernelGGL(k_msm_accum<C>, dim3((unsigned)((smax + 255) / 256), (unsigned)batch), dim3(256), 0, st,
                       ws.entries, emax, ws.offsets, NB, table, K, (uint32_t)smax, ws.bsum, ws.heads, ws.tails,
                       ws.tailk, ws.sstate);
  }
  reduce.emplace(ctx, st, reduce_span);
  if (merge == Merge::Inline)
    KZGX_TRY(big_merge_inline(ctx->curve, ws.heads, ws.tails, ws.tailk, ws.sstate, (uint32_t)smax, NB, (uint32_t)nwg,
                              ws.bsum, ghead, gtail, gtailk, gflag, st));
  else
    hipLaunchKernelGGL(k_msm_merge<C>, dim3((unsigned)nwg, (unsigned)batch), dim3(ACC_WG), 0, st, ws.heads, ws.tails,
                       ws.tailk, ws.sstate, (uint32_t)smax, NB, (uint32_t)nwg, ws.bsum, ghead, gtail, gtailk, gflag);
  hipLaunchKernelGGL(k_msm_wg_fixup<C>, dim3((unsigned)((nwg + 63) / 64), (unsigned)batch), dim3(64), 0, st, NB,
                     (uint32_t)nwg, ghead, gtail, gtailk, gflag, ws.bsum);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

template <class C, int CB>
int msm_batch_impl(Ctx* ctx, const uint32_t* d_scalars, size_t n, size_t batch, size_t stride_words, uint32_t* d_out,
                   uint32_t* d_out_inf, hipStream_t st, uint32_t point_base, uint32_t point_stride,
                   uint32_t* xyzz_out, const uint32_t* d_tab, size_t n_rows) {
  constexpr int W = Win<CB>::W;
  constexpr uint32_t NB = Win<CB>::NB;
  const size_t emax = (size_t)n * W;
  const uint32_t K = segment_len(ctx, batch * emax);
  const size_t nblk = (n + SORT_BLK - 1) / SORT_BLK;
  const size_t XB = xyzz_words<C>() * sizeof(uint32_t);
  if (batch > 65535 || nblk > 65535) return KZGX_ERR_ARG;  // grid limits of the sort
  WsLease wsp = ctx->ws_for(st);
  if (!wsp) return KZGX_ERR_ARG;  // workspace binding failed (device sync error)
  MsmWs& ws = *wsp;
  // counts: per-(MSM, count block) histograms; cursors: their write bases
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.counts, batch * nblk * NB * 4, &ws.counts_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.cursors, batch * nblk * NB * 4, &ws.cursors_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.offsets, batch * (NB + 1) * 4, &ws.offsets_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.entries, batch * emax * 4, &ws.entries_b));
  const bool small = batch <= KZGX_SMALL_BATCH_J;
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.rt, batch * (NB / (small ? RED_J_SMALL : RED_J)) * 2 * XB, &ws.rt_b));
  const SrsSrc src{stride_words, point_base, point_stride, (uint32_t)n_rows, emax};
  dim3 blk(256);
  dim3 gs((unsigned)nblk, (unsigned)batch);
  {
    ProfScope p(ctx, st, "msm_count");
    hipLaunchKernelGGL((k_msm_count<CB, SrsSrc>), gs, blk, 0, st, src, d_scalars, (uint32_t)n, ctx->d_inf, ws.counts,
                       (uint32_t)nblk);
  }
  {
    ProfScope p(ctx, st, "msm_scan");
    hipLaunchKernelGGL(k_msm_scan<CB>, dim3((unsigned)batch), blk, 0, st, ws.counts, (uint32_t)nblk, ws.offsets,
                       ws.cursors);
  }
  {
    ProfScope p(ctx, st, "msm_scatter");
    hipLaunchKernelGGL((k_msm_scatter<CB, SrsSrc>), gs, blk, 0, st, src, d_scalars, (uint32_t)n, ctx->d_inf, ws.counts,
                       ws.cursors, (uint32_t)nblk, ws.entries);
  }
  std::optional<ProfScope> reduce;
  KZGX_TRY(accum_stage<C>(ctx, ws, batch, emax, NB, d_tab, K, st, Merge::Called, "msm_accum", "msm_reduce", reduce));
  if (small) return bucket_reduce<C, NB, RED_J_SMALL>(ctx, ws, batch, st, d_out, d_out_inf, xyzz_out);
  return bucket_reduce<C, NB, RED_J>(ctx, ws, batch, st, d_out, d_out_inf, xyzz_out);
}

// window 0 of the small table is the Montgomery SRS prefix (window 0 of the
// main table); k_table_build derives the others.  Built on the calling
// stream and ordered by an event: every later call waits on it on the
// device, so calls on other streams never see it half built and no _device
// entry point blocks the host (it was a stream sync).
template <class C>
static int small_table_ready(Ctx* ctx, hipStream_t st) {
  if (ctx->n_small) {
    if (ctx->small_ev) KZGX_TRY_HIP(hipStreamWaitEvent(st, ctx->small_ev, 0));
    return KZGX_OK;
  }
  if (ctx->c == KZGX_SMALL_WINDOW_BITS || !ctx->n_srs || !ctx->d_table) return KZGX_OK;
  const size_t pw = affine_words<C>() * sizeof(uint32_t);
  const size_t ns = ctx->n_srs < SMALL_MAX_POINTS ? ctx->n_srs : SMALL_MAX_POINTS;
  constexpr int WS = Win<KZGX_SMALL_WINDOW_BITS>::W;
  if (!ctx->small_ev) KZGX_TRY_HIP(hipEventCreateWithFlags(&ctx->small_ev, hipEventDisableTiming));
  KZGX_TRY(dev_alloc(ctx, (void**)&ctx->d_table_small, (size_t)WS * ns * pw, &ctx->table_small_bytes));
  KZGX_TRY_HIP(hipMemcpyAsync(ctx->d_table_small, ctx->d_table, ns * pw, hipMemcpyDeviceToDevice, st));
  table_build<C>(ctx->d_table_small, ctx->d_inf, ns, WS, KZGX_SMALL_WINDOW_BITS, st);
  KZGX_TRY_HIP(hipGetLastError());
  KZGX_TRY_HIP(hipEventRecord(ctx->small_ev, st));
  ctx->n_small = ns;
  return KZGX_OK;
}

template <class C>
static int msm_batch_c(Ctx* ctx, const uint32_t* d_scalars, size_t n, size_t batch, size_t stride_words,
                       uint32_t* d_out, uint32_t* d_out_inf, hipStream_t st, uint32_t point_base,
                       uint32_t point_stride, uint32_t* xyzz_out) {
  // small batches inside the small table's prefix: the short-reduction window
  const size_t last = (size_t)point_base + (batch ? (batch - 1) * (size_t)point_stride : 0) + n;
  if (batch <= ctx->small_batch && last <= SMALL_MAX_POINTS) KZGX_TRY(small_table_ready<C>(ctx, st));
  if (ctx->n_small && batch <= ctx->small_batch && last <= ctx->n_small)
    return msm_batch_impl<C, KZGX_SMALL_WINDOW_BITS>(ctx, d_scalars, n, batch, stride_words, d_out, d_out_inf, st,
                                                     point_base, point_stride, xyzz_out, ctx->d_table_small,
                                                     ctx->n_small);
  const uint32_t* T = ctx->d_table;
  const size_t R = ctx->n_srs;
  switch (ctx->c) {
    case 10: return msm_batch_impl<C, 10>(ctx, d_scalars, n, batch, stride_words, d_out, d_out_inf, st, point_base, point_stride, xyzz_out, T, R);
    case 11: return msm_batch_impl<C, 11>(ctx, d_scalars, n, batch, stride_words, d_out, d_out_inf, st, point_base, point_stride, xyzz_out, T, R);
    case 12: return msm_batch_impl<C, 12>(ctx, d_scalars, n, batch, stride_words, d_out, d_out_inf, st, point_base, point_stride, xyzz_out, T, R);
    case 13: return msm_batch_impl<C, 13>(ctx, d_scalars, n, batch, stride_words, d_out, d_out_inf, st, point_base, point_stride, xyzz_out, T, R);
    default: return KZGX_ERR_INTERNAL;
  }
}


// One large MSM is cut into chunks of MSM_CHUNK points that run as a batch
// of independent MSMs over consecutive SRS ranges (point_stride), each
// reduced to an XYZZ partial, then summed by one workgroup.  Every chunk has
// the bucket occupancy the batched path is tuned for, so a degree-2^20
// commitment fills the chip instead of waiting on 2^(c-1) very long buckets.
constexpr size_t MSM_CHUNK = 4096;

template <class C>
static int msm_single_chunked(Ctx* ctx, const uint32_t* d_scalars, size_t n, uint32_t* d_out, uint32_t* d_out_inf,
                              hipStream_t st) {
  const size_t XB = xyzz_words<C>() * sizeof(uint32_t);
  const size_t full = n / MSM_CHUNK, rest = n % MSM_CHUNK;
  const size_t parts = full + (rest ? 1 : 0);
  WsLease ws = ctx->ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  KZGX_TRY(dev_alloc(ctx, (void**)&ws->parts, parts * XB, &ws->parts_b));
  uint32_t* parts_buf = ws->parts;
  if (full)
    KZGX_TRY(msm_batch_c<C>(ctx, d_scalars, MSM_CHUNK, full, MSM_CHUNK * 8, d_out, d_out_inf, st, 0, MSM_CHUNK,
                            parts_buf));
  if (rest) {
    // the tail chunk: a batch of one over SRS points [full * CHUNK, n)
    KZGX_TRY(msm_batch_c<C>(ctx, d_scalars + full * MSM_CHUNK * 8, rest, 1, rest * 8, d_out, d_out_inf, st,
                            (uint32_t)(full * MSM_CHUNK), 0, parts_buf + full * xyzz_words<C>()));
  }
  {
    ProfScope p(ctx, st, "msm_reduce");
    hipLaunchKernelGGL(k_xyzz_sum<C>, dim3(1), dim3(256), 256 * XB, st, parts_buf, (uint32_t)parts, d_out, d_out_inf);
  }
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

template <class C, int CB>
static int msm_big_impl(Ctx* ctx, const uint32_t* d_scalars, size_t n, uint32_t* d_out, uint32_t* d_out_inf,
                        hipStream_t st, uint32_t* xyzz_out) {
  constexpr int W = Win<CB>::W;
  constexpr uint32_t NB = Win<CB>::NB;
  const size_t emax = (size_t)n * W;
  // count / scatter blocks of 2048 scalars: each thread ranks two scalars'
  // digits, so the LDS-atomic -> store chains stay short (~128 blocks of 8192
  // measured 215 us for the 2^20 scatter); the scan reads nblk NB counters
  const uint32_t per = 2048;
  const size_t nblk = (n + per - 1) / per;
  const uint32_t K = segment_len(ctx, emax);
  // KZGX_BIG_ONEPASS (set at all; tests/test_gpu_env_hooks.py): the one-pass
  // sort + called merge below, which otherwise needs an SRS above 2 M points
  static const bool one_pass = std::getenv("KZGX_BIG_ONEPASS") != nullptr;
  if (!one_pass && (size_t)W * ctx->n_srs < ((size_t)1 << BigFine<CB>::IDX) && n <= (size_t)65535 * 1536) {
    const uint32_t per2 = big2_per<CB>();
    const size_t nblk2 = (n + per2 - 1) / per2;
    const size_t XB = xyzz_words<C>() * sizeof(uint32_t);
    const size_t s_ub = emax / K + NB;  // segments: sum ceil(len_k / K) <= emax / K + NB
    WsLease wsp = ctx->ws_for(st);
    if (!wsp) return KZGX_ERR_ARG;
    MsmWs& ws = *wsp;
    KZGX_TRY(dev_alloc(ctx, (void**)&ws.counts, nblk2 * BIG_NC * 4, &ws.counts_b));
    // bases | tot | coff | segn | flag | segl
    KZGX_TRY(dev_alloc(ctx, (void**)&ws.cursors, ((nblk2 + 3) * BIG_NC + 2 + NB) * 4, &ws.cursors_b));
    KZGX_TRY(dev_alloc(ctx, (void**)&ws.offsets, (NB + 1) * 4, &ws.offsets_b));
    KZGX_TRY(dev_alloc(ctx, (void**)&ws.parts, emax * 4, &ws.parts_b));  // pass-1 entries
    KZGX_TRY(dev_alloc(ctx, (void**)&ws.entries, emax * 4, &ws.entries_b));
    KZGX_TRY(dev_alloc(ctx, (void**)&ws.rt, big_reduce_rt_bytes(ctx->curve, NB), &ws.rt_b));
    uint32_t* bases = ws.cursors;
    uint32_t* tot = bases + nblk2 * BIG_NC;
    uint32_t* coff = tot + BIG_NC;
    uint32_t* segn = coff + BIG_NC + 1;
    uint32_t* flag = segn + BIG_NC;
    uint32_t* segl = flag + 2;
    {
      ProfScope p(ctx, st, "msm_sort");
      hipLaunchKernelGGL(k_big2_count<CB>, dim3((unsigned)nblk2), dim3(BIG_TPB), 0, st, d_scalars, (uint32_t)n,
                         ctx->d_inf, per2, (uint32_t)nblk2, ws.counts);
      hipLaunchKernelGGL(k_big2_binscan, dim3(BIG_NC), dim3(256), 0, st, ws.counts, (uint32_t)nblk2, bases, tot);
      hipLaunchKernelGGL(k_scan1024, dim3(1), dim3(1024), 0, st, tot, coff);
      hipLaunchKernelGGL(k_big2_scatter<CB>, dim3((unsigned)nblk2), dim3(BIG_TPB), 0, st, d_scalars, (uint32_t)n,
                         ctx->d_inf, (uint32_t)nblk2, ws.counts, coff, bases, ws.parts, (uint32_t)ctx->n_srs);
      hipLaunchKernelGGL(k_big2_fine<CB>, dim3(BIG_NC), dim3(256), 0, st, ws.parts, coff, K, ws.entries, ws.offsets,
                         segl, segn);
    }
    // accumulation: K-entry segments across bucket boundaries with the
    // merge of crossing partials, or bucket-aligned segments summed by the
    // reduction (no merge, but measured 1.83 vs 1.31 ms of accumulation on
    // 2^20 + 1 points at the same VALU count and cache hit rate,
    // profiles/r05_big_msm_pmc.json -- an unexplained gap, left measured)
    // (bucket-aligned segments when K was cut to <= 32 to spread a smaller
    // MSM: buckets then span ~20 segments and the merge's chains dominate --
    // 131 073 points 0.64 vs 0.84 ms, while 2^20 + 1 points take 2.20 vs
    // 2.62 ms with the merge)
    if (K <= 32) {
      KZGX_TRY(dev_alloc(ctx, (void**)&ws.tailk, (NB + 1) * 4, &ws.tailk_b));  // seg_off
      KZGX_TRY(dev_alloc(ctx, (void**)&ws.heads, s_ub * XB, &ws.heads_b));     // segment partials
      uint32_t* seg_off = ws.tailk;
      hipLaunchKernelGGL(k_big2_segscan<CB>, dim3(1), dim3(1024), 0, st, segl, segn, seg_off, flag);
      {
        ProfScope p(ctx, st, "msm_accum");
        hipLaunchKernelGGL(k_big_accum<C>, dim3((unsigned)((s_ub + 255) / 256)), dim3(256), 0, st, ws.entries,
                           ws.offsets, seg_off, NB, ctx->d_table_big, K, ws.heads);
      }
      KZGX_TRY_HIP(hipGetLastError());
      ProfScope p(ctx, st, "msm_reduce");
      return big_reduce_seg(ctx->curve, seg_off, ws.heads, NB, (uint32_t)s_ub, flag, ws.rt, d_out, d_out_inf, st,
                            xyzz_out);
    }
    std::optional<ProfScope> reduce;
    KZGX_TRY(accum_stage<C>(ctx, ws, 1, emax, NB, ctx->d_table_big, K, st, Merge::Inline, "msm_accum", "msm_reduce",
                            reduce));
    return big_reduce(ctx->curve, ws.offsets, NB, ws.bsum, ws.rt, d_out, d_out_inf, st, xyzz_out);
  }
  // the one-pass sort's per-block LDS histograms hold NB counters: not at
  // c = 17 (256 KB); big_window_bits picks 17 only where the two-pass sort
  // above applies
  if constexpr (CB > 16) {
    return KZGX_ERR_INTERNAL;
  } else {
  if (nblk > 65535) return KZGX_ERR_ARG;
  WsLease wsp = ctx->ws_for(st);
  if (!wsp) return KZGX_ERR_ARG;
  MsmWs& ws = *wsp;
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.counts, nblk * NB * 4, &ws.counts_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.cursors, (nblk + 1) * NB * 4, &ws.cursors_b));  // bases | totals
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.offsets, (NB + 1) * 4, &ws.offsets_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.entries, emax * 4, &ws.entries_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.rt, big_reduce_rt_bytes(ctx->curve, NB), &ws.rt_b));
  uint32_t* tot = ws.cursors + nblk * NB;
  {
    ProfScope p(ctx, st, "msm_sort");
    hipLaunchKernelGGL(k_big_count<CB>, dim3((unsigned)nblk), dim3(BIG_TPB), 0, st, d_scalars, (uint32_t)n, ctx->d_inf,
                       per, ws.counts);
    hipLaunchKernelGGL(k_big_tot<CB>, dim3((NB + 255) / 256), dim3(256), 0, st, ws.counts, (uint32_t)nblk, tot);
    hipLaunchKernelGGL(k_big_scan<CB>, dim3(1), dim3(1024), 0, st, tot, ws.offsets);
    hipLaunchKernelGGL(k_big_bases<CB>, dim3((NB + 255) / 256), dim3(256), 0, st, ws.counts, (uint32_t)nblk,
                       ws.offsets, ws.cursors);
    hipLaunchKernelGGL(k_big_scatter<CB>, dim3((unsigned)nblk), dim3(BIG_TPB), 0, st, d_scalars, (uint32_t)n,
                       ctx->d_inf, per, ws.cursors, ws.entries, (uint32_t)ctx->n_srs);
  }
  std::optional<ProfScope> reduce;
  KZGX_TRY(accum_stage<C>(ctx, ws, 1, emax, NB, ctx->d_table_big, K, st, Merge::Called, "msm_accum", "msm_reduce",
                          reduce));
  return big_reduce(ctx->curve, ws.offsets, NB, ws.bsum, ws.rt, d_out, d_out_inf, st, xyzz_out);
  }
}

template <class C>
static int msm_big(Ctx* ctx, const uint32_t* d_scalars, size_t n, uint32_t* d_out, uint32_t* d_out_inf,
                   hipStream_t st, uint32_t* xyzz_out = nullptr) {
  switch (ctx->c_big) {
    case 12: return msm_big_impl<C, 12>(ctx, d_scalars, n, d_out, d_out_inf, st, xyzz_out);
    case 13: return msm_big_impl<C, 13>(ctx, d_scalars, n, d_out, d_out_inf, st, xyzz_out);
    case 14: return msm_big_impl<C, 14>(ctx, d_scalars, n, d_out, d_out_inf, st, xyzz_out);
    case 15: return msm_big_impl<C, 15>(ctx, d_scalars, n, d_out, d_out_inf, st, xyzz_out);
    case 16: return msm_big_impl<C, 16>(ctx, d_scalars, n, d_out, d_out_inf, st, xyzz_out);
    case 17: return msm_big_impl<C, 17>(ctx, d_scalars, n, d_out, d_out_inf, st, xyzz_out);
    default: return KZGX_ERR_INTERNAL;
  }
}

// --------------------------------------------------------------------------
// variable-base MSM over caller points (kzgx_msm_g1_points)
// --------------------------------------------------------------------------
// out = sum_k s_k P_k with no table of doublings: window w of every scalar
// goes to its OWN bucket set, so an MSM of n points with W windows is a batch
// of W bucket sets over one point table (the caller's points, converted to
// Montgomery form once per call).  n is cut into chunks of VAR_CHUNK points
// (the one-workgroup scan, as msm_single_chunked), so the batch is
// chunks x W bucket sets of at most VAR_CHUNK entries each: set b = ch W + w
// holds digit w of the scalars of chunk ch.  Every kernel of the batch is the
// batched Pippenger's: the sort (k_msm_count / k_msm_scan / k_msm_scatter)
// runs on PointSrc below, which emits one digit per (point, window), and
// accumulation, segment merge and the bucket running sums see one more batch
// of bucket sets over a table (accum_stage, bucket_reduce).  k_var_horner then sums
// the chunks of every window and folds sum_w 2^(c w) S_w by Horner's rule
// (c doublings a step, XYZZ, one affine conversion).  A window whose digits
// are all zero (the upper half for 128-bit scalars) has no entries: its
// accumulation threads exit, and Horner does not double an infinite prefix.
// Points repeat (one commitment opened at many points): the bucket additions
// are curve.hpp's complete formulas, P + P and P + (-P) included.
constexpr uint32_t VAR_SPT = 16;             // points per thread in count / scatter
constexpr uint32_t VAR_BLK = 256 * VAR_SPT;  // points per count block: one digit per point, so a block needs
                                             // this many to outweigh its 2^(c-1)-counter histogram row
constexpr size_t VAR_CHUNK = (size_t)1 << 17;
constexpr int VAR_MAX_W = Win<10>::W;

// caller points (canonical affine, optional uint32 infinity flags) -> Montgomery
template <class C>
__global__ void k_var_to_mont(const uint32_t* __restrict__ canon, const uint32_t* __restrict__ flags,
                              uint32_t* __restrict__ table, uint8_t* __restrict__ inf, uint32_t n) {
  constexpr int AW = affine_words<C>();
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Affine<C> a;
  bool finite = affine_from_canonical<C>(canon + (size_t)i * 2 * C::Fp::N, a);
  if (flags && flags[i]) finite = false;
  inf[i] = finite ? 0 : 1;
  affine_store<C>(table + (size_t)i * AW, a);
}

// signed digit w of a scalar (the recoding's carry chain runs from window 0)
template <int CB>
KZGX_DEV int var_digit(const uint32_t (&s)[8], int w) {
  uint32_t carry = 0;
  int mine = 0;
#pragma unroll
  for (int v = 0; v < Win<CB>::W; v++) {
    const int d = digit_at<CB>(s, v, carry);
    if (v == w) mine = d;
  }
  return mine;
}

// the sort's digit source (see SrsSrc): bucket set b = ch W + w gets digit w
// of point ch L + li, li < L; an entry is the point's row in ws.var_tab
struct PointSrc {
  static constexpr uint32_t SPT = VAR_SPT;
  static constexpr uint32_t digits_per_point(int) { return 1; }
  uint32_t L;  // points per chunk = entries per bucket set
  KZGX_DEV size_t entries_base(uint32_t b) const { return (size_t)b * L; }
  template <int CB, class F>
  KZGX_DEV void digits(const uint32_t* __restrict__ scalars, const uint8_t* __restrict__ inf, uint32_t n, uint32_t b,
                       uint32_t li, F emit) const {
    constexpr int W = Win<CB>::W;
    const uint32_t gi = b / W * L + li;
    if (li < L && gi < n && !inf[gi]) {
      uint32_t s[8];
      load_scalar(scalars + (size_t)gi * 8, s);
      const int d = var_digit<CB>(s, (int)(b % W));
      if (d != 0) emit(d, gi);
    }
  }
};

// parts[ch W + w]: the XYZZ sum of window w of chunk ch.  Thread w sums its
// window over the chunks; thread 0 then folds sum_w 2^(c w) S_w from the top
// window down and converts once.  chunks == 0 gives infinity.
template <class C>
__global__ __launch_bounds__(64) void k_var_horner(const uint32_t* __restrict__ parts, uint32_t chunks, int W, int c,
                                                   uint32_t* __restrict__ out, uint32_t* __restrict__ out_inf) {
  constexpr int XW = xyzz_words<C>();
  __shared__ uint32_t lds[VAR_MAX_W * XW];
  const int t = (int)threadIdx.x;
  if (t < W) {
    Xyzz<C> acc = xyzz_inf<C>();
    for (uint32_t ch = 0; ch < chunks; ch++) acc = xyzz_add<C>(acc, xyzz_load<C>(parts + ((size_t)ch * W + t) * XW));
    xyzz_store<C>(lds + t * XW, acc);
  }
  __syncthreads();
  if (t != 0) return;
  Xyzz<C> acc = xyzz_load<C>(lds + (W - 1) * XW);
#pragma unroll 1
  for (int w = W - 2; w >= 0; w--) {
    if (!xyzz_is_inf<C>(acc)) {
#pragma unroll 1
      for (int s = 0; s < c; s++) acc = xyzz_dbl<C>(acc);
    }
    acc = xyzz_add<C>(acc, xyzz_load<C>(lds + w * XW));
  }
  constexpr int N = C::Fp::N;
  uint32_t wx[N], wy[N];
  const bool fin = xyzz_to_canonical_lane<C>(acc, wx, wy);
#pragma unroll
  for (int k = 0; k < N; k++) {
    out[k] = wx[k];
    out[N + k] = wy[k];
  }
  *out_inf = fin ? 0u : 1u;
}

// The window for chunks of L points: the smallest modelled cost
// W(c) (L + 3 2^(c-1)) -- L mixed additions per window against a bucket
// reduction of 2 full additions (~1.5 mixed ones each) per bucket -- over the
// windows the batched kernels are built for.  KZGX_VAR_WINDOW pins it (A/B).
static int var_window_bits(size_t L) {
  static const int pin = std::getenv("KZGX_VAR_WINDOW") ? std::atoi(std::getenv("KZGX_VAR_WINDOW")) : 0;
  if (pin >= 10 && pin <= 13) return pin;
  int best = 10;
  size_t best_cost = ~(size_t)0;
  for (int c = 10; c <= 13; c++) {
    const size_t cost = (size_t)((257 + c - 1) / c) * (L + 3 * ((size_t)1 << (c - 1)));
    if (cost < best_cost) {
      best_cost = cost;
      best = c;
    }
  }
  return best;
}

// the chunks x W window sums of n table points into ws.var_parts
template <class C, int CB>
static int msm_points_impl(Ctx* ctx, MsmWs& ws, const uint32_t* d_scalars, size_t n, size_t L, size_t chunks,
                           hipStream_t st) {
  constexpr int W = Win<CB>::W;
  constexpr uint32_t NB = Win<CB>::NB;
  const size_t batch = chunks * W;
  const size_t emax = L;  // one digit per (point, window)
  const uint32_t K = segment_len(ctx, batch * emax);
  const size_t nblk = (L + VAR_BLK - 1) / VAR_BLK;
  const size_t XB = xyzz_words<C>() * sizeof(uint32_t);
  if (batch > 65535 || nblk > 65535) return KZGX_ERR_ARG;  // grid limits of the sort
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.counts, batch * nblk * NB * 4, &ws.counts_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.cursors, batch * nblk * NB * 4, &ws.cursors_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.offsets, batch * (NB + 1) * 4, &ws.offsets_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.entries, batch * emax * 4, &ws.entries_b));
  KZGX_TRY(dev_alloc(ctx, (void**)&ws.rt, batch * (NB / RED_J) * 2 * XB, &ws.rt_b));
  const PointSrc src{(uint32_t)L};
  dim3 blk(256);
  dim3 gs((unsigned)nblk, (unsigned)batch);
  {
    ProfScope p(ctx, st, "var_sort");
    hipLaunchKernelGGL((k_msm_count<CB, PointSrc>), gs, blk, 0, st, src, d_scalars, (uint32_t)n, ws.var_inf, ws.counts,
                       (uint32_t)nblk);
    hipLaunchKernelGGL(k_msm_scan<CB>, dim3((unsigned)batch), blk, 0, st, ws.counts, (uint32_t)nblk, ws.offsets,
                       ws.cursors);
    hipLaunchKernelGGL((k_msm_scatter<CB, PointSrc>), gs, blk, 0, st, src, d_scalars, (uint32_t)n, ws.var_inf,
                       ws.counts, ws.cursors, (uint32_t)nblk, ws.entries);
  }
  std::optional<ProfScope> reduce;
  KZGX_TRY(accum_stage<C>(ctx, ws, batch, emax, NB, ws.var_tab, K, st, Merge::Called, "var_accum", "var_reduce", reduce));
  return bucket_reduce<C, NB, RED_J>(ctx, ws, batch, st, nullptr, nullptr, ws.var_parts);
}

template <class C>
static int msm_points_c(Ctx* ctx, MsmWs& ws, const PointSeg* segs, int nseg, const uint32_t* d_scalars,
                        uint32_t* d_out, uint32_t* d_out_inf, hipStream_t st) {
  constexpr size_t PWB = affine_words<C>() * sizeof(uint32_t);
  const size_t XB = xyzz_words<C>() * sizeof(uint32_t);
  size_t n = 0;
  for (int k = 0; k < nseg; k++) n += segs[k].n;
  if (n > MSM_POINTS_MAX) return KZGX_ERR_ARG;
  const size_t L = n < VAR_CHUNK ? n : VAR_CHUNK;
  const size_t chunks = n ? (n + L - 1) / L : 0;
  const int c = var_window_bits(L);
  const int W = (257 + c - 1) / c;
  if (n) {
    KZGX_TRY(dev_alloc(ctx, (void**)&ws.var_tab, n * PWB, &ws.var_tab_b));
    KZGX_TRY(dev_alloc(ctx, (void**)&ws.var_inf, n, &ws.var_inf_b));
    KZGX_TRY(dev_alloc(ctx, (void**)&ws.var_parts, chunks * W * XB, &ws.var_parts_b));
    size_t at = 0;
    for (int k = 0; k < nseg; k++) {
      if (!segs[k].n) continue;
      hipLaunchKernelGGL(k_var_to_mont<C>, dim3((unsigned)((segs[k].n + 255) / 256)), dim3(256), 0, st, segs[k].xy,
                         segs[k].inf, ws.var_tab + at * affine_words<C>(), ws.var_inf + at, (uint32_t)segs[k].n);
      at += segs[k].n;
    }
    KZGX_TRY_HIP(hipGetLastError());
    switch (c) {
      case 10: KZGX_TRY((msm_points_impl<C, 10>(ctx, ws, d_scalars, n, L, chunks, st))); break;
      case 11: KZGX_TRY((msm_points_impl<C, 11>(ctx, ws, d_scalars, n, L, chunks, st))); break;
      case 12: KZGX_TRY((msm_points_impl<C, 12>(ctx, ws, d_scalars, n, L, chunks, st))); break;
      case 13: KZGX_TRY((msm_points_impl<C, 13>(ctx, ws, d_scalars, n, L, chunks, st))); break;
      default: return KZGX_ERR_INTERNAL;
    }
  }
  ProfScope p(ctx, st, "var_horner");
  hipLaunchKernelGGL(k_var_horner<C>, dim3(1), dim3(64), 0, st, ws.var_parts, (uint32_t)chunks, W, c, d_out,
                     d_out_inf);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

// ---- per-curve entry points ---------------------------------------------
// This file is compiled once per curve (Makefile: build/msm.o with
// KZGX_MSM_CURVE=BN254G1 and KZGX_MSM_MAIN, build/msm_bls.o with
// KZGX_MSM_CURVE=BLS12381G1): each object instantiates MsmCurve<C> -- every
// point-arithmetic kernel of one curve -- and only the main one holds the
// curve dispatch below, which reaches the other curve's object through
// MsmCurve's out-of-line members (extern template: no implicit
// instantiation here).  The two halves compile side by side (VERDICT r05,
// "build": this translation unit was a 6-minute serial step).
template <class C>
struct MsmCurve {
  static int srs_upload(Ctx* ctx, const uint32_t* d_canon, size_t n);
  static int batch(Ctx* ctx, const uint32_t* d_scalars, size_t n, size_t batch, size_t stride_words, uint32_t* d_out,
                   uint32_t* d_out_inf, hipStream_t st);
  static int chunked(Ctx* ctx, const uint32_t* d_scalars, size_t n, uint32_t* d_out, uint32_t* d_out_inf,
                     hipStream_t st);
  static int big(Ctx* ctx, const uint32_t* d_scalars, size_t n, uint32_t* d_out, uint32_t* d_out_inf, hipStream_t st,
                 uint32_t* xyzz_out);
  static int xyzz_sum(const uint32_t* d_parts, size_t count, uint32_t* d_out, uint32_t* d_out_inf, hipStream_t st);
  static int points(Ctx* ctx, MsmWs& ws, const PointSeg* segs, int nseg, const uint32_t* d_scalars, uint32_t* d_out,
                    uint32_t* d_out_inf, hipStream_t st);
};

template <class C>
int MsmCurve<C>::srs_upload(Ctx* ctx, const uint32_t* d_canon, size_t n) {
  return srs_upload_impl<C>(ctx, d_canon, n);
}
template <class C>
int MsmCurve<C>::batch(Ctx* ctx, const uint32_t* d_scalars, size_t n, size_t batch, size_t stride_words,
                       uint32_t* d_out, uint32_t* d_out_inf, hipStream_t st) {
  return msm_batch_c<C>(ctx, d_scalars, n, batch, stride_words, d_out, d_out_inf, st, 0, 0, nullptr);
}
template <class C>
int MsmCurve<C>::chunked(Ctx* ctx, const uint32_t* d_scalars, size_t n, uint32_t* d_out, uint32_t* d_out_inf,
                         hipStream_t st) {
  return msm_single_chunked<C>(ctx, d_scalars, n, d_out, d_out_inf, st);
}
template <class C>
int MsmCurve<C>::big(Ctx* ctx, const uint32_t* d_scalars, size_t n, uint32_t* d_out, uint32_t* d_out_inf,
                     hipStream_t st, uint32_t* xyzz_out) {
  return msm_big<C>(ctx, d_scalars, n, d_out, d_out_inf, st, xyzz_out);
}
template <class C>
int MsmCurve<C>::xyzz_sum(const uint32_t* d_parts, size_t count, uint32_t* d_out, uint32_t* d_out_inf,
                          hipStream_t st) {
  hipLaunchKernelGGL(k_xyzz_sum<C>, dim3(1), dim3(256), 256 * xyzz_words<C>() * 4, st, d_parts, (uint32_t)count,
                     d_out, d_out_inf);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

template <class C>
int MsmCurve<C>::points(Ctx* ctx, MsmWs& ws, const PointSeg* segs, int nseg, const uint32_t* d_scalars,
                        uint32_t* d_out, uint32_t* d_out_inf, hipStream_t st) {
  return msm_points_c<C>(ctx, ws, segs, nseg, d_scalars, d_out, d_out_inf, st);
}

#ifndef KZGX_MSM_CURVE
#error "msm.hip is compiled per curve: -DKZGX_MSM_CURVE=BN254G1|BLS12381G1 (see the Makefile)"
#endif
#ifdef KZGX_MSM_MAIN
extern template struct MsmCurve<BN254G1>;
extern template struct MsmCurve<BLS12381G1>;
#endif
template struct MsmCurve<KZGX_MSM_CURVE>;

#ifdef KZGX_MSM_MAIN
// ---- curve dispatch (main object only) ----------------------------------
int srs_upload(Ctx* ctx, const uint32_t* d_canon, size_t n) {
  return ctx->curve == KZGX_CURVE_BN254 ? MsmCurve<BN254G1>::srs_upload(ctx, d_canon, n)
                                        : MsmCurve<BLS12381G1>::srs_upload(ctx, d_canon, n);
}

bool window_bits_supported(int c) { return c >= 10 && c <= 13; }

int xyzz_sum(Ctx* ctx, const uint32_t* d_parts, size_t count, uint32_t* d_out, uint32_t* d_out_inf, hipStream_t st) {
  return ctx->curve == KZGX_CURVE_BN254 ? MsmCurve<BN254G1>::xyzz_sum(d_parts, count, d_out, d_out_inf, st)
                                        : MsmCurve<BLS12381G1>::xyzz_sum(d_parts, count, d_out, d_out_inf, st);
}

int msm_batch(Ctx* ctx, const uint32_t* d_scalars, size_t n, size_t batch, size_t stride_words, uint32_t* d_out,
              uint32_t* d_out_inf, hipStream_t st) {
  const bool bn = ctx->curve == KZGX_CURVE_BN254;
  if (fixed_usable(ctx, n)) return fixed_msm(ctx, d_scalars, n, batch, stride_words, d_out, d_out_inf, st, nullptr);
  // inside the default table's prefix: single calls and small batches take
  // its one-launch latency path (k_fixed_accum_lat) instead of eight
  // Pippenger launches whose bucket reduction is a ~20-addition chain;
  // larger batches its batched kernel when its window beats Pippenger
  {
    const FixedTable& d = ctx->fixed_def;
    const int min_c = ctx->curve == KZGX_CURVE_BN254 ? KZGX_DEFAULT_TABLE_BATCH_MIN_C_BN : KZGX_DEFAULT_TABLE_BATCH_MIN_C_BLS;
    // batch <= 16: the latency kernel (fixed_msm_impl), whatever the
    // small-window Pippenger knob (kzgx_set_small_batch) says
    if (fixed_table_usable(d, n) && (batch <= 16 || d.c >= min_c))
      return fixed_msm_table(ctx, ctx->fixed_def, d_scalars, n, batch, stride_words, d_out, d_out_inf, st, nullptr);
  }
// Single MSMs chunk from 2^17 points: below, one un-chunked Pippenger (the
// segment length shrinks to spread it) has one reduction level less; above,
// its one-workgroup scan over n / 512 count blocks serialises (measured,
// profiles/r02_chunk_threshold.json: 65 536 points 1.31 vs 1.74 ms,
// 2^23 points 76 vs 25 ms).
#ifndef KZGX_CHUNK_MIN
#define KZGX_CHUNK_MIN (32 * MSM_CHUNK)
#endif
  // one large MSM: the wide-window path (its table exists for SRSs of
  // >= big_min_points() points)
  if (batch == 1 && ctx->c_big && n >= big_min_points())
    return bn ? MsmCurve<BN254G1>::big(ctx, d_scalars, n, d_out, d_out_inf, st, nullptr)
              : MsmCurve<BLS12381G1>::big(ctx, d_scalars, n, d_out, d_out_inf, st, nullptr);
  if (batch == 1 && n >= KZGX_CHUNK_MIN)
    return bn ? MsmCurve<BN254G1>::chunked(ctx, d_scalars, n, d_out, d_out_inf, st)
              : MsmCurve<BLS12381G1>::chunked(ctx, d_scalars, n, d_out, d_out_inf, st);
  return bn ? MsmCurve<BN254G1>::batch(ctx, d_scalars, n, batch, stride_words, d_out, d_out_inf, st)
            : MsmCurve<BLS12381G1>::batch(ctx, d_scalars, n, batch, stride_words, d_out, d_out_inf, st);
}

int msm_points(Ctx* ctx, MsmWs& ws, const PointSeg* segs, int nseg, const uint32_t* d_scalars, uint32_t* d_out,
               uint32_t* d_out_inf, hipStream_t st) {
  return ctx->curve == KZGX_CURVE_BN254
             ? MsmCurve<BN254G1>::points(ctx, ws, segs, nseg, d_scalars, d_out, d_out_inf, st)
             : MsmCurve<BLS12381G1>::points(ctx, ws, segs, nseg, d_scalars, d_out, d_out_inf, st);
}

// One MSM left projective: the XYZZ sum of sum_i s_i SRS_i in d_rec
// (xyzz_record_words words), for callers that add it to other partials before
// the one affine conversion (the sharded commitment).  The paths
// that end in a reduction launch (the main table's few-MSM kernels, the
// wide-window Pippenger) store the XYZZ sum instead of inverting; the rest
// (single calls of <= 2^16 points: default table, chunked Pippenger) end in
// an affine point, lifted to a record.
int msm_partial_xyzz(Ctx* ctx, const uint32_t* d_scalars, size_t n, uint32_t* d_rec, hipStream_t st) {
  const bool bn = ctx->curve == KZGX_CURVE_BN254;
  if (fixed_usable(ctx, n)) return fixed_msm(ctx, d_scalars, n, 1, n * 8, nullptr, nullptr, st, d_rec);
  if (ctx->c_big && n >= big_min_points())
    return bn ? MsmCurve<BN254G1>::big(ctx, d_scalars, n, nullptr, nullptr, st, d_rec)
              : MsmCurve<BLS12381G1>::big(ctx, d_scalars, n, nullptr, nullptr, st, d_rec);
  const size_t pw = 2 * (size_t)(bn ? BN254G1::Fp::N : BLS12381G1::Fp::N);
  KZGX_TRY(dev_alloc(ctx, (void**)&ctx->d_lift, (pw + 4) * sizeof(uint32_t), &ctx->lift_b));
  KZGX_TRY(msm_batch(ctx, d_scalars, n, 1, n * 8, ctx->d_lift, ctx->d_lift + pw, st));
  return affine_to_xyzz(ctx->curve, ctx->d_lift, ctx->d_lift + pw, d_rec, st);
}

#endif  // KZGX_MSM_MAIN

}  // namespace kzgx

#ifdef KZGX_MSM_MAIN
namespace kzgx {
// device bring-up (kzgx_setup.hpp): one launch loads this code object
__global__ void k_warm_msm() {}
int warm_msm(hipStream_t st) {
  hipLaunchKernelGGL(k_warm_msm, dim3(1), dim3(64), 0, st);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}
}  // namespace kzgx
#endif  // KZGX_MSM_MAIN
