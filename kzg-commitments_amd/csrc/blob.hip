// Blob proofs for gfx950 (include/kzg_gpu.h "blob proofs", DESIGN.md "Blob proofs"):
// the three kernels that keep a blob-level prove / verify on the device.
//
// k_blob_challenge  z_b = int_be(SHA-256(M_b)) mod r, one lane per blob.  The lane
//   walks its message (blob_msg.hpp: header, the blob's elements, the commitment
//   record, the padding) as a serial chain of (80 + 32 n) / 64 + 1 compressions;
//   an element is two 16-byte loads, turned into big-endian message words in
//   registers (a byte swap for KZGX_BLOB_BYTES, a word reversal for limbs) and
//   compared with r on the way.  SHA-256 is sha256.hpp's, the code the host helper
//   and the CPU tests run.
//
// k_evals_at  y = P(z) from P's values on the size-n domain, one workgroup per
//   (polynomial, point):  y = (z^n - 1) / n  sum_i f_i w^i / (z - w^i).  A lane owns
//   the terms i = tid, tid + 256, ... and folds them into ONE fraction N / D,
//     N <- N (z - w^i) + f_i w^i D,   D <- D (z - w^i)
//   -- three products a term and no inversion (Montgomery's trick with the running
//   product kept as the denominator instead of a stored prefix, so nothing is kept
//   per term and n may be 2^22).  The 256 fractions are added pairwise through LDS
//   (N1 D2 + N2 D1 over D1 D2) and the workgroup leaves its fraction in workspace.
//   A lane that meets z - w^i = 0 skips the term and publishes f_i, which is then
//   the answer, exactly (z^n - 1 = 0 kills every other term).  N and f are
//   canonical, D and the twiddles Montgomery values: canonical x Montgomery is
//   canonical, as in ntt.hip, so no conversion pass runs.  n = 1 and n < 256 leave
//   lanes at the neutral fraction 0 / 1.
// k_evals_at_finish  one lane per (polynomial, point): the ONE Fermat inversion a
//   fraction costs, and y = N / D (z^n - 1) / n.  A kernel of its own so that the
//   inversions of a batch run side by side instead of one lane of each workgroup
//   holding its CU slot for a 255-squaring chain (measured: DESIGN.md "Blob proofs").
//
// k_blob_decode  big-endian bytes -> canonical limbs plus a per-blob flag, for the
//   prove path only (its inverse NTT wants limbs); one workgroup per blob, a first
//   pass for the flag, a second that writes the limbs, or zeros for an invalid blob
//   (the zero polynomial: commitment and proof come out as the identity).
#include <hip/hip_runtime.h>

#include "blob.hpp"
#include "blob_msg.hpp"
#include "field.hpp"

namespace kzgx {

namespace {

// element i of a blob as 8 message words, most significant first
KZGX_DEV void blob_elem_be(const uint4* __restrict__ base, uint64_t i, bool bytes, uint32_t e[8]) {
  const uint4 a = base[2 * i], b = base[2 * i + 1];
  if (bytes) {
    e[0] = __builtin_bswap32(a.x);
    e[1] = __builtin_bswap32(a.y);
    e[2] = __builtin_bswap32(a.z);
    e[3] = __builtin_bswap32(a.w);
    e[4] = __builtin_bswap32(b.x);
    e[5] = __builtin_bswap32(b.y);
    e[6] = __builtin_bswap32(b.z);
    e[7] = __builtin_bswap32(b.w);
  } else {  // little-endian limbs: the words in reverse
    e[0] = b.w;
    e[1] = b.z;
    e[2] = b.y;
    e[3] = b.x;
    e[4] = a.w;
    e[5] = a.z;
    e[6] = a.y;
    e[7] = a.x;
  }
}

struct alignas(16) FrArg {
  uint32_t v[8];
};

}  // namespace

template <class FR>
__global__ __launch_bounds__(64) void k_blob_challenge(const uint4* __restrict__ blobs,
                                                       const uint8_t* __restrict__ records, uint32_t log2n,
                                                       uint32_t count, uint32_t bytes, uint32_t* __restrict__ z_out,
                                                       uint32_t* __restrict__ ok_out) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= count) return;
  const uint4* base = blobs + ((size_t)b << (log2n + 1));
  const uint8_t* rb = records + (size_t)b * 48;
  uint32_t rec[12];
#pragma unroll
  for (int j = 0; j < 12; j++)
    rec[j] = ((uint32_t)rb[4 * j] << 24) | ((uint32_t)rb[4 * j + 1] << 16) | ((uint32_t)rb[4 * j + 2] << 8) |
             (uint32_t)rb[4 * j + 3];
  const bool by = bytes != 0;  // uniform: a kernel argument
  uint32_t h[8], z[8];
  const bool ok = blob_digest(
      log2n, [&](uint64_t i, uint32_t* e) { blob_elem_be(base, i, by, e); }, rec, FR::P, h);
  blob_reduce(h, FR::P, z);
  uint32_t* o = z_out + (size_t)b * 8;
  reinterpret_cast<uint4*>(o)[0] = make_uint4(z[0], z[1], z[2], z[3]);
  reinterpret_cast<uint4*>(o)[1] = make_uint4(z[4], z[5], z[6], z[7]);
  if (ok_out) ok_out[b] = (ok || !by) ? 1u : 0u;
}

constexpr uint32_t EVALS_AT_THREADS = 256;

template <class FR>
__global__ __launch_bounds__(EVALS_AT_THREADS) void k_evals_at(const uint4* __restrict__ evals, size_t eval_stride,
                                                               uint32_t k, uint32_t bytes, uint32_t bitrev,
                                                               const uint32_t* __restrict__ table, uint32_t K,
                                                               const uint32_t* __restrict__ zs,
                                                               uint32_t* __restrict__ frac) {
  constexpr int N = FR::N;
  constexpr uint32_t T = EVALS_AT_THREADS;
  __shared__ alignas(16) uint32_t sh_n[T * N], sh_d[T * N], sh_found[N];
  __shared__ uint32_t sh_hit;
  const uint32_t tid = threadIdx.x, n = 1u << k;
  const size_t blk = blockIdx.x;
  if (tid == 0) sh_hit = 0;
  __syncthreads();
  const uint4* base = evals + blk * eval_stride * 2;
  const Fe<FR> zm = fe_to_mont<FR>(fe_load<FR>(zs + blk * N));
  const bool by = bytes != 0;
  Fe<FR> num = fe_zero<FR>(), den = fe_one<FR>();
  for (uint32_t p = tid; p < n; p += T) {
    const uint32_t e = (bitrev && k) ? __brev(p) >> (32 - k) : p;
    const Fe<FR> w = k == 0 ? fe_one<FR>() : ntt_tw<FR>(table, K, k, e, false);
    uint32_t be[8];
    blob_elem_be(base, p, by, be);
    Fe<FR> f;
#pragma unroll
    for (int j = 0; j < N; j++) f.v[j] = be[N - 1 - j];
    const Fe<FR> d = fe_sub<FR>(zm, w);
    if (fe_is_zero<FR>(d)) {  // z is this domain point: y = f, reduced (at most one lane, the w^i are distinct)
      fe_store<FR>(sh_found, fe_mul<FR>(f, fe_one<FR>()));
      sh_hit = 1;
    } else {
      const Fe<FR> a = fe_mul<FR>(f, w);
      num = fe_add<FR>(fe_mul<FR>(num, d), fe_mul<FR>(a, den));
      den = fe_mul<FR>(den, d);
    }
  }
  fe_store<FR>(sh_n + tid * N, num);
  fe_store<FR>(sh_d + tid * N, den);
  __syncthreads();
  for (uint32_t s = T / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const Fe<FR> n1 = fe_load<FR>(sh_n + tid * N), d1 = fe_load<FR>(sh_d + tid * N);
      const Fe<FR> n2 = fe_load<FR>(sh_n + (tid + s) * N), d2 = fe_load<FR>(sh_d + (tid + s) * N);
      fe_store<FR>(sh_n + tid * N, fe_add<FR>(fe_mul<FR>(n1, d2), fe_mul<FR>(n2, d1)));
      fe_store<FR>(sh_d + tid * N, fe_mul<FR>(d1, d2));
    }
    __syncthreads();
  }
  if (tid != 0) return;
  // the fraction N | D, or f_i | 0 on a domain point (D is a product of nonzero factors: never 0 otherwise)
  uint32_t* o = frac + blk * 2 * N;
  fe_store<FR>(o, sh_hit ? fe_load<FR>(sh_found) : fe_load<FR>(sh_n));
  fe_store<FR>(o + N, sh_hit ? fe_zero<FR>() : fe_load<FR>(sh_d));
}

template <class FR>
__global__ __launch_bounds__(64) void k_evals_at_finish(const uint32_t* __restrict__ frac, uint32_t k, FrArg ninv,
                                                        const uint32_t* __restrict__ zs, uint32_t count,
                                                        uint32_t* __restrict__ ys) {
  constexpr int N = FR::N;
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  const Fe<FR> num = fe_load<FR>(frac + (size_t)j * 2 * N), den = fe_load<FR>(frac + (size_t)j * 2 * N + N);
  const Fe<FR> sum = fe_mul<FR>(num, fe_inv<FR>(den));  // canonical
  Fe<FR> zn = fe_to_mont<FR>(fe_load<FR>(zs + (size_t)j * N));
  for (uint32_t i = 0; i < k; i++) zn = fe_sqr<FR>(zn);
  const Fe<FR> fac = fe_mul<FR>(fe_sub<FR>(zn, fe_one<FR>()), fe_const<FR>(ninv.v));  // (z^n - 1) / n
  fe_store<FR>(ys + (size_t)j * N, fe_is_zero<FR>(den) ? num : fe_mul<FR>(sum, fac));
}

template <class FR>
__global__ __launch_bounds__(256) void k_blob_decode(const uint4* __restrict__ bytes, uint32_t log2n,
                                                     uint32_t* __restrict__ out, uint32_t* __restrict__ ok) {
  const uint32_t tid = threadIdx.x, n = 1u << log2n;
  const size_t b = blockIdx.x;
  const uint4* base = bytes + (b << (log2n + 1));
  uint4* dst = reinterpret_cast<uint4*>(out) + (b << (log2n + 1));
  int bad = 0;
  for (uint32_t p = tid; p < n; p += 256) {
    uint32_t e[8];
    blob_elem_be(base, p, true, e);
    bad |= blob_words_lt(e, FR::P) ? 0 : 1;
  }
  bad = __syncthreads_or(bad);
  for (uint32_t p = tid; p < n; p += 256) {
    uint32_t e[8];
    blob_elem_be(base, p, true, e);
    dst[2 * (size_t)p] = bad ? make_uint4(0, 0, 0, 0) : make_uint4(e[7], e[6], e[5], e[4]);
    dst[2 * (size_t)p + 1] = bad ? make_uint4(0, 0, 0, 0) : make_uint4(e[3], e[2], e[1], e[0]);
  }
  if (tid == 0) ok[b] = bad ? 0u : 1u;
}

__global__ __launch_bounds__(256) void k_blob_gate(uint32_t* __restrict__ ok, const uint32_t* __restrict__ a,
                                                   const uint32_t* __restrict__ b, const uint32_t* __restrict__ c,
                                                   uint32_t count) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const uint32_t g = a[k] & (b ? b[k] : 1u) & (c ? c[k] : 1u);
  ok[k] = (ok[k] && g) ? 1u : 0u;
}

// --------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------
void sha256_host(const uint8_t* msg, size_t len, uint8_t out[32]) { sha256_bytes(msg, len, out); }

void blob_challenge_host(const void* blob, unsigned log2n, bool bytes, const uint8_t* record, uint64_t* z, int* ok) {
  using FR = BLS12381Fr;
  uint32_t rec[12], h[8], zw[8];
  for (int j = 0; j < 12; j++)
    rec[j] = ((uint32_t)record[4 * j] << 24) | ((uint32_t)record[4 * j + 1] << 16) |
             ((uint32_t)record[4 * j + 2] << 8) | (uint32_t)record[4 * j + 3];
  const uint8_t* pb = static_cast<const uint8_t*>(blob);
  const uint64_t* pl = static_cast<const uint64_t*>(blob);
  const bool good = blob_digest(
      log2n,
      [&](uint64_t i, uint32_t* e) {
        for (int j = 0; j < 8; j++) {
          if (bytes) {
            const uint8_t* q = pb + 32 * i + 4 * j;
            e[j] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3];
          } else {
            const uint64_t limb = pl[4 * i + (7 - j) / 2];
            e[j] = (uint32_t)(((7 - j) & 1) ? limb >> 32 : limb);
          }
        }
      },
      rec, FR::P, h);
  blob_reduce(h, FR::P, zw);
  for (int i = 0; i < 4; i++) z[i] = (uint64_t)zw[2 * i] | ((uint64_t)zw[2 * i + 1] << 32);
  if (ok) *ok = (good || !bytes) ? 1 : 0;
}

int blob_challenges(Ctx* ctx, const void* d_blobs, unsigned log2n, size_t count, bool bytes, const uint8_t* d_records,
                    uint32_t* d_z, uint32_t* d_ok, hipStream_t st) {
  if (ctx->curve != KZGX_CURVE_BLS12381 || (int)log2n > ntt_max_log2(ctx->curve)) return KZGX_ERR_ARG;
  if (count == 0) return KZGX_OK;
  if (!d_blobs || !d_records || !d_z || count > 0x7fffffffu) return KZGX_ERR_ARG;
  hipLaunchKernelGGL(k_blob_challenge<BLS12381Fr>, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, st,
                     (const uint4*)d_blobs, d_records, (uint32_t)log2n, (uint32_t)count, bytes ? 1u : 0u, d_z, d_ok);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int evals_at(Ctx* ctx, const void* d_evals, unsigned log2n, size_t eval_stride, bool bytes, bool bitrev,
             const uint32_t* d_z, size_t count, uint32_t* d_y, uint32_t* d_frac, hipStream_t st) {
  if (ctx->curve != KZGX_CURVE_BLS12381 || (int)log2n > ntt_max_log2(ctx->curve)) return KZGX_ERR_ARG;
  if (count == 0) return KZGX_OK;
  if (!d_evals || !d_z || !d_y || !d_frac || count > 0x7fffffffu) return KZGX_ERR_ARG;
  KZGX_TRY(ntt_twiddles(ctx, log2n, st));
  FrArg ninv;
  for (int w = 0; w < 8; w++) ninv.v[w] = BLS12381FrNtt::NINV_M[log2n][w];
  hipLaunchKernelGGL(k_evals_at<BLS12381Fr>, dim3((unsigned)count), dim3(EVALS_AT_THREADS), 0, st,
                     (const uint4*)d_evals, eval_stride, (uint32_t)log2n, bytes ? 1u : 0u, bitrev ? 1u : 0u,
                     (const uint32_t*)ctx->d_ntt_tw, (uint32_t)ctx->ntt_log2, d_z, d_frac);
  KZGX_TRY_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_evals_at_finish<BLS12381Fr>, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, st,
                     (const uint32_t*)d_frac, (uint32_t)log2n, ninv, d_z, (uint32_t)count, d_y);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int blob_decode(Ctx* ctx, const uint8_t* d_bytes, unsigned log2n, size_t count, uint32_t* d_out, uint32_t* d_ok,
                hipStream_t st) {
  if (ctx->curve != KZGX_CURVE_BLS12381 || (int)log2n > ntt_max_log2(ctx->curve)) return KZGX_ERR_ARG;
  if (count == 0) return KZGX_OK;
  if (!d_bytes || !d_out || !d_ok || count > 0x7fffffffu) return KZGX_ERR_ARG;
  hipLaunchKernelGGL(k_blob_decode<BLS12381Fr>, dim3((unsigned)count), dim3(256), 0, st, (const uint4*)d_bytes,
                     (uint32_t)log2n, d_out, d_ok);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

int blob_gate(uint32_t* d_ok, const uint32_t* d_a, const uint32_t* d_b, const uint32_t* d_c, size_t count,
              hipStream_t st) {
  if (count == 0) return KZGX_OK;
  if (!d_ok || !d_a || count > 0xffffffffu) return KZGX_ERR_ARG;
  hipLaunchKernelGGL(k_blob_gate, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, d_ok, d_a, d_b, d_c,
                     (uint32_t)count);
  KZGX_TRY_HIP(hipGetLastError());
  return KZGX_OK;
}

}  // namespace kzgx
