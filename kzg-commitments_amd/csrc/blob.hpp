// Blob proofs (blob.hip): host-side declarations shared with kzgx_api.hip.
#pragma once
#include "kzgx_internal.hpp"

namespace kzgx {

// a call's blobs run in chunks of at most this many field elements (one blob at least)
constexpr size_t BLOB_CHUNK_SCALARS = KZGX_BLOB_CHUNK_SCALARS;

// host arithmetic, no device: SHA-256, and the challenge of one blob (elements as
// canonical limbs, or 32-byte big-endian with bytes); *ok = 0 iff an element is >= r
void sha256_host(const uint8_t* msg, size_t len, uint8_t out[32]);
void blob_challenge_host(const void* blob, unsigned log2n, bool bytes, const uint8_t* record, uint64_t* z, int* ok);

// z[b] = H(blob_b || record_b) mod r, canonical words; ok[b] = 0 iff bytes and an
// element of blob b is >= r.  Blobs are packed, 2^log2n elements each.
int blob_challenges(Ctx* ctx, const void* d_blobs, unsigned log2n, size_t count, bool bytes, const uint8_t* d_records,
                    uint32_t* d_z, uint32_t* d_ok, hipStream_t st);
// y[k] = P_k(z[k]) by the barycentric formula, P_k given by its 2^log2n values at
// d_evals + k * eval_stride elements (0: one shared polynomial); the twiddle table of
// the size-2^log2n domain is built here (st ordered behind it).  d_frac: scratch of
// EVALS_AT_FRAC_BYTES per point (each workgroup's fraction, inverted by a second launch)
constexpr size_t EVALS_AT_FRAC_BYTES = 64;
int evals_at(Ctx* ctx, const void* d_evals, unsigned log2n, size_t eval_stride, bool bytes, bool bitrev,
             const uint32_t* d_z, size_t count, uint32_t* d_y, uint32_t* d_frac, hipStream_t st);
// big-endian bytes -> canonical limbs; ok[b] = 0 and all-zero limbs for a blob with an element >= r
int blob_decode(Ctx* ctx, const uint8_t* d_bytes, unsigned log2n, size_t count, uint32_t* d_out, uint32_t* d_ok,
                hipStream_t st);
// ok[k] &= a[k] & b[k] & c[k] (b, c may be null)
int blob_gate(uint32_t* d_ok, const uint32_t* d_a, const uint32_t* d_b, const uint32_t* d_c, size_t count,
              hipStream_t st);

}  // namespace kzgx
