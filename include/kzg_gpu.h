/* kzg_gpu.h -- C ABI of the MI355X KZG engine (libkzgx.so).
 *
 * This is the drop-in boundary under the reference's C++ API
 * (kzg::trusted_setup, /root/reference/src/kzg.h:182-290).  The reference has
 * no FFI of its own; these entry points replace, one for one:
 *
 *   kzgx_msm_g1*            trusted_setup::polyeval_G1  src/trusted_setup.cpp:149-174
 *                           (private, declared src/kzg.h:187) -- the G1 MSM
 *                           behind create_commit (:137-142), verify_commit
 *                           (:144-147), create_proof (:227), verify_proof (:246)
 *   kzgx_quotient_single*   q = (P - I) / Z for one opening, trusted_setup.cpp:214-225
 *                           (chunk_length == 1: I = P(z), Z = X - z)
 *   kzgx_prove_single_batch create_proof(poly, z, 1) for many (poly, z) pairs
 *   kzgx_poly_eval          evaluate_polynomial_points, src/util.cpp:186-211
 *   kzgx_poly_interpolate   polyfit / linear_roots_and_polyfit, src/util.cpp:172-184
 *   kzgx_gen_srs_g1*        trusted_setup(int) G1 part, trusted_setup.cpp:21-74,123-135
 *   kzgx_load_srs_g1        trusted_setup(const string&) G1 part, trusted_setup.cpp:76-101
 *
 * and add what the reference does not have (each marked "extension" below):
 * aggregated verification, batched point validation, and the evaluation form --
 * kzgx_ntt*, kzgx_commit_evals_batch*, kzgx_prove_evals_batch*: a radix-2 Fr NTT
 * and commits / openings of polynomials given by their values on a power-of-two
 * domain of roots of unity (BLS12-381 up to 2^22 values; BN254 only up to 4);
 * kzgx_g1_ntt*, kzgx_prove_all_*: the same transform over G1 points, and all n
 * openings of a polynomial on its size-n domain in Theta(n log n) group operations;
 * kzgx_prove_cosets_*, kzgx_coset_points: one opening per coset (cell) of that
 * domain or of the twice larger one, all cosets at once;
 * kzgx_verify_cells_aggregate*: one pairing check for many such cells;
 * kzgx_verify_cells_each*: one verdict per cell of such a batch;
 * kzgx_sha256, kzgx_blob_challenge(s), kzgx_evals_at_batch*, kzgx_prove_blobs_batch*,
 * kzgx_verify_blobs_batch*, kzgx_verify_blobs_each* (flag KZGX_BLOB_BYTES): blob proofs --
 * the Fiat-Shamir challenge of a blob hashed on the device, the value of an
 * evaluation-form polynomial at any point, and blob-level prove / verify on 32-byte
 * big-endian scalars and compressed points;
 * kzgx_prove_multi_batch*, kzgx_verify_multi_batch*: batch openings -- many polynomials
 * opened at shared points with one proof per point (both curves);
 * kzgx_shplonk_commit*, kzgx_shplonk_open*, kzgx_shplonk_verify*: Shplonk openings -- many
 * polynomials opened at different point sets under one proof of two G1 points (both curves).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / HIP types in signatures
 *     (streams are passed as void*, NULL = the context's own stream);
 *   - scalars / Fr elements: 4 x uint64 little-endian, canonical (< r);
 *   - G1 points: canonical affine x || y, each coordinate W64 = 4 (BN254) or
 *     6 (BLS12-381) uint64 little-endian limbs; infinity is x = y = 0 (never
 *     on either curve since b != 0) and is also flagged in *_is_inf outputs;
 *   - "_device" entry points take device pointers and enqueue work
 *     asynchronously on the given stream; the others take host pointers and
 *     block until the result is on the host;
 *   - every function returns KZGX_OK (0) or a negative status; kzgx_strerror
 *     names it.  The C++ facade (include/kzg.h) maps statuses onto the
 *     reference's exception types.
 *   - one context per thread (contexts are not internally locked).
 *   - a context keeps MSM workspaces for up to 8 streams at once, so calls
 *     on different streams run concurrently; a 9th distinct stream takes
 *     over the least recently bound workspace after a device-wide
 *     synchronisation (correct, but serialising: reuse streams).
 */
#ifndef KZG_GPU_H
#define KZG_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KZGX_OK 0
#define KZGX_ERR_ARG -1        /* invalid argument (std::invalid_argument) */
#define KZGX_ERR_HIP -2        /* HIP runtime failure */
#define KZGX_ERR_OOM -3        /* device allocation failed */
#define KZGX_ERR_NO_SRS -4     /* no SRS loaded */
#define KZGX_ERR_DEGREE -5     /* more coefficients than SRS points */
#define KZGX_ERR_INTERNAL -6
#define KZGX_ERR_NO_DEVICE -7  /* no usable gfx950 device */
#define KZGX_ERR_DIV_ZERO -8   /* duplicate interpolation node (NTL: division by zero) */

#define KZGX_CURVE_BN254 0     /* miracl-core BN254 (Nogami), config/curve_BN254 */
#define KZGX_CURVE_BLS12381 1  /* BLS12-381, config/curve_BLS12381 */

typedef struct kzgx_ctx kzgx_ctx;

const char* kzgx_strerror(int status);
/* uint64 limbs per base-field coordinate (4 or 6), or -1 */
int kzgx_base_limbs(int curve);

/* Device bring-up for `curve` on `device`, meant to run once, outside any
 * timed region: HIP initialisation, every kernel code object of the library
 * loaded, and the per-process generator tables (comb tables of G1 and G2,
 * used by SRS generation and verify) built.  Replaces the device-independent
 * kzg::init of the reference (src/kzg.h:33-38, kzg.cpp init; its benchmark
 * calls it before timing, benchmark/benchmark.cpp:104).  Optional: without
 * it the first setup pays the same work. */
int kzgx_init_device(int curve, int device);
int kzgx_create(kzgx_ctx** out, int curve, int device);
void kzgx_destroy(kzgx_ctx* ctx);
int kzgx_sync(kzgx_ctx* ctx);
int kzgx_curve(const kzgx_ctx* ctx);
size_t kzgx_srs_size(const kzgx_ctx* ctx);
/* the context's own HIP stream (hipStream_t), used when stream == NULL */
void* kzgx_stream(kzgx_ctx* ctx);

/* per-kernel timing: when enabled, every launch of a named kernel
 * ("msm_count", "msm_scan", "msm_scatter", "msm_accum", "msm_reduce",
 * "quotient_single") is bracketed by HIP events on its launch stream;
 * kzgx_prof_read sums (and then drops) the records of one name. */
int kzgx_prof_enable(kzgx_ctx* ctx, int on);
int kzgx_prof_read(kzgx_ctx* ctx, const char* name, double* total_ms, int* count);
int kzgx_prof_clear(kzgx_ctx* ctx);

/* tuning: signed-digit window bits (10..13; default 12 or $KZGX_WINDOW_BITS),
 * settable only before the SRS is loaded; entries per accumulation thread */
int kzgx_set_window_bits(kzgx_ctx* ctx, int c);
int kzgx_set_segment(kzgx_ctx* ctx, unsigned k);
/* tuning: table-less MSM batches of at most max_batch MSMs (default 16; 0 =
 * never) over the first 65536 SRS points run at window 10 on a second window
 * table built with the SRS: a single commit's bucket reduction is a chain of
 * dependent additions as deep as the bucket count, so the shorter window
 * answers one call sooner (BN254 degree 4096: 0.545 vs 0.712 ms) */
int kzgx_set_small_batch(kzgx_ctx* ctx, unsigned max_batch);

/* fixed-base precomputation (the SRS is fixed for a trusted_setup's
 * lifetime): store M[w][i][j] = (j+1) 2^(c w) SRS[i] for the first n_points
 * SRS points, w < ceil((bits(r)+1)/c), j < 2^(c-1), affine (BN254: 64-B
 * packed words; BLS12-381: 112-B radix-2^29 limbs).  Every MSM with
 * n <= n_points then runs as a plain sum of table points (no bucket sort /
 * reduction).  Built now if an SRS is installed, else when one is; rebuilt
 * on every SRS change.  c = 0 turns it off (Pippenger for every MSM).
 * c in {4, 7..17}; BN254 c = 17 over 4097 points (15 windows) takes
 * 257.8 GB of device memory, c = 16 137.5 GB. */
int kzgx_set_fixed_base(kzgx_ctx* ctx, int c, size_t n_points);
/* table layout for the next build: -1 = automatic (the default: point-major
 * M[i][w][j] for c <= 12, where the few-large-MSM kernel walks one point's
 * windows in order; window-major M[w][i][j] above), 0 = window-major,
 * 1 = point-major.  Results are identical; only speed differs (DESIGN.md
 * section 3).  Extension with no reference counterpart. */
int kzgx_set_fixed_base_layout(kzgx_ctx* ctx, int layout);
/* the default table (extension, no reference counterpart): odd multiples at
 * window c over the first n_points SRS points, built with every SRS load.
 * c = -1 (the default) picks the widest c <= 12 whose table fits 4.5% of the
 * device memory and its free memory less 4 GiB: over 4097 points BN254
 * c = 12 (11.8 GB), BLS12-381 c = 11 (9.7 GB) on an MI355X.  MSMs that fit in
 * it and that the main table (kzgx_set_fixed_base) does not serve take it:
 * batches of at most kzgx_set_small_batch MSMs (single create_commit /
 * create_proof calls) its one-launch path, larger batches its batched
 * kernel when c >= 10 (BN254) / 11 (BLS12-381), below which the batched
 * Pippenger is as fast.  c = 0 turns it off (every such MSM then runs the
 * table-less Pippenger, as the reference allocates nothing beyond the SRS);
 * c in {4, 7..17} fixes the window.  Rebuilt at once when an SRS is
 * installed. */
int kzgx_set_default_table(kzgx_ctx* ctx, int c, size_t n_points);
int kzgx_default_table_info(const kzgx_ctx* ctx, int* c, size_t* n_points, size_t* bytes);
/* Contexts on one device whose SRS begins with the same n_points points (word
 * for word) share one default table, counted by reference: the last context
 * using it frees it.  *count / *bytes: the shared default tables live on
 * `device` and their device bytes.  Extension, no reference counterpart. */
int kzgx_shared_tables(int device, size_t* count, size_t* bytes);
/* Freed table blocks of 64 MB .. 32 GB are kept per device (32 GB in all)
 * for later table builds, since the driver wipes released VRAM before reuse
 * ("SRS").  They are released when the last context of
 * the device is destroyed, on an allocation failure, or by this call. */
int kzgx_release_cached_memory(int device);
/* layout of the built table: *point_major = 1 (M[i][w][j]) or 0 (M[w][i][j]) */
int kzgx_fixed_base_layout(const kzgx_ctx* ctx, int* point_major);
/* built table: the window bits asked for (0 = none), points covered, device
 * bytes of everything built for them (the window and the block table) */
int kzgx_fixed_base_info(const kzgx_ctx* ctx, int* c, size_t* n_points, size_t* bytes);
/* The block table (extension, no reference counterpart).
 * kzgx_set_fixed_base(c, n) means "the fastest fixed-base tables inside
 * kzgx_fixed_base_bytes(c, n)": from 1024 tabled points on it builds a table
 * of the signed subset sums of blocks of g consecutive SRS points (2^(g-1)
 * entries per block, the widest g <= 25 that leaves room) beside a window
 * table at the widest c' <= c that fits the rest -- BN254 c = 17 over 4097
 * points: g = 25 (176.1 GB) + c' = 15 (73.0 GB).  Batches of >= 64 MSMs with
 * n <= n_points then cost ceil(n / g) bits(r) mixed additions per MSM and one
 * shared pass of bits(r) doublings instead of n ceil(bits(r) / c); single
 * calls, batches below 64 and XYZZ partial records stay on the window table.
 * g = -1: that automatic choice (the default, or $KZGX_FIXED_JOINT read at
 * kzgx_create); 0: no block table, the window table at c alone; 2..25: that
 * block size at any n_points, serving every batch >= 1 (tests), KZGX_ERR_ARG
 * if it does not fit the footprint.  Rebuilds at once when a table is set. */
int kzgx_set_fixed_joint(kzgx_ctx* ctx, int g);
/* built block table: block size (0 = none), blocks, device bytes */
int kzgx_fixed_joint_info(const kzgx_ctx* ctx, int* g, size_t* blocks, size_t* bytes);
/* built window table: its own window bits (<= the request) and device bytes */
int kzgx_fixed_window_info(const kzgx_ctx* ctx, int* c, size_t* bytes);
/* block ranges per MSM of the block table's accumulation (each lane sums
 * blocks / ranges entries and the Horner pass folds ranges times the
 * partials; 0 = automatic: 1; <= 8; $KZGX_FIXED_JOINT_RANGES at kzgx_create) */
int kzgx_set_fixed_joint_ranges(kzgx_ctx* ctx, unsigned ranges);
/* Residency reserve of the block table's accumulation: wave slots per CU
 * that its launches leave free, so that the tail passes of a call on another
 * stream (Horner stages, finish, the quotient) find registers beside it
 * instead of waiting for a residency boundary.  Held by an unused dynamic
 * LDS size per workgroup, the smallest for which the device's occupancy
 * query answers r workgroups fewer; the kernel and its results are the same
 * at every r.  r = 0: none (the plain launch); r = -1: the curve's default
 * (the default, or $KZGX_FIXED_ACCUM_RESERVE read at kzgx_create); an r
 * beyond what 64 KiB of dynamic LDS can hold back is clamped (at least one
 * workgroup per CU stays); r < -1: KZGX_ERR_ARG.  Takes effect with the next
 * call. */
int kzgx_set_fixed_accum_reserve(kzgx_ctx* ctx, int r);
/* the request (-1 = default), the reserve in effect for the accumulation
 * kernel the next call launches, the dynamic LDS bytes per workgroup that
 * hold it (0 with no reserve), and which kernel that is: bit 0 = the one that
 * tests for table entries at infinity (the built table has some), bit 1 =
 * the endomorphism split's.  Only the split's tail is fitted to the room a
 * reserve leaves (stage 2 in half-wavefront workgroups, the tail kernels'
 * issue priority); with KZGX_FIXED_JOINT_GLV=0 a reserve holds the slots
 * back but stage 2 keeps its full LDS and still waits for a residency. */
int kzgx_fixed_accum_reserve_info(const kzgx_ctx* ctx, int* request, int* reserve, size_t* lds_bytes, int* variant);
/* device bytes a table of window c over n_points would take (no context) */
int kzgx_fixed_base_bytes(int curve, int c, size_t n_points, size_t* bytes);
/* bounded-memory precompute: the widest supported window c <= 17 whose
 * table over n_points fits budget_bytes AND the device's free memory
 * (less a 4 GiB margin for workspaces); builds it (as kzgx_set_fixed_base)
 * and returns it in *c_out, or installs no table (*c_out = 0: every MSM on
 * Pippenger) when even c = 7 does not fit.  n_points is clamped to the
 * installed SRS; KZGX_ERR_NO_SRS before one is loaded (the free-memory
 * check needs the SRS and its window tables in place).  Extension with no
 * reference counterpart: trusted_setup::precompute_budget. */
int kzgx_set_fixed_base_budget(kzgx_ctx* ctx, size_t budget_bytes, size_t n_points, int* c_out);
/* SRS points summed per accumulation thread on the fixed-base path
 * (0 = automatic, the default: 16 for batches of >= 64 MSMs, else enough
 * threads to fill the GPU, with a wavefront-level fold for single MSMs).
 * Ignored by calls the block table serves: their lanes are bit planes. */
int kzgx_set_fixed_points_per_thread(kzgx_ctx* ctx, unsigned p);
/* measurement: mixed additions per second of the MSM accumulation loop
 * (the XYZZ mixed add k_fixed_accum inlines, same waves per SIMD) on
 * L1-resident operands over the whole GPU -- the VALU ceiling the bench's
 * valu_roofline divides by.  Needs an SRS (its first points are the operands). */
int kzgx_microbench_mixed_add(kzgx_ctx* ctx, double* adds_per_s);
/* measurement: the hardware issue ceiling of v_mad_u64_u32 (lane
 * operations per second; 8 independent chains per lane, whole GPU) -- the
 * denominator of the bench's mad_issue roofline */
int kzgx_microbench_mad_u64(kzgx_ctx* ctx, double* lane_ops_per_s);
/* the same, plus the core clock (GHz) the ceiling ran at: one lane of the
 * launch counts core clocks against the constant-rate wall clock */
int kzgx_microbench_mad_u64_clock(kzgx_ctx* ctx, double* lane_ops_per_s, double* core_ghz);
/* measurement: enqueue on stream (NULL = the context's) a one-wavefront
 * probe that spins for spin_us of wall time and writes three uint64 to the
 * device buffer d_out: core clocks elapsed, wall ticks elapsed, wall clock
 * rate (kHz).  Enqueued beside a running batch it reads that batch's clock
 * (the DVFS clock is one per device); it occupies one wave slot. */
int kzgx_clock_probe(kzgx_ctx* ctx, void* stream, unsigned spin_us, void* d_out);

/* ---- SRS ---------------------------------------------------------------- */
/* upload n canonical affine points as the G1 SRS (replaces any previous one) */
int kzgx_load_srs_g1(kzgx_ctx* ctx, const uint64_t* xy, size_t n);
/* generate [tau^(start+i)] G1, i < n, on the GPU and install it as the SRS */
int kzgx_gen_srs_g1(kzgx_ctx* ctx, const uint64_t* tau, size_t start, size_t n);
/* copy the installed SRS back (canonical affine) */
int kzgx_get_srs_g1(kzgx_ctx* ctx, uint64_t* xy, size_t n);

/* ---- MSM (polyeval_G1) ---------------------------------------------------- */
/* out = sum_{i<n} scalars[i] * SRS[i].  n == 0 gives infinity. */
int kzgx_msm_g1(kzgx_ctx* ctx, const uint64_t* scalars, size_t n, uint64_t* out_xy, int* out_is_inf);
/* batch of independent MSMs over the same SRS prefix: scalars[b*n + i] */
int kzgx_msm_g1_batch(kzgx_ctx* ctx, const uint64_t* scalars, size_t n, size_t batch, uint64_t* out_xy,
                      int* out_is_inf);
/* device pointers; scalar_stride = distance between consecutive MSMs in
 * scalars; out_xy: batch x 2 x W64 limbs; out_is_inf: batch x uint32 */
int kzgx_msm_g1_batch_device(kzgx_ctx* ctx, const void* d_scalars, size_t n, size_t batch, size_t scalar_stride,
                             void* d_out_xy, void* d_out_is_inf, void* stream);

/* ---- single-opening proofs (create_proof(poly, z, 1)) --------------------- */
/* q_j = (P_j - P_j(z_j)) / (X - z_j) (n-1 coefficients), y_j = P_j(z_j).
 * coeff_stride == 0 -> every opening uses the same polynomial. */
int kzgx_quotient_single_batch_device(kzgx_ctx* ctx, const void* d_coeffs, size_t n, size_t coeff_stride,
                                      const void* d_z, size_t batch, void* d_q, size_t q_stride, void* d_y,
                                      void* stream);
/* the same with host pointers (the q = (P - I) / Z step of create_proof,
 * trusted_setup.cpp:225, batched): q_out holds batch x (n - 1) scalars,
 * y_out (may be NULL) batch scalars; coeff_stride in scalars (0: shared P) */
int kzgx_quotient_single_batch(kzgx_ctx* ctx, const uint64_t* coeffs, size_t n, size_t coeff_stride,
                               const uint64_t* zs, size_t batch, uint64_t* q_out, uint64_t* y_out);
/* quotient + MSM per opening; host pointers.  out_y may be NULL. */
int kzgx_prove_single_batch(kzgx_ctx* ctx, const uint64_t* coeffs, size_t n, size_t coeff_stride,
                            const uint64_t* zs, size_t batch, uint64_t* out_xy, int* out_is_inf, uint64_t* out_y);
/* device pipeline: quotients into the workspace, then one batched MSM */
int kzgx_prove_single_batch_device(kzgx_ctx* ctx, const void* d_coeffs, size_t n, size_t coeff_stride,
                                   const void* d_z, size_t batch, void* d_out_xy, void* d_out_is_inf, void* d_y,
                                   void* stream);

/* ---- multi-point opening (create_proof(poly, off, len), any len >= 1) ------ */
/* proof = MSM of q = (P - I) / Z, I the interpolant of P at the len points
 * xs, Z = prod (X - xs[i]) (trusted_setup.cpp:214-227); all on the GPU.
 * P is normalized first; deg P < len gives q = 0 -> infinity. */
int kzgx_prove_range(kzgx_ctx* ctx, const uint64_t* coeffs, size_t n, const uint64_t* xs, size_t len,
                     uint64_t* out_xy, int* out_is_inf);

/* ---- scalar-field polynomial ops ----------------------------------------- */
/* ys[j] = P(xs[j]), j < m */
int kzgx_poly_eval(kzgx_ctx* ctx, const uint64_t* coeffs, size_t n, const uint64_t* xs, size_t m, uint64_t* ys);
/* unique interpolant of degree < n through (xs[i], ys[i]); coeffs: n entries */
int kzgx_poly_interpolate(kzgx_ctx* ctx, const uint64_t* xs, const uint64_t* ys, size_t n, uint64_t* coeffs);

/* Z = prod (X - xs[i]) (build_linear_roots_tree, src/util.cpp:269-284); z_out: n+1 entries */
int kzgx_poly_vanishing(kzgx_ctx* ctx, const uint64_t* xs, size_t n, uint64_t* z_out);

/* ---- G1 helpers ------------------------------------------------------------ */
/* *ok = 1 iff xy is a canonical on-curve affine point (ECP_fromOctet's check,
 * used by deserialize_ECP, src/util.cpp:98-115) */
int kzgx_g1_validate(kzgx_ctx* ctx, const uint64_t* xy, int* ok);
/* out = sum of count affine points (is_inf may be NULL); host pointers */
int kzgx_g1_sum(kzgx_ctx* ctx, const uint64_t* xy, const int* is_inf, size_t count, uint64_t* out_xy, int* out_is_inf);
/* The same on device pointers, enqueued on stream (NULL = the context's):
 * d_xy count canonical affine points (2 W64 words each), d_inf count uint32
 * infinity flags (may be NULL), d_out_xy one point, d_out_inf one uint32.
 * The fold of the sharded commit's gathered partials without a
 * host round trip. */
int kzgx_g1_sum_device(kzgx_ctx* ctx, const void* d_xy, const void* d_inf, size_t count, void* d_out_xy,
                       void* d_out_inf, void* stream);
/* The same fold over packed records, the exchange format of the sharded
 * commitment (python/kzgx_dist.py): record k is 2 W64 uint64 (x || y,
 * canonical little-endian) followed by one uint64 infinity word (nonzero =
 * infinity); the sum is written as one record.  One launch, one wave
 * (strided sums, a shuffle tree, a wave-uniform inversion).  Device
 * pointers; stream as kzgx_msm_g1_batch_device. */
int kzgx_g1_sum_packed_device(kzgx_ctx* ctx, const void* d_records, size_t count, void* d_out_record, void* stream);
/* Projective partials (round 6): the sharded commitment's per-rank MSM left
 * as one XYZZ point (X, Y, ZZ, ZZZ in the library's radix-2^29 Montgomery
 * limbs; ZZ = 0 is infinity) -- an exchange format between ranks running this
 * library, kzgx_partial_record_words(curve) uint64 words (BN254 18,
 * BLS12-381 28) -- so no rank inverts; kzgx_g1_sum_partials_device adds
 * count such records and converts the sum once, into one packed affine
 * record (as kzgx_g1_sum_packed_device).  Device pointers; stream as
 * kzgx_msm_g1_batch_device.  n = 0 gives the identity record. */
int kzgx_partial_record_words(int curve);
int kzgx_msm_g1_partial_device(kzgx_ctx* ctx, const void* d_scalars, size_t n, void* d_out_record, void* stream);
int kzgx_g1_sum_partials_device(kzgx_ctx* ctx, const void* d_records, size_t count, void* d_out_record, void* stream);
/* One commitment sharded over several contexts, typically one per GPU (the
 * one-process form of SURVEY 8e's sharded commit; bench.py's configs[4] runs
 * the one-process-per-GPU form over RCCL).  Context k holds the SRS slice
 * starting at point starts[k] (kzgx_gen_srs_g1(ctx, tau, starts[k], n_k) or
 * kzgx_load_srs_g1); the slices must be contiguous from 0 (starts[k + 1] ==
 * starts[k] + |SRS_k|, else KZGX_ERR_ARG) and cover n (else
 * KZGX_ERR_DEGREE).  Every context runs the partial MSM of its slice of
 * scalars[0..n) on its own stream, concurrently; the projective partials are
 * then folded exactly on ctxs[0] (affine result, bit-exact with one MSM). */
int kzgx_msm_g1_sharded(kzgx_ctx* const* ctxs, const size_t* starts, size_t nctx, const uint64_t* scalars,
                        size_t n, uint64_t* out_xy, int* out_is_inf);

/* ---- verify half: G2 setup, polyeval_G2, pairing ----------------------------
 * G2 points are canonical affine on the sextic twist (BN254: D-type
 * y^2 = x^3 + 2/(1+i); BLS12-381: M-type y^2 = x^3 + 4(1+i)), Fp2 = Fp[i],
 * i^2 = -1, stored as x.re || x.im || y.re || y.im (4 x W64 limbs); all zero
 * = infinity.  Fp12 values are 12 canonical Fp elements in tower order
 * (Fp6 = Fp2[v]/(v^3 - (1+i)), Fp12 = Fp6[w]/(w^2 - v)):
 * c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2, each (re, im). */
/* generate [tau^(start+i)] G2, i < n (G2 half of generate_elements_range,
 * src/trusted_setup.cpp:123-135) and install it */
int kzgx_gen_srs_g2(kzgx_ctx* ctx, const uint64_t* tau, size_t start, size_t n);
/* install n canonical affine G2 points (G2 half of the setup-file loader,
 * src/trusted_setup.cpp:103-118) */
int kzgx_load_srs_g2(kzgx_ctx* ctx, const uint64_t* xy, size_t n);
int kzgx_get_srs_g2(kzgx_ctx* ctx, uint64_t* xy, size_t n);
size_t kzgx_srs_g2_size(const kzgx_ctx* ctx);
/* ok[k] = 1 iff point k is canonical and on the twist (ECP2_fromOctet) */
int kzgx_g2_validate(kzgx_ctx* ctx, const uint64_t* xy, size_t count, int* ok);
/* out = sum_{i<n} scalars[i] [tau^i]G2 (polyeval_G2, src/trusted_setup.cpp:176-201) */
int kzgx_msm_g2(kzgx_ctx* ctx, const uint64_t* scalars, size_t n, uint64_t* out_xy, int* out_is_inf);
/* out[k] = e(P_k, Q_k): optimal ate pairing + final exponentiation
 * (miracl PAIR_ate + PAIR_fexp, src/trusted_setup.cpp:240-250); inf flags may be NULL */
int kzgx_pairing(kzgx_ctx* ctx, const uint64_t* g1_xy, const int* g1_inf, const uint64_t* g2_xy, const int* g2_inf,
                 size_t count, uint64_t* out);
/* trusted_setup::verify_proof (src/trusted_setup.cpp:230-254): *ok =
 * e(proof, [Z(tau)]G2) == e(C - [I(tau)]G1, G2[0]) for the npoints opened
 * points (xs, ys); npoints >= |SRS G1| gives *ok = 0; npoints == 0 is
 * KZGX_ERR_ARG; needs a G2 setup of >= npoints + 1 points.  npoints == 1
 * runs as kzgx_verify_single_batch with one opening (same boolean). */
int kzgx_verify_proof(kzgx_ctx* ctx, const uint64_t* commit_xy, int commit_inf, const uint64_t* proof_xy,
                      int proof_inf, const uint64_t* xs, const uint64_t* ys, size_t npoints, int* ok);
/* batch of single-point verifies (verify_proof with one opened point each):
 * ok[k] = e(proof_k, [tau - z_k]G2) == e(commit_k - [y_k]G1, G2), evaluated as
 * one two-Miller-loop product and one final exponentiation per opening (a
 * wave or a lane each, see kzgx_set_verify_wave_max).  Needs G1[0] = G and
 * G2[0..1]; inf arrays may be NULL. */
int kzgx_verify_single_batch(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf,
                             const uint64_t* proofs_xy, const int* proof_inf, const uint64_t* zs, const uint64_t* ys,
                             size_t count, int* ok);
/* device pointers (inf flags uint32, may be NULL), ok: count x uint32 */
int kzgx_verify_single_batch_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf,
                                    const void* d_proofs, const void* d_proof_inf, const void* d_z, const void* d_y,
                                    size_t count, void* d_ok, void* stream);
/* Batches of at most max_count openings (default 4096) run one 64-lane wave
 * per opening (Fp12 products spread over the wave, setup-derived line and
 * [y]G tables built on first use); larger batches run one lane per opening.
 * Both give the same booleans; 0 forces the lane-per-opening kernel. */
int kzgx_set_verify_wave_max(kzgx_ctx* ctx, size_t max_count);

/* ---- variable-base G1 MSM and aggregated verification (extensions) ---------- */
/* out = sum_{k<n} scalars[k] * points[k] over caller-supplied points: n
 * canonical affine points (x || y, all-zero = infinity; is_inf optional
 * flags, nonzero = infinity) and n canonical scalars (4 x uint64, < r).  No
 * SRS is needed.  n == 0 gives infinity.  Points may repeat and may be each
 * other's negatives.  Every step is an exact group operation: the affine
 * result is bit-exact with any other correct evaluation.  At most
 * KZGX_MSM_POINTS_MAX points per call, else KZGX_ERR_ARG.  KZG commitments
 * are additively homomorphic, so this is also a linear combination of
 * commitments.  Points are taken as canonical and on the curve (not checked). */
#define KZGX_MSM_POINTS_MAX ((size_t)1 << 22)
int kzgx_msm_g1_points(kzgx_ctx* ctx, const uint64_t* points_xy, const int* is_inf, const uint64_t* scalars, size_t n,
                       uint64_t* out_xy, int* out_is_inf);
/* device pointers, enqueued on stream (NULL = the context's): d_is_inf n x
 * uint32 (may be NULL), d_out_xy one point, d_out_is_inf one uint32 */
int kzgx_msm_g1_points_device(kzgx_ctx* ctx, const void* d_points_xy, const void* d_is_inf, const void* d_scalars,
                              size_t n, void* d_out_xy, void* d_out_is_inf, void* stream);
/* Aggregated check of count single-point openings with challenges r_k:
 *   *ok = e(sum r_k proof_k, [tau]G2) == e(sum r_k (commit_k - [y_k]G + [z_k] proof_k), G2)
 * -- two variable-base MSMs (over the proofs; over commits, proofs and G1[0]
 * with the scalars r_k, r_k z_k and -sum r_k y_k) and ONE two-pairing product,
 * instead of one product per opening.
 *  SRS: needs G1[0] = G and G2[0..1] as kzgx_verify_single_batch does, else
 *   KZGX_ERR_NO_SRS.
 *  challenges: count x 4 uint64 canonical scalars.  NULL (host entry only):
 *   the library draws independent 128-bit values from std::random_device (as
 *   the reference draws tau), r_0 = 1.  NULL on the device entry is
 *   KZGX_ERR_ARG.  count == 0 gives *ok = 1; at most KZGX_MSM_POINTS_MAX / 2
 *   - 1 openings per call, else KZGX_ERR_ARG.
 *  Points are taken as canonical and on the curve, exactly as
 *   kzgx_verify_single_batch takes them (the C++ facade's deserialize
 *   validates).  Subgroup membership is NOT checked here on BLS12-381: a
 *   caller who needs it uses kzgx_verify_aggregate_checked(_device) below, or
 *   checks the points first with kzgx_g1_check_batch(_device) -- components
 *   outside the prime-order subgroup are the known weakness of
 *   random-combination checks.
 *  Equivalence: with explicit challenges the answer is a deterministic
 *   function of the inputs (the equation above, nothing else).  It equals the
 *   AND of the per-opening verifies when every opening is valid, and whenever
 *   exactly one opening is invalid and every challenge is nonzero.  Several
 *   invalid openings can cancel for particular challenges (two errors +d and
 *   -d under equal challenges pass), so challenges the prover can predict
 *   prove nothing; with unpredictable 128-bit challenges the probability of a
 *   difference from the AND is <= 2^-128. */
int kzgx_verify_aggregate(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf, const uint64_t* proofs_xy,
                          const int* proof_inf, const uint64_t* zs, const uint64_t* ys, const uint64_t* challenges,
                          size_t count, int* ok);
/* device pointers (inf flags uint32, may be NULL), d_ok: one uint32;
 * asynchronous on stream (NULL = the context's) */
int kzgx_verify_aggregate_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf, const void* d_proofs,
                                 const void* d_proof_inf, const void* d_z, const void* d_y, const void* d_challenges,
                                 size_t count, void* d_ok, void* stream);


/* ---- batched point validation, prime-order subgroup checks (extensions) ------
 * One launch for any number of points, one lane per point.  With subgroup != 0
 * a point must also lie in the order-r subgroup: on BN254 G1 the cofactor is 1
 * and the flag adds nothing; on BLS12-381 G1 the test is [x^2]P = (beta x, -y)
 * (exactly membership, DESIGN.md "Point validation"); on both G2 twists it is
 * the definitional [r]Q = O.  The optimal ate pairing is bilinear only on
 * G1 x G2, so the per-opening and the aggregated verify are the same predicate
 * only for members. */
/* ok[k] = 1 iff point k is canonical, on the curve and, if subgroup != 0, in the
 * prime-order subgroup; infinite entries (flag or all-zero) pass.  count == 0 is KZGX_OK.
 * is_inf may be NULL; at most KZGX_MSM_POINTS_MAX points per call, else KZGX_ERR_ARG. */
int kzgx_g1_check_batch(kzgx_ctx* ctx, const uint64_t* xy, const int* is_inf, size_t count, int subgroup, int* ok);
/* device pointers; d_ok count x uint32 and d_all_ok one uint32 (either may be NULL, not both);
 * asynchronous on stream (NULL = the context's).  *d_all_ok = the AND of the
 * flags (1 for count == 0), folded on the device. */
int kzgx_g1_check_batch_device(kzgx_ctx* ctx, const void* d_xy, const void* d_is_inf, size_t count, int subgroup,
                               void* d_ok, void* d_all_ok, void* stream);
/* the same for G2 points (4 x W64 limbs each) */
int kzgx_g2_check_batch(kzgx_ctx* ctx, const uint64_t* xy, const int* is_inf, size_t count, int subgroup, int* ok);
/* every installed G1 / G2 SRS point, checked where it lies on the device (no copy of the SRS);
 * *g2_ok = 1 when no G2 setup is installed; KZGX_ERR_NO_SRS without a G1 SRS */
int kzgx_srs_check(kzgx_ctx* ctx, int subgroup, int* g1_ok, int* g2_ok);
/* kzgx_verify_aggregate(_device) preceded by the G1 check of every commit and proof:
 * *ok = 0 as soon as one of them fails, whatever the pairing equation says; otherwise the
 * aggregate's answer.  The device form stays asynchronous (the AND is folded on the device).
 * Arguments, limits and statuses as kzgx_verify_aggregate(_device). */
int kzgx_verify_aggregate_checked(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf,
                                  const uint64_t* proofs_xy, const int* proof_inf, const uint64_t* zs,
                                  const uint64_t* ys, const uint64_t* challenges, size_t count, int subgroup, int* ok);
int kzgx_verify_aggregate_checked_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf,
                                         const void* d_proofs, const void* d_proof_inf, const void* d_z,
                                         const void* d_y, const void* d_challenges, size_t count, int subgroup,
                                         void* d_ok, void* stream);

/* ---- evaluation form (extensions) -------------------------------------------------
 * Polynomials given by their values on the size-2^k domain of roots of unity
 * {w^i}, w = kzgx_domain_root(curve, k), instead of by monomial coefficients:
 * a batched radix-2 NTT over Fr, and commits / single-point openings that run
 * the inverse NTT into context workspace and hand the coefficients to the
 * kzgx_msm_g1_batch_device / kzgx_prove_single_batch_device pipelines as they
 * are.  No reference counterpart.
 *  Domain: BLS12-381's r - 1 is divisible by 2^32, w = 7^((r-1)/2^k); BN254
 *   (Nogami)'s r - 1 only by 4, w = 2^((r-1)/2^k), so there the feature stops
 *   at n = 4 and kzgx_poly_interpolate remains the way from values to
 *   coefficients.
 *  forward: out[i] = sum_j in[j] w^(i j);  inverse (KZGX_NTT_INVERSE):
 *   out[j] = n^-1 sum_i in[i] w^(-i j).  The coefficient side is always in
 *   natural order.  With KZGX_NTT_BITREV the evaluation side (forward output,
 *   inverse input) is indexed by the k-bit reversal of i, the order
 *   data-availability blobs use.  Scalars are canonical in and out.
 *  Transforms up to 2^KZGX_NTT_TILE_LOG2 run in one pass out of LDS, larger
 *   ones in two passes through a workspace of batch x n scalars.
 *  Statuses: log2n > kzgx_ntt_max_log2(curve), a stride smaller than n (except
 *   eval_stride == 0 below), an unknown flag bit: KZGX_ERR_ARG; 2^log2n larger
 *   than the installed SRS: KZGX_ERR_DEGREE; no SRS: KZGX_ERR_NO_SRS;
 *   batch == 0: KZGX_OK. */
#define KZGX_NTT_MAX_LOG2 22
#define KZGX_NTT_TILE_LOG2 12
#define KZGX_NTT_INVERSE 1
#define KZGX_NTT_BITREV 2
/* largest log2 n the curve's scalar field allows, capped at KZGX_NTT_MAX_LOG2:
 * BLS12-381 22, BN254 2; -1 for an unknown curve.  Host arithmetic, no device. */
int kzgx_ntt_max_log2(int curve);
/* the domain generator w of order 2^log2n, canonical 4 x uint64.  Host
 * arithmetic, no device; valid up to the field's 2-adicity (BLS12-381: 32,
 * BN254: 2), KZGX_ERR_ARG beyond */
int kzgx_domain_root(int curve, unsigned log2n, uint64_t* root);
/* batch transforms of n = 2^log2n scalars, in[b * n + i]; host pointers (in == out allowed) */
int kzgx_ntt(kzgx_ctx* ctx, const uint64_t* in, unsigned log2n, size_t batch, int flags, uint64_t* out);
/* device pointers, asynchronous on stream (NULL = the context's); transform b
 * at d_in + b * in_stride scalars, written to d_out + b * out_stride scalars;
 * scalars between the transforms are neither read nor written.  d_in == d_out
 * is allowed (with equal strides) */
int kzgx_ntt_device(kzgx_ctx* ctx, const void* d_in, size_t in_stride, void* d_out, size_t out_stride,
                    unsigned log2n, size_t batch, int flags, void* stream);
/* commit_k = MSM(inverse NTT of evals_k, SRS): bit-exact with committing to
 * the interpolant.  flags: 0 or KZGX_NTT_BITREV.  The evaluations are only read. */
int kzgx_commit_evals_batch(kzgx_ctx* ctx, const uint64_t* evals, unsigned log2n, size_t batch, int flags,
                            uint64_t* out_xy, int* out_is_inf);
int kzgx_commit_evals_batch_device(kzgx_ctx* ctx, const void* d_evals, unsigned log2n, size_t batch,
                                   size_t eval_stride, int flags, void* d_out_xy, void* d_out_is_inf,
                                   void* stream);
/* single-point openings of polynomials given by evaluations; eval_stride == 0:
 * one shared polynomial.  z may be any scalar, a domain point included;
 * y_k = P_k(z_k) (d_y / out_y may be NULL).  flags: 0 or KZGX_NTT_BITREV */
int kzgx_prove_evals_batch(kzgx_ctx* ctx, const uint64_t* evals, unsigned log2n, size_t eval_stride,
                           const uint64_t* zs, size_t batch, int flags, uint64_t* out_xy, int* out_is_inf,
                           uint64_t* out_y);
int kzgx_prove_evals_batch_device(kzgx_ctx* ctx, const void* d_evals, unsigned log2n, size_t eval_stride,
                                  const void* d_z, size_t batch, int flags, void* d_out_xy,
                                  void* d_out_is_inf, void* d_y, void* stream);

/* ---- G1 NTT (extension) ---------------------------------------------------------------
 * The discrete Fourier transform of the evaluation form over G1 points instead
 * of scalars, on the same domains and with the same index conventions as
 * kzgx_ntt:  forward: out[i] = sum_j [w^(i j)] in[j];  inverse
 * (KZGX_NTT_INVERSE): out[j] = [n^-1] sum_i [w^(-i j)] in[i].  The coefficient
 * side is in natural order; with KZGX_NTT_BITREV the evaluation side is indexed
 * by the bit reversal of i.  The inverse transform of an SRS prefix is the
 * Lagrange-basis setup of that domain.  No reference counterpart.
 *  Points are canonical affine in and out, batch x n of them, packed; all-zero
 *   or a set flag is infinity (in_is_inf may be NULL), as in kzgx_msm_g1_points,
 *   and like there they are taken as on the curve (not checked).  Every step is
 *   an exact group operation (equal, opposite and infinite operands included),
 *   so the result is bit-exact with any other correct evaluation.  No SRS is
 *   needed.
 *  One launch per radix-2 stage, one lane per butterfly; a twiddle costs one
 *   255-bit scalar multiplication.  The transforms of a call run in chunks of at
 *   most KZGX_G1_NTT_CHUNK_POINTS points (one transform at least), which bounds
 *   the workspace at max(KZGX_G1_NTT_CHUNK_POINTS, n) XYZZ records (224 B each
 *   on BLS12-381, 144 B on BN254).
 *  Statuses: log2n > kzgx_ntt_max_log2(curve) or an unknown flag bit:
 *   KZGX_ERR_ARG; batch == 0: KZGX_OK. */
#define KZGX_G1_NTT_CHUNK_POINTS 262144
int kzgx_g1_ntt(kzgx_ctx* ctx, const uint64_t* in_xy, const int* in_is_inf, unsigned log2n, size_t batch, int flags,
                uint64_t* out_xy, int* out_is_inf);
/* device pointers (flags uint32, d_in_is_inf may be NULL), asynchronous on
 * stream (NULL = the context's); the input is only read, d_out_xy may not
 * overlap it */
int kzgx_g1_ntt_device(kzgx_ctx* ctx, const void* d_in_xy, const void* d_in_is_inf, void* d_out_xy,
                       void* d_out_is_inf, unsigned log2n, size_t batch, int flags, void* stream);

/* ---- all-domain openings (extension) ------------------------------------------------
 * The n = 2^log2n single-point proofs of a polynomial of n coefficients at every
 * point of the size-n domain at once (Feist-Khovratovich, "FK20"): proof (b, i)
 * opens polynomial b at z = w^i, w = kzgx_domain_root(curve, log2n), and is the
 * same group element -- the same canonical limbs -- as
 * kzgx_prove_single_batch / kzgx_prove_evals_batch give for that z.  With
 * KZGX_NTT_BITREV proof i sits at the bit reversal of i.  No reference
 * counterpart.
 *  Work: one Fr NTT of 2n scalars, 2n scalar multiplications by the cached setup
 *   X = G1-DFT_2n(SRS[n-2], ..., SRS[0], O, ...), an inverse G1 NTT of 2n points
 *   and a forward one of n: Theta(n log n) group operations per polynomial, where
 *   the n separate openings cost Theta(n^2).  X is built from the installed SRS
 *   on the first call of each log2n (or by kzgx_prove_all_prepare), on the
 *   call's stream with other streams ordered behind it, kept by the context, and
 *   dropped whenever the G1 SRS is replaced.
 *  in: batch x n scalars -- coefficients, or with KZGX_PROVE_ALL_EVALS the values
 *   on the domain (bit-reversed if KZGX_NTT_BITREV is set), taken through the
 *   inverse NTT into workspace first.  The input is only read.  in_stride of
 *   the device form: scalars between consecutive polynomials.
 *  out_xy / out_is_inf: batch x n points and flags; out_y / d_y (may be NULL):
 *   batch x n values P_b(w^i) in the same order.
 *  Batching: a call runs in chunks of max(1, KZGX_G1_NTT_CHUNK_POINTS / 2n)
 *   polynomials, so its workspace is bounded by max(KZGX_G1_NTT_CHUNK_POINTS, 2n)
 *   XYZZ records plus as many scalars, per stream.
 *  When it pays (BLS12-381, MI355X, profiles/prove_all.json, DESIGN.md
 *   "All-domain openings and the G1 NTT"): a call costs about 140 ms whatever it
 *   carries up to a few hundred thousand points, so one polynomial of n = 2^12
 *   is SLOWER than kzgx_prove_evals_batch over the domain (143 against 61 ms);
 *   the crossover is about 3 polynomials per call at n = 2^12 (32 of them: 197
 *   against 1904 ms) and about n = 2^13 for a single polynomial (2^14: 163
 *   against 890 ms; 2^16: 195 ms).  No path is chosen silently: this entry
 *   always runs FK20, kzgx_prove_evals_batch always the n separate openings.
 *  Statuses: log2n > kzgx_ntt_max_log2(curve) - 1 (the size-2n domain must
 *   exist: BLS12-381 up to 21, BN254 up to 1), in_stride < n, an unknown flag:
 *   KZGX_ERR_ARG; no SRS: KZGX_ERR_NO_SRS; 2^log2n larger than the installed SRS:
 *   KZGX_ERR_DEGREE; batch == 0: KZGX_OK. */
#define KZGX_PROVE_ALL_EVALS 4   /* input is evaluations on the domain, not coefficients */
/* optional: builds X for log2n now (blocks until it is built) */
int kzgx_prove_all_prepare(kzgx_ctx* ctx, unsigned log2n);
int kzgx_prove_all_batch(kzgx_ctx* ctx, const uint64_t* in, unsigned log2n, size_t batch, int flags,
                         uint64_t* out_xy, int* out_is_inf, uint64_t* out_y);
/* device pointers, asynchronous on stream (NULL = the context's) */
int kzgx_prove_all_batch_device(kzgx_ctx* ctx, const void* d_in, unsigned log2n, size_t batch, size_t in_stride,
                                int flags, void* d_out_xy, void* d_out_is_inf, void* d_y, void* stream);

/* ---- coset (cell) openings (extension) -------------------------------------------------
 * One proof per coset of l = 2^log2l points instead of one per point (the
 * multi-point form of Feist-Khovratovich): for n = 2^log2n coefficients, m = n / l,
 * ext = 1 with KZGX_PROVE_COSETS_EXTENDED else 0, there are R = m 2^ext cosets of
 * the size-D domain, D = R l (n, or 2n when extended), w = kzgx_domain_root(curve,
 * log2 D).  Coset i holds the points x(i, j) = w^(i + R j), j < l, the roots of
 * X^l - a_i with a_i = w^(i l), and proof (b, i) = [q(tau)]G for q = P_b div
 * (X^l - a_i): the same group element -- the same canonical limbs -- as
 * kzgx_prove_range(P_b, xs = x(i, .)).  No reference counterpart.
 *  Order: naturally proof i sits at index i and y[i l + j] = P(x(i, j)).  With
 *   KZGX_NTT_BITREV proof i sits at the R-bit reversal of i and y is the
 *   bit-reversed size-D evaluation array, whose chunk p of l consecutive values
 *   is coset brev_R(p) with its points in bit-reversed order (brev_D(p l + q) =
 *   brev_R(p) + R brev_l(q)): the cell layout of data-availability blobs.
 *   kzgx_coset_points returns the l points of chunk `index` of y in y's order for
 *   the given flags (only KZGX_NTT_BITREV and KZGX_PROVE_COSETS_EXTENDED matter),
 *   the xs to hand to kzgx_verify_proof; host arithmetic, no device.
 *  Work: a setup of l G1 NTTs of 2m points over the strided SRS (2n packed affine
 *   points, built on the first call of each (log2n, log2l) or by
 *   kzgx_prove_cosets_prepare, kept by the context, dropped with the G1 SRS), then
 *   per polynomial l Fr NTTs of 2m scalars, 2n scalar multiplications folded l to
 *   1 inside the wave (k_fkm_pointwise_sum: no per-term point reaches memory), an
 *   inverse G1 NTT of 2m points and a forward one of R.  log2l = 0, ext = 0 gives
 *   kzgx_prove_all_batch's output.  m = 1: every quotient is zero, every proof
 *   infinity.
 *  in: batch x n scalars -- coefficients, or with KZGX_PROVE_ALL_EVALS the values
 *   on the size-n domain (bit-reversed over n if KZGX_NTT_BITREV), as in
 *   kzgx_prove_all_batch.  The input is only read.
 *  out_xy / out_is_inf: batch x R points and flags; out_y / d_y (may be NULL):
 *   batch x D values.
 *  Batching: chunks of max(1, KZGX_G1_NTT_CHUNK_POINTS / 2n) polynomials; per
 *   polynomial the workspace is 2m XYZZ records, 2n scalars, and D scalars for y.
 *  When it pays (BLS12-381, MI355X, profiles/prove_cosets.json, DESIGN.md "Coset
 *   openings (multi-point FK20)"): a (12, 6) extended call is a chain of 15
 *   latency-bound launches, about 73 ms per chunk of up to 32 polynomials, against
 *   0.79 ms per kzgx_prove_range call (host wall clock): 1 polynomial 73.4 against
 *   101.9 ms, 8: 75.3 against 811 ms, 64: 158.1 against 6488 ms.  A call that
 *   carries fewer than about 90 cosets in all is SLOWER than the separate calls;
 *   with log2l = 0 the time is kzgx_prove_all_batch's.  No path is chosen silently.
 *  Statuses: log2l > log2n, log2n - log2l + 1 or log2n + ext larger than
 *   kzgx_ntt_max_log2(curve), in_stride < n, an unknown flag, a NULL pointer:
 *   KZGX_ERR_ARG; no SRS: KZGX_ERR_NO_SRS; 2^log2n larger than the installed SRS:
 *   KZGX_ERR_DEGREE; batch == 0: KZGX_OK. */
#define KZGX_PROVE_COSETS_EXTENDED 8 /* cosets of the size-2n domain (R = 2 n / l) */
int kzgx_coset_points(int curve, unsigned log2n, unsigned log2l, int flags, size_t index, uint64_t* xs);
/* optional: builds the setup of (log2n, log2l) now (blocks until it is built) */
int kzgx_prove_cosets_prepare(kzgx_ctx* ctx, unsigned log2n, unsigned log2l);
int kzgx_prove_cosets_batch(kzgx_ctx* ctx, const uint64_t* in, unsigned log2n, unsigned log2l, size_t batch,
                            int flags, uint64_t* out_xy, int* out_is_inf, uint64_t* out_y);
/* device pointers, asynchronous on stream (NULL = the context's) */
int kzgx_prove_cosets_batch_device(kzgx_ctx* ctx, const void* d_in, unsigned log2n, unsigned log2l, size_t batch,
                                   size_t in_stride, int flags, void* d_out_xy, void* d_out_is_inf, void* d_y,
                                   void* stream);

/* ---- aggregated cell verification (extension) -------------------------------------------
 * One pairing check for count coset openings ("cells") of n_commits commitments,
 * the consumer side of kzgx_prove_cosets_batch.  Notation as above: n = 2^log2n,
 * l = 2^log2l, ext = 1 with KZGX_PROVE_COSETS_EXTENDED else 0, R = 2^(log2n - log2l
 * + ext) cosets of the size-D domain, D = R l, w = kzgx_domain_root(curve, log2 D),
 * coset i = {w^(i + R j), j < l} = the roots of X^l - a_i, a_i = w^(i l).  Cell k is
 * (commitment c_k, coset i_k, proof pi_k, values y_kj = claimed P(x(i_k, j)),
 * challenge r_k).  Its interpolant of degree < l is
 *   I_k(X) = sum_t w^(-i_k t) INTT_l(y_k)[t] X^t
 * (INTT_l: kzgx_ntt with KZGX_NTT_INVERSE at size l), and the call computes
 *   S_t   = sum_k r_k w^(-i_k t) INTT_l(y_k)[t]                      (t < l)
 *   rho_c = sum_{k : c_k = c} r_k                                    (c < n_commits)
 *   A     = sum_k r_k pi_k
 *   B     = sum_c rho_c C_c + sum_k (r_k a_(i_k)) pi_k - sum_t S_t G1[t]
 *   *ok   = e(A, G2[l]) == e(B, G2[0])
 * -- one batched size-l inverse NTT, a fold over the cells, two variable-base MSMs
 * (count points; n_commits + count + l points) and ONE two-pairing product; no
 * interpolation over arbitrary points and no G2 MSM.  With log2l = 0 this is
 * kzgx_verify_aggregate's equation at z_k = w^(i_k).  No reference counterpart.
 *  commits: n_commits distinct commitments, each passed once (unused ones are
 *   harmless); commit_index[k] < n_commits names cell k's.  proofs: count points.
 *   ys: count x l canonical scalars, packed.  Infinity as in kzgx_msm_g1_points
 *   (all-zero or a set flag; the flag arrays may be NULL).
 *  flags: KZGX_NTT_BITREV and KZGX_PROVE_COSETS_EXTENDED only.  Without
 *   KZGX_NTT_BITREV cell_index[k] is the coset i and ys[k] is in the order j = 0 ..
 *   l - 1: the natural output of kzgx_prove_cosets_batch.  With it cell_index[k] is
 *   the chunk number p of the bit-reversed size-D evaluation array -- the coset is
 *   brev_R(p) and the l values are in bit-reversed order -- so proof p and y[p] of
 *   kzgx_prove_cosets_batch(..., KZGX_NTT_BITREV) are passed as they come, and
 *   kzgx_coset_points with the same flags and index lists the cell's points.
 *  challenges: count x 4 uint64 canonical scalars, as in kzgx_verify_aggregate:
 *   explicit ones make the answer a deterministic function of the inputs (the
 *   equation above, nothing else); NULL (host entries only) lets the library draw
 *   independent 128-bit values, r_0 = 1; NULL on a device entry is KZGX_ERR_ARG.
 *   The equivalence with the AND of the per-cell kzgx_verify_proof calls is
 *   kzgx_verify_aggregate's: equal when every cell is valid, and whenever exactly
 *   one is invalid under nonzero challenges; errors can cancel under challenges
 *   the prover predicts.  Which cell failed is not reported here:
 *   kzgx_verify_cells_each (below) gives one verdict per cell.
 *  Setup: a G1 SRS of at least l points with G1[t] = [tau^t]G for t < l, and a G2
 *   setup of at least l + 1 points.  The call never touches n SRS points, so
 *   2^log2n may exceed the installed SRS: a verifier of the data-availability
 *   shape (log2n = 12, log2l = 6, extended) needs 64 G1 and 65 G2 points.
 *  Points are taken as canonical and on the curve, as in kzgx_verify_aggregate.
 *   The _checked forms first run the G1 check of kzgx_g1_check_batch over the
 *   n_commits commitments and the count proofs and force *ok = 0 when one fails,
 *   exactly like kzgx_verify_aggregate_checked(_device).
 *  Device entries: device pointers (indices and infinity flags uint32, d_ok one
 *   uint32), asynchronous on stream (NULL = the context's), no host read-back.
 *   An index out of range (commit_index >= n_commits, cell_index >= R) reads
 *   nothing out of bounds and forces *d_ok = 0 (a flag folded on the device).
 *  Workspace: count x l scalars for the transforms plus the MSMs'; count x l is
 *   capped at KZGX_VERIFY_CELLS_VALUES_MAX (512 MiB of scalars).
 *  When it pays (BLS12-381, MI355X, profiles/verify_cells.json, DESIGN.md "Cell
 *   verification"): at (12, 6) extended, bit-reversed, a device call costs about
 *   10 ms whatever it carries -- 128 cells 9.9 ms, 1024 cells 9.7 ms, 8192 cells of
 *   64 blobs 10.4 ms (788k cells/s) -- against 4.05 ms per kzgx_verify_proof call of
 *   one cell (host wall clock): 519, 4155 and 33152 ms, x52, x430 and x3189.  The
 *   call is latency-bound: the two MSMs' window sums and Horner steps take about
 *   7 ms and the pairing product 3 ms at every count, the fold kernels 0.03 to
 *   0.15 ms (0.3% to 1.5% of the call) and the inverse NTTs 0.03 to 0.04 ms.  Only a
 *   call of 1 or 2 cells is SLOWER than the separate calls (the crossover is at
 *   2.4 calls' worth).  The checked form with the subgroup test costs x1.15 at
 *   8192 cells (11.7 against 10.2 ms).  No path is chosen silently.
 *  Statuses: log2l > log2n or log2n + ext > kzgx_ntt_max_log2(curve), an unknown
 *   flag (KZGX_NTT_INVERSE and KZGX_PROVE_ALL_EVALS included), a NULL required
 *   pointer, n_commits + count + l > KZGX_MSM_POINTS_MAX, count x l >
 *   KZGX_VERIFY_CELLS_VALUES_MAX, and on the host entries an index >= n_commits or
 *   >= R: KZGX_ERR_ARG; no G1 SRS or fewer than l + 1 G2 points: KZGX_ERR_NO_SRS;
 *   fewer than l G1 points: KZGX_ERR_DEGREE; count == 0: *ok = 1 (n_commits may
 *   then be 0). */
#define KZGX_VERIFY_CELLS_VALUES_MAX ((size_t)1 << 24)
int kzgx_verify_cells_aggregate(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf, size_t n_commits,
                                const uint32_t* commit_index, const uint32_t* cell_index, const uint64_t* proofs_xy,
                                const int* proof_inf, const uint64_t* ys, const uint64_t* challenges, size_t count,
                                unsigned log2n, unsigned log2l, int flags, int* ok);
int kzgx_verify_cells_aggregate_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf,
                                       size_t n_commits, const void* d_commit_index, const void* d_cell_index,
                                       const void* d_proofs, const void* d_proof_inf, const void* d_ys,
                                       const void* d_challenges, size_t count, unsigned log2n, unsigned log2l,
                                       int flags, void* d_ok, void* stream);
int kzgx_verify_cells_aggregate_checked(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf,
                                        size_t n_commits, const uint32_t* commit_index, const uint32_t* cell_index,
                                        const uint64_t* proofs_xy, const int* proof_inf, const uint64_t* ys,
                                        const uint64_t* challenges, size_t count, unsigned log2n, unsigned log2l,
                                        int flags, int subgroup, int* ok);
int kzgx_verify_cells_aggregate_checked_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf,
                                               size_t n_commits, const void* d_commit_index,
                                               const void* d_cell_index, const void* d_proofs,
                                               const void* d_proof_inf, const void* d_ys, const void* d_challenges,
                                               size_t count, unsigned log2n, unsigned log2l, int flags, int subgroup,
                                               void* d_ok, void* stream);

/* ---- per-cell verdicts (extension) -------------------------------------------------------
 * kzgx_verify_cells_each*: the same batch, one answer per cell.  With the notation
 * above, for every cell k
 *   ok[k] = e(pi_k, G2[l]) == e(C_(c_k) - [I_k(tau)]G1 + [a_(i_k)]pi_k, G2[0])
 * -- the boolean of kzgx_verify_proof(C_(c_k), pi_k, xs = kzgx_coset_points(...,
 * cell_index[k]), ys = y_k), with one exception: kzgx_verify_proof answers 0 when
 * npoints >= the G1 SRS's size, this entry needs l G1 and l + 1 G2 points like the
 * aggregate and answers the equation.  There are no challenges: the answer is
 * deterministic and exact per cell, and errors that cancel in the aggregate under
 * equal challenges are reported as separate failures.  Use it after the aggregate
 * said 0, or instead of it, to find the cells to drop (kzgx_recover_cells takes the
 * rest) and their sender.
 *  Arguments: kzgx_verify_cells_aggregate's without `challenges`; ok: count entries.
 *  Pipeline, in chunks of at most KZGX_VERIFY_CELLS_EACH_CHUNK cells and
 *   KZGX_VERIFY_CELLS_EACH_CHUNK_VALUES values (kzgx_set_verify_cells_chunk(ctx,
 *   cells) overrides the former, 0 = default, at most 65535: a test knob): the
 *   size-l inverse NTTs, a twiddle per coefficient (I_k), one batched fixed-base
 *   MSM of the chunk's interpolants over G1[0..l) (the context's table settings pick
 *   its path as for kzgx_msm_g1_batch), one lane per cell for C - [I(tau)]G1, and
 *   the two kernels of kzgx_verify_single_batch_device on (C', pi, z = a, y = 0)
 *   with G2[l] in G2[1]'s place -- the wave-per-opening one for count <=
 *   kzgx_set_verify_wave_max's bound, else the lane-per-opening one; both give the
 *   same booleans.  The workspace per stream is bounded by the chunk, not by count.
 *   The first call for a coset size l stages G2[0] || G2[l] and, on the wave path,
 *   builds their line tables (one stream synchronisation, as the first
 *   kzgx_verify_single_batch_device after a setup); both are dropped with the setup.
 *  The _checked forms first run the G1 check of kzgx_g1_check_batch over the
 *   commitments and the proofs and force ok[k] = 0 for a cell whose proof or
 *   commitment fails it: a bad commitment zeroes every cell that names it and no
 *   other.
 *  Device entries: device pointers (indices, infinity flags and d_ok uint32, count
 *   words), asynchronous on stream, no host read-back.  An index out of range
 *   (commit_index >= n_commits, cell_index >= R) reads nothing out of bounds and
 *   gives d_ok[k] = 0 for that cell only.
 *  When it pays (BLS12-381, MI355X, profiles/verify_cells_each.json, DESIGN.md
 *   "Per-cell verdicts"): at (12, 6) extended, bit-reversed, a device call takes
 *   7.9 ms for 128 cells, 16.8 ms for 1024 and 109.0 ms for 8192 (75k cells/s),
 *   against 4.03 ms per kzgx_verify_proof call of one cell (host wall clock, 64
 *   calls timed and scaled): 516, 4119 and 33012 ms, x66, x246 and x303.  One
 *   cell: 1.9 against 4.0 ms; two cells are a TIE with the separate calls (7.4
 *   against 7.3 ms, spreads overlapping).  It LOSES to
 *   kzgx_verify_cells_aggregate_device, which pays one pairing product whatever
 *   the count (9.9 to 10.3 ms), from about 300 cells on (interpolated): x0.80 at
 *   128 cells, x1.62 at 1024, x10.7 at 8192 -- run the aggregate first and this
 *   call only on a batch it refused.  The count pairing products are the call:
 *   90% of it at 128 cells, 97% at 8192 (106 ms); the batched MSM takes 0.6 to
 *   3.4 ms with the default table (1.1 to 22.5 ms without), the inverse NTTs and
 *   twiddles under 0.08 ms, the subtraction 0.13 ms.  At 8192 cells the default
 *   bound picks the SLOWER pairing kernel: the lane-per-opening one takes 75.6 ms
 *   there (x1.44; 68 ms at any count below about 4000, where it loses); the two
 *   cross near 5000 cells, and kzgx_set_verify_wave_max moves the switch.  The
 *   lane kernel also still walks the 256 doublings of [y]G for y = 0.
 *  Statuses: those of kzgx_verify_cells_aggregate (the same argument, limit and
 *   setup checks, and on the host entries KZGX_ERR_ARG for an index out of range);
 *   count == 0: KZGX_OK, nothing is written (n_commits may then be 0). */
#define KZGX_VERIFY_CELLS_EACH_CHUNK 16384
#define KZGX_VERIFY_CELLS_EACH_CHUNK_VALUES ((size_t)1 << 21)
int kzgx_verify_cells_each(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf, size_t n_commits,
                           const uint32_t* commit_index, const uint32_t* cell_index, const uint64_t* proofs_xy,
                           const int* proof_inf, const uint64_t* ys, size_t count, unsigned log2n, unsigned log2l,
                           int flags, int* ok);
int kzgx_verify_cells_each_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf, size_t n_commits,
                                  const void* d_commit_index, const void* d_cell_index, const void* d_proofs,
                                  const void* d_proof_inf, const void* d_ys, size_t count, unsigned log2n,
                                  unsigned log2l, int flags, void* d_ok, void* stream);
int kzgx_verify_cells_each_checked(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf,
                                   size_t n_commits, const uint32_t* commit_index, const uint32_t* cell_index,
                                   const uint64_t* proofs_xy, const int* proof_inf, const uint64_t* ys, size_t count,
                                   unsigned log2n, unsigned log2l, int flags, int subgroup, int* ok);
int kzgx_verify_cells_each_checked_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf,
                                          size_t n_commits, const void* d_commit_index, const void* d_cell_index,
                                          const void* d_proofs, const void* d_proof_inf, const void* d_ys,
                                          size_t count, unsigned log2n, unsigned log2l, int flags, int subgroup,
                                          void* d_ok, void* stream);
int kzgx_set_verify_cells_chunk(kzgx_ctx* ctx, size_t cells);

/* ---- compressed points (extension) -------------------------------------------------------
 * Commitments, proofs and published setups travel as compressed points: x and one
 * bit of y.  These calls turn packed records into the canonical x || y limbs every
 * other entry takes, and back, one lane per record in one launch; the root is
 * y = (x^3 + b)^((p + 1) / 4) (both primes are 3 mod 4), accepted iff y^2 = x^3 + b
 * (DESIGN.md "Compressed points").  No reference counterpart beyond the octet
 * family of ECP_toOctet(..., true), which KZGX_ENC_SEC1 matches.
 *  KZGX_ENC_ZCASH (BLS12-381 only; the ZCash / IETF encoding): a G1 record is 48
 *   bytes, x big-endian; byte 0 carries 0x80 C (compressed, must be 1), 0x40 I
 *   (infinity) and 0x20 S (sign: y > (p - 1) / 2).  I = 1 requires S = 0 and every
 *   other bit zero.  x is the record with the three flag bits cleared and must be
 *   < p.  A G2 record is 96 bytes, x.im || x.re, flags in byte 0; S = 1 means
 *   y.im > (p - 1) / 2, or y.im = 0 and y.re > (p - 1) / 2.  BN254 has only two
 *   spare bits: KZGX_ERR_ARG there.  Uncompressed records (C = 0) are not offered.
 *  KZGX_ENC_SEC1 (both curves, G1 only): 1 + MODBYTES bytes (33 / 49), prefix
 *   0x02 | (y mod 2), then x big-endian -- the compressed counterpart of the 0x04
 *   octet.  Infinity is prefix 0x00 with an all-zero x (this library's convention,
 *   INTEGRATION.md).  Every other prefix is invalid, 0x04 included.
 *  Records are packed without padding; the limbs are W64 per coordinate, x || y
 *   (G2: x.re, x.im, y.re, y.im).
 *  Decompression: ok[k] = 1 iff record k is well-formed, x canonical and x^3 + b a
 *   square, and, with subgroup != 0, the point lies in the order-r subgroup (the
 *   tests of kzgx_g1_check_batch / kzgx_g2_check_batch, in the same launch).  A
 *   record that fails decodes to infinity: all-zero limbs, out_is_inf = 1, ok = 0.
 *   A valid identity record gives all-zero limbs, out_is_inf = 1, ok = 1.
 *   out_is_inf may be NULL on the host entries.
 *  Compression validates nothing: the sign comes from y as given.  Infinity (a set
 *   flag or all-zero limbs; is_inf may be NULL) writes the identity record.
 *  Device entries: device pointers (flags uint32), asynchronous on stream (NULL =
 *   the context's); d_ok and d_all_ok as in kzgx_g1_check_batch_device (either may
 *   be NULL, not both; *d_all_ok = AND of the flags, 1 for count == 0); d_out_is_inf
 *   may be NULL.
 *  Statuses: an unknown encoding, KZGX_ENC_ZCASH or any G2 call on BN254, a NULL
 *   required pointer, more than KZGX_MSM_POINTS_MAX records: KZGX_ERR_ARG, raised
 *   before any device work; count == 0: KZGX_OK.  No SRS is needed.
 *  When it pays: README "Compressed points" and profiles/point_codec.json. */
#define KZGX_ENC_ZCASH 0
#define KZGX_ENC_SEC1 1
/* record length in bytes, 0 if (curve, group 1 or 2, encoding) is not offered; host arithmetic, no device */
size_t kzgx_point_bytes(int curve, int group, int encoding);
int kzgx_g1_decompress_batch(kzgx_ctx* ctx, const uint8_t* bytes, size_t count, int encoding, int subgroup,
                             uint64_t* out_xy, int* out_is_inf, int* ok);
int kzgx_g1_decompress_batch_device(kzgx_ctx* ctx, const void* d_bytes, size_t count, int encoding, int subgroup,
                                    void* d_out_xy, void* d_out_is_inf, void* d_ok, void* d_all_ok, void* stream);
int kzgx_g1_compress_batch(kzgx_ctx* ctx, const uint64_t* xy, const int* is_inf, size_t count, int encoding,
                           uint8_t* out);
int kzgx_g1_compress_batch_device(kzgx_ctx* ctx, const void* d_xy, const void* d_is_inf, size_t count, int encoding,
                                  void* d_out, void* stream);
/* G2, KZGX_ENC_ZCASH, BLS12-381, host pointers (a setup's G2 half: a cold path) */
int kzgx_g2_decompress_batch(kzgx_ctx* ctx, const uint8_t* bytes, size_t count, int subgroup, uint64_t* out_xy,
                             int* out_is_inf, int* ok);
int kzgx_g2_compress_batch(kzgx_ctx* ctx, const uint64_t* xy, const int* is_inf, size_t count, uint8_t* out);
/* kzgx_verify_cells_aggregate_checked(_device) on compressed commitments and proofs:
 * ONE decompress + check launch over both arrays, the unchanged aggregate on the
 * recovered points (held in context workspace), and the device-side gate: a record
 * that does not decode forces *ok = 0 like a point that fails the check.  Arguments,
 * limits and statuses as the _checked forms, plus the encoding's. */
int kzgx_verify_cells_aggregate_bytes(kzgx_ctx* ctx, const uint8_t* commits_bytes, size_t n_commits,
                                      const uint32_t* commit_index, const uint32_t* cell_index,
                                      const uint8_t* proofs_bytes, const uint64_t* ys, const uint64_t* challenges,
                                      size_t count, unsigned log2n, unsigned log2l, int flags, int encoding,
                                      int subgroup, int* ok);
int kzgx_verify_cells_aggregate_bytes_device(kzgx_ctx* ctx, const void* d_commits_bytes, size_t n_commits,
                                             const void* d_commit_index, const void* d_cell_index,
                                             const void* d_proofs_bytes, const void* d_ys, const void* d_challenges,
                                             size_t count, unsigned log2n, unsigned log2l, int flags, int encoding,
                                             int subgroup, void* d_ok, void* stream);

/* ---- cell recovery (extension) -----------------------------------------------------------
 * Rebuilds erasure-coded blobs from any half of their cells: the inverse of
 * kzgx_prove_cosets_batch(..., KZGX_PROVE_COSETS_EXTENDED), whose size-2n domain
 * carries a polynomial of n coefficients at rate 1/2.  Notation as above: n =
 * 2^log2n, l = 2^log2l, D = 2n, R = D / l cosets ("cells"), w = kzgx_domain_root(
 * curve, log2 D), w_R = w^l, coset i = {w^(i + R j), j < l} = the roots of X^l -
 * w_R^i.  Per blob, with M the cosets it has no cell of (|M| <= R / 2):
 *   Z(X) = Zs(X^l), Zs(Y) = prod_{i in M} (Y - w_R^i)        -- constant on a coset;
 *   E[e] = y[e] Zs(w_R^(e mod R)) on received cosets, 0 on the others: the values of
 *    P Z on the domain, deg(P Z) < n + |M| l <= D, so Q = INTT_D(E) exactly;
 *   P(g w^e) = NTT_D(g^j Q[j])[e] / Zs(g^l w_R^(e mod R)) for the field's NTT
 *    generator g (BLS12-381: 7, BN254: 2; g^l w_R^p = w_R^i would need g^D = 1, so no
 *    divisor is zero); P's coefficients = g^(-j) INTT_D of that, truncated to n;
 *   out_y = NTT_D of the zero-extended coefficients.
 * Four size-D transforms (kzgx_ntt's kernels) and six small Fr kernels per chunk; the
 * locator costs R |M| products and R inversions per blob, and no coefficient of Z is
 * ever formed.  No interpolation over arbitrary points.  No reference counterpart.
 *  cells: a flat list exactly as kzgx_verify_cells_aggregate takes it: cell k belongs
 *   to blob blob_index[k] < n_blobs, is cell cell_index[k] < R and has l values at
 *   ys + k l.  Any order; the cells of different blobs may interleave; blobs may have
 *   different erasure patterns and different counts (>= R / 2 each).  The inputs are
 *   only read.
 *  flags: KZGX_PROVE_COSETS_EXTENDED must be set (without it the domain has no
 *   redundancy), so one flag word serves prove, verify and recover.  KZGX_NTT_BITREV
 *   as in the other two cell calls: cell_index is then the chunk number p of the
 *   bit-reversed evaluation array and the l values come in bit-reversed order.
 *  out_y: n_blobs x D scalars in exactly the layout of kzgx_prove_cosets_batch's y for
 *   the same flags; out_coeffs: n_blobs x n.  Either may be NULL, not both in the
 *   plain forms.  The _and_proofs forms add the n_blobs x R proofs of
 *   kzgx_prove_cosets_batch in its order: the recovered coefficients go to
 *   kzgx_prove_cosets_batch_device as they lie on the device, so these forms need the
 *   G1 SRS and share that call's cached setup; the plain forms need no SRS at all.
 *  ok[b] = 1 iff a polynomial of degree < n takes every value supplied for blob b: the
 *   recovered values are compared with all of them, an exact test, not a random one.
 *   With exactly R / 2 cells every input is consistent (any n values on n points
 *   interpolate), so ok is always 1 there and a corrupted value goes unnoticed; from
 *   R / 2 + 1 cells on a single wrong value gives ok = 0.  A blob with ok = 0 gets
 *   all-zero out_y and out_coeffs, and its proofs are the zero polynomial's: infinity.
 *  Device entries: device pointers (indices and ok uint32), asynchronous on stream
 *   (NULL = the context's), no host read-back, nothing read out of bounds.  A blob with
 *   fewer than R / 2 distinct cells, a duplicate (blob, cell) or a cell_index >= R gets
 *   ok = 0; a blob_index >= n_blobs forces ok = 0 for every blob of the call.
 *  Batching: chunks of max(1, KZGX_RECOVER_CHUNK_SCALARS / D) blobs, so the workspace
 *   is bounded per stream by max(KZGX_RECOVER_CHUNK_SCALARS, D) scalars for the
 *   transforms in place, as many for a two-pass transform's intermediate, half as
 *   many for the coefficients, and 2 R scalars + R + 4 words per blob of the chunk for
 *   the locator and the cell map.  Each chunk reads the whole index list once.
 *  When it pays (BLS12-381, MI355X, profiles/recover_cells.json, DESIGN.md "Cell
 *   recovery"): at (12, 6), bit-reversed, 64 random cells of 128 per blob, a device call is
 *   latency-bound at about 1 ms per chunk -- 1 blob 1.02 ms, 8 blobs 1.03 ms, 64 blobs
 *   1.10 ms (58k blobs/s) -- against 0.48 to 0.51 ms for its four transforms alone
 *   (kzgx_ntt_device, same run): x2.1 to x2.2 of that floor, and the locator is the
 *   difference (0.49 ms at every size: one lane per (blob, p) runs |M| dependent products
 *   and a Fermat inverse; a wave-level batch inversion is not built).  The shift passes
 *   are 0.02 to 0.03 ms each.  With the proofs the call costs what
 *   kzgx_prove_cosets_batch_device costs plus 0.7 to 0.8 ms (74.4 against 73.6 ms for 1
 *   blob, 159.3 against 158.5 ms for 64): x1.005 to x1.010.  The route that existed
 *   before, kzgx_poly_interpolate of a blob's 4096 received points (host pointers, one
 *   blob per call), took 1.41 ms of host wall clock for one blob: a single blob is about
 *   LEVEL with it, and the recovery wins only with the batch (one call for any number of
 *   blobs) or when the values of the missing cells, the consistency answer or device
 *   pointers are wanted.  No path is chosen silently.
 *  Statuses: log2l > log2n, log2n + 1 > kzgx_ntt_max_log2(curve), R >
 *   2^KZGX_RECOVER_MAX_LOG2_CELLS, KZGX_PROVE_COSETS_EXTENDED missing or an unknown
 *   flag, a NULL required pointer, and on the host entries an index out of range, a
 *   duplicate (blob, cell) or a blob with fewer than R / 2 cells: KZGX_ERR_ARG; the
 *   _and_proofs forms: no SRS: KZGX_ERR_NO_SRS, 2^log2n larger than the installed SRS:
 *   KZGX_ERR_DEGREE; n_blobs == 0: KZGX_OK. */
#define KZGX_RECOVER_MAX_LOG2_CELLS 12 /* R <= 4096: the locator costs R |M| products per blob */
#define KZGX_RECOVER_CHUNK_SCALARS 1048576
int kzgx_recover_cells(kzgx_ctx* ctx, const uint32_t* blob_index, const uint32_t* cell_index, const uint64_t* ys,
                       size_t count, size_t n_blobs, unsigned log2n, unsigned log2l, int flags, uint64_t* out_y,
                       uint64_t* out_coeffs, int* ok);
int kzgx_recover_cells_device(kzgx_ctx* ctx, const void* d_blob_index, const void* d_cell_index, const void* d_ys,
                              size_t count, size_t n_blobs, unsigned log2n, unsigned log2l, int flags,
                              void* d_out_y, void* d_out_coeffs, void* d_ok, void* stream);
int kzgx_recover_cells_and_proofs(kzgx_ctx* ctx, const uint32_t* blob_index, const uint32_t* cell_index,
                                  const uint64_t* ys, size_t count, size_t n_blobs, unsigned log2n, unsigned log2l,
                                  int flags, uint64_t* out_y, uint64_t* out_coeffs, uint64_t* out_proofs_xy,
                                  int* out_proofs_is_inf, int* ok);
int kzgx_recover_cells_and_proofs_device(kzgx_ctx* ctx, const void* d_blob_index, const void* d_cell_index,
                                         const void* d_ys, size_t count, size_t n_blobs, unsigned log2n,
                                         unsigned log2l, int flags, void* d_out_y, void* d_out_coeffs,
                                         void* d_out_proofs_xy, void* d_out_proofs_is_inf, void* d_ok,
                                         void* stream);

/* ---- blob proofs (extension) --------------------------------------------------------------
 * The blob-level half of the data-availability path (EIP-4844's compute_blob_kzg_proof and
 * verify_blob_kzg_proof(_batch)): a blob's proof opens its polynomial at the Fiat-Shamir
 * challenge z = H(blob || commitment), so the hash, the value y = P(z) and the byte-level
 * scalar encoding all run on the device.  BLS12-381 only: every entry below returns
 * KZGX_ERR_ARG on BN254 (no usable domain, no ZCash encoding).  No reference counterpart.
 *  Blobs: n = 2^log2n field elements each, packed, the values of P_b (degree < n) on the
 *   size-n domain of kzgx_domain_root(curve, log2n), in natural order or, with
 *   KZGX_NTT_BITREV, in bit-reversed order (Ethereum's).  Default encoding: the library's
 *   scalars (4 x uint64 little-endian limbs, canonical, taken as such).  With
 *   KZGX_BLOB_BYTES: 32 n bytes, element i at bytes [32 i, 32 i + 32), big-endian, each
 *   < r; a blob with any element >= r is INVALID, although the value is congruent to a
 *   valid one.
 *  Commitments and proofs are KZGX_ENC_ZCASH G1 records (48 bytes).
 *  Challenge of (blob, commitment record): z = int_be(SHA-256(M)) mod r with
 *   M = "FSBLOBVERIFY_V1_" (16 bytes) || n as 16-byte big-endian || the blob's 32 n bytes
 *   || the 48-byte record, the blob's bytes being each element as 32-byte big-endian in the
 *   order given (formed in registers from limbs).  |M| = 80 + 32 n; 2^256 div r = 2, so the
 *   reduction subtracts r zero, one or two times.  kzgx_blob_challenge is the executable
 *   statement of this layout.
 *  Value: y = P(z) = (z^n - 1) / n  sum_i f_i w^i / (z - w^i) on the order given; when z
 *   is the domain point w^i, y is exactly f_i.  The same canonical limbs as the y of
 *   kzgx_prove_evals_batch.
 *  Kernels (csrc/blob.hip, DESIGN.md "Blob proofs"): the challenge is one lane per blob,
 *   a serial chain of (80 + 32 n) / 64 + 1 compressions, range-checking each element on the
 *   way; the value is one workgroup per (polynomial, point), each lane folding its strided
 *   slice of the n terms into one fraction (three products a term, no inversion), the
 *   fractions added pairwise through LDS, and ONE Fermat inversion per value in a second
 *   launch, one lane per value.
 *  Device pointers to blobs, z and y must be 16-byte aligned (KZGX_ERR_ARG otherwise), as
 *   scalar arrays are read and written 16 bytes at a time.
 *  When it pays (BLS12-381, MI355X, profiles/blob_proofs.json, DESIGN.md "Blob proofs"; n =
 *   4096, bit-reversed bytes, device pointers, 1 / 8 / 64 / 2048 blobs):
 *   - the challenge kernel takes 7.2 to 8.0 ms WHATEVER the count (2050 dependent
 *     compressions per lane): against a device-to-host copy of the blobs plus a host SHA-256
 *     (0.11 / 0.63 / 4.9 / 224 ms of wall clock) it is SLOWER for 1, 8 and 64 blobs (x74, x13,
 *     x1.5) and x29 faster at 2048; the crossover is near a hundred blobs;
 *   - kzgx_evals_at_batch_device takes 0.55 / 0.51 / 0.48 / 0.87 ms against 0.17 / 0.27 / 0.28 /
 *     1.28 ms for kzgx_ntt_device (inverse) + kzgx_quotient_single_batch_device: SLOWER below
 *     about a thousand values (one workgroup and one Fermat inversion per value: a 0.5 ms
 *     floor), x0.68 at 2048, and it needs neither limbs nor that route's two count x n buffers;
 *   - kzgx_verify_blobs_batch_device takes 16.3 / 18.1 / 18.2 / 18.8 ms against 7.2 / 9.6 / 9.9 /
 *     10.0 ms for kzgx_verify_aggregate_checked_device with z and y supplied (x2.25 .. x1.83):
 *     the hash is the difference;
 *   - kzgx_prove_blobs_batch_device takes 8.8 / 9.9 / 17.6 / 80.4 ms against 0.94 / 1.83 / 10.0 /
 *     66.4 ms for kzgx_commit_evals_batch_device + kzgx_prove_evals_batch_device with z
 *     supplied (x9.4, x5.4, x1.76, x1.21).
 *   A caller with a handful of blobs already on the host should hash there.  No path is
 *   chosen silently: every entry always runs the device path.
 *  Statuses (every entry): BN254, an unknown flag, a NULL required pointer, log2n >
 *   kzgx_ntt_max_log2(curve), NULL challenges on a device entry: KZGX_ERR_ARG, raised
 *   before any device work. */
#define KZGX_BLOB_BYTES 16 /* blob elements are 32-byte big-endian, checked < r */
#define KZGX_BLOB_CHUNK_SCALARS 2097152
/* Host utilities, no device and no context.  kzgx_sha256: the SHA-256 digest of len
 * bytes.  kzgx_blob_challenge: z (4 x uint64) of one blob and one 48-byte record, host
 * arithmetic; flags: KZGX_BLOB_BYTES only (the order is the order given, so
 * KZGX_NTT_BITREV is accepted and changes nothing); *ok_out = 0 iff an element is >= r
 * (always 1 for limbs) -- z is then still the hash of the bytes as given. */
int kzgx_sha256(const uint8_t* msg, size_t len, uint8_t out[32]);
int kzgx_blob_challenge(int curve, const void* blob, unsigned log2n, int flags, const uint8_t* commit_record,
                        uint64_t* z_out, int* ok_out);
/* count blobs + count records -> z (count x 4 uint64) and ok (count flags; may be NULL).
 * No SRS is needed.  flags as kzgx_blob_challenge.  count == 0: KZGX_OK.  Device form:
 * device pointers, d_ok count x uint32, asynchronous on stream (NULL = the context's). */
int kzgx_blob_challenges(kzgx_ctx* ctx, const void* blobs, unsigned log2n, size_t count, int flags,
                         const uint8_t* commit_records, uint64_t* z_out, int* ok_out);
int kzgx_blob_challenges_device(kzgx_ctx* ctx, const void* d_blobs, unsigned log2n, size_t count, int flags,
                                const void* d_commit_records, void* d_z, void* d_ok, void* stream);
/* y_k = P_k(z_k), k < count, for polynomials given by their evaluations: polynomial k at
 * evals + k * eval_stride elements (eval_stride == 0: one shared polynomial; else >= n;
 * the host form copies (count - 1) eval_stride + n elements).  flags: KZGX_NTT_BITREV,
 * KZGX_BLOB_BYTES.  No SRS is needed.  With KZGX_BLOB_BYTES the elements are NOT checked
 * here (an element >= r is used reduced); kzgx_blob_challenges reports canonicity.
 * Replaces, for a verifier, the inverse NTT into a coefficient buffer plus
 * kzgx_quotient_single_batch_device with the quotient discarded. */
int kzgx_evals_at_batch(kzgx_ctx* ctx, const void* evals, unsigned log2n, size_t eval_stride, const uint64_t* zs,
                        size_t count, int flags, uint64_t* ys);
int kzgx_evals_at_batch_device(kzgx_ctx* ctx, const void* d_evals, unsigned log2n, size_t eval_stride,
                               const void* d_z, size_t count, int flags, void* d_y, void* stream);
/* blobs -> commitment records and proof records (count x 48 bytes each), optionally the
 * challenges z and the values y (count x 4 uint64; either may be NULL).  Pipeline, in
 * chunks of max(1, KZGX_BLOB_CHUNK_SCALARS / n) blobs: [decode, KZGX_BLOB_BYTES only] ->
 * kzgx_commit_evals_batch_device -> compress for every chunk; ONE challenge launch for the
 * whole call (the hash takes as long for one blob as for thousands); then [decode] ->
 * kzgx_prove_evals_batch_device at z -> compress for every chunk.  The workspace per
 * stream is bounded by the chunk plus 36 bytes per blob of the call.
 *  An invalid blob (KZGX_BLOB_BYTES, an element >= r): on the device form the identity
 *   record for both outputs, ok[b] = 0 (d_ok: count x uint32, may be NULL), y = 0 and z the
 *   hash of the bytes as given with the identity record; its neighbours are unaffected.  On
 *   the host form KZGX_ERR_ARG (the outputs are then unspecified).
 *  A caller who already holds the commitments composes kzgx_blob_challenges_device with
 *   kzgx_prove_evals_batch_device and pays no second commit.
 *  Statuses: count > 65535 (the prove path's batch limit): KZGX_ERR_ARG; no SRS:
 *   KZGX_ERR_NO_SRS; 2^log2n larger than the installed SRS: KZGX_ERR_DEGREE; count == 0:
 *   KZGX_OK. */
int kzgx_prove_blobs_batch(kzgx_ctx* ctx, const void* blobs, unsigned log2n, size_t count, int flags,
                           uint8_t* commit_records, uint8_t* proof_records, uint64_t* z_out, uint64_t* y_out);
int kzgx_prove_blobs_batch_device(kzgx_ctx* ctx, const void* d_blobs, unsigned log2n, size_t count, int flags,
                                  void* d_commit_records, void* d_proof_records, void* d_z, void* d_y, void* d_ok,
                                  void* stream);
/* One answer for count (blob, commitment record, proof record) triples with challenges r_k:
 * exactly kzgx_verify_aggregate's equation on (C_k, pi_k, z_k, y_k, r_k), z_k and y_k as
 * defined above, ANDed with "every record decodes (and, with subgroup != 0, lies in the
 * order-r subgroup) and every element is canonical".  Pipeline: ONE decompress-and-check
 * launch over both record arrays (as kzgx_verify_cells_aggregate_bytes), the challenges,
 * the values, the unchanged kzgx_verify_aggregate_device, and the AND of all decode and
 * canonical flags folded on the device: the device form stays asynchronous.
 *  challenges: count x 4 uint64 canonical scalars.  The library does not hash to get them
 *   (a verifier's randomness need not be Fiat-Shamir): explicit challenges give a
 *   deterministic answer; NULL on the host entry draws 128-bit values as
 *   kzgx_verify_aggregate does; NULL on the device entry is KZGX_ERR_ARG.
 *  Needs G1[0] and G2[0..1] only (else KZGX_ERR_NO_SRS): 2^log2n may exceed the SRS.
 *  count == 0 gives *ok = 1; count > KZGX_MSM_POINTS_MAX / 2 - 1: KZGX_ERR_ARG.  d_ok: one
 *   uint32. */
int kzgx_verify_blobs_batch(kzgx_ctx* ctx, const void* blobs, unsigned log2n, size_t count, int flags,
                            const uint8_t* commit_records, const uint8_t* proof_records, const uint64_t* challenges,
                            int subgroup, int* ok);
int kzgx_verify_blobs_batch_device(kzgx_ctx* ctx, const void* d_blobs, unsigned log2n, size_t count, int flags,
                                   const void* d_commit_records, const void* d_proof_records,
                                   const void* d_challenges, int subgroup, void* d_ok, void* stream);
/* The same front end, then kzgx_verify_single_batch_device: one verdict per blob (ok /
 * d_ok: count entries), no challenges.  A blob whose own record does not decode (or fails
 * the subgroup test) or that has an element >= r gets 0; no other blob is affected.  Errors
 * that cancel in the aggregate under equal challenges are reported separately here.
 * count == 0: KZGX_OK, nothing is written.  Limits as kzgx_verify_blobs_batch. */
int kzgx_verify_blobs_each(kzgx_ctx* ctx, const void* blobs, unsigned log2n, size_t count, int flags,
                           const uint8_t* commit_records, const uint8_t* proof_records, int subgroup, int* ok);
int kzgx_verify_blobs_each_device(kzgx_ctx* ctx, const void* d_blobs, unsigned log2n, size_t count, int flags,
                                  const void* d_commit_records, const void* d_proof_records, int subgroup,
                                  void* d_ok, void* stream);

/* ---- setup ceremony (extension) -----------------------------------------------------------
 * A setup is sound when G1[i] = [tau^i] P0 and G2[j] = [tau^j] Q0 for one tau that nobody
 * knows.  kzgx_srs_check tests each point on its own (canonical, on the curve, in the
 * subgroup); a file of valid subgroup points that are not consecutive powers passes it.
 * The entries here are one step of a powers-of-tau ceremony (DESIGN.md "Setup ceremony"):
 * re-randomise tau with a fresh secret, test that a setup has the structure above, and test
 * one contribution against its predecessor.  No transcript format, no verifier of a chain
 * of contributions and no hashing of s: callers compose those from these three. */
/* G1[i] <- [s^(g1_start+i)] G1[i], G2[j] <- [s^(g2_start+j)] G2[j] for every installed
 * point, one lane per point on the device (a 256-bit double-and-add over the lane's own
 * point; the two halves run side by side on two streams): a setup for tau becomes a setup
 * for tau s.  Infinite entries stay infinite.
 *  s: canonical, 4 uint64.  s = 0 or s >= r: KZGX_ERR_ARG, before any device work (the
 *   setup is unchanged).  No G1 SRS: KZGX_ERR_NO_SRS.
 *  g1_start / g2_start: the power of the first installed point, as kzgx_gen_srs_g1's
 *   start (a sharded context that holds powers start.. passes the same start).
 *  The G2 half is updated iff one is installed; both halves are computed into fresh buffers
 *   and installed together, so a failure leaves the old setup, never half of each.
 *  witness_g2_xy (8 / 12 uint64, may be NULL): [s] times the curve's G2 generator, what
 *   kzgx_srs_verify_update needs beside the old and the new G1[1].
 *  Afterwards the context is as after kzgx_load_srs_g1 + kzgx_load_srs_g2 of the new
 *   points: every derived table (the MSM tables, the G2 window table, the verify tables)
 *   and every cached all-domain / coset setup is rebuilt from them, on the call or on first
 *   use.  A default table shared with other contexts is released, not written: the other
 *   contexts keep the table of the old setup.
 *  The call zeroes its device copy of s before it returns; the caller's copy is the
 *   caller's to forget. */
int kzgx_srs_update(kzgx_ctx* ctx, const uint64_t* s, size_t g1_start, size_t g2_start, uint64_t* witness_g2_xy);
/* Is the installed setup (P_0..P_(n-1); Q_0..Q_(m-1)) a run of consecutive powers of one tau?
 *  A  = sum_{i<n-1} rho^i P_i      B  = sum_{i<n-1} rho^i P_(i+1)     one batch of two G1 MSMs
 *  A2 = sum_{j<m-1} sigma^j Q_j    B2 = sum_{j<m-1} sigma^j Q_(j+1)   the G2 MSM, twice
 *  *g1_ok = [e(B, Q_0) == e(A, Q_1)] and P_0 != O and (n < 2 or P_1 != O)
 *  *g2_ok = [e(P_1, A2) == e(P_0, B2)] and Q_0 != O
 * and, with KZGX_SRS_STRUCT_GENERATORS in flags, both also require P_0 and Q_0 to be the
 * curve's generators (what kzgx_gen_srs_g1 / kzgx_gen_srs_g2 start from).  The powers of the
 * challenges are built on the device (one launch per challenge, each lane its own power).
 *  rho, sigma: canonical scalars, 4 uint64 each.  Explicit values make the answer exactly
 *   the equations above and nothing else: errors that cancel under that rho pass.  NULL
 *   draws a 128-bit value from std::random_device, as kzgx_verify_aggregate does (the
 *   bound below then reads (n - 2) / 2^128).
 *  Two conditions, as for the aggregate:
 *   - the pairing is bilinear only on the order-r subgroups, so the test means something
 *     only for members: run kzgx_srs_check with subgroup = 1 first;
 *   - for members, a setup that is not consecutive powers passes with probability at most
 *     (n - 2) / r over a uniform rho ((m - 2) / r over sigma): a nonzero polynomial of that
 *     degree in the challenge vanishes.
 *  n = 1: *g1_ok comes from the non-degeneracy test alone, and *g2_ok = 0 (its equation
 *   needs P_1).  No G1 SRS, or fewer than 2 G2 points: KZGX_ERR_NO_SRS.  rho or sigma >= r,
 *   unknown flag bits: KZGX_ERR_ARG. */
int kzgx_srs_verify_structure(kzgx_ctx* ctx, const uint64_t* rho, const uint64_t* sigma, int flags, int* g1_ok,
                              int* g2_ok);
#define KZGX_SRS_STRUCT_GENERATORS 1 /* also require G1[0], G2[0] == the curve's generators */
/* One contribution against its predecessor: prev and new are G1[1] ([tau]G1) before and
 * after, W the contributor's witness [s]G2gen.
 *  *ok = [e(new, G2gen) == e(prev, W)] and W != O and new != O
 * (all-zero = O), two pairings in one batch.  Needs no SRS.  NULL arguments: KZGX_ERR_ARG.
 * As above, meaningful only for subgroup members (kzgx_g1_check_batch, kzgx_g2_check_batch). */
int kzgx_srs_verify_update(kzgx_ctx* ctx, const uint64_t* prev_tau_g1_xy, const uint64_t* new_tau_g1_xy,
                           const uint64_t* witness_g2_xy, int* ok);

/* ---- batch openings: many polynomials at shared points, one proof each (extensions) ----
 * A prover that has committed to many polynomials opens them at the same few points and
 * ships ONE proof per point, not one per (polynomial, point) pair: KZG is additively
 * homomorphic, so the openings of a group at z are one opening of a weighted sum of the
 * polynomials -- one Fr fold over the coefficients and one MSM per point.  Needs no
 * evaluation domain and serves both curves.  No reference counterpart.
 *
 * Definitions.
 *  - n_polys polynomials P_0 .. P_(n_polys-1) have n >= 1 coefficients each.  They are
 *    canonical scalars.  Polynomial j sits at coeffs + j * coeff_stride (in scalars).
 *    Shorter polynomials are zero-padded by the caller.
 *  - n_groups groups.  Group g opens at the point z_g, which may be any canonical scalar.
 *  - count claims, sorted by group.  The claims of group g are k in
 *    [group_start[g], group_start[g+1]).
 *     - group_start has n_groups + 1 uint32 entries and is non-decreasing.
 *     - group_start[0] = 0 and group_start[n_groups] = count.
 *     - Claim k names polynomial poly_index[k] on the prover side, or commitment
 *       commit_index[k] on the verifier side.
 *     - A polynomial may appear in several groups and more than once in one group.
 *     - A group may be empty.
 *  - Weights w_k, one canonical scalar per claim.
 *     - With the flag KZGX_MULTI_WEIGHT_POWERS, weights holds one scalar gamma_g per group,
 *       and w_k = gamma_g^(k - group_start[g]).  This is the usual "powers of a
 *       Fiat-Shamir challenge".
 *     - The library hashes nothing.  The caller derives gamma, as with every other
 *       challenge in this library.
 *  - F_g = sum_{k in g} w_k P_(poly_index[k]).
 *  - y_k = P_(poly_index[k])(z_g).
 *  - Y_g = sum_{k in g} w_k y_k = F_g(z_g).
 *  - pi_g = [q_g(tau)]G1, where q_g = (F_g - Y_g) / (X - z_g).
 *     - An empty group, or F_g constant, gives pi_g = infinity.
 *  - Verifier, with challenges r_g (one per group) and commitments C_c:
 *     - s_c = sum_{k : commit_index[k] = c} r_(g(k)) w_k
 *     - t = sum_k r_(g(k)) w_k y_k
 *     - *ok = e(sum_g r_g pi_g, G2[1]) == e(sum_c s_c C_c + sum_g (r_g z_g) pi_g - [t] G1[0], G2[0])
 *     - This is exactly kzgx_verify_aggregate's equation on
 *       (C'_g = sum w_k C_k, pi_g, z_g, Y_g, r_g).
 *     - It costs two variable-base MSMs (n_groups points; n_commits + n_groups + 1 points)
 *       and one two-pairing product, whatever count is.
 *
 * Prove.  out_xy / out_is_inf: the n_groups proofs; out_y (may be NULL): the count values
 *  y_k; out_Y (may be NULL): the n_groups values Y_g.  Pipeline, per chunk of
 *  max(1, KZGX_MULTI_CHUNK_SCALARS / n) groups (kzgx_set_multi_chunk changes the figure), at
 *  most 65535 of them, the limit of the prove path: the fold kernel writes F_g into
 *  workspace, then the unchanged kzgx_prove_single_batch_device(F, n, stride n, z, groups)
 *  gives pi_g and Y_g -- one quotient launch and one batched MSM per chunk, never one per
 *  claim, and the MSM on whatever path the context's table settings choose, as for any other
 *  batch.  pi_g is bit for bit what kzgx_prove_single_batch returns for the polynomial F_g
 *  at z_g.  The values y_k come from an evaluation kernel over the claims, in batches sized
 *  by the same figure (the device entry cannot know which claims a chunk of groups holds
 *  without reading group_start back, so the claims are walked on their own): a wavefront per
 *  claim up to KZGX_MULTI_EVAL_SLICE coefficients, slices of KZGX_MULTI_EVAL_SLICE
 *  coefficients per workgroup and a second small launch above.  Workspace per stream is
 *  bounded by the chunk (max(chunk, n) scalars for F, as many for the quotients, and at most
 *  max(chunk, n / KZGX_MULTI_EVAL_SLICE + 1) slice partials), not by count.
 * Verify.  commits: n_commits canonical affine points; proofs: n_groups; ys: count values;
 *  challenges: n_groups canonical scalars r_g.  The _checked forms run the
 *  kzgx_g1_check_batch test over the n_commits commitments and the n_groups proofs first
 *  and force *ok = 0 when a point fails, exactly as kzgx_verify_aggregate_checked does, with
 *  the same subgroup argument.
 *
 * Host entries validate and return KZGX_ERR_ARG before any device work for: a NULL required
 *  pointer, n == 0, coeff_stride < n, an unknown flag bit, a group_start that is not
 *  non-decreasing from 0 to count, an index >= n_polys or >= n_commits, a z, weight or
 *  challenge >= r, count or n_groups >= 2^31, n_commits + n_groups + 1 >
 *  KZGX_MSM_POINTS_MAX.  challenges == NULL on the host verify draws independent 128-bit
 *  values with r_0 = 1, as kzgx_verify_aggregate does.  weights == NULL is always
 *  KZGX_ERR_ARG: the prover and the verifier must agree on the weights.
 * Device entries are asynchronous on stream (NULL = the context's) and read nothing back
 *  (n == 1 excepted: the prove path's empty MSM synchronises).  They check what the host can
 *  see (pointers, sizes, flags).  An out-of-range index or a malformed group_start reads
 *  nothing out of bounds: group ranges are clamped to [0, count], a claim with an index out
 *  of range contributes nothing and its y_k is 0.  Such an input forces *d_ok = 0 (d_ok: one
 *  uint32; on the prove side it may be NULL and reports only this validation).  NULL
 *  challenges are KZGX_ERR_ARG.
 * Other statuses: no SRS: KZGX_ERR_NO_SRS (the verify needs G1[0] and G2[0..1] only);
 *  n - 1 larger than the SRS on the prove side: KZGX_ERR_DEGREE; n_groups == 0 (then count
 *  must be 0): KZGX_OK with *ok = 1.
 *
 * Soundness.  With explicit weights and challenges the answer is a deterministic function
 *  of the inputs: the equation above and nothing else.  A valid batch passes.  Errors can
 *  cancel under weights or challenges the prover can predict (two wrong values +d and -d in
 *  one group under equal weights pass; so do errors in two groups that cancel under the
 *  given r), so gamma and r must come from a transcript that binds the commitments, the
 *  points and the claimed values (gamma) and the proofs as well (r); with unpredictable
 *  128-bit values a false claim passes with probability <= (claims per group + 1) / 2^128.
 *  Points are taken as canonical and on the curve.  Subgroup membership is not checked here
 *  on BLS12-381: that is the _checked forms' business, as for kzgx_verify_aggregate.
 * Out of scope: evaluation-form input (run kzgx_ntt_device first); any hashing of
 *  transcripts; per-group verdicts (fold the commitments with kzgx_msm_g1_points and use
 *  kzgx_verify_single_batch).  Openings of different polynomials at different point sets
 *  under one proof are the Shplonk entries below. */
#define KZGX_MULTI_WEIGHT_POWERS 1 /* weights: one gamma_g per group, w_k = gamma_g^(k - group_start[g]) */
#define KZGX_MULTI_CHUNK_SCALARS 2097152 /* scalars of folded polynomials per internal chunk */
#define KZGX_MULTI_EVAL_SLICE 4096 /* coefficients per workgroup of the sliced evaluation */
int kzgx_prove_multi_batch(kzgx_ctx* ctx, const uint64_t* coeffs, size_t n, size_t coeff_stride, size_t n_polys,
                           const uint32_t* poly_index, const uint32_t* group_start, size_t n_groups,
                           const uint64_t* zs, const uint64_t* weights, size_t count, int flags, uint64_t* out_xy,
                           int* out_is_inf, uint64_t* out_y, uint64_t* out_Y);
int kzgx_prove_multi_batch_device(kzgx_ctx* ctx, const void* d_coeffs, size_t n, size_t coeff_stride, size_t n_polys,
                                  const void* d_poly_index, const void* d_group_start, size_t n_groups,
                                  const void* d_zs, const void* d_weights, size_t count, int flags, void* d_out_xy,
                                  void* d_out_is_inf, void* d_out_y, void* d_out_Y, void* d_ok, void* stream);
int kzgx_verify_multi_batch(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf, size_t n_commits,
                            const uint32_t* commit_index, const uint32_t* group_start, size_t n_groups,
                            const uint64_t* zs, const uint64_t* ys, const uint64_t* weights,
                            const uint64_t* proofs_xy, const int* proof_inf, const uint64_t* challenges, size_t count,
                            int flags, int* ok);
int kzgx_verify_multi_batch_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf, size_t n_commits,
                                   const void* d_commit_index, const void* d_group_start, size_t n_groups,
                                   const void* d_zs, const void* d_ys, const void* d_weights, const void* d_proofs,
                                   const void* d_proof_inf, const void* d_challenges, size_t count, int flags,
                                   void* d_ok, void* stream);
int kzgx_verify_multi_batch_checked(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf,
                                    size_t n_commits, const uint32_t* commit_index, const uint32_t* group_start,
                                    size_t n_groups, const uint64_t* zs, const uint64_t* ys, const uint64_t* weights,
                                    const uint64_t* proofs_xy, const int* proof_inf, const uint64_t* challenges,
                                    size_t count, int flags, int subgroup, int* ok);
int kzgx_verify_multi_batch_checked_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf,
                                           size_t n_commits, const void* d_commit_index, const void* d_group_start,
                                           size_t n_groups, const void* d_zs, const void* d_ys,
                                           const void* d_weights, const void* d_proofs, const void* d_proof_inf,
                                           const void* d_challenges, size_t count, int flags, int subgroup,
                                           void* d_ok, void* stream);
/* test knob: scalars per internal chunk of the prove pipeline (0 restores KZGX_MULTI_CHUNK_SCALARS) */
int kzgx_set_multi_chunk(kzgx_ctx* ctx, size_t scalars);

/* ---- Shplonk openings: many polynomials at different point sets, one two-point proof (extensions) ----
 * A proof system opens different polynomials at different point sets -- most at z, some at
 * z and z w, a few at z, z w and z / w -- and wants one constant-size proof for the whole
 * table.  This is the scheme of BDFG20 section 4 ("Shplonk"): the proof is two G1 points
 * (W, W'), whatever the table holds, and the verifier pays two variable-base MSMs and one
 * two-pairing product.  Needs no evaluation domain and serves both curves.  No reference
 * counterpart.
 *
 * Definitions.
 *  - Polynomials as for the batch openings: n_polys rows of n >= 1 canonical coefficients,
 *    row j at coeffs + j * coeff_stride.
 *  - T: n_points canonical scalars t_0, t_1, ... (points).  Entries of T are told apart BY
 *    INDEX: the same value may sit at two indices, and two sets naming them are unrelated.
 *  - n_sets opening sets.  Set s names the d_s >= 1 entries
 *    set_points[set_point_start[s] .. set_point_start[s+1]) of T (uint32 indices, no index
 *    twice in one set, d_s <= KZGX_SHPLONK_SET_MAX) and the m_s >= 0 claims
 *    k in [claim_start[s], claim_start[s+1]).  Both start arrays have n_sets + 1 uint32
 *    entries, are non-decreasing and run from 0 to n_set_points and to count.
 *  - Claim k names polynomial poly_index[k] (prover) or commitment commit_index[k] (verifier)
 *    and has the weight w_k: one canonical scalar per claim, or, with the flag
 *    KZGX_SHPLONK_WEIGHT_POWERS, weights is ONE scalar gamma and w_k = gamma^k over the
 *    global claim index k.
 *  - Values.  y_(k,i) = P_(poly_index[k])(t_i) for the points of the claim's set, laid out
 *    claim by claim: claim k of set s holds its d_s values, in the set's point order, at
 *    v_s + (k - claim_start[s]) d_s with v_s = sum_(s' < s) d_s' m_s'.  n_values must be
 *    sum_s d_s m_s.
 *  - Z_s = prod_(i in S_s)(X - t_i), F_s = sum_(k in s) w_k P_k, r_k the interpolant of P_k
 *    on S_s, zeta_s = prod_(i in T \ S_s)(z - t_i), Z_T(z) = prod_(i in T)(z - t_i).
 *  - Step 1 (kzgx_shplonk_commit): h = sum_s (F_s - R_s) / Z_s = sum_s (F_s div Z_s), n
 *    scalars with h[n-1] = 0, and W = [h(tau)]G1.  Also the values y.
 *  - Step 2 (kzgx_shplonk_open), for a challenge z the caller derives AFTER seeing W:
 *    G = sum_k zeta_(s(k)) w_k P_k - Z_T(z) h and W' = [(G - G(z)) / (X - z)]G1.  W' is bit
 *    for bit what kzgx_prove_single_batch returns for the polynomial G at z, and the value
 *    it returns, G(z), equals t below for a correct h.
 *  - Verifier.  l_(s,i)(z) = c_(s,i) prod_(j in S_s, j != i)(z - t_j) with
 *    c_(s,i) = 1 / prod_(j != i)(t_i - t_j); r_k(z) = sum_i y_(k,i) l_(s,i)(z);
 *    s_c = sum_(k : commit_index[k] = c) zeta_(s(k)) w_k; t = sum_k zeta_(s(k)) w_k r_k(z);
 *     *ok = e(W', G2[1]) == e(sum_c s_c C_c - [t] G1[0] - Z_T(z) W + z W', G2[0]).
 *    Cost: two variable-base MSMs (1 point; n_commits + 3 points) and one two-pairing
 *    product, whatever T, the sets and the claims are.
 *  Everything is in product form, with no division by (z - t_i): z in T is allowed, and
 *  the answer is then still the equation, though no longer sound.  Two equal VALUES inside
 *  one set make c_(s,i) undefined: KZGX_ERR_DIV_ZERO on the host, *d_ok = 0 on the device.
 *  Equal values at different indices in different sets are fine.
 *
 * Commit.  out_xy / out_is_inf: W.  out_h: the n scalars of h (step 2 takes them back).
 *  out_y (may be NULL): the n_values values.  h comes from a fused multi-point quotient:
 *  F div Z_s = sum_(i in S_s) c_(s,i) (F - F(t_i)) / (X - t_i), so h is a weighted sum of
 *  independent single-point quotients; field sums run in a fixed order without atomics, so
 *  the result is bit-reproducible.  The sets are walked in chunks of
 *  max(1, KZGX_SHPLONK_CHUNK_SCALARS / n) (kzgx_set_shplonk_chunk changes the figure):
 *  the batch openings' fold kernel writes a chunk's F_s into workspace and the quotient
 *  kernels add the chunk's share to h.  Up to KZGX_SHPLONK_TILE coefficients the quotient is
 *  one launch per chunk; above, two more launches carry sums across the tiles.  Workspace per
 *  stream is bounded by the chunk (max(chunk, n) scalars for F, at most n / 16 + 128 per
 *  set of the chunk for the carries), plus one scalar per (set, point) pair and, for the
 *  values, about two per value.  The values come from the batch openings' evaluation kernel
 *  over the (claim, point) list.
 * Open.  The same table, h (n scalars) and z; out_xy / out_is_inf: W'; out_Gz (may be
 *  NULL): G(z).  One fold of all claims under the weights zeta_(s(k)) w_k, one axpy, then
 *  the unchanged kzgx_prove_single_batch_device.
 * Verify.  commits: n_commits canonical affine points; ys: the n_values values;
 *  proof_xy: W then W' (2 points), proof_inf: their 2 flags (may be NULL).  The _checked
 *  forms run the kzgx_g1_check_batch test over the commitments, W and W' first and force
 *  *ok = 0 when a point fails, with the same subgroup argument as
 *  kzgx_verify_multi_batch_checked.
 *
 * Host entries validate and return KZGX_ERR_ARG before any device work for: a NULL required
 *  pointer, n == 0, coeff_stride < n, an unknown flag bit, n_sets == 0 or >= 2^16, a start
 *  array that does not run non-decreasing from 0 to its total, d_s == 0 or
 *  > KZGX_SHPLONK_SET_MAX, n_points == 0 or > KZGX_SHPLONK_POINTS_MAX, an index out of range,
 *  the same index twice in one set, a scalar >= r, n_values != sum_s d_s m_s, count >= 2^31.
 *  Then: equal values in one set: KZGX_ERR_DIV_ZERO; no SRS: KZGX_ERR_NO_SRS (the verify
 *  needs G1[0] and G2[0..1] only); n - 1 larger than the SRS on the prove side:
 *  KZGX_ERR_DEGREE.
 * Device entries are asynchronous on stream (NULL = the context's) and read nothing back
 *  (n == 1 excepted, as for the batch openings).  They check what the host can see
 *  (pointers, sizes, flags; n_values < 2^31).  Whatever the index arrays hold, nothing is
 *  read or written out of bounds: start ranges are clamped to their totals and a set to its
 *  first KZGX_SHPLONK_SET_MAX points, a point index >= n_points is skipped, a claim naming a
 *  polynomial or commitment out of range contributes nothing and its values are 0, values
 *  past n_values are neither written nor read.  Any such input, a repeated index or equal
 *  values in one set, or a wrong n_values forces *d_ok = 0 (one uint32; it may be NULL on
 *  the commit and open side, where it reports only this validation; the open side does not
 *  need c_(s,i) and does not look for equal values).  With *d_ok = 0 the outputs are
 *  defined but meaningless.
 *
 * Soundness.  The library hashes nothing.  With explicit weights and z the answer is a
 *  deterministic function of the inputs: the equation above and nothing else.  An honest
 *  proof passes.  gamma must come from a transcript that binds the commitments, T, the sets
 *  and the claimed values; z must bind W as well -- that is why there are two prover
 *  entries and not one: a prover that knows z before it fixes W can make a false claim
 *  pass.  With unpredictable values a false claim passes with probability about
 *  (count + n) / r.  Points are taken as canonical and on the curve; subgroup membership is
 *  the _checked forms' business.
 * Out of scope: transcript hashing; batching several Shplonk proofs into one check;
 *  evaluation-form input (run kzgx_ntt_device first); a command-line verb. */
#define KZGX_SHPLONK_WEIGHT_POWERS 1 /* weights: one gamma, w_k = gamma^k over the global claim index */
#define KZGX_SHPLONK_SET_MAX 64 /* points per opening set */
#define KZGX_SHPLONK_POINTS_MAX 4096 /* entries of T */
#define KZGX_SHPLONK_CHUNK_SCALARS 2097152 /* scalars of folded polynomials per internal chunk */
#define KZGX_SHPLONK_TILE 2048 /* coefficients per workgroup of the fused quotient: above, carries cross tiles */
int kzgx_shplonk_commit(kzgx_ctx* ctx, const uint64_t* coeffs, size_t n, size_t coeff_stride, size_t n_polys,
                        const uint64_t* points, size_t n_points, const uint32_t* set_point_start,
                        const uint32_t* set_points, size_t n_set_points, const uint32_t* claim_start,
                        const uint32_t* poly_index, size_t n_sets, const uint64_t* weights, size_t count,
                        size_t n_values, int flags, uint64_t* out_xy, int* out_is_inf, uint64_t* out_h,
                        uint64_t* out_y);
int kzgx_shplonk_commit_device(kzgx_ctx* ctx, const void* d_coeffs, size_t n, size_t coeff_stride, size_t n_polys,
                               const void* d_points, size_t n_points, const void* d_set_point_start,
                               const void* d_set_points, size_t n_set_points, const void* d_claim_start,
                               const void* d_poly_index, size_t n_sets, const void* d_weights, size_t count,
                               size_t n_values, int flags, void* d_out_xy, void* d_out_is_inf, void* d_out_h,
                               void* d_out_y, void* d_ok, void* stream);
int kzgx_shplonk_open(kzgx_ctx* ctx, const uint64_t* coeffs, size_t n, size_t coeff_stride, size_t n_polys,
                      const uint64_t* points, size_t n_points, const uint32_t* set_point_start,
                      const uint32_t* set_points, size_t n_set_points, const uint32_t* claim_start,
                      const uint32_t* poly_index, size_t n_sets, const uint64_t* weights, size_t count, int flags,
                      const uint64_t* h, const uint64_t* z, uint64_t* out_xy, int* out_is_inf, uint64_t* out_Gz);
int kzgx_shplonk_open_device(kzgx_ctx* ctx, const void* d_coeffs, size_t n, size_t coeff_stride, size_t n_polys,
                             const void* d_points, size_t n_points, const void* d_set_point_start,
                             const void* d_set_points, size_t n_set_points, const void* d_claim_start,
                             const void* d_poly_index, size_t n_sets, const void* d_weights, size_t count, int flags,
                             const void* d_h, const void* d_z, void* d_out_xy, void* d_out_is_inf, void* d_out_Gz,
                             void* d_ok, void* stream);
int kzgx_shplonk_verify(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf, size_t n_commits,
                        const uint32_t* commit_index, const uint64_t* points, size_t n_points,
                        const uint32_t* set_point_start, const uint32_t* set_points, size_t n_set_points,
                        const uint32_t* claim_start, size_t n_sets, const uint64_t* ys, size_t n_values,
                        const uint64_t* weights, size_t count, const uint64_t* z, const uint64_t* proof_xy,
                        const int* proof_inf, int flags, int* ok);
int kzgx_shplonk_verify_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf, size_t n_commits,
                               const void* d_commit_index, const void* d_points, size_t n_points,
                               const void* d_set_point_start, const void* d_set_points, size_t n_set_points,
                               const void* d_claim_start, size_t n_sets, const void* d_ys, size_t n_values,
                               const void* d_weights, size_t count, const void* d_z, const void* d_proof_xy,
                               const void* d_proof_inf, int flags, void* d_ok, void* stream);
int kzgx_shplonk_verify_checked(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf, size_t n_commits,
                                const uint32_t* commit_index, const uint64_t* points, size_t n_points,
                                const uint32_t* set_point_start, const uint32_t* set_points, size_t n_set_points,
                                const uint32_t* claim_start, size_t n_sets, const uint64_t* ys, size_t n_values,
                                const uint64_t* weights, size_t count, const uint64_t* z, const uint64_t* proof_xy,
                                const int* proof_inf, int flags, int subgroup, int* ok);
int kzgx_shplonk_verify_checked_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf,
                                       size_t n_commits, const void* d_commit_index, const void* d_points,
                                       size_t n_points, const void* d_set_point_start, const void* d_set_points,
                                       size_t n_set_points, const void* d_claim_start, size_t n_sets,
                                       const void* d_ys, size_t n_values, const void* d_weights, size_t count,
                                       const void* d_z, const void* d_proof_xy, const void* d_proof_inf, int flags,
                                       int subgroup, void* d_ok, void* stream);
/* test knob: scalars per internal chunk of the commit pipeline (0 restores KZGX_SHPLONK_CHUNK_SCALARS) */
int kzgx_set_shplonk_chunk(kzgx_ctx* ctx, size_t scalars);

#ifdef __cplusplus
}
#endif

#endif /* KZG_GPU_H */
