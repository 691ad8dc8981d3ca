// Internal (host-side) declarations shared by the libkzgx translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <cstdlib>
#include <vector>

#include "../../include/kzg_gpu.h"

#ifndef KZGX_ACCUM_WAVES
#define KZGX_ACCUM_WAVES 3  // min waves per SIMD for k_msm_accum (VGPR budget)
#endif

#ifndef KZGX_BS_WAVES
#define KZGX_BS_WAVES 2  // min waves per SIMD for k_msm_bucket_sums
#endif

#ifndef KZGX_WINDOW_BITS
#define KZGX_WINDOW_BITS 12  // default signed-digit window (10..13 supported)
#endif

#define KZGX_TRY(expr)                 \
  do {                                 \
    int _rc = (expr);                  \
    if (_rc != KZGX_OK) return _rc;    \
  } while (0)

#define KZGX_TRY_HIP(expr)                              \
  do {                                                  \
    hipError_t _e = (expr);                             \
    if (_e != hipSuccess) return ::kzgx::hip_fail(_e);  \
  } while (0)

namespace kzgx {

int hip_fail(hipError_t e);

// an on/off environment switch: set and starting with '1' (DESIGN.md lists
// every variable the library reads)
static bool env_is_1(const char* name) {
  const char* e = std::getenv(name);
  return e && e[0] == '1';
}

struct MsmWs {
  uint32_t *counts = nullptr, *offsets = nullptr, *cursors = nullptr, *entries = nullptr;
  uint32_t *bsum = nullptr, *heads = nullptr, *tails = nullptr, *tailk = nullptr, *rt = nullptr, *q = nullptr,
           *parts = nullptr, *fpart = nullptr, *fsum = nullptr, *gpart = nullptr, *gmeta = nullptr, *qbig = nullptr;
  uint8_t* sstate = nullptr;
  // variable-base MSM over caller points (msm.hip msm_points): the points in
  // Montgomery form, their infinity flags, the per-(chunk, window) XYZZ sums;
  // verify_aggregate's scalars (r | r z | -sum r y) and its two MSM results
  uint32_t *var_tab = nullptr, *var_parts = nullptr, *var_scal = nullptr, *var_pt = nullptr;
  uint8_t* var_inf = nullptr;
  size_t var_tab_b = 0, var_parts_b = 0, var_scal_b = 0, var_pt_b = 0, var_inf_b = 0;
  uint32_t* lat_cnt = nullptr;  // [64] arrival counters of the one-launch latency path (msm_fixed.hip)
  uint32_t* jidx = nullptr;     // the block table path's (MSM, block, plane) index words (msm_joint.hip)
  size_t jidx_b = 0;
  // evaluation form (ntt.hip, kzgx_api.hip): the two-pass transform's intermediate,
  // and the coefficients handed on to the MSM / the opening pipeline
  uint32_t *ntt_tmp = nullptr, *ntt_coef = nullptr;
  size_t ntt_tmp_b = 0, ntt_coef_b = 0;
  // G1 NTT and all-domain openings (g1_ntt.hip): the XYZZ records of a chunk of
  // transforms, and the chunk's extended coefficient vectors / their transforms
  uint32_t *g1n_rec = nullptr, *fk_c = nullptr;
  size_t g1n_rec_b = 0, fk_c_b = 0;
  // coset openings (g1_ntt.hip): a chunk's zero-padded coefficients / natural-order values for y
  uint32_t* fkm_y = nullptr;
  size_t fkm_y_b = 0;
  // cell recovery (recover.hip): a chunk's size-D arrays (transformed in place), its
  // coefficients when the caller takes none, and the locator values / cell map / flags
  uint32_t *rec_w = nullptr, *rec_coef = nullptr, *rec_aux = nullptr;
  size_t rec_w_b = 0, rec_coef_b = 0, rec_aux_b = 0;
  size_t counts_b = 0, offsets_b = 0, cursors_b = 0, entries_b = 0, bsum_b = 0, heads_b = 0, tails_b = 0, tailk_b = 0,
         rt_b = 0, q_b = 0, parts_b = 0, fpart_b = 0, fsum_b = 0, gpart_b = 0, gmeta_b = 0, sstate_b = 0, qbig_b = 0;
  hipStream_t owner = nullptr;  // workspaces are per stream so calls on
  bool used = false;            // different streams may run concurrently
  uint64_t bound_at = 0;        // Ctx::ws_clock when bound to owner
  hipEvent_t done = nullptr;    // recorded on the owner stream after the last call that used this slot
  bool done_recorded = false;
};

struct Ctx;
// A workspace bound to a stream for the length of one call.  Its destructor
// records the slot's `done` event on that stream after everything the call
// enqueued, so rebinding the slot later waits on the event -- never on the
// old owner stream's handle, which the caller may have destroyed since.
class WsLease {
 public:
  WsLease(Ctx* c, MsmWs* w, hipStream_t st) : c_(c), w_(w), st_(st) {}
  WsLease(const WsLease&) = delete;
  WsLease& operator=(const WsLease&) = delete;
  ~WsLease();
  MsmWs* operator->() const { return w_; }
  MsmWs& operator*() const { return *w_; }
  bool operator!() const { return w_ == nullptr; }
  MsmWs* get() const { return w_; }

 private:
  Ctx* c_;
  MsmWs* w_;
  hipStream_t st_;
};

constexpr int KZGX_MAX_STREAMS = 8;

// Fr NTT (ntt.hip): the largest transform, the largest one a workgroup runs
// out of LDS (2^12 x 32 B = 128 KiB of the CU's 160 KiB), and the 32 KiB tile
// of the small sizes
constexpr int NTT_MAX_LOG2 = KZGX_NTT_MAX_LOG2;
constexpr int NTT_TILE_LOG2 = KZGX_NTT_TILE_LOG2;
constexpr int NTT_SMALL_TILE_LOG2 = 10;
// G1 NTT (g1_ntt.hip): a call's transforms run in chunks of at most this many
// XYZZ records of workspace (one transform at least)
constexpr size_t G1_NTT_CHUNK_RECORDS = KZGX_G1_NTT_CHUNK_POINTS;

// all-domain openings (g1_ntt.hip): X = G1-DFT_2n of the reversed SRS prefix
// for n = 2^k, packed affine Montgomery points with their infinity flags;
// ev is recorded behind the build
struct FkSetup {
  uint32_t *x = nullptr, *inf = nullptr;
  size_t x_b = 0, inf_b = 0;
  bool ready = false;
  hipEvent_t ev = nullptr;
};

// signed subset sums of blocks of g consecutive SRS points (msm_joint.hip):
// entry j < 2^(g_b - 1) of block b = P_top + sum_i (2 j_i - 1) P_i, packed
// affine (x = y = 0: infinity), block stride 2^(g - 1) entries
struct JointTable {
  int g_req = 0;        // -1 automatic, 0 off, 2..25 forced (kzgx_set_fixed_joint)
  uint32_t ranges = 0;  // block ranges per MSM of the accumulation, 0 = automatic
  bool glv = false;     // split every scalar with the curve endomorphism: 2 x 128 planes (KZGX_FIXED_JOINT_GLV)
  // the accumulation's residency reserve (msm_joint.hip "Residency reserve"):
  // wave slots per CU its launch leaves free, -1 = the curve's default
  // (kzgx_set_fixed_accum_reserve, KZGX_FIXED_ACCUM_RESERVE); what
  // joint_reserve_resolve made of it per kernel variant [2 glv + inf]: the
  // reserve in effect and the unused dynamic LDS bytes per workgroup that hold it
  int reserve_req = -1;
  int reserve[4] = {0, 0, 0, 0};
  uint32_t reserve_lds[4] = {0, 0, 0, 0};
  int g = 0;            // built table
  uint32_t blocks = 0;
  size_t n_t = 0;
  uint32_t* d = nullptr;
  size_t bytes = 0;
  uint64_t n_inf = 0;  // entries at infinity (0: the accumulation tests none)
};

// precomputed odd multiples of the SRS prefix (msm_fixed.hip, indexed by
// the regular odd digits of fixed_accum.hpp):
// M[w][i][j] = (2 j + 1) 2^(c w) P_i, packed affine, w < W, i < n_t, j < 2^(c-1)
struct FixedTable {
  int c_req = 0;        // requested window bits (0 = off)
  size_t n_req = 0;     // requested SRS prefix length
  uint32_t pts_per_thread = 0;  // 0 = automatic (fixed_msm_impl)
  int c = 0, W = 0;     // built table
  size_t n_t = 0;
  int layout_req = -1;       // -1 automatic, 0 window-major, 1 point-major
  bool point_major = false;  // built: M[i][w][j] instead of M[w][i][j] (msm_fixed.hip)
  uint32_t* d = nullptr;
  size_t bytes = 0;
  uint8_t* inf = nullptr;  // [n_t] infinite SRS points (skipped)
  bool any_inf = true;     // some flag of inf is set (else the kernels get no flags)
  uint32_t fin0 = UINT32_MAX;  // first finite point of the prefix (k_fixed_accum's identity terms)
  int shared = 0;  // registry id of a shared default table (kzgx_api.hip), 0 = owned by this context
  // the block table built beside it inside the same footprint (the main
  // table only; serves the batched calls, msm_joint.hip)
  JointTable joint;
};

// per-device table memory (kzgx_api.hip): the cached block of the last freed
// default-size table, and the registry of default tables shared by contexts
// with the same device, curve, window and SRS prefix
hipError_t table_malloc(void** p, size_t bytes);
void table_free(void* p, size_t bytes);
void table_cache_release();
size_t table_cache_bytes();
bool table_share_attach(int device, int curve, int c_req, const uint32_t* d_canon, size_t key_words, hipStream_t st,
                        FixedTable& ft);
void table_share_register(int device, int curve, const uint32_t* d_canon, size_t key_words, hipStream_t st,
                          FixedTable& ft);
void table_share_release(FixedTable& ft);
void shared_tables_info(int device, size_t* count, size_t* bytes);

// optional per-kernel timing with HIP events on the launch stream
struct ProfRec {
  const char* name;
  hipEvent_t a, b;
};

// the default table (Ctx::fixed_def): odd multiples of the first 4097 SRS
// points (degree-4096 calls and below) at the widest window c <= 12 whose
// table fits KZGX_DEFAULT_TABLE_PERMILLE of the device's memory -- 45 per
// mille = 13 GB of an MI355X: BN254 c = 12 (11.8 GB), BLS12-381 c = 11
// (9.7 GB).  -1 = that automatic choice, 0 = none, c = a fixed window.
#ifndef KZGX_DEFAULT_TABLE_BITS
#define KZGX_DEFAULT_TABLE_BITS -1
#endif
#ifndef KZGX_DEFAULT_TABLE_POINTS
#define KZGX_DEFAULT_TABLE_POINTS 4097
#endif
#ifndef KZGX_DEFAULT_TABLE_PERMILLE
#define KZGX_DEFAULT_TABLE_PERMILLE 45
#endif
// batches larger than Ctx::small_batch use the default table from this
// window on (below it the batched Pippenger is as fast or faster).  cfg2
// shape, BN254: c = 10 138k-141k / 11 148k-151k / 12 161k-164k against
// Pippenger's 130k per second; cfg4 shape, BLS12-381: c = 10 63k-64k /
// 12 75k against 64k (profiles/r04_default_table_windows.json)
#ifndef KZGX_DEFAULT_TABLE_BATCH_MIN_C_BN
#define KZGX_DEFAULT_TABLE_BATCH_MIN_C_BN 10
#endif
#ifndef KZGX_DEFAULT_TABLE_BATCH_MIN_C_BLS
#define KZGX_DEFAULT_TABLE_BATCH_MIN_C_BLS 11
#endif

// batches of at most this many MSMs use the small-window table (msm.hip)
#ifndef KZGX_SMALL_BATCH
#define KZGX_SMALL_BATCH 16
#endif

struct Ctx {
  int curve = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  int c = KZGX_WINDOW_BITS;  // window bits
  int W = 0;                 // windows
  uint32_t seg_k = 128;      // entries per accumulation thread
  size_t n_srs = 0;
  uint32_t* d_table = nullptr;  // [W][n_srs] affine Montgomery points
  size_t table_bytes = 0;
  // small-batch window table (msm.hip, msm_batch_c): [W_s][n_small] at
  // window KZGX_SMALL_WINDOW_BITS over the first n_small SRS points
  uint32_t* d_table_small = nullptr;
  size_t table_small_bytes = 0;
  size_t n_small = 0;
  hipEvent_t small_ev = nullptr;  // recorded after the small table's build (small_table_ready)
  // wide-window table of the large single MSMs (msm.hip, msm_big):
  // [W_big][n_srs] at c_big bits, built with an SRS of >= 2^16 points
  uint32_t* d_table_big = nullptr;
  size_t table_big_bytes = 0;
  int c_big = 0;  // 0: none / stale
  size_t small_batch = KZGX_SMALL_BATCH;  // largest batch that uses it (0: never)
  uint8_t* d_inf = nullptr;  // [n_srs]
  size_t inf_bytes = 0;
  MsmWs ws[KZGX_MAX_STREAMS];
  FixedTable fixed;
  // the default table: odd multiples at a bounded window over the first SRS
  // points, built with the SRS, read by the MSMs the main table does not
  // serve (msm.hip msm_batch; kzgx_set_default_table); c_req -1 = the
  // window is picked from the memory budget at each build
  FixedTable fixed_def{KZGX_DEFAULT_TABLE_BITS, KZGX_DEFAULT_TABLE_POINTS};
  // the workspace bound to stream st (claimed on first use; every lookup
  // refreshes its use stamp).  With more than KZGX_MAX_STREAMS distinct
  // streams the least recently USED slot is rebound once the work of its
  // last call has drained: hipEventSynchronize of the slot's own event,
  // recorded by the lease after that call's last enqueue (other streams and
  // contexts keep running, and the old owner stream may already be
  // destroyed).  A null lease only if that synchronisation fails.
  uint64_t ws_clock = 0;
  MsmWs* ws_find(hipStream_t st) {
    for (auto& w : ws)
      if (w.used && w.owner == st) return &w;
    return nullptr;
  }
  WsLease ws_for(hipStream_t st) {
    if (MsmWs* w = ws_find(st)) {
      w->bound_at = ++ws_clock;
      return WsLease(this, w, st);
    }
    for (auto& w : ws)
      if (!w.used) {
        w.used = true;
        w.owner = st;
        w.bound_at = ++ws_clock;
        return WsLease(this, &w, st);
      }
    MsmWs* lru = &ws[0];
    for (auto& w : ws)
      if (w.bound_at < lru->bound_at) lru = &w;
    if (lru->done_recorded && hipEventSynchronize(lru->done) != hipSuccess) return WsLease(this, nullptr, st);
    lru->done_recorded = false;
    lru->owner = st;
    lru->bound_at = ++ws_clock;
    return WsLease(this, lru, st);
  }
  // end of a call's use of w on st (WsLease destructor)
  void ws_release(MsmWs* w, hipStream_t st) {
    if (!w->done && hipEventCreateWithFlags(&w->done, hipEventDisableTiming) != hipSuccess) {
      w->done = nullptr;
      (void)hipStreamSynchronize(st);  // no event: drain now, while st is known to be alive
      return;
    }
    w->done_recorded = hipEventRecord(w->done, st) == hipSuccess;
    if (!w->done_recorded) (void)hipStreamSynchronize(st);
  }
  bool prof_on = false;
  std::vector<ProfRec> prof;
  void* d_poly_ws = nullptr;  // scratch for the Fr polynomial kernels
  size_t poly_ws_b = 0;
  void* d_poly_ws2 = nullptr;  // scratch of the multi-point opening pipeline
  size_t poly_ws2_b = 0;
  void* d_g2_ws = nullptr;  // G2 MSM terms (pairing.hip)
  size_t g2_ws_b = 0;
  uint32_t* d_lift = nullptr;  // msm_partial_xyzz's affine result before the lift
  size_t lift_b = 0;
  // Fr NTT twiddles (ntt.hip): w^j, j <= 2^(ntt_log2 - 1), Montgomery form, for
  // the 2^ntt_log2-th root (-1: none yet); ntt_ev is recorded behind the build
  uint32_t* d_ntt_tw = nullptr;
  size_t ntt_tw_b = 0;
  int ntt_log2 = -1;
  hipEvent_t ntt_ev = nullptr;
  // all-domain openings: the setup of each size n = 2^k in use, dropped
  // (ready = false) whenever the G1 SRS is replaced
  FkSetup fk[NTT_MAX_LOG2];
  // coset openings: the setup of each (log2n, log2l) in use -- x[i][t] = value i
  // of G1-DFT_2m of the stride-l SRS slice t, 2n points -- dropped with fk
  FkSetup fkm[NTT_MAX_LOG2 + 1][NTT_MAX_LOG2 + 1];
  // staging for host-pointer entry points
  void* d_stage[4] = {nullptr, nullptr, nullptr, nullptr};
  size_t stage_b[4] = {0, 0, 0, 0};
  int base_words() const { return curve == KZGX_CURVE_BN254 ? 8 : 12; }
};

inline WsLease::~WsLease() {
  if (w_) c_->ws_release(w_, st_);
}

// bracket one launch with events when profiling is enabled
struct ProfScope {
  Ctx* ctx;
  hipStream_t st;
  ProfRec rec;
  ProfScope(Ctx* c, hipStream_t s, const char* name) : ctx(c), st(s) {
    rec.name = nullptr;
    if (!ctx->prof_on) return;
    rec.name = name;
    (void)hipEventCreate(&rec.a);
    (void)hipEventCreate(&rec.b);
    (void)hipEventRecord(rec.a, st);
  }
  ~ProfScope() {
    if (!rec.name) return;
    (void)hipEventRecord(rec.b, st);
    ctx->prof.push_back(rec);
  }
};

// grow-only device allocation (frees the old block)
int dev_alloc(Ctx* ctx, void** p, size_t bytes, size_t* cap);

bool window_bits_supported(int c);
bool fixed_bits_supported(int c);
int fixed_windows(int curve, int c);
int fixed_build(Ctx* ctx, const uint32_t* d_canon, size_t n_srs);  // the main and the default table
int fixed_build_table(Ctx* ctx, FixedTable& ft, const uint32_t* d_canon, size_t n_srs);
int fixed_rebuild_default(Ctx* ctx, const uint32_t* d_canon, size_t n_srs);
void fixed_free(Ctx* ctx);  // the main table
void fixed_free_table(FixedTable& ft);
bool fixed_usable(const Ctx* ctx, size_t n);
bool fixed_table_usable(const FixedTable& ft, size_t n);
int fixed_msm_table(Ctx* ctx, FixedTable& ft, const uint32_t* d_scalars, size_t n, size_t batch, size_t stride_words,
                    uint32_t* d_out, uint32_t* d_out_inf, hipStream_t st, uint32_t* xyzz_out);
int fixed_msm(Ctx* ctx, const uint32_t* d_scalars, size_t n, size_t batch, size_t stride_words, uint32_t* d_out,
              uint32_t* d_out_inf, hipStream_t st, uint32_t* xyzz_out);
// the block table (msm_joint.hip): bytes of one at block size g over n
// points; the (g, window bits) split of set_fixed_base(c, n)'s footprint;
// build / free; whether it serves a call, and the call
size_t joint_table_bytes(int curve, int g, size_t n);
int joint_plan(int curve, int c, size_t n, int g_req, int* g, int* c_win);
int joint_build(Ctx* ctx, JointTable& jt, const uint32_t* d_canon, size_t n, int g);
void joint_free(JointTable& jt);
bool joint_serves(const FixedTable& ft, size_t n, size_t batch, bool xyzz_out);
int joint_msm(Ctx* ctx, FixedTable& ft, const uint32_t* d_scalars, size_t n, size_t batch, size_t stride_words,
              uint32_t* d_out, uint32_t* d_out_inf, hipStream_t st);
// planes per MSM in the block table path's index and partial arrays (>=
// SCALAR_BITS; the planes past SCALAR_BITS are never read), and the planes
// per segment of its Horner pass (joint_horner.hip): stage 1 folds JOINT_SEG
// planes in a lone lane, stage 2 the JOINT_NSEG segment sums in an 8-lane
// group.  Chain per MSM: bits - 1 cooperative doublings whatever the
// segment, JOINT_SEG - 1 lone-lane doublings and additions before them,
// JOINT_NSEG R cooperative additions among them.  Measured per 2048-MSM BN254
// launch, stage 1 + stage 2: 4 planes 0.147 + 0.856 ms, 8 planes 0.216 +
// 0.729 ms, 16 planes 0.261 + 0.649 ms (profiles/joint_horner_serial_kernel_stats_seg*.csv).
// With the endomorphism split (two chains of 127 doublings, stage 1 inlined):
// 8 planes 0.156 + 0.351 ms, 16 planes 0.187 + 0.324 ms (profiles/joint_glv_*.csv).
constexpr uint32_t JOINT_PL = 256;
constexpr uint32_t JOINT_SEG = 16;
constexpr uint32_t JOINT_NSEG = JOINT_PL / JOINT_SEG;
static_assert(JOINT_NSEG * JOINT_SEG == JOINT_PL, "whole segments");
// part[batch][R][JOINT_PL] XYZZ plane sums -> sums[batch] XYZZ; segs: scratch of batch R JOINT_NSEG records
template <class C>
int joint_horner_launch(const uint32_t* part, uint32_t batch, uint32_t R, uint32_t* segs, uint32_t* sums,
                        hipStream_t st);
// the endomorphism split's pass: planes [0, 128) and [128, 256) are the two
// halves' own sums S_1, S_2 (all JOINT_PL planes live); sums: 2 batch records;
// out = S_1 + phi(S_2), canonical affine and infinity flags as k_fixed_finish's;
// narrow: stage 2 in half-wavefront workgroups with half the LDS (beside a
// reserved residency of the accumulation)
template <class C>
int joint_horner_glv_launch(const uint32_t* part, uint32_t batch, uint32_t R, uint32_t* segs, uint32_t* sums,
                            uint32_t* out, uint32_t* out_inf, bool narrow, hipStream_t st);
// the split's default for a curve, and the split of count host scalars as the
// index pass forms it (9 words each: |k1|, |k2|, sign bits) to host out
bool joint_glv_default(int curve);
// the accumulation's residency reserve: the default for a curve, and jt.reserve_req
// resolved against the current device's occupancy query into jt.reserve / jt.reserve_lds
int joint_reserve_default(int curve);
int joint_reserve_resolve(int curve, JointTable& jt);
int joint_glv_debug(Ctx* ctx, const uint32_t* scalars, size_t count, uint32_t* out);
int srs_upload(Ctx* ctx, const uint32_t* d_canon, size_t n);
// mixed additions / s of the fixed-base accumulation loop on L1-resident operands (msm_fixed.hip)
int microbench_mixed_add(Ctx* ctx, double* rate);
int microbench_mad_u64(Ctx* ctx, double* rate, double* ghz);
int clock_probe(Ctx* ctx, hipStream_t st, uint32_t spin_us, uint64_t* d_out);
size_t fixed_table_bytes(int curve, int c, size_t n);
int debug_latency(Ctx* ctx, int op, uint32_t iters, double* res);  // ns, core clocks per op
// one workgroup sums count XYZZ points -> canonical affine (msm.hip)
int xyzz_sum(Ctx* ctx, const uint32_t* d_parts, size_t count, uint32_t* d_out, uint32_t* d_out_inf, hipStream_t st);
int msm_batch(Ctx* ctx, const uint32_t* d_scalars, size_t n, size_t batch, size_t stride_words, uint32_t* d_out,
              uint32_t* d_out_inf, hipStream_t st);
// variable-base MSM (msm.hip): out = sum_k s_k P_k over the concatenation of
// nseg arrays of canonical affine points (inf: uint32 flags or null); the
// total scalars are contiguous in d_scalars.  ws: the caller's lease on st.
struct PointSeg {
  const uint32_t* xy;
  const uint32_t* inf;
  size_t n;
};
constexpr size_t MSM_POINTS_MAX = KZGX_MSM_POINTS_MAX;
int msm_points(Ctx* ctx, MsmWs& ws, const PointSeg* segs, int nseg, const uint32_t* d_scalars, uint32_t* d_out,
               uint32_t* d_out_inf, hipStream_t st);
// verify_aggregate's scalars (poly.hip): d_out = r_0..r_{n-1} | r_k z_k | -sum r_k y_k  (2 n + 1 scalars,
// followed by 256 scalars of scratch for the block sums)
int aggregate_scalars(Ctx* ctx, const uint32_t* d_z, const uint32_t* d_y, const uint32_t* d_r, size_t n,
                      uint32_t* d_out, hipStream_t st);
// verify_cells_aggregate's scalars (poly.hip): from d_T = the count x l inverse transforms of the cells'
// values, d_out = rho_c (n_commits) | s_k = r_k a_(i_k) (count) | -S_t (l), followed by
// cells_fold_slices(count, log2l) * l scalars and as many words of scratch; *d_gate = 1 iff every
// commit_index < n_commits and every cell_index < R = 2^(log2D - log2l).  The twiddle table of the
// size-2^log2D domain must be built (ntt_twiddles) with st ordered behind it.
size_t cells_fold_slices(size_t count, unsigned log2l);
int cells_scalars(Ctx* ctx, const uint32_t* d_T, const uint32_t* d_r, const uint32_t* d_cell_index,
                  const uint32_t* d_commit_index, size_t count, size_t n_commits, unsigned log2l, unsigned log2D,
                  bool bitrev, uint32_t* d_out, uint32_t* d_gate, hipStream_t st);
// verify_cells_each (poly.hip, pairing.hip).  cells_coeffs: in place, d_T = the count x l inverse transforms
// becomes the cells' interpolants I_k (canonical coefficients); d_a[k] = a_(i_k) (canonical), d_bad[k] = 1
// iff commit_index[k] >= n_commits or cell_index[k] >= R.  The twiddle table as for cells_scalars.
// cells_sub: d_out[k] = commits[commit_index[k]] - d_b[k] (canonical affine, infinity flags; no gather for a
// bad cell).  cells_gate: d_ok[k] &= !d_bad[k], and, with d_commit_ok / d_proof_ok (both or neither), &=
// d_commit_ok[commit_index[k]] & d_proof_ok[k].
int cells_coeffs(Ctx* ctx, uint32_t* d_T, const uint32_t* d_cell_index, const uint32_t* d_commit_index, size_t count,
                 size_t n_commits, unsigned log2l, unsigned log2D, bool bitrev, uint32_t* d_a, uint32_t* d_bad,
                 hipStream_t st);
int cells_sub(Ctx* ctx, const uint32_t* d_commits, const uint32_t* d_commit_inf, const uint32_t* d_commit_index,
              const uint32_t* d_bad, const uint32_t* d_b, const uint32_t* d_b_inf, size_t count, uint32_t* d_out,
              uint32_t* d_out_inf, hipStream_t st);
int cells_gate(uint32_t* d_ok, const uint32_t* d_bad, const uint32_t* d_commit_index, const uint32_t* d_commit_ok,
               const uint32_t* d_proof_ok, size_t count, hipStream_t st);
// one MSM as an XYZZ record, no affine conversion (msm.hip)
int msm_partial_xyzz(Ctx* ctx, const uint32_t* d_scalars, size_t n, uint32_t* d_rec, hipStream_t st);
int gen_srs_points(Ctx* ctx, const uint32_t* tau_canon_host, size_t start, size_t n, uint32_t* d_out_canon,
                   hipStream_t st);
int g1_validate(Ctx* ctx, const uint32_t* d_xy, uint32_t* d_ok, hipStream_t st);
int g1_sum(Ctx* ctx, const uint32_t* d_xy, const uint32_t* d_inf, size_t count, uint32_t* d_out, uint32_t* d_out_inf,
           hipStream_t st);

// scalar field (Fr) kernels, poly.hip
int quotient_single(Ctx* ctx, const uint32_t* d_coeffs, size_t n, size_t coeff_stride_words, const uint32_t* d_z,
                    size_t batch, uint32_t* d_q, size_t q_stride_words, uint32_t* d_y, hipStream_t st);
int poly_eval(Ctx* ctx, const uint32_t* d_coeffs, size_t n, const uint32_t* d_x, size_t m, uint32_t* d_y,
              hipStream_t st);
int poly_vanishing(Ctx* ctx, const uint32_t* d_x, size_t n, uint32_t* d_Z, hipStream_t st);
int prove_range_poly(Ctx* ctx, const uint32_t* d_P, size_t n, const uint32_t* d_x, size_t len, uint32_t* d_q,
                     size_t* nq, hipStream_t st);
int poly_interpolate(Ctx* ctx, const uint32_t* d_x, const uint32_t* d_y, size_t n, uint32_t* d_coeffs,
                     hipStream_t st);
int verify_ws_reserve(Ctx* ctx, size_t n);  // poly.hip: workspaces of an n-point verify_proof
int g2_ws_reserve(Ctx* ctx, size_t n);      // pairing.hip: an n-point G2 MSM's workspace

// Fr NTT (ntt.hip): batch transforms of 2^log2n scalars, in_stride / out_stride
// scalars apart (d_in == d_out allowed with equal strides); bitrev: the
// evaluation side is in bit-reversed order.  Asynchronous on st.
int ntt_max_log2(int curve);
int ntt(Ctx* ctx, const uint32_t* d_in, size_t in_stride, uint32_t* d_out, size_t out_stride, unsigned log2n,
        size_t batch, bool inverse, bool bitrev, hipStream_t st);
// the twiddle table of at least the 2^log2n-th root is built, and st ordered
// behind the build; then Ctx::d_ntt_tw / ntt_log2 describe it
int ntt_twiddles(Ctx* ctx, unsigned log2n, hipStream_t st);

// G1 NTT (g1_ntt.hip): batch transforms of 2^log2n canonical affine points
// (d_in_inf: uint32 flags or null), packed; same conventions as ntt().  ws:
// the caller's lease on st.
int g1_ntt(Ctx* ctx, MsmWs& ws, const uint32_t* d_in_xy, const uint32_t* d_in_inf, uint32_t* d_out_xy,
           uint32_t* d_out_inf, unsigned log2n, size_t batch, bool inverse, bool bitrev, hipStream_t st);
// all-domain openings (FK20): the setup X of size 2^log2n from the installed
// SRS (built once, st ordered behind the build), and the batch x n proofs of
// polynomials given by n coefficients each, stride scalars apart
int prove_all_setup(Ctx* ctx, MsmWs& ws, const uint32_t* d_srs_canon, unsigned log2n, hipStream_t st);
int prove_all(Ctx* ctx, MsmWs& ws, const uint32_t* d_srs_canon, const uint32_t* d_coeffs, size_t stride,
              unsigned log2n, size_t batch, bool bitrev, uint32_t* d_out_xy, uint32_t* d_out_inf, hipStream_t st);
void prove_all_drop(Ctx* ctx);  // the SRS changed: every setup is stale
// coset openings (multi-point FK20): the setup of (log2n, log2l), and the batch x R
// proofs, R = 2^(log2n - log2l + ext) cosets of the size-D domain, D = R 2^log2l;
// d_y (may be null): the batch x D values in coset order, or the bit-reversed
// evaluation array with bitrev
int prove_cosets_setup(Ctx* ctx, MsmWs& ws, const uint32_t* d_srs_canon, unsigned log2n, unsigned log2l,
                       hipStream_t st);
int prove_cosets(Ctx* ctx, MsmWs& ws, const uint32_t* d_srs_canon, const uint32_t* d_coeffs, size_t stride,
                 unsigned log2n, unsigned log2l, size_t batch, bool ext, bool bitrev, uint32_t* d_out_xy,
                 uint32_t* d_out_inf, uint32_t* d_y, hipStream_t st);

// cell recovery (recover.hip): blobs b0 .. b0 + cb - 1 of a call (cb 2^(log2n + 1) <=
// max(RECOVER_CHUNK_SCALARS, 2^(log2n + 1))) from the flat cell list of the whole call;
// d_out_y / d_out_coeffs / d_ok point at blob b0's entries.  d_out_y and d_out_coeffs
// may be null; with want_coef and no d_out_coeffs the coefficients (zero for a failed
// blob) are left in ws.rec_coef, packed, for the proofs.  ws: the caller's lease on st.
constexpr size_t RECOVER_CHUNK_SCALARS = KZGX_RECOVER_CHUNK_SCALARS;
int recover_cells(Ctx* ctx, MsmWs& ws, const uint32_t* d_blob_index, const uint32_t* d_cell_index,
                  const uint32_t* d_ys, size_t count, size_t n_blobs, size_t b0, size_t cb, unsigned log2n,
                  unsigned log2l, bool bitrev, bool want_coef, uint32_t* d_out_y, uint32_t* d_out_coeffs,
                  uint32_t* d_ok, hipStream_t st);

// verify path: G2 SRS, polyeval_G2, pairing (pairing.hip)
int gen_srs_g2_points(Ctx* ctx, const uint32_t* d_tau, size_t start, size_t n, uint32_t* d_out, hipStream_t st);
// d_tab (optional): g2_table_build's windowed multiples of the G2 SRS
size_t g2_table_bytes(int curve, size_t n);
int g2_table_build(Ctx* ctx, const uint32_t* d_srs2, size_t n, uint32_t* d_tab, hipStream_t st);
int msm_g2(Ctx* ctx, const uint32_t* d_scalars, const uint32_t* d_srs2, size_t n, uint32_t* d_out,
           uint32_t* d_out_inf, hipStream_t st,
           const uint32_t* d_tab = nullptr);
int g2_validate(Ctx* ctx, const uint32_t* d_xy, size_t count, uint32_t* d_ok, hipStream_t st);
int pairing_batch(Ctx* ctx, const uint32_t* d_g1, const uint32_t* d_g1_inf, const uint32_t* d_g2,
                  const uint32_t* d_g2_inf, size_t count, uint32_t* d_out, hipStream_t st);
int verify_single_batch(Ctx* ctx, const uint32_t* d_commits, const uint32_t* d_commit_inf, const uint32_t* d_proofs,
                        const uint32_t* d_proof_inf, const uint32_t* d_z, const uint32_t* d_y, size_t count,
                        const uint32_t* d_g1_0, const uint32_t* d_g2_01, uint32_t* d_ok, hipStream_t st);
// wave-per-opening verify (pairing.hip): setup-derived tables, then the batch
size_t verify_wave_bytes(int curve);
// g1_comb: the generator's comb (kzgx_setup.hpp GenTables), copied into the
// buffer when G1[0] is the generator; null: computed from G1[0]
int verify_wave_prepare(Ctx* ctx, const uint32_t* d_g1_0, const uint32_t* d_g2_01, const uint32_t* g1_comb,
                        uint32_t* d_buf, hipStream_t st);
int verify_wave_batch(Ctx* ctx, const uint32_t* d_commits, const uint32_t* d_commit_inf, const uint32_t* d_proofs,
                      const uint32_t* d_proof_inf, const uint32_t* d_z, const uint32_t* d_y, size_t count,
                      const uint32_t* d_g1_0, const uint32_t* d_buf, uint32_t* d_ok, hipStream_t st);
// one wave: *ok = e(P_0, Q_0) e(-P_1, Q_1) == 1 (p: 2 canonical affine G1
// points, q: 2 canonical G2 points, inf flags may be NULL; scratch of
// pair2_wave_scratch_bytes for the line tables)
size_t pair2_wave_scratch_bytes(int curve);
int pair2_wave(Ctx* ctx, const uint32_t* d_p, const uint32_t* d_p_inf, const uint32_t* d_q, const uint32_t* d_q_inf,
               uint32_t* d_scratch, uint32_t* d_ok, hipStream_t st);
// the same with Q_1 = G2[0] (d_vw: verify_wave_prepare's buffer) in one
// launch of three waves, Q_0's line chain overlapping the Miller loop; *ok = 2
// for a degenerate chain (rerun pair2_wave); d_q: Q_0 alone, d_q_inf: its flag
int pair2_fused(Ctx* ctx, const uint32_t* d_p, const uint32_t* d_p_inf, const uint32_t* d_q, const uint32_t* d_q_inf,
                const uint32_t* d_vw, uint32_t* d_ok, hipStream_t st);
// batched point validation (subgroup.hip): d_ok[k] = 1 iff point k is
// canonical, on the curve / twist and, with subgroup != 0, of order dividing
// r; infinite entries (d_inf flag, may be NULL, or all-zero words) pass
int g1_check(Ctx* ctx, const uint32_t* d_xy, const uint32_t* d_inf, size_t count, int subgroup, uint32_t* d_ok,
             hipStream_t st);
// two G1 arrays in one launch: d_ok holds count0 + count1 flags, the first array's first
int g1_check2(Ctx* ctx, const uint32_t* d_xy0, const uint32_t* d_inf0, size_t count0, const uint32_t* d_xy1,
              const uint32_t* d_inf1, size_t count1, int subgroup, uint32_t* d_ok, hipStream_t st);
int g2_check(Ctx* ctx, const uint32_t* d_xy, const uint32_t* d_inf, size_t count, int subgroup, uint32_t* d_ok,
             hipStream_t st);
// *d_all = AND of count flags (1 when count == 0); *d_ok = *d_ok && *d_gate
int flags_and(const uint32_t* d_flags, size_t count, uint32_t* d_all, hipStream_t st);
int flag_gate(uint32_t* d_ok, const uint32_t* d_gate, hipStream_t st);
// compressed points (codec.hip).  point_bytes: the record length, 0 when
// (curve, group, encoding) is not offered.  g1_decompress2: two packed record
// arrays in one launch (count1 may be 0), results for count0 + count1 points in
// that order: canonical x || y words, infinity flags (may be null), ok flags.
// The G2 pair is BLS12-381 / KZGX_ENC_ZCASH only.
size_t point_bytes(int curve, int group, int encoding);
int g1_decompress2(Ctx* ctx, const uint8_t* d_b0, size_t count0, const uint8_t* d_b1, size_t count1, int encoding,
                   int subgroup, uint32_t* d_xy, uint32_t* d_inf, uint32_t* d_ok, hipStream_t st);
int g1_compress(Ctx* ctx, const uint32_t* d_xy, const uint32_t* d_inf, size_t count, int encoding, uint8_t* d_out,
                hipStream_t st);
int g2_decompress(Ctx* ctx, const uint8_t* d_b, size_t count, int subgroup, uint32_t* d_xy, uint32_t* d_inf,
                  uint32_t* d_ok, hipStream_t st);
int g2_compress(Ctx* ctx, const uint32_t* d_xy, const uint32_t* d_inf, size_t count, uint8_t* d_out, hipStream_t st);
int g1_sub(Ctx* ctx, const uint32_t* d_a, const uint32_t* d_a_inf, const uint32_t* d_b, const uint32_t* d_b_inf,
           uint32_t* d_out, uint32_t* d_out_inf, hipStream_t st);

}  // namespace kzgx
