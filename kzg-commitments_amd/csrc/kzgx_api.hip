// C ABI of libkzgx.so (declared in include/kzg_gpu.h).  Thin host layer:
// argument checks, staging copies for the host-pointer entry points, and
// dispatch into the HIP kernels of msm.hip / poly.hip / srs.hip.  No compute
// happens on the host and there is no CPU fallback: without a gfx950 device
// kzgx_create fails with KZGX_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>

#include <array>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <random>
#include <string>
#include <vector>

#include "blob.hpp"
#include "curve_consts.h"
#include "fr_host.hpp"
#include "kzgx_internal.hpp"
#include "kzgx_setup.hpp"
#include "multi_open.hpp"
#include "shplonk.hpp"

// a generated G2 SRS of at most this many points gets its polyeval_G2 window
// table at setup (kzgx_gen_srs_g2); larger ones on first use
#ifndef KZGX_G2TAB_EAGER_MAX
#define KZGX_G2TAB_EAGER_MAX 16385
#endif

struct kzgx_ctx {
  kzgx::Ctx c;
  uint32_t* d_srs_canon = nullptr;  // installed SRS, canonical affine
  size_t srs_canon_b = 0;
  uint32_t* d_srs2_canon = nullptr;  // installed G2 SRS, canonical affine (x.re, x.im, y.re, y.im)
  size_t srs2_canon_b = 0;
  size_t n_srs2 = 0;
  // wave-per-opening verify: tables derived from G1[0], G2[0..1] (built on
  // first use, dropped when either SRS changes)
  uint32_t* d_vw = nullptr;
  size_t vw_b = 0;
  bool vw_ready = false;
  size_t vw_max = 8192;  // batches up to this size take the wave path
  // per-cell verification (kzgx_verify_cells_each), per coset size l: the staged
  // pair G2[0] || G2[l] of the lane path and, on the wave path's first use, the
  // buffer verify_wave_prepare builds from it; dropped when either SRS changes
  struct CellsG2 {
    uint32_t *d_q = nullptr, *d_vw = nullptr;
  };
  std::map<size_t, CellsG2> cells_g2;
  size_t cells_chunk = 0;  // cells per internal chunk (0 = KZGX_VERIFY_CELLS_EACH_CHUNK)
  // windowed multiples of the G2 SRS for polyeval_G2 (built on first use)
  uint32_t* d_g2tab = nullptr;
  size_t g2tab_b = 0;
  size_t g2tab_n = 0;  // points covered; 0 = stale
  // per-point flags of the batched point checks, one buffer per workspace
  // slot of c.ws (so per stream, as the MSM workspaces are)
  uint32_t* d_chk[kzgx::KZGX_MAX_STREAMS] = {};
  size_t chk_b[kzgx::KZGX_MAX_STREAMS] = {};
  // the blob entries' buffers (decoded limbs, recovered points, z, y, flags), per slot as d_chk
  uint32_t* d_blob[kzgx::KZGX_MAX_STREAMS] = {};
  size_t blob_b[kzgx::KZGX_MAX_STREAMS] = {};
  // the batch openings' buffers (a chunk's folded polynomials, the sliced evaluation's partials, the
  // verifier's gate word), per slot as d_chk; multi_chunk: scalars per chunk (0 = KZGX_MULTI_CHUNK_SCALARS)
  uint32_t* d_multi[kzgx::KZGX_MAX_STREAMS] = {};
  size_t multi_b[kzgx::KZGX_MAX_STREAMS] = {};
  size_t multi_chunk = 0;
  // the Shplonk openings' buffers (pair constants, a chunk's folded polynomials and tile carries, the
  // value list, the verifier's scalars), per slot as d_chk; shplonk_chunk: scalars per chunk
  // (0 = KZGX_SHPLONK_CHUNK_SCALARS)
  uint32_t* d_shp[kzgx::KZGX_MAX_STREAMS] = {};
  size_t shp_b[kzgx::KZGX_MAX_STREAMS] = {};
  size_t shplonk_chunk = 0;

  // pinned, device-mapped host staging for the host-pointer entry points
  // (kzgx_msm_g1_batch, kzgx_prove_single_batch): inputs are copied into it
  // and read by the kernels in place (small) or DMA'd from it (large); the
  // last kernel of a call writes its results straight into it, so a call
  // makes no device-to-host copy and synchronises once
  uint8_t* h_pin = nullptr;
  uint8_t* d_pin = nullptr;  // device address of h_pin
  size_t pin_b = 0;

  // verify_proof's side stream (from the device pool, on first use): the G2
  // half ([Z(tau)]G2) runs there beside the G1 half (I, [I(tau)]G1, C - it)
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
};

// a setup changed: the per-cell verify's G2 pairs and line tables are stale
// (hipFree waits for the work that may still read them)
static void cells_g2_drop(kzgx_ctx* ctx) {
  for (auto& e : ctx->cells_g2) {
    if (e.second.d_q) (void)hipFree(e.second.d_q);
    if (e.second.d_vw) (void)hipFree(e.second.d_vw);
  }
  ctx->cells_g2.clear();
}

namespace kzgx {

int hip_fail(hipError_t e) { return e == hipErrorOutOfMemory ? KZGX_ERR_OOM : KZGX_ERR_HIP; }

// Freed table blocks are cached per device for later tables.  A
// trusted_setup per degree (the reference benchmark,
// benchmark/benchmark.cpp:19-38) otherwise frees one default table and
// allocates the next.  Why that matters: the amdgpu driver wipes released
// VRAM before it hands it out again, at ~30 GB/s, and work on a block that
// lands on freed memory waits for that wipe (137 GB freed -> the next large
// hipMalloc 4.1-4.9 s, 0.3 ms on clean memory; scripts/probe_alloc.hip,
// profiles/r06_probe_alloc.jsonl).  So a freed block of 64 MB .. 32 GB is kept (up to 32 GB per device in all,
// oldest evicted first), a request takes the smallest cached block that
// fits it with at most 2x + 64 MB slack, and a request nothing fits gets a
// fresh allocation beside the cached blocks -- freeing them first would put
// it on memory that is being wiped.  The cache is released on an allocation
// failure, when the last context of the device is destroyed, and by
// kzgx_release_cached_memory; KZGX_NO_TABLE_CACHE=1 turns it off.
namespace {
struct TableBlock {
  void* p = nullptr;
  size_t bytes = 0;
};
constexpr size_t CACHE_MIN = (size_t)64 << 20;
constexpr size_t CACHE_CAP = (size_t)32 << 30;
std::mutex g_table_mu;
std::vector<TableBlock> g_table_cache[64];  // oldest first
size_t g_cache_bytes[64];
std::map<void*, size_t> g_block_bytes;  // true size of each block table_malloc handed out
int g_live_ctx[64];  // live contexts per device (guarded by g_table_mu)
bool table_cache_off() {
  static const bool off = kzgx::env_is_1("KZGX_NO_TABLE_CACHE");
  return off;
}
int current_device() {
  int dev = 0;
  return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 ? dev : -1;
}
void cache_release_locked(int dev) {
  for (auto& b : g_table_cache[dev]) {
    g_block_bytes.erase(b.p);
    (void)hipFree(b.p);
  }
  g_table_cache[dev].clear();
  g_cache_bytes[dev] = 0;
}
}  // namespace

void table_cache_release() {
  const int dev = current_device();
  if (dev < 0) return;
  std::lock_guard<std::mutex> lk(g_table_mu);
  cache_release_locked(dev);
}

// a context created (+1) or destroyed (-1) on `dev`; the last one to go
// releases the device's cached blocks (nothing else would)
void ctx_live_add(int dev, int delta) {
  if (dev < 0 || dev >= 64) return;
  std::lock_guard<std::mutex> lk(g_table_mu);
  g_live_ctx[dev] += delta;
  if (g_live_ctx[dev] <= 0) {
    g_live_ctx[dev] = 0;
    cache_release_locked(dev);
  }
}

// bytes held by the current device's cached blocks: memory a table build may
// count as free (table_malloc reuses them or releases them on failure)
size_t table_cache_bytes() {
  const int dev = current_device();
  if (dev < 0) return 0;
  std::lock_guard<std::mutex> lk(g_table_mu);
  return g_cache_bytes[dev];
}

hipError_t table_malloc(void** p, size_t bytes) {
  const int dev = current_device();
  if (dev >= 0) {
    std::lock_guard<std::mutex> lk(g_table_mu);
    auto& c = g_table_cache[dev];
    int best = -1;
    for (int k = 0; k < (int)c.size(); k++)
      if (c[k].bytes >= bytes && c[k].bytes <= 2 * bytes + CACHE_MIN && (best < 0 || c[k].bytes < c[best].bytes))
        best = k;
    if (best >= 0) {
      *p = c[best].p;
      g_cache_bytes[dev] -= c[best].bytes;
      c.erase(c.begin() + best);
      return hipSuccess;
    }
  }
  hipError_t e = hipMalloc(p, bytes);
  if (e == hipErrorOutOfMemory && dev >= 0) {  // the cached blocks may be what is missing
    (void)hipGetLastError();
    {
      std::lock_guard<std::mutex> lk(g_table_mu);
      cache_release_locked(dev);
    }
    e = hipMalloc(p, bytes);
  }
  if (e == hipSuccess) {
    std::lock_guard<std::mutex> lk(g_table_mu);
    g_block_bytes[*p] = bytes;
  }
  return e;
}

void table_free(void* p, size_t bytes) {
  if (!p) return;
  const int dev = current_device();
  std::lock_guard<std::mutex> lk(g_table_mu);
  const auto it = g_block_bytes.find(p);
  if (it != g_block_bytes.end()) bytes = it->second;  // the block's own size (it may have served a smaller table)
  // blocks of 64 MB .. 32 GB: an opt-in table of hundreds of GB is freed at once
  if (table_cache_off() || bytes < CACHE_MIN || bytes > CACHE_CAP || dev < 0) {
    if (it != g_block_bytes.end()) g_block_bytes.erase(it);
    (void)hipFree(p);
    return;
  }
  auto& c = g_table_cache[dev];
  c.push_back(TableBlock{p, bytes});
  g_cache_bytes[dev] += bytes;
  while (g_cache_bytes[dev] > CACHE_CAP && !c.empty()) {  // oldest first
    g_cache_bytes[dev] -= c.front().bytes;
    g_block_bytes.erase(c.front().p);
    (void)hipFree(c.front().p);
    c.erase(c.begin());
  }
}

// Shared default tables: contexts on one
// device whose SRS starts with the same points (compared word for word, not
// by a hash) and that pick the same window share one default table, counted
// by reference.  kzgx_msm_g1_sharded-style callers and repeated trusted
// setups then hold one 11.8 GB table, not one per context.
namespace {
struct SharedTable {
  int id = 0;
  int device = 0, curve = 0;
  uint32_t* d_key = nullptr;  // device copy of the canonical SRS prefix the table was built from
  size_t key_words = 0;
  FixedTable t;  // owner's view of the table (d, inf, c, W, n_t, ...)
  int refs = 0;
};
std::vector<SharedTable> g_shared;  // guarded by g_table_mu
int g_shared_next = 1;

// *differ = (a[0..words) != b[0..words)), both on the device, compared by a
// kernel that stores into a mapped host word: the setup path makes no
// device-to-host copy (a 32 KB one stalled 6-18 ms now and then inside the
// reference benchmark's 512-term setup, profiles/r06_kzg_bench_trace_setup.txt)
__global__ void k_words_differ(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, size_t words,
                               volatile uint32_t* __restrict__ flag) {
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < words; k += (size_t)gridDim.x * blockDim.x)
    if (a[k] != b[k]) *flag = 1u;  // every writer stores the same value
}
int words_differ(const uint32_t* a, const uint32_t* b, size_t words, hipStream_t st, bool* differ) {
  thread_local uint32_t* h_flag = nullptr;  // mapped pinned word, kept for the thread
  thread_local uint32_t* d_flag = nullptr;
  if (!h_flag) {
    KZGX_TRY_HIP(hipHostMalloc((void**)&h_flag, 64, hipHostMallocMapped | hipHostMallocCoherent));
    KZGX_TRY_HIP(hipHostGetDevicePointer((void**)&d_flag, h_flag, 0));
  }
  *(volatile uint32_t*)h_flag = 0u;
  const unsigned blocks = (unsigned)std::min<size_t>((words + 255) / 256, 1024);
  hipLaunchKernelGGL(k_words_differ, dim3(blocks ? blocks : 1), dim3(256), 0, st, a, b, words, d_flag);
  KZGX_TRY_HIP(hipGetLastError());
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  *differ = *(volatile uint32_t*)h_flag != 0u;
  return KZGX_OK;
}
}  // namespace

bool table_share_attach(int device, int curve, int c_req, const uint32_t* d_canon, size_t key_words, hipStream_t st,
                        FixedTable& ft) {
  std::lock_guard<std::mutex> lk(g_table_mu);
  for (auto& e : g_shared) {
    if (e.device != device || e.curve != curve || (c_req > 0 && e.t.c != c_req) || e.key_words != key_words) continue;
    bool differ = true;
    if (words_differ(e.d_key, d_canon, key_words, st, &differ) != KZGX_OK || differ) continue;
    const uint32_t ppt = ft.pts_per_thread;
    const int c_keep = ft.c_req;
    const size_t n_keep = ft.n_req;
    const int layout_keep = ft.layout_req;
    ft = e.t;
    ft.pts_per_thread = ppt;
    ft.c_req = c_keep;
    ft.n_req = n_keep;
    ft.layout_req = layout_keep;
    ft.shared = e.id;
    e.refs++;
    return true;
  }
  return false;
}

// ft (just built from d_canon's first key_words words) becomes shareable; a
// failure to keep the key just leaves it unshared
void table_share_register(int device, int curve, const uint32_t* d_canon, size_t key_words, hipStream_t st,
                          FixedTable& ft) {
  uint32_t* d_key = nullptr;
  if (hipMalloc((void**)&d_key, key_words * 4) != hipSuccess) {
    (void)hipGetLastError();
    return;
  }
  if (hipMemcpyAsync(d_key, d_canon, key_words * 4, hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    (void)hipFree(d_key);
    return;
  }
  std::lock_guard<std::mutex> lk(g_table_mu);
  SharedTable e;
  e.id = g_shared_next++;
  e.device = device;
  e.curve = curve;
  e.d_key = d_key;
  e.key_words = key_words;
  e.t = ft;
  e.refs = 1;
  ft.shared = e.id;
  g_shared.push_back(std::move(e));
}

// drop ft's reference; the last one frees the table (into the block cache)
void table_share_release(FixedTable& ft) {
  void* d = nullptr;
  uint8_t* inf = nullptr;
  uint32_t* key = nullptr;
  size_t bytes = 0;
  {
    std::lock_guard<std::mutex> lk(g_table_mu);
    for (size_t k = 0; k < g_shared.size(); k++) {
      if (g_shared[k].id != ft.shared) continue;
      if (--g_shared[k].refs == 0) {
        d = g_shared[k].t.d;
        inf = g_shared[k].t.inf;
        key = g_shared[k].d_key;
        bytes = g_shared[k].t.bytes;
        g_shared.erase(g_shared.begin() + (long)k);
      }
      break;
    }
  }
  if (d) table_free(d, bytes);
  if (inf) (void)hipFree(inf);
  if (key) (void)hipFree(key);
}

void shared_tables_info(int device, size_t* count, size_t* bytes) {
  std::lock_guard<std::mutex> lk(g_table_mu);
  size_t c = 0, b = 0;
  for (auto& e : g_shared)
    if (e.device == device) c++, b += e.t.bytes;
  *count = c;
  *bytes = b;
}

int dev_alloc(Ctx* ctx, void** p, size_t bytes, size_t* cap) {
  (void)ctx;
  if (bytes == 0) bytes = 16;
  if (*p && bytes <= *cap) return KZGX_OK;
  if (*p) {
    KZGX_TRY_HIP(hipDeviceSynchronize());
    KZGX_TRY_HIP(hipFree(*p));
    *p = nullptr;
    *cap = 0;
  }
  // round up to limit re-allocation churn
  size_t want = bytes + bytes / 8;
  hipError_t e = hipMalloc(p, want);
  if (e != hipSuccess) {
    *p = nullptr;
    table_cache_release();  // a cached table block may be what is missing
    e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
      *p = nullptr;
      return hip_fail(e);
    }
    want = bytes;
  }
  *cap = want;
  return KZGX_OK;
}

}  // namespace kzgx

using kzgx::Ctx;

namespace {

int activate(kzgx_ctx* ctx) {
  if (!ctx) return KZGX_ERR_ARG;
  KZGX_TRY_HIP(hipSetDevice(ctx->c.device));
  return KZGX_OK;
}

hipStream_t pick(kzgx_ctx* ctx, void* stream) { return stream ? (hipStream_t)stream : ctx->c.stream; }

int stage(kzgx_ctx* ctx, int slot, size_t bytes, void** out) {
  KZGX_TRY(kzgx::dev_alloc(&ctx->c, &ctx->c.d_stage[slot], bytes, &ctx->c.stage_b[slot]));
  *out = ctx->c.d_stage[slot];
  return KZGX_OK;
}

size_t point_words(const kzgx_ctx* ctx) { return 2 * (size_t)ctx->c.base_words(); }

// the context's pinned mapped staging of at least `bytes` (grow-only)
int pin_stage(kzgx_ctx* ctx, size_t bytes) {
  if (ctx->h_pin && bytes <= ctx->pin_b) return KZGX_OK;
  if (ctx->h_pin) {
    KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
    (void)hipHostFree(ctx->h_pin);
    ctx->h_pin = ctx->d_pin = nullptr;
    ctx->pin_b = 0;
  }
  const size_t want = std::max<size_t>(bytes + bytes / 8, (size_t)1 << 20);
  void* h = nullptr;
  KZGX_TRY_HIP(hipHostMalloc(&h, want, hipHostMallocMapped | hipHostMallocCoherent));
  void* d = nullptr;
  const hipError_t e = hipHostGetDevicePointer(&d, h, 0);
  if (e != hipSuccess) {
    (void)hipHostFree(h);
    return kzgx::hip_fail(e);
  }
  ctx->h_pin = static_cast<uint8_t*>(h);
  ctx->d_pin = static_cast<uint8_t*>(d);
  ctx->pin_b = want;
  return KZGX_OK;
}

// kernels read inputs up to this size straight from the mapped staging
// (PCIe reads, no copy launch); larger inputs are DMA'd to device memory
constexpr size_t PIN_DIRECT_MAX = (size_t)256 << 10;

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// x mod r for a 4 x 64-bit little-endian value: the reference converts its
// evaluation points into ZZ_p (src/trusted_setup.cpp:214-219), so x and x + r
// are the same point.  Argument normalisation only (a handful of compares and
// subtractions per point), done before the repeated-point check.
template <class FR>
std::array<uint64_t, 4> fr_reduce(const uint64_t* x) {
  uint64_t r[4], v[4] = {x[0], x[1], x[2], x[3]};
  for (int i = 0; i < 4; i++) r[i] = (uint64_t)FR::P[2 * i] | ((uint64_t)FR::P[2 * i + 1] << 32);
  for (;;) {
    int i = 3;
    while (i >= 0 && v[i] == r[i]) i--;
    if (i >= 0 && v[i] < r[i]) break;  // v < r (i < 0: v == r, reduces to 0)
    unsigned __int128 borrow = 0;
    for (int k = 0; k < 4; k++) {
      const unsigned __int128 d = (unsigned __int128)v[k] - r[k] - borrow;
      v[k] = (uint64_t)d;
      borrow = (d >> 64) & 1;
    }
  }
  return {v[0], v[1], v[2], v[3]};
}

// gfx950 device check shared by kzgx_create and kzgx_init_device
int device_ok(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return KZGX_ERR_NO_DEVICE;
  if (device < 0 || device >= ndev) return KZGX_ERR_ARG;
  hipDeviceProp_t prop;
  KZGX_TRY_HIP(hipGetDeviceProperties(&prop, device));
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) return KZGX_ERR_NO_DEVICE;
  return KZGX_OK;
}

int setup_finish(kzgx_ctx* ctx);

}  // namespace

extern "C" {

const char* kzgx_strerror(int s) {
  switch (s) {
    case KZGX_OK: return "ok";
    case KZGX_ERR_ARG: return "invalid argument";
    case KZGX_ERR_HIP: return "HIP runtime error";
    case KZGX_ERR_OOM: return "device out of memory";
    case KZGX_ERR_NO_SRS: return "no SRS loaded";
    case KZGX_ERR_DEGREE: return "polynomial degree be at most one less than the setup size (num_coeffs)";
    case KZGX_ERR_INTERNAL: return "internal error";
    case KZGX_ERR_NO_DEVICE: return "no gfx950 (MI355X) device available";
    case KZGX_ERR_DIV_ZERO: return "division by zero (duplicate interpolation point)";
    default: return "unknown status";
  }
}

int kzgx_base_limbs(int curve) {
  return curve == KZGX_CURVE_BN254 ? 4 : curve == KZGX_CURVE_BLS12381 ? 6 : -1;
}

// Context streams are pooled per device: creating one costs 1.5-2 ms (the
// first few of a process up to 8.5 ms, each new hardware queue), and the
// reference benchmark builds one trusted_setup per degree
// (profiles/r05_kzg_bench_trace: the 128-term setup's stream creation was a
// third of its time).  Destroyed contexts return theirs after a sync.
namespace {
std::mutex g_stream_mu;
std::vector<hipStream_t> g_stream_pool[64];
constexpr size_t STREAM_POOL_MAX = 4;
hipError_t stream_take(int device, hipStream_t* s) {
  if (device >= 0 && device < 64) {
    std::lock_guard<std::mutex> lk(g_stream_mu);
    if (!g_stream_pool[device].empty()) {
      *s = g_stream_pool[device].back();
      g_stream_pool[device].pop_back();
      return hipSuccess;
    }
  }
  return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}
void stream_give(int device, hipStream_t s) {
  if (!s) return;
  if (device >= 0 && device < 64) {
    std::lock_guard<std::mutex> lk(g_stream_mu);
    if (g_stream_pool[device].size() < STREAM_POOL_MAX) {
      g_stream_pool[device].push_back(s);
      return;
    }
  }
  (void)hipStreamDestroy(s);
}
}  // namespace

int kzgx_init_device(int curve, int device) {
  if (curve != KZGX_CURVE_BN254 && curve != KZGX_CURVE_BLS12381) return KZGX_ERR_ARG;
  KZGX_TRY(device_ok(device));
  KZGX_TRY_HIP(hipSetDevice(device));
  // the streams of the first contexts (kzg::init's default context, the
  // first trusted_setup), created here, outside the timed regions
  hipStream_t spare[3] = {nullptr, nullptr, nullptr};  // (+1: verify_proof's side stream)
  for (auto& s2 : spare) KZGX_TRY_HIP(stream_take(device, &s2));
  for (auto s2 : spare) stream_give(device, s2);
  hipStream_t st = nullptr;
  KZGX_TRY_HIP(stream_take(device, &st));
  struct StreamGuard {
    hipStream_t s;
    int d;
    ~StreamGuard() {
      (void)hipStreamSynchronize(s);
      stream_give(d, s);
    }
  } sg{st, device};
  // every code object of the library, once (the first launch of any kernel
  // of a translation unit loads its whole object)
  int (*const warm[])(hipStream_t) = {
      kzgx::warm_setup,      kzgx::warm_msm,        kzgx::warm_msm_fixed,   kzgx::warm_poly,
      kzgx::warm_srs,        kzgx::warm_pairing,    kzgx::warm_verify_wave, kzgx::warm_latency,
      kzgx::warm_fixed_bn_a, kzgx::warm_fixed_bn_b, kzgx::warm_fixed_bn_c,  kzgx::warm_fixed_bn_d,
      kzgx::warm_fixed_bls_a, kzgx::warm_fixed_bls_b, kzgx::warm_fixed_bls_c, kzgx::warm_fixed_bls_d,
      kzgx::warm_subgroup,   kzgx::warm_msm_joint,  kzgx::warm_joint_horner, kzgx::warm_srs_update};
  for (auto f : warm) KZGX_TRY(f(st));
  // the generator comb tables (per process, per device and curve)
  kzgx::GenTables g;
  KZGX_TRY(kzgx::gen_tables_get(curve, device, st, &g));
  // the pinned-allocation path of the host-pointer calls
  void* h = nullptr;
  KZGX_TRY_HIP(hipHostMalloc(&h, 4096, hipHostMallocMapped | hipHostMallocCoherent));
  (void)hipHostFree(h);
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  return KZGX_OK;
}

int kzgx_create(kzgx_ctx** out, int curve, int device) {
  if (!out || (curve != KZGX_CURVE_BN254 && curve != KZGX_CURVE_BLS12381)) return KZGX_ERR_ARG;
  *out = nullptr;
  KZGX_TRY(device_ok(device));
  kzgx_ctx* ctx = new (std::nothrow) kzgx_ctx();
  if (!ctx) return KZGX_ERR_OOM;
  ctx->c.curve = curve;
  ctx->c.device = device;
  if (const char* e = getenv("KZGX_WINDOW_BITS")) {
    int c = atoi(e);
    if (kzgx::window_bits_supported(c)) ctx->c.c = c;
  }
  ctx->c.W = (257 + ctx->c.c - 1) / ctx->c.c;
  // the block table beside the main fixed-base table: automatic unless
  // $KZGX_FIXED_JOINT says otherwise (0 = off: the window table alone)
  ctx->c.fixed.joint.g_req = -1;
  if (const char* e = getenv("KZGX_FIXED_JOINT")) {
    const int g = atoi(e);
    if (g == -1 || g == 0 || (g >= 2 && g <= 25)) ctx->c.fixed.joint.g_req = g;
  }
  // the block table's endomorphism split: the curve's default unless set (1 on, 0 the 254 / 255-plane path)
  ctx->c.fixed.joint.glv = kzgx::joint_glv_default(curve);
  if (const char* e = getenv("KZGX_FIXED_JOINT_GLV")) {
    if (e[0] == '0' && !e[1]) ctx->c.fixed.joint.glv = false;
    if (e[0] == '1' && !e[1]) ctx->c.fixed.joint.glv = true;
  }
  if (const char* e = getenv("KZGX_FIXED_JOINT_RANGES")) {  // kzgx_set_fixed_joint_ranges' default, for A/B runs
    const int r = atoi(e);
    if (r >= 0 && r <= 8) ctx->c.fixed.joint.ranges = (uint32_t)r;
  }
  // the block table accumulation's residency reserve: the curve's default
  // unless set (-1, or wave slots per CU left free; anything else is ignored)
  if (const char* e = getenv("KZGX_FIXED_ACCUM_RESERVE")) {
    char* end = nullptr;
    const long r = strtol(e, &end, 10);
    if (end != e && !*end && r >= -1 && r <= 64) ctx->c.fixed.joint.reserve_req = (int)r;
  }
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = stream_take(device, &ctx->c.stream);
  if (e != hipSuccess) {
    delete ctx;
    return kzgx::hip_fail(e);
  }
  if (const int rc = kzgx::joint_reserve_resolve(curve, ctx->c.fixed.joint)) {
    stream_give(device, ctx->c.stream);
    delete ctx;
    return rc;
  }
  kzgx::ctx_live_add(device, +1);
  *out = ctx;
  return KZGX_OK;
}

int kzgx_release_cached_memory(int device) {
  if (device < 0 || device >= 64) return KZGX_ERR_ARG;
  int prev = 0;
  KZGX_TRY_HIP(hipGetDevice(&prev));
  KZGX_TRY_HIP(hipSetDevice(device));
  kzgx::table_cache_release();
  return hipSetDevice(prev) == hipSuccess ? KZGX_OK : KZGX_ERR_HIP;
}

int kzgx_shared_tables(int device, size_t* count, size_t* bytes) {
  if (!count || !bytes || device < 0 || device >= 64) return KZGX_ERR_ARG;
  kzgx::shared_tables_info(device, count, bytes);
  return KZGX_OK;
}

void kzgx_destroy(kzgx_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->c.device);
  (void)hipStreamSynchronize(ctx->c.stream);
  (void)kzgx_prof_clear(ctx);
  cells_g2_drop(ctx);
  Ctx& c = ctx->c;
  void* bufs[] = {c.d_table, c.d_table_small, c.d_table_big, c.d_inf, c.d_stage[0], c.d_stage[1], c.d_stage[2], c.d_stage[3],
                  c.d_poly_ws, c.d_poly_ws2, ctx->d_srs_canon, ctx->d_srs2_canon, c.d_g2_ws, ctx->d_vw, ctx->d_g2tab,
                  c.d_lift, c.d_ntt_tw};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  for (void* p : ctx->d_chk)
    if (p) (void)hipFree(p);
  for (void* p : ctx->d_blob)
    if (p) (void)hipFree(p);
  for (void* p : ctx->d_multi)
    if (p) (void)hipFree(p);
  for (void* p : ctx->d_shp)
    if (p) (void)hipFree(p);
  for (auto& f : c.fk) {
    if (f.x) (void)hipFree(f.x);
    if (f.inf) (void)hipFree(f.inf);
    if (f.ev) (void)hipEventDestroy(f.ev);
  }
  for (auto& row : c.fkm)
    for (auto& f : row) {
      if (f.x) (void)hipFree(f.x);
      if (f.inf) (void)hipFree(f.inf);
      if (f.ev) (void)hipEventDestroy(f.ev);
    }
  kzgx::fixed_free(&c);
  kzgx::fixed_free_table(c.fixed_def);
  for (auto& w : c.ws) {
    void* wb[] = {w.counts, w.offsets, w.cursors, w.entries, w.bsum,  w.heads,
                  w.tails,  w.tailk,   w.rt,      w.q,       w.parts, w.fpart, w.fsum, w.gpart, w.gmeta, w.sstate, w.qbig,
                  w.lat_cnt, w.var_tab, w.var_parts, w.var_scal, w.var_pt, w.var_inf, w.ntt_tmp, w.ntt_coef,
                  w.g1n_rec, w.fk_c, w.fkm_y, w.jidx, w.rec_w, w.rec_coef, w.rec_aux};
    for (void* p : wb)
      if (p) (void)hipFree(p);
    if (w.done) (void)hipEventDestroy(w.done);
  }
  if (ctx->h_pin) (void)hipHostFree(ctx->h_pin);
  if (c.small_ev) (void)hipEventDestroy(c.small_ev);
  if (c.ntt_ev) (void)hipEventDestroy(c.ntt_ev);
  if (ctx->side) {
    (void)hipStreamSynchronize(ctx->side);
    stream_give(c.device, ctx->side);
  }
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  (void)hipStreamSynchronize(c.stream);
  stream_give(c.device, c.stream);
  kzgx::ctx_live_add(c.device, -1);
  delete ctx;
}

int kzgx_sync(kzgx_ctx* ctx) {
  KZGX_TRY(activate(ctx));
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  return KZGX_OK;
}

void* kzgx_stream(kzgx_ctx* ctx) { return ctx ? (void*)ctx->c.stream : nullptr; }

int kzgx_prof_enable(kzgx_ctx* ctx, int on) {
  KZGX_TRY(activate(ctx));
  ctx->c.prof_on = on != 0;
  return KZGX_OK;
}

int kzgx_prof_read(kzgx_ctx* ctx, const char* name, double* total_ms, int* count) {
  KZGX_TRY(activate(ctx));
  if (!name || !total_ms || !count) return KZGX_ERR_ARG;
  double tot = 0;
  int cnt = 0;
  std::vector<kzgx::ProfRec> keep;
  for (auto& r : ctx->c.prof) {
    if (std::strcmp(r.name, name) != 0) {
      keep.push_back(r);
      continue;
    }
    KZGX_TRY_HIP(hipEventSynchronize(r.b));
    float ms = 0;
    KZGX_TRY_HIP(hipEventElapsedTime(&ms, r.a, r.b));
    tot += ms;
    cnt++;
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  ctx->c.prof.swap(keep);
  *total_ms = tot;
  *count = cnt;
  return KZGX_OK;
}

int kzgx_prof_clear(kzgx_ctx* ctx) {
  KZGX_TRY(activate(ctx));
  for (auto& r : ctx->c.prof) {
    (void)hipEventSynchronize(r.b);
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  ctx->c.prof.clear();
  return KZGX_OK;
}

int kzgx_set_window_bits(kzgx_ctx* ctx, int c) {
  KZGX_TRY(activate(ctx));
  if (!kzgx::window_bits_supported(c)) return KZGX_ERR_ARG;
  if (ctx->c.n_srs != 0) return KZGX_ERR_ARG;  // the fixed-base table depends on c
  ctx->c.c = c;
  ctx->c.W = (257 + c - 1) / c;
  return KZGX_OK;
}

int kzgx_set_small_batch(kzgx_ctx* ctx, unsigned max_batch) {
  KZGX_TRY(activate(ctx));
  if (max_batch > 65535) return KZGX_ERR_ARG;
  ctx->c.small_batch = max_batch;
  return KZGX_OK;
}

int kzgx_set_segment(kzgx_ctx* ctx, unsigned k) {
  KZGX_TRY(activate(ctx));
  if (k < 1 || k > 4096) return KZGX_ERR_ARG;
  ctx->c.seg_k = k;
  return KZGX_OK;
}

int kzgx_set_fixed_base(kzgx_ctx* ctx, int c, size_t n_points) {
  KZGX_TRY(activate(ctx));
  if (!kzgx::fixed_bits_supported(c)) return KZGX_ERR_ARG;
  if (c != 0 && n_points == 0) return KZGX_ERR_ARG;
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  kzgx::fixed_free(&ctx->c);
  ctx->c.fixed.c_req = c;
  ctx->c.fixed.n_req = c ? n_points : 0;
  if (c != 0 && ctx->c.n_srs != 0)
    KZGX_TRY(kzgx::fixed_build_table(&ctx->c, ctx->c.fixed, ctx->d_srs_canon, ctx->c.n_srs));  // the default table stays
  return KZGX_OK;
}

int kzgx_set_default_table(kzgx_ctx* ctx, int c, size_t n_points) {
  KZGX_TRY(activate(ctx));
  if (c != -1 && !kzgx::fixed_bits_supported(c)) return KZGX_ERR_ARG;
  if (c != 0 && n_points == 0) return KZGX_ERR_ARG;
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  kzgx::fixed_free_table(ctx->c.fixed_def);
  ctx->c.fixed_def.c_req = c;
  ctx->c.fixed_def.n_req = c ? n_points : 0;
  if (c != 0 && ctx->c.n_srs != 0) KZGX_TRY(kzgx::fixed_rebuild_default(&ctx->c, ctx->d_srs_canon, ctx->c.n_srs));
  return KZGX_OK;
}

int kzgx_default_table_info(const kzgx_ctx* ctx, int* c, size_t* n_points, size_t* bytes) {
  if (!ctx) return KZGX_ERR_ARG;
  if (c) *c = ctx->c.fixed_def.c;
  if (n_points) *n_points = ctx->c.fixed_def.n_t;
  if (bytes) *bytes = ctx->c.fixed_def.bytes;
  return KZGX_OK;
}

int kzgx_set_fixed_base_layout(kzgx_ctx* ctx, int layout) {
  KZGX_TRY(activate(ctx));
  if (layout < -1 || layout > 1) return KZGX_ERR_ARG;
  ctx->c.fixed.layout_req = layout;
  return KZGX_OK;
}

int kzgx_fixed_base_layout(const kzgx_ctx* ctx, int* point_major) {
  if (!ctx || !point_major) return KZGX_ERR_ARG;
  *point_major = ctx->c.fixed.point_major ? 1 : 0;
  return KZGX_OK;
}

int kzgx_fixed_base_info(const kzgx_ctx* ctx, int* c, size_t* n_points, size_t* bytes) {
  if (!ctx) return KZGX_ERR_ARG;
  if (c) *c = ctx->c.fixed.c ? ctx->c.fixed.c_req : 0;  // the request; the window table itself may be narrower
  if (n_points) *n_points = ctx->c.fixed.n_t;
  if (bytes) *bytes = ctx->c.fixed.bytes + ctx->c.fixed.joint.bytes;
  return KZGX_OK;
}

int kzgx_set_fixed_joint(kzgx_ctx* ctx, int g) {
  KZGX_TRY(activate(ctx));
  if (g != -1 && g != 0 && (g < 2 || g > 25)) return KZGX_ERR_ARG;
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  const int keep = ctx->c.fixed.joint.g_req;
  ctx->c.fixed.joint.g_req = g;
  if (ctx->c.fixed.c_req != 0 && ctx->c.n_srs != 0) {
    const int rc = kzgx::fixed_build_table(&ctx->c, ctx->c.fixed, ctx->d_srs_canon, ctx->c.n_srs);
    if (rc == KZGX_ERR_ARG) ctx->c.fixed.joint.g_req = keep;  // no split fits: the tables stay as they were
    return rc;
  }
  return KZGX_OK;
}

int kzgx_set_fixed_joint_ranges(kzgx_ctx* ctx, unsigned ranges) {
  KZGX_TRY(activate(ctx));
  if (ranges > 8) return KZGX_ERR_ARG;  // 0 = automatic
  ctx->c.fixed.joint.ranges = ranges;
  return KZGX_OK;
}

int kzgx_set_fixed_accum_reserve(kzgx_ctx* ctx, int r) {
  KZGX_TRY(activate(ctx));
  if (r < -1) return KZGX_ERR_ARG;  // -1 = the curve's default; an over-large r is clamped
  kzgx::JointTable& jt = ctx->c.fixed.joint;
  const int keep = jt.reserve_req;
  jt.reserve_req = r;
  const int rc = kzgx::joint_reserve_resolve(ctx->c.curve, jt);  // later launches only
  if (rc != KZGX_OK) jt.reserve_req = keep;
  return rc;
}

int kzgx_fixed_accum_reserve_info(const kzgx_ctx* ctx, int* request, int* reserve, size_t* lds_bytes, int* variant) {
  if (!ctx) return KZGX_ERR_ARG;
  const kzgx::JointTable& jt = ctx->c.fixed.joint;
  const int v = (jt.glv ? 2 : 0) + (jt.n_inf ? 1 : 0);  // the kernel variant the next call launches
  if (request) *request = jt.reserve_req;
  if (reserve) *reserve = jt.reserve[v];
  if (lds_bytes) *lds_bytes = jt.reserve_lds[v];
  if (variant) *variant = v;
  return KZGX_OK;
}

int kzgx_fixed_joint_info(const kzgx_ctx* ctx, int* g, size_t* blocks, size_t* bytes) {
  if (!ctx) return KZGX_ERR_ARG;
  if (g) *g = ctx->c.fixed.joint.g;
  if (blocks) *blocks = ctx->c.fixed.joint.blocks;
  if (bytes) *bytes = ctx->c.fixed.joint.bytes;
  return KZGX_OK;
}

int kzgx_fixed_window_info(const kzgx_ctx* ctx, int* c, size_t* bytes) {
  if (!ctx) return KZGX_ERR_ARG;
  if (c) *c = ctx->c.fixed.c;
  if (bytes) *bytes = ctx->c.fixed.bytes;
  return KZGX_OK;
}

int kzgx_fixed_base_bytes(int curve, int c, size_t n_points, size_t* bytes) {
  if (!bytes || (curve != KZGX_CURVE_BN254 && curve != KZGX_CURVE_BLS12381) || !kzgx::fixed_bits_supported(c))
    return KZGX_ERR_ARG;
  *bytes = kzgx::fixed_table_bytes(curve, c, n_points);
  return KZGX_OK;
}

int kzgx_set_fixed_base_budget(kzgx_ctx* ctx, size_t budget_bytes, size_t n_points, int* c_out) {
  KZGX_TRY(activate(ctx));
  if (!c_out || n_points == 0) return KZGX_ERR_ARG;
  *c_out = 0;
  // the budget is sized against the free HBM after the SRS and its window
  // tables exist, and for the points that will actually be tabled
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  if (n_points > ctx->c.n_srs) n_points = ctx->c.n_srs;
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  kzgx::fixed_free(&ctx->c);  // the old table's memory counts as free
  size_t free_b = 0, total_b = 0;
  KZGX_TRY_HIP(hipMemGetInfo(&free_b, &total_b));
  free_b += kzgx::table_cache_bytes();  // reused or released by table_malloc
  const size_t margin = (size_t)4 << 30;
  const size_t avail = free_b > margin ? free_b - margin : 0;
  const size_t cap = budget_bytes < avail ? budget_bytes : avail;
  for (int c = 17; c >= 7; c--) {
    if (kzgx::fixed_table_bytes(ctx->c.curve, c, n_points) > cap) continue;
    const int rc = kzgx_set_fixed_base(ctx, c, n_points);
    if (rc == KZGX_OK) {
      *c_out = c;
      return KZGX_OK;
    }
    if (rc != KZGX_ERR_OOM) {
      ctx->c.fixed.c_req = 0;  // no half-requested window left for the next SRS upload
      ctx->c.fixed.n_req = 0;
      return rc;
    }
  }
  ctx->c.fixed.c_req = 0;
  ctx->c.fixed.n_req = 0;
  return KZGX_OK;
}

int kzgx_microbench_mad_u64(kzgx_ctx* ctx, double* lane_ops_per_s) {
  KZGX_TRY(activate(ctx));
  if (!lane_ops_per_s) return KZGX_ERR_ARG;
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  return kzgx::microbench_mad_u64(&ctx->c, lane_ops_per_s, nullptr);
}

int kzgx_microbench_mad_u64_clock(kzgx_ctx* ctx, double* lane_ops_per_s, double* core_ghz) {
  KZGX_TRY(activate(ctx));
  if (!lane_ops_per_s || !core_ghz) return KZGX_ERR_ARG;
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  return kzgx::microbench_mad_u64(&ctx->c, lane_ops_per_s, core_ghz);
}

int kzgx_clock_probe(kzgx_ctx* ctx, void* stream, unsigned spin_us, void* d_out) {
  KZGX_TRY(activate(ctx));
  if (!d_out || spin_us == 0 || spin_us > 10000000u) return KZGX_ERR_ARG;
  return kzgx::clock_probe(&ctx->c, pick(ctx, stream), spin_us, static_cast<uint64_t*>(d_out));
}

int kzgx_microbench_mixed_add(kzgx_ctx* ctx, double* adds_per_s) {
  KZGX_TRY(activate(ctx));
  if (!adds_per_s) return KZGX_ERR_ARG;
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  return kzgx::microbench_mixed_add(&ctx->c, adds_per_s);
}

int kzgx_set_fixed_points_per_thread(kzgx_ctx* ctx, unsigned p) {
  KZGX_TRY(activate(ctx));
  if (p > 1024) return KZGX_ERR_ARG;  // 0 = automatic
  ctx->c.fixed.pts_per_thread = p;
  return KZGX_OK;
}

int kzgx_curve(const kzgx_ctx* ctx) { return ctx ? ctx->c.curve : -1; }

size_t kzgx_srs_size(const kzgx_ctx* ctx) { return ctx ? ctx->c.n_srs : 0; }

int kzgx_load_srs_g1(kzgx_ctx* ctx, const uint64_t* xy, size_t n) {
  KZGX_TRY(activate(ctx));
  ctx->vw_ready = false;
  cells_g2_drop(ctx);
  kzgx::prove_all_drop(&ctx->c);
  if (!xy || n == 0) return KZGX_ERR_ARG;
  const size_t bytes = n * point_words(ctx) * 4;
  KZGX_TRY(kzgx::dev_alloc(&ctx->c, (void**)&ctx->d_srs_canon, bytes, &ctx->srs_canon_b));
  KZGX_TRY_HIP(hipMemcpyAsync(ctx->d_srs_canon, xy, bytes, hipMemcpyHostToDevice, ctx->c.stream));
  KZGX_TRY(kzgx::srs_upload(&ctx->c, ctx->d_srs_canon, n));
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  return setup_finish(ctx);
}

int kzgx_gen_srs_g1(kzgx_ctx* ctx, const uint64_t* tau, size_t start, size_t n) {
  KZGX_TRY(activate(ctx));
  ctx->vw_ready = false;
  cells_g2_drop(ctx);
  kzgx::prove_all_drop(&ctx->c);
  if (!tau || n == 0 || n > 0x7fffffffu) return KZGX_ERR_ARG;
  const size_t bytes = n * point_words(ctx) * 4;
  KZGX_TRY(kzgx::dev_alloc(&ctx->c, (void**)&ctx->d_srs_canon, bytes, &ctx->srs_canon_b));
  void* d_tau;
  KZGX_TRY(stage(ctx, 0, 32, &d_tau));
  KZGX_TRY_HIP(hipMemcpyAsync(d_tau, tau, 32, hipMemcpyHostToDevice, ctx->c.stream));
  kzgx::GenTables g;
  KZGX_TRY(kzgx::gen_tables_get(ctx->c.curve, ctx->c.device, ctx->c.stream, &g));
  KZGX_TRY(kzgx::gen_srs_g1_comb(ctx->c.curve, (const uint32_t*)d_tau, start, n, g.g1_comb, ctx->d_srs_canon,
                                 ctx->c.stream));
  KZGX_TRY(kzgx::srs_upload(&ctx->c, ctx->d_srs_canon, n));
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  return setup_finish(ctx);
}

int kzgx_get_srs_g1(kzgx_ctx* ctx, uint64_t* xy, size_t n) {
  KZGX_TRY(activate(ctx));
  if (!xy) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  if (n > ctx->c.n_srs) return KZGX_ERR_ARG;
  KZGX_TRY_HIP(hipMemcpyAsync(xy, ctx->d_srs_canon, n * point_words(ctx) * 4, hipMemcpyDeviceToHost, ctx->c.stream));
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  return KZGX_OK;
}

int kzgx_msm_g1_batch_device(kzgx_ctx* ctx, const void* d_scalars, size_t n, size_t batch, size_t scalar_stride,
                             void* d_out_xy, void* d_out_is_inf, void* stream) {
  KZGX_TRY(activate(ctx));
  if (batch == 0) return KZGX_OK;
  if (!d_out_xy || !d_out_is_inf || (n > 0 && !d_scalars) || batch > 65535) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  if (n > ctx->c.n_srs) return KZGX_ERR_DEGREE;
  if (batch > 1 && scalar_stride < n) return KZGX_ERR_ARG;
  hipStream_t st = pick(ctx, stream);
  if (n == 0) {  // zero polynomial: ECP_inf (trusted_setup.cpp:150-154)
    KZGX_TRY_HIP(hipMemsetAsync(d_out_xy, 0, batch * point_words(ctx) * 4, st));
    std::vector<uint32_t> ones(batch, 1u);
    KZGX_TRY_HIP(hipMemcpyAsync(d_out_is_inf, ones.data(), batch * 4, hipMemcpyHostToDevice, st));
    KZGX_TRY_HIP(hipStreamSynchronize(st));
    return KZGX_OK;
  }
  return kzgx::msm_batch(&ctx->c, (const uint32_t*)d_scalars, n, batch, scalar_stride * 8, (uint32_t*)d_out_xy,
                         (uint32_t*)d_out_is_inf, st);
}

int kzgx_msm_g1_batch(kzgx_ctx* ctx, const uint64_t* scalars, size_t n, size_t batch, uint64_t* out_xy,
                      int* out_is_inf) {
  KZGX_TRY(activate(ctx));
  if (batch == 0) return KZGX_OK;
  if (!out_xy || !out_is_inf || (n > 0 && !scalars)) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  if (n > ctx->c.n_srs) return KZGX_ERR_DEGREE;
  const size_t sb = n * batch * 32, ob = batch * point_words(ctx) * 4;
  // pinned layout: [results | flags | scalars]; results are written by the
  // last kernel into mapped host memory (no D2H copy).  Scalars up to
  // PIN_DIRECT_MAX are read by the kernels from the pinned copy; larger
  // ones are DMA'd straight from the caller's buffer (no host copy, and the
  // pinned buffer stays small: ADVICE r04)
  const bool direct = sb <= PIN_DIRECT_MAX;
  const size_t o_off = 0, i_off = align256(ob), s_off = i_off + align256(batch * 4);
  KZGX_TRY(pin_stage(ctx, s_off + (direct ? sb : 0)));
  void* d_s = nullptr;
  if (n) {
    if (direct) {
      std::memcpy(ctx->h_pin + s_off, scalars, sb);
      d_s = ctx->d_pin + s_off;
    } else {
      KZGX_TRY(stage(ctx, 0, sb, &d_s));
      KZGX_TRY_HIP(hipMemcpyAsync(d_s, scalars, sb, hipMemcpyHostToDevice, ctx->c.stream));
    }
  }
  KZGX_TRY(kzgx_msm_g1_batch_device(ctx, d_s, n, batch, n, ctx->d_pin + o_off, ctx->d_pin + i_off, nullptr));
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  std::memcpy(out_xy, ctx->h_pin + o_off, ob);
  const uint32_t* inf = reinterpret_cast<const uint32_t*>(ctx->h_pin + i_off);
  for (size_t b = 0; b < batch; b++) out_is_inf[b] = (int)inf[b];
  return KZGX_OK;
}

int kzgx_msm_g1(kzgx_ctx* ctx, const uint64_t* scalars, size_t n, uint64_t* out_xy, int* out_is_inf) {
  return kzgx_msm_g1_batch(ctx, scalars, n, 1, out_xy, out_is_inf);
}

int kzgx_quotient_single_batch_device(kzgx_ctx* ctx, const void* d_coeffs, size_t n, size_t coeff_stride,
                                      const void* d_z, size_t batch, void* d_q, size_t q_stride, void* d_y,
                                      void* stream) {
  KZGX_TRY(activate(ctx));
  if (batch == 0) return KZGX_OK;
  if (!d_z || (n > 0 && !d_coeffs) || (n > 1 && !d_q) || n > 0xffffffffu) return KZGX_ERR_ARG;
  if (batch > 1 && coeff_stride != 0 && coeff_stride < n) return KZGX_ERR_ARG;
  return kzgx::quotient_single(&ctx->c, (const uint32_t*)d_coeffs, n, coeff_stride * 8, (const uint32_t*)d_z, batch,
                               (uint32_t*)d_q, q_stride * 8, (uint32_t*)d_y, pick(ctx, stream));
}

int kzgx_quotient_single_batch(kzgx_ctx* ctx, const uint64_t* coeffs, size_t n, size_t coeff_stride,
                               const uint64_t* zs, size_t batch, uint64_t* q_out, uint64_t* y_out) {
  KZGX_TRY(activate(ctx));
  if (batch == 0) return KZGX_OK;
  if (!zs || (n > 0 && !coeffs) || (n > 1 && !q_out) || n > 0xffffffffu) return KZGX_ERR_ARG;
  if (batch > 1 && coeff_stride != 0 && coeff_stride < n) return KZGX_ERR_ARG;
  const size_t nc = coeff_stride == 0 ? n : (batch - 1) * coeff_stride + n;  // coefficient rows read
  const size_t nq = n > 1 ? n - 1 : 0;
  void *d_c = nullptr, *d_z, *d_q = nullptr, *d_y;
  if (nc) KZGX_TRY(stage(ctx, 0, nc * 32, &d_c));
  KZGX_TRY(stage(ctx, 1, batch * 32, &d_z));
  if (nq) KZGX_TRY(stage(ctx, 2, batch * nq * 32, &d_q));
  KZGX_TRY(stage(ctx, 3, batch * 32, &d_y));
  hipStream_t st = ctx->c.stream;
  if (nc) KZGX_TRY_HIP(hipMemcpyAsync(d_c, coeffs, nc * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_z, zs, batch * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY(kzgx::quotient_single(&ctx->c, (const uint32_t*)d_c, n, coeff_stride * 8, (const uint32_t*)d_z, batch,
                                 (uint32_t*)d_q, nq * 8, (uint32_t*)d_y, st));
  if (nq) KZGX_TRY_HIP(hipMemcpyAsync(q_out, d_q, batch * nq * 32, hipMemcpyDeviceToHost, st));
  if (y_out) KZGX_TRY_HIP(hipMemcpyAsync(y_out, d_y, batch * 32, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  return KZGX_OK;
}

int kzgx_prove_single_batch_device(kzgx_ctx* ctx, const void* d_coeffs, size_t n, size_t coeff_stride,
                                   const void* d_z, size_t batch, void* d_out_xy, void* d_out_is_inf, void* d_y,
                                   void* stream) {
  KZGX_TRY(activate(ctx));
  if (batch == 0) return KZGX_OK;
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  const size_t nq = n > 0 ? n - 1 : 0;
  if (nq > ctx->c.n_srs) return KZGX_ERR_DEGREE;
  hipStream_t st = pick(ctx, stream);
  kzgx::WsLease ws = ctx->c.ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  void* d_q = nullptr;
  if (nq) {
    KZGX_TRY(kzgx::dev_alloc(&ctx->c, (void**)&ws->q, nq * batch * 32, &ws->q_b));
    d_q = ws->q;
  }
  KZGX_TRY(kzgx_quotient_single_batch_device(ctx, d_coeffs, n, coeff_stride, d_z, batch, d_q, nq, d_y, st));
  return kzgx_msm_g1_batch_device(ctx, d_q, nq, batch, nq, d_out_xy, d_out_is_inf, st);
}

int kzgx_prove_range(kzgx_ctx* ctx, const uint64_t* coeffs, size_t n, const uint64_t* xs, size_t len,
                     uint64_t* out_xy, int* out_is_inf) {
  KZGX_TRY(activate(ctx));
  if (!xs || !out_xy || !out_is_inf || len == 0 || (n > 0 && !coeffs) || len > (1u << 24)) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  while (n > 0 && (coeffs[4 * (n - 1)] | coeffs[4 * (n - 1) + 1] | coeffs[4 * (n - 1) + 2] | coeffs[4 * (n - 1) + 3]) == 0)
    n--;  // NTL keeps polynomials normalized
  if (n > len && n - len > ctx->c.n_srs) return KZGX_ERR_DEGREE;
  // the points as residues mod r (x and x + r are one point, as in ZZ_p)
  std::vector<uint64_t> xr(4 * len);
  for (size_t i = 0; i < len; i++) {
    const auto v = ctx->c.curve == KZGX_CURVE_BN254 ? fr_reduce<kzgx::BN254Fr>(xs + 4 * i)
                                                    : fr_reduce<kzgx::BLS12381Fr>(xs + 4 * i);
    std::copy(v.begin(), v.end(), xr.begin() + 4 * i);
  }
  {
    // repeated points: the reference's interpolation (NTL polyfit) fails on
    // them, so does this call (P div Z alone would still be defined)
    std::vector<std::array<uint64_t, 4>> sorted(len);
    for (size_t i = 0; i < len; i++) sorted[i] = {xr[4 * i + 3], xr[4 * i + 2], xr[4 * i + 1], xr[4 * i]};
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return KZGX_ERR_DIV_ZERO;
  }
  hipStream_t st = ctx->c.stream;
  kzgx::WsLease ws = ctx->c.ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  void *d_c = nullptr, *d_x, *d_o;
  if (n) KZGX_TRY(stage(ctx, 0, n * 32, &d_c));
  KZGX_TRY(stage(ctx, 1, len * 32, &d_x));
  KZGX_TRY(stage(ctx, 2, point_words(ctx) * 4 + 16, &d_o));
  if (n) KZGX_TRY_HIP(hipMemcpyAsync(d_c, coeffs, n * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_x, xr.data(), len * 32, hipMemcpyHostToDevice, st));
  size_t nq = 0;
  if (n > len) {
    KZGX_TRY(kzgx::dev_alloc(&ctx->c, (void**)&ws->q, (n - len) * 32, &ws->q_b));
    KZGX_TRY(kzgx::prove_range_poly(&ctx->c, (const uint32_t*)d_c, n, (const uint32_t*)d_x, len, ws->q, &nq, st));
  }
  uint32_t* d_oi = (uint32_t*)((char*)d_o + point_words(ctx) * 4);
  KZGX_TRY(kzgx_msm_g1_batch_device(ctx, ws->q, nq, 1, nq, d_o, d_oi, st));
  uint32_t oi = 0;
  KZGX_TRY_HIP(hipMemcpyAsync(out_xy, d_o, point_words(ctx) * 4, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipMemcpyAsync(&oi, d_oi, 4, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  *out_is_inf = (int)oi;
  return KZGX_OK;
}

int kzgx_prove_single_batch(kzgx_ctx* ctx, const uint64_t* coeffs, size_t n, size_t coeff_stride,
                            const uint64_t* zs, size_t batch, uint64_t* out_xy, int* out_is_inf, uint64_t* out_y) {
  KZGX_TRY(activate(ctx));
  if (batch == 0) return KZGX_OK;
  if (!zs || !out_xy || !out_is_inf || (n > 0 && !coeffs)) return KZGX_ERR_ARG;
  if (batch > 1 && coeff_stride != 0 && coeff_stride < n) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  const size_t npolys = coeff_stride == 0 ? 1 : batch;
  const size_t cb = (npolys - 1) * coeff_stride * 32 + n * 32;
  const size_t ob = batch * point_words(ctx) * 4;
  // pinned layout: [results | flags | y | z | coefficients]; outputs are
  // written by the kernels into mapped host memory (no D2H copies)
  const bool direct = cb <= PIN_DIRECT_MAX;  // as kzgx_msm_g1_batch
  const size_t o_off = 0, i_off = align256(ob), y_off = i_off + align256(batch * 4),
               z_off = y_off + align256(batch * 32), c_off = z_off + align256(batch * 32);
  KZGX_TRY(pin_stage(ctx, c_off + (direct ? cb : 0)));
  std::memcpy(ctx->h_pin + z_off, zs, batch * 32);
  void* d_c = nullptr;
  if (n) {
    if (direct) {
      std::memcpy(ctx->h_pin + c_off, coeffs, cb);
      d_c = ctx->d_pin + c_off;
    } else {
      KZGX_TRY(stage(ctx, 0, cb, &d_c));
      KZGX_TRY_HIP(hipMemcpyAsync(d_c, coeffs, cb, hipMemcpyHostToDevice, ctx->c.stream));
    }
  }
  KZGX_TRY(kzgx_prove_single_batch_device(ctx, d_c, n, coeff_stride, ctx->d_pin + z_off, batch, ctx->d_pin + o_off,
                                          ctx->d_pin + i_off, ctx->d_pin + y_off, nullptr));
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  std::memcpy(out_xy, ctx->h_pin + o_off, ob);
  const uint32_t* inf = reinterpret_cast<const uint32_t*>(ctx->h_pin + i_off);
  for (size_t b = 0; b < batch; b++) out_is_inf[b] = (int)inf[b];
  if (out_y) std::memcpy(out_y, ctx->h_pin + y_off, batch * 32);
  return KZGX_OK;
}

int kzgx_poly_eval(kzgx_ctx* ctx, const uint64_t* coeffs, size_t n, const uint64_t* xs, size_t m, uint64_t* ys) {
  KZGX_TRY(activate(ctx));
  if (m == 0) return KZGX_OK;
  if (!xs || !ys || (n > 0 && !coeffs) || n > 0xffffffffu || m > 0xffffffffu) return KZGX_ERR_ARG;
  void *d_c = nullptr, *d_x, *d_y;
  if (n) KZGX_TRY(stage(ctx, 0, n * 32, &d_c));
  KZGX_TRY(stage(ctx, 1, m * 32, &d_x));
  KZGX_TRY(stage(ctx, 2, m * 32, &d_y));
  if (n) KZGX_TRY_HIP(hipMemcpyAsync(d_c, coeffs, n * 32, hipMemcpyHostToDevice, ctx->c.stream));
  KZGX_TRY_HIP(hipMemcpyAsync(d_x, xs, m * 32, hipMemcpyHostToDevice, ctx->c.stream));
  KZGX_TRY(kzgx::poly_eval(&ctx->c, (const uint32_t*)d_c, n, (const uint32_t*)d_x, m, (uint32_t*)d_y, ctx->c.stream));
  KZGX_TRY_HIP(hipMemcpyAsync(ys, d_y, m * 32, hipMemcpyDeviceToHost, ctx->c.stream));
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  return KZGX_OK;
}

int kzgx_poly_interpolate(kzgx_ctx* ctx, const uint64_t* xs, const uint64_t* ys, size_t n, uint64_t* coeffs) {
  KZGX_TRY(activate(ctx));
  if (n == 0) return KZGX_OK;
  if (!xs || !ys || !coeffs || n > (1u << 24)) return KZGX_ERR_ARG;
  void *d_x, *d_y, *d_c;
  KZGX_TRY(stage(ctx, 0, n * 32, &d_x));
  KZGX_TRY(stage(ctx, 1, n * 32, &d_y));
  KZGX_TRY(stage(ctx, 2, n * 32, &d_c));
  KZGX_TRY_HIP(hipMemcpyAsync(d_x, xs, n * 32, hipMemcpyHostToDevice, ctx->c.stream));
  KZGX_TRY_HIP(hipMemcpyAsync(d_y, ys, n * 32, hipMemcpyHostToDevice, ctx->c.stream));
  int rc = kzgx::poly_interpolate(&ctx->c, (const uint32_t*)d_x, (const uint32_t*)d_y, n, (uint32_t*)d_c,
                                  ctx->c.stream);
  if (rc != KZGX_OK) return rc;
  KZGX_TRY_HIP(hipMemcpyAsync(coeffs, d_c, n * 32, hipMemcpyDeviceToHost, ctx->c.stream));
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  return KZGX_OK;
}

int kzgx_poly_vanishing(kzgx_ctx* ctx, const uint64_t* xs, size_t n, uint64_t* z_out) {
  KZGX_TRY(activate(ctx));
  if (!z_out) return KZGX_ERR_ARG;
  if (n == 0) {  // empty product = 1
    std::memset(z_out, 0, 32);
    z_out[0] = 1;
    return KZGX_OK;
  }
  if (!xs || n > (1u << 24)) return KZGX_ERR_ARG;
  void *d_x, *d_z;
  KZGX_TRY(stage(ctx, 0, n * 32, &d_x));
  KZGX_TRY(stage(ctx, 1, (n + 1) * 32, &d_z));
  KZGX_TRY_HIP(hipMemcpyAsync(d_x, xs, n * 32, hipMemcpyHostToDevice, ctx->c.stream));
  KZGX_TRY(kzgx::poly_vanishing(&ctx->c, (const uint32_t*)d_x, n, (uint32_t*)d_z, ctx->c.stream));
  KZGX_TRY_HIP(hipMemcpyAsync(z_out, d_z, (n + 1) * 32, hipMemcpyDeviceToHost, ctx->c.stream));
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  return KZGX_OK;
}

int kzgx_g1_validate(kzgx_ctx* ctx, const uint64_t* xy, int* ok) {
  KZGX_TRY(activate(ctx));
  if (!xy || !ok) return KZGX_ERR_ARG;
  const size_t pb = point_words(ctx) * 4;
  void* d_p;
  KZGX_TRY(stage(ctx, 0, pb + 16, &d_p));
  uint32_t* d_ok = (uint32_t*)((char*)d_p + pb);
  KZGX_TRY_HIP(hipMemcpyAsync(d_p, xy, pb, hipMemcpyHostToDevice, ctx->c.stream));
  KZGX_TRY(kzgx::g1_validate(&ctx->c, (const uint32_t*)d_p, d_ok, ctx->c.stream));
  uint32_t v = 0;
  KZGX_TRY_HIP(hipMemcpyAsync(&v, d_ok, 4, hipMemcpyDeviceToHost, ctx->c.stream));
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  *ok = (int)v;
  return KZGX_OK;
}

int kzgx_g1_sum(kzgx_ctx* ctx, const uint64_t* xy, const int* is_inf, size_t count, uint64_t* out_xy,
                int* out_is_inf) {
  KZGX_TRY(activate(ctx));
  if (!out_xy || !out_is_inf || (count > 0 && !xy)) return KZGX_ERR_ARG;
  const size_t pb = point_words(ctx) * 4;
  void *d_p, *d_f, *d_o;
  KZGX_TRY(stage(ctx, 0, count * pb + 16, &d_p));
  KZGX_TRY(stage(ctx, 1, count * 4 + 16, &d_f));
  KZGX_TRY(stage(ctx, 2, pb + 16, &d_o));
  std::vector<uint32_t> f(count);
  for (size_t i = 0; i < count; i++) f[i] = is_inf ? (uint32_t)(is_inf[i] != 0) : 0u;
  if (count) {
    KZGX_TRY_HIP(hipMemcpyAsync(d_p, xy, count * pb, hipMemcpyHostToDevice, ctx->c.stream));
    KZGX_TRY_HIP(hipMemcpyAsync(d_f, f.data(), count * 4, hipMemcpyHostToDevice, ctx->c.stream));
  }
  uint32_t* d_oi = (uint32_t*)((char*)d_o + pb);
  KZGX_TRY(kzgx::g1_sum(&ctx->c, (const uint32_t*)d_p, (const uint32_t*)d_f, count, (uint32_t*)d_o, d_oi,
                        ctx->c.stream));
  uint32_t oi = 0;
  KZGX_TRY_HIP(hipMemcpyAsync(out_xy, d_o, pb, hipMemcpyDeviceToHost, ctx->c.stream));
  KZGX_TRY_HIP(hipMemcpyAsync(&oi, d_oi, 4, hipMemcpyDeviceToHost, ctx->c.stream));
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  *out_is_inf = (int)oi;
  return KZGX_OK;
}

int kzgx_g1_sum_device(kzgx_ctx* ctx, const void* d_xy, const void* d_inf, size_t count, void* d_out_xy,
                       void* d_out_inf, void* stream) {
  KZGX_TRY(activate(ctx));
  if (!d_out_xy || !d_out_inf || (count > 0 && !d_xy) || count > 0xffffffffu) return KZGX_ERR_ARG;
  return kzgx::g1_sum(&ctx->c, (const uint32_t*)d_xy, (const uint32_t*)d_inf, count, (uint32_t*)d_out_xy,
                      (uint32_t*)d_out_inf, pick(ctx, stream));
}

int kzgx_g1_sum_packed_device(kzgx_ctx* ctx, const void* d_records, size_t count, void* d_out_record, void* stream) {
  KZGX_TRY(activate(ctx));
  if (!d_out_record || (count > 0 && !d_records) || count > 0xffffffu) return KZGX_ERR_ARG;
  return kzgx::g1_fold_packed(ctx->c.curve, (const uint32_t*)d_records, count, (uint32_t*)d_out_record,
                              pick(ctx, stream));
}

int kzgx_partial_record_words(int curve) {
  if (curve != KZGX_CURVE_BN254 && curve != KZGX_CURVE_BLS12381) return -1;
  return (int)(kzgx::xyzz_record_words(curve) / 2);
}

int kzgx_msm_g1_partial_device(kzgx_ctx* ctx, const void* d_scalars, size_t n, void* d_out_record, void* stream) {
  KZGX_TRY(activate(ctx));
  if (!d_out_record || (n > 0 && !d_scalars)) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  if (n > ctx->c.n_srs) return KZGX_ERR_DEGREE;
  hipStream_t st = pick(ctx, stream);
  if (n == 0) {  // the identity: ZZ = 0
    KZGX_TRY_HIP(hipMemsetAsync(d_out_record, 0, kzgx::xyzz_record_words(ctx->c.curve) * 4, st));
    return KZGX_OK;
  }
  return kzgx::msm_partial_xyzz(&ctx->c, (const uint32_t*)d_scalars, n, (uint32_t*)d_out_record, st);
}

int kzgx_g1_sum_partials_device(kzgx_ctx* ctx, const void* d_records, size_t count, void* d_out_record, void* stream) {
  KZGX_TRY(activate(ctx));
  if (!d_out_record || (count > 0 && !d_records) || count > 0xffffffu) return KZGX_ERR_ARG;
  return kzgx::g1_fold_xyzz(ctx->c.curve, (const uint32_t*)d_records, count, (uint32_t*)d_out_record,
                            pick(ctx, stream));
}

int kzgx_msm_g1_sharded(kzgx_ctx* const* ctxs, const size_t* starts, size_t nctx, const uint64_t* scalars,
                        size_t n, uint64_t* out_xy, int* out_is_inf) {
  if (!ctxs || !starts || nctx == 0 || (n > 0 && !scalars) || !out_xy || !out_is_inf) return KZGX_ERR_ARG;
  std::vector<size_t> cnt(nctx, 0);
  for (size_t k = 0; k < nctx; k++) {
    kzgx_ctx* c = ctxs[k];
    if (!c || c->c.curve != ctxs[0]->c.curve) return KZGX_ERR_ARG;
    for (size_t j = 0; j < k; j++)
      if (ctxs[j] == c) return KZGX_ERR_ARG;  // shards share per-context staging: one slice per context
    if (c->c.n_srs == 0) return KZGX_ERR_NO_SRS;
    if (starts[k] != (k == 0 ? 0 : starts[k - 1] + ctxs[k - 1]->c.n_srs)) return KZGX_ERR_ARG;  // contiguous
    cnt[k] = starts[k] >= n ? 0 : std::min(n - starts[k], c->c.n_srs);
  }
  if (starts[nctx - 1] + ctxs[nctx - 1]->c.n_srs < n) return KZGX_ERR_DEGREE;
  const size_t pb = point_words(ctxs[0]) * 4;
  // projective partial records (round 6): no shard converts its partial to
  // affine; the fold's one inversion is the step's only one
  const size_t rb = kzgx::xyzz_record_words(ctxs[0]->c.curve) * 4;
  kzgx_ctx* c0 = ctxs[0];
  // the fold's inputs live on ctxs[0]'s device: nctx partial records
  // (all-zero = infinity: empty shards contribute nothing)
  void *d_gather, *d_res;
  KZGX_TRY(activate(c0));
  KZGX_TRY(stage(c0, 2, nctx * rb + 16, &d_gather));
  KZGX_TRY(stage(c0, 3, pb + 16, &d_res));
  KZGX_TRY_HIP(hipMemsetAsync(d_gather, 0, nctx * rb, c0->c.stream));
  hipEvent_t zeroed;
  KZGX_TRY_HIP(hipEventCreateWithFlags(&zeroed, hipEventDisableTiming));
  std::vector<hipEvent_t> done;
  struct EvGuard {
    std::vector<hipEvent_t>* v;
    hipEvent_t z;
    ~EvGuard() {
      for (auto e : *v) (void)hipEventDestroy(e);
      (void)hipEventDestroy(z);
    }
  } evg{&done, zeroed};
  KZGX_TRY_HIP(hipEventRecord(zeroed, c0->c.stream));
  // every shard's partial MSM on its own context's stream, then a
  // device-to-device (peer) copy of the partial point to ctxs[0]: no host
  // round trip between the partial MSMs and the fold
  for (size_t k = 0; k < nctx; k++) {
    if (!cnt[k]) continue;
    kzgx_ctx* c = ctxs[k];
    KZGX_TRY(activate(c));
    void *d_s, *d_o;
    KZGX_TRY(stage(c, 0, cnt[k] * 32, &d_s));
    KZGX_TRY(stage(c, 1, rb + 16, &d_o));
    KZGX_TRY_HIP(hipMemcpyAsync(d_s, scalars + starts[k] * 4, cnt[k] * 32, hipMemcpyHostToDevice, c->c.stream));
    KZGX_TRY(kzgx::msm_partial_xyzz(&c->c, (const uint32_t*)d_s, cnt[k], (uint32_t*)d_o, c->c.stream));
    KZGX_TRY_HIP(hipStreamWaitEvent(c->c.stream, zeroed, 0));
    KZGX_TRY_HIP(hipMemcpyPeerAsync((char*)d_gather + k * rb, c0->c.device, d_o, c->c.device, rb, c->c.stream));
    hipEvent_t e;
    KZGX_TRY_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    done.push_back(e);
    KZGX_TRY_HIP(hipEventRecord(e, c->c.stream));
  }
  KZGX_TRY(activate(c0));
  for (auto e : done) KZGX_TRY_HIP(hipStreamWaitEvent(c0->c.stream, e, 0));
  uint32_t* d_oi = (uint32_t*)((char*)d_res + pb);  // the packed record's infinity word
  KZGX_TRY(kzgx::g1_fold_xyzz(c0->c.curve, (const uint32_t*)d_gather, nctx, (uint32_t*)d_res, c0->c.stream));
  uint32_t oi = 0;
  KZGX_TRY_HIP(hipMemcpyAsync(out_xy, d_res, pb, hipMemcpyDeviceToHost, c0->c.stream));
  KZGX_TRY_HIP(hipMemcpyAsync(&oi, d_oi, 4, hipMemcpyDeviceToHost, c0->c.stream));
  KZGX_TRY_HIP(hipStreamSynchronize(c0->c.stream));
  *out_is_inf = (int)oi;
  return KZGX_OK;
}

/* ---- verify half: G2 SRS, polyeval_G2, pairing, verify_proof ---------------- */
namespace {
// the G2 SRS's windowed table for n points (rebuilt when the SRS changed or
// more points are needed); nullptr (plain per-term path) if it cannot be had
const uint32_t* g2_table(kzgx_ctx* ctx, size_t n, hipStream_t st) {
  if (ctx->g2tab_n >= n) return ctx->d_g2tab;
  const size_t all = ctx->n_srs2;
  ctx->g2tab_n = 0;
  if (kzgx::dev_alloc(&ctx->c, (void**)&ctx->d_g2tab, kzgx::g2_table_bytes(ctx->c.curve, all), &ctx->g2tab_b) !=
          KZGX_OK ||
      kzgx::g2_table_build(&ctx->c, ctx->d_srs2_canon, all, ctx->d_g2tab, st) != KZGX_OK ||
      hipStreamSynchronize(st) != hipSuccess)
    return nullptr;
  ctx->g2tab_n = all;
  return ctx->d_g2tab;
}

// the wave verify's setup-derived buffer ([y]G table, the line tables of
// G2[0] and G2[1]), built on first use after a setup
int vw_ensure(kzgx_ctx* ctx, hipStream_t st) {
  if (ctx->vw_ready) return KZGX_OK;
  KZGX_TRY(kzgx::dev_alloc(&ctx->c, (void**)&ctx->d_vw, kzgx::verify_wave_bytes(ctx->c.curve), &ctx->vw_b));
  kzgx::GenTables g;
  KZGX_TRY(kzgx::gen_tables_get(ctx->c.curve, ctx->c.device, st, &g));
  KZGX_TRY(kzgx::verify_wave_prepare(&ctx->c, ctx->d_srs_canon, ctx->d_srs2_canon, g.g1_comb, ctx->d_vw, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));  // one-time; later calls may come on other streams
  ctx->vw_ready = true;
  return KZGX_OK;
}

int side_ready(kzgx_ctx* ctx) {
  if (!ctx->side) KZGX_TRY_HIP(stream_take(ctx->c.device, &ctx->side));
  if (!ctx->ev_fork) KZGX_TRY_HIP(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
  if (!ctx->ev_join) KZGX_TRY_HIP(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
  return KZGX_OK;
}

// KZGX_PAIR2_SPLIT=1 (tests/test_gpu_env_hooks.py): the multi-point verify's
// pairing as two launches (k_vlines_wave, then k_pair2_wave) from the start,
// the path k_pair2_fused otherwise falls back to when it reports ok == 2
bool split_pair2() {
  static const bool on = kzgx::env_is_1("KZGX_PAIR2_SPLIT");
  return on;
}

}  // namespace

size_t kzgx_srs_g2_size(const kzgx_ctx* ctx) { return ctx ? ctx->n_srs2 : 0; }

int kzgx_gen_srs_g2(kzgx_ctx* ctx, const uint64_t* tau, size_t start, size_t n) {
  KZGX_TRY(activate(ctx));
  ctx->vw_ready = false;
  cells_g2_drop(ctx);
  ctx->g2tab_n = 0;
  if (!tau || n == 0 || n > 0x7fffffffu) return KZGX_ERR_ARG;
  const size_t bytes = n * 2 * point_words(ctx) * 4;
  KZGX_TRY(kzgx::dev_alloc(&ctx->c, (void**)&ctx->d_srs2_canon, bytes, &ctx->srs2_canon_b));
  void* d_tau;
  KZGX_TRY(stage(ctx, 0, 32, &d_tau));
  KZGX_TRY_HIP(hipMemcpyAsync(d_tau, tau, 32, hipMemcpyHostToDevice, ctx->c.stream));
  kzgx::GenTables g;
  KZGX_TRY(kzgx::gen_tables_get(ctx->c.curve, ctx->c.device, ctx->c.stream, &g));
  KZGX_TRY(kzgx::gen_srs_g2_comb(ctx->c.curve, (const uint32_t*)d_tau, start, n, g.g2_comb, ctx->d_srs2_canon,
                                 ctx->c.stream));
  // polyeval_G2's window table from the same comb (one comb evaluation per
  // entry, ~1 ms at 4097 points) so no verify_proof(poly, 0, N) pays the
  // 4.3-ms doubling chains of building it from the points (k_g2_tab, still
  // the path of a loaded G2 SRS); large SRSs keep it for first use
  const bool eager = n <= KZGX_G2TAB_EAGER_MAX;
  if (eager) {
    KZGX_TRY(kzgx::dev_alloc(&ctx->c, (void**)&ctx->d_g2tab, kzgx::g2_table_bytes(ctx->c.curve, n), &ctx->g2tab_b));
    KZGX_TRY(kzgx::g2_table_comb(ctx->c.curve, (const uint32_t*)d_tau, start, n, g.g2_comb, ctx->d_g2tab,
                                 ctx->c.stream));
  }
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  ctx->g2tab_n = eager ? n : 0;
  ctx->n_srs2 = n;
  return setup_finish(ctx);
}

int kzgx_load_srs_g2(kzgx_ctx* ctx, const uint64_t* xy, size_t n) {
  KZGX_TRY(activate(ctx));
  ctx->vw_ready = false;
  cells_g2_drop(ctx);
  ctx->g2tab_n = 0;
  if (!xy || n == 0) return KZGX_ERR_ARG;
  const size_t bytes = n * 2 * point_words(ctx) * 4;
  KZGX_TRY(kzgx::dev_alloc(&ctx->c, (void**)&ctx->d_srs2_canon, bytes, &ctx->srs2_canon_b));
  KZGX_TRY_HIP(hipMemcpyAsync(ctx->d_srs2_canon, xy, bytes, hipMemcpyHostToDevice, ctx->c.stream));
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  ctx->n_srs2 = n;
  return setup_finish(ctx);
}

int kzgx_get_srs_g2(kzgx_ctx* ctx, uint64_t* xy, size_t n) {
  KZGX_TRY(activate(ctx));
  if (!xy) return KZGX_ERR_ARG;
  if (ctx->n_srs2 == 0) return KZGX_ERR_NO_SRS;
  if (n > ctx->n_srs2) return KZGX_ERR_ARG;
  KZGX_TRY_HIP(
      hipMemcpyAsync(xy, ctx->d_srs2_canon, n * 2 * point_words(ctx) * 4, hipMemcpyDeviceToHost, ctx->c.stream));
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  return KZGX_OK;
}

int kzgx_g2_validate(kzgx_ctx* ctx, const uint64_t* xy, size_t count, int* ok) {
  KZGX_TRY(activate(ctx));
  if (count == 0) return KZGX_OK;
  if (!xy || !ok) return KZGX_ERR_ARG;
  const size_t pb = 2 * point_words(ctx) * 4;
  void *d_p, *d_ok;
  KZGX_TRY(stage(ctx, 0, count * pb, &d_p));
  KZGX_TRY(stage(ctx, 1, count * 4, &d_ok));
  KZGX_TRY_HIP(hipMemcpyAsync(d_p, xy, count * pb, hipMemcpyHostToDevice, ctx->c.stream));
  KZGX_TRY(kzgx::g2_validate(&ctx->c, (const uint32_t*)d_p, count, (uint32_t*)d_ok, ctx->c.stream));
  std::vector<uint32_t> v(count);
  KZGX_TRY_HIP(hipMemcpyAsync(v.data(), d_ok, count * 4, hipMemcpyDeviceToHost, ctx->c.stream));
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  for (size_t k = 0; k < count; k++) ok[k] = (int)v[k];
  return KZGX_OK;
}

int kzgx_msm_g2(kzgx_ctx* ctx, const uint64_t* scalars, size_t n, uint64_t* out_xy, int* out_is_inf) {
  KZGX_TRY(activate(ctx));
  if (!out_xy || !out_is_inf || (n > 0 && !scalars) || n > (1u << 24)) return KZGX_ERR_ARG;
  if (ctx->n_srs2 == 0) return KZGX_ERR_NO_SRS;
  if (n > ctx->n_srs2) return KZGX_ERR_DEGREE;
  const size_t pb = 2 * point_words(ctx) * 4;
  void *d_s = nullptr, *d_o;
  if (n) KZGX_TRY(stage(ctx, 0, n * 32, &d_s));
  KZGX_TRY(stage(ctx, 1, pb + 16, &d_o));
  if (n) KZGX_TRY_HIP(hipMemcpyAsync(d_s, scalars, n * 32, hipMemcpyHostToDevice, ctx->c.stream));
  uint32_t* d_oi = (uint32_t*)((char*)d_o + pb);
  KZGX_TRY(kzgx::msm_g2(&ctx->c, (const uint32_t*)d_s, ctx->d_srs2_canon, n, (uint32_t*)d_o, d_oi, ctx->c.stream,
                        n ? g2_table(ctx, n, ctx->c.stream) : nullptr));
  uint32_t oi = 0;
  KZGX_TRY_HIP(hipMemcpyAsync(out_xy, d_o, pb, hipMemcpyDeviceToHost, ctx->c.stream));
  KZGX_TRY_HIP(hipMemcpyAsync(&oi, d_oi, 4, hipMemcpyDeviceToHost, ctx->c.stream));
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  *out_is_inf = (int)oi;
  return KZGX_OK;
}

int kzgx_pairing(kzgx_ctx* ctx, const uint64_t* g1_xy, const int* g1_inf, const uint64_t* g2_xy, const int* g2_inf,
                 size_t count, uint64_t* out) {
  KZGX_TRY(activate(ctx));
  if (count == 0) return KZGX_OK;
  if (!g1_xy || !g2_xy || !out || count > (1u << 20)) return KZGX_ERR_ARG;
  const size_t p1 = point_words(ctx) * 4, p2 = 2 * p1, fb = 6 * p1;
  void *d_1, *d_2, *d_f, *d_o;
  KZGX_TRY(stage(ctx, 0, count * p1, &d_1));
  KZGX_TRY(stage(ctx, 1, count * p2, &d_2));
  KZGX_TRY(stage(ctx, 2, count * 8, &d_f));
  KZGX_TRY(stage(ctx, 3, count * fb, &d_o));
  std::vector<uint32_t> f(2 * count);
  for (size_t k = 0; k < count; k++) {
    f[k] = g1_inf ? (uint32_t)(g1_inf[k] != 0) : 0u;
    f[count + k] = g2_inf ? (uint32_t)(g2_inf[k] != 0) : 0u;
  }
  KZGX_TRY_HIP(hipMemcpyAsync(d_1, g1_xy, count * p1, hipMemcpyHostToDevice, ctx->c.stream));
  KZGX_TRY_HIP(hipMemcpyAsync(d_2, g2_xy, count * p2, hipMemcpyHostToDevice, ctx->c.stream));
  KZGX_TRY_HIP(hipMemcpyAsync(d_f, f.data(), count * 8, hipMemcpyHostToDevice, ctx->c.stream));
  KZGX_TRY(kzgx::pairing_batch(&ctx->c, (const uint32_t*)d_1, (const uint32_t*)d_f, (const uint32_t*)d_2,
                               (const uint32_t*)d_f + count, count, (uint32_t*)d_o, ctx->c.stream));
  KZGX_TRY_HIP(hipMemcpyAsync(out, d_o, count * fb, hipMemcpyDeviceToHost, ctx->c.stream));
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  return KZGX_OK;
}

int kzgx_verify_proof(kzgx_ctx* ctx, const uint64_t* commit_xy, int commit_inf, const uint64_t* proof_xy,
                      int proof_inf, const uint64_t* xs, const uint64_t* ys, size_t npoints, int* ok) {
  KZGX_TRY(activate(ctx));
  if (!commit_xy || !proof_xy || !ok || (npoints > 0 && (!xs || !ys)) || npoints > (1u << 24)) return KZGX_ERR_ARG;
  if (npoints < 1) return KZGX_ERR_ARG;  // "expected_data size must be 1 or greater"
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  *ok = 0;
  if (npoints >= ctx->c.n_srs) return KZGX_OK;  // trusted_setup.cpp:235-236
  if (ctx->n_srs2 < npoints + 1) return KZGX_ERR_NO_SRS;
  if (npoints == 1) {  // I = y, Z = X - x: the single-opening product check
    const int cf = commit_inf != 0, pf = proof_inf != 0;
    return kzgx_verify_single_batch(ctx, commit_xy, &cf, proof_xy, &pf, xs, ys, 1, ok);
  }
  hipStream_t st = ctx->c.stream;
  const size_t n = npoints;
  const size_t p1 = point_words(ctx) * 4, p2 = 2 * p1, fb = 6 * p1;
  // one device block: x | y | I | Z | G1 in (commit, proof) | G1 work | G2 in | flags | Fp12 out
  const size_t o_x = 0, o_y = o_x + n * 32, o_I = o_y + n * 32, o_Z = o_I + n * 32, o_g1 = o_Z + (n + 1) * 32;
  const size_t o_w = o_g1 + 4 * p1, o_g2 = o_w + 2 * p1, o_f = o_g2 + 2 * p2, o_o = o_f + 64;
  const size_t o_ln = (o_o + 2 * fb + 255) & ~(size_t)255;
  void* d;
  KZGX_TRY(stage(ctx, 3, o_ln + kzgx::pair2_wave_scratch_bytes(ctx->c.curve), &d));
  char* b = (char*)d;
  uint32_t* g1 = (uint32_t*)(b + o_g1);  // [proof, p2, commit, msm(I)]
  uint32_t* fl = (uint32_t*)(b + o_f);   // [proof_inf, p2_inf, p1_inf, srs2_0_inf, commit_inf, msmI_inf]
  uint32_t hf[8] = {(uint32_t)(proof_inf != 0), 0, 0, 0, (uint32_t)(commit_inf != 0), 0, 0, 0};
  KZGX_TRY_HIP(hipMemcpyAsync(b + o_x, xs, n * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(b + o_y, ys, n * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(g1, proof_xy, p1, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync((char*)g1 + 2 * p1, commit_xy, p1, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(fl, hf, sizeof(hf), hipMemcpyHostToDevice, st));
  // Z and I (linear_roots_and_polyfit, util.cpp:172-178): Z first, then the
  // G2 half (p1 = [Z(tau)]G2, ~0.9 ms of lone-lane G2 chains) forks onto the
  // side stream while this stream takes the G1 half (I, [I(tau)]G1, C - it)
  KZGX_TRY(kzgx::poly_vanishing(&ctx->c, (const uint32_t*)(b + o_x), n, (uint32_t*)(b + o_Z), st));
  KZGX_TRY(side_ready(ctx));
  hipStream_t sd = ctx->side;
  KZGX_TRY_HIP(hipEventRecord(ctx->ev_fork, st));
  KZGX_TRY_HIP(hipStreamWaitEvent(sd, ctx->ev_fork, 0));
  uint32_t* g2 = (uint32_t*)(b + o_g2);
  const int rg2 =
      kzgx::msm_g2(&ctx->c, (const uint32_t*)(b + o_Z), ctx->d_srs2_canon, n + 1, g2, fl + 2, sd, g2_table(ctx, n + 1, sd));
  // (joined before any return below: the side work writes into this call's staging)
  const hipError_t jr = hipEventRecord(ctx->ev_join, sd);
  auto join = [&]() { return hipStreamWaitEvent(st, ctx->ev_join, 0); };
  if (rg2 != KZGX_OK || jr != hipSuccess) {
    (void)hipStreamSynchronize(sd);
    return rg2 != KZGX_OK ? rg2 : kzgx::hip_fail(jr);
  }
  int rg1 = kzgx::poly_interpolate(&ctx->c, (const uint32_t*)(b + o_x), (const uint32_t*)(b + o_y), n,
                                   (uint32_t*)(b + o_I), st);
  // p2 = C - [I(tau)]G1
  if (rg1 == KZGX_OK)
    rg1 = kzgx::msm_batch(&ctx->c, (const uint32_t*)(b + o_I), n, 1, n * 8, (uint32_t*)((char*)g1 + 3 * p1), fl + 5, st);
  if (rg1 == KZGX_OK)
    rg1 = kzgx::g1_sub(&ctx->c, (const uint32_t*)((char*)g1 + 2 * p1), fl + 4, (const uint32_t*)((char*)g1 + 3 * p1),
                       fl + 5, (uint32_t*)((char*)g1 + p1), fl + 1, st);
  KZGX_TRY_HIP(join());
  if (rg1 != KZGX_OK) {
    (void)hipStreamSynchronize(st);
    return rg1;
  }
  // the second pairing's G2 input = G2[0] (the two-launch path reads it here)
  KZGX_TRY_HIP(hipMemcpyAsync((char*)g2 + p2, ctx->d_srs2_canon, p2, hipMemcpyDeviceToDevice, st));
  // e(proof, p1) == e(p2, G2[0])  <=>  e(proof, p1) e(-p2, G2[0]) == 1 (one wave, one final
  // exponentiation; the booleans of the reference's FP12_equals)
  uint32_t* d_ok = (uint32_t*)(b + o_o);
  uint32_t v = 2;
  if (!split_pair2()) {  // one launch: [Z(tau)]G2's lines overlap the Miller loop
    KZGX_TRY(vw_ensure(ctx, st));
    KZGX_TRY(kzgx::pair2_fused(&ctx->c, g1, fl, g2, fl + 2, ctx->d_vw, d_ok, st));
    KZGX_TRY_HIP(hipMemcpyAsync(&v, d_ok, 4, hipMemcpyDeviceToHost, st));
    KZGX_TRY_HIP(hipStreamSynchronize(st));
  }
  if (v == 2) {  // (a degenerate line chain, or KZGX_PAIR2_SPLIT): two launches
    KZGX_TRY(kzgx::pair2_wave(&ctx->c, g1, fl, g2, fl + 2, (uint32_t*)(b + o_ln), d_ok, st));
    KZGX_TRY_HIP(hipMemcpyAsync(&v, d_ok, 4, hipMemcpyDeviceToHost, st));
    KZGX_TRY_HIP(hipStreamSynchronize(st));
  }
  *ok = v ? 1 : 0;
  return KZGX_OK;
}

int kzgx_verify_single_batch_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf,
                                    const void* d_proofs, const void* d_proof_inf, const void* d_z, const void* d_y,
                                    size_t count, void* d_ok, void* stream) {
  KZGX_TRY(activate(ctx));
  if (count == 0) return KZGX_OK;
  if (!d_commits || !d_proofs || !d_z || !d_y || !d_ok || count > (1u << 26)) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0 || ctx->n_srs2 < 2) return KZGX_ERR_NO_SRS;
  hipStream_t st = pick(ctx, stream);
  if (count <= ctx->vw_max) {
    KZGX_TRY(vw_ensure(ctx, st));
    return kzgx::verify_wave_batch(&ctx->c, (const uint32_t*)d_commits, (const uint32_t*)d_commit_inf,
                                   (const uint32_t*)d_proofs, (const uint32_t*)d_proof_inf, (const uint32_t*)d_z,
                                   (const uint32_t*)d_y, count, ctx->d_srs_canon, ctx->d_vw, (uint32_t*)d_ok, st);
  }
  return kzgx::verify_single_batch(&ctx->c, (const uint32_t*)d_commits, (const uint32_t*)d_commit_inf,
                                   (const uint32_t*)d_proofs, (const uint32_t*)d_proof_inf, (const uint32_t*)d_z,
                                   (const uint32_t*)d_y, count, ctx->d_srs_canon, ctx->d_srs2_canon,
                                   (uint32_t*)d_ok, st);
}

int kzgx_set_verify_wave_max(kzgx_ctx* ctx, size_t max_count) {
  if (!ctx) return KZGX_ERR_ARG;
  ctx->vw_max = max_count;
  return KZGX_OK;
}

int kzgx_verify_single_batch(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf,
                             const uint64_t* proofs_xy, const int* proof_inf, const uint64_t* zs, const uint64_t* ys,
                             size_t count, int* ok) {
  KZGX_TRY(activate(ctx));
  if (count == 0) return KZGX_OK;
  if (!commits_xy || !proofs_xy || !zs || !ys || !ok || count > (1u << 26)) return KZGX_ERR_ARG;
  const size_t pb = point_words(ctx) * 4;
  if (count <= ctx->vw_max && count * (2 * pb + 76) <= PIN_DIRECT_MAX) {
    // the wave path (single verify_proof calls): inputs and the result in
    // the context's mapped pinned staging -- the kernel copies each opening's
    // inputs into LDS in one round trip and writes its boolean straight into
    // host memory, so the call makes no copy at all (it made five H2D and
    // one D2H copies from pageable memory, ~10 us each)
    const size_t o_ok = 0, o_c = align256(count * 4), o_p = o_c + align256(count * pb);
    const size_t o_z = o_p + align256(count * pb), o_y = o_z + count * 32, o_f = align256(o_y + count * 32);
    KZGX_TRY(pin_stage(ctx, o_f + count * 8));
    uint8_t* h = ctx->h_pin;
    std::memcpy(h + o_c, commits_xy, count * pb);
    std::memcpy(h + o_p, proofs_xy, count * pb);
    std::memcpy(h + o_z, zs, count * 32);
    std::memcpy(h + o_y, ys, count * 32);
    uint32_t* hf = reinterpret_cast<uint32_t*>(h + o_f);
    for (size_t k = 0; k < count; k++) {
      hf[k] = commit_inf ? (uint32_t)(commit_inf[k] != 0) : 0u;
      hf[count + k] = proof_inf ? (uint32_t)(proof_inf[k] != 0) : 0u;
    }
    uint8_t* d = ctx->d_pin;
    KZGX_TRY(kzgx_verify_single_batch_device(ctx, d + o_c, d + o_f, d + o_p, d + o_f + count * 4, d + o_z, d + o_y,
                                             count, d + o_ok, nullptr));
    KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
    const uint32_t* v = reinterpret_cast<const uint32_t*>(h + o_ok);
    for (size_t k = 0; k < count; k++) ok[k] = (int)v[k];
    return KZGX_OK;
  }
  void *d_c, *d_p, *d_s, *d_f;
  KZGX_TRY(stage(ctx, 0, count * pb, &d_c));
  KZGX_TRY(stage(ctx, 1, count * pb, &d_p));
  KZGX_TRY(stage(ctx, 2, count * 64, &d_s));
  KZGX_TRY(stage(ctx, 3, count * 12, &d_f));
  std::vector<uint32_t> fl(2 * count);
  for (size_t k = 0; k < count; k++) {
    fl[k] = commit_inf ? (uint32_t)(commit_inf[k] != 0) : 0u;
    fl[count + k] = proof_inf ? (uint32_t)(proof_inf[k] != 0) : 0u;
  }
  hipStream_t st = ctx->c.stream;
  KZGX_TRY_HIP(hipMemcpyAsync(d_c, commits_xy, count * pb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_p, proofs_xy, count * pb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_s, zs, count * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync((char*)d_s + count * 32, ys, count * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_f, fl.data(), count * 8, hipMemcpyHostToDevice, st));
  uint32_t* d_ok = (uint32_t*)d_f + 2 * count;
  KZGX_TRY(kzgx_verify_single_batch_device(ctx, d_c, d_f, d_p, (uint32_t*)d_f + count, d_s,
                                           (char*)d_s + count * 32, count, d_ok, nullptr));
  std::vector<uint32_t> v(count);
  KZGX_TRY_HIP(hipMemcpyAsync(v.data(), d_ok, count * 4, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  for (size_t k = 0; k < count; k++) ok[k] = (int)v[k];
  return KZGX_OK;
}

// ---- variable-base MSM over caller points, aggregated verification ---------
int kzgx_msm_g1_points_device(kzgx_ctx* ctx, const void* d_points_xy, const void* d_is_inf, const void* d_scalars,
                              size_t n, void* d_out_xy, void* d_out_is_inf, void* stream) {
  KZGX_TRY(activate(ctx));
  if (!d_out_xy || !d_out_is_inf || (n > 0 && (!d_points_xy || !d_scalars)) || n > KZGX_MSM_POINTS_MAX)
    return KZGX_ERR_ARG;
  hipStream_t st = pick(ctx, stream);
  kzgx::WsLease ws = ctx->c.ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  const kzgx::PointSeg seg{(const uint32_t*)d_points_xy, (const uint32_t*)d_is_inf, n};
  return kzgx::msm_points(&ctx->c, *ws, &seg, 1, (const uint32_t*)d_scalars, (uint32_t*)d_out_xy,
                          (uint32_t*)d_out_is_inf, st);
}

int kzgx_msm_g1_points(kzgx_ctx* ctx, const uint64_t* points_xy, const int* is_inf, const uint64_t* scalars, size_t n,
                       uint64_t* out_xy, int* out_is_inf) {
  KZGX_TRY(activate(ctx));
  if (!out_xy || !out_is_inf || (n > 0 && (!points_xy || !scalars)) || n > KZGX_MSM_POINTS_MAX) return KZGX_ERR_ARG;
  const size_t pb = point_words(ctx) * 4;
  void *d_p, *d_f, *d_s, *d_o;
  KZGX_TRY(stage(ctx, 0, n * pb + 16, &d_p));
  KZGX_TRY(stage(ctx, 1, n * 4 + 16, &d_f));
  KZGX_TRY(stage(ctx, 2, n * 32 + 16, &d_s));
  KZGX_TRY(stage(ctx, 3, pb + 16, &d_o));
  hipStream_t st = ctx->c.stream;
  std::vector<uint32_t> f(n);
  for (size_t i = 0; i < n; i++) f[i] = is_inf ? (uint32_t)(is_inf[i] != 0) : 0u;
  if (n) {
    KZGX_TRY_HIP(hipMemcpyAsync(d_p, points_xy, n * pb, hipMemcpyHostToDevice, st));
    KZGX_TRY_HIP(hipMemcpyAsync(d_f, f.data(), n * 4, hipMemcpyHostToDevice, st));
    KZGX_TRY_HIP(hipMemcpyAsync(d_s, scalars, n * 32, hipMemcpyHostToDevice, st));
  }
  uint32_t* d_oi = (uint32_t*)((char*)d_o + pb);
  KZGX_TRY(kzgx_msm_g1_points_device(ctx, d_p, d_f, d_s, n, d_o, d_oi, nullptr));
  uint32_t oi = 0;
  KZGX_TRY_HIP(hipMemcpyAsync(out_xy, d_o, pb, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipMemcpyAsync(&oi, d_oi, 4, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  *out_is_inf = (int)oi;
  return KZGX_OK;
}

int kzgx_verify_aggregate_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf, const void* d_proofs,
                                 const void* d_proof_inf, const void* d_z, const void* d_y, const void* d_challenges,
                                 size_t count, void* d_ok, void* stream) {
  KZGX_TRY(activate(ctx));
  if (!d_ok || !d_challenges) return KZGX_ERR_ARG;
  if (count > 0 && (!d_commits || !d_proofs || !d_z || !d_y)) return KZGX_ERR_ARG;
  if (2 * count + 1 > KZGX_MSM_POINTS_MAX) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0 || ctx->n_srs2 < 2) return KZGX_ERR_NO_SRS;
  hipStream_t st = pick(ctx, stream);
  if (count == 0) {
    KZGX_TRY_HIP(hipMemsetD32Async((hipDeviceptr_t)d_ok, 1, 1, st));
    return KZGX_OK;
  }
  kzgx::Ctx* c = &ctx->c;
  kzgx::WsLease ws = c->ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  const size_t pw = point_words(ctx);
  // scalars r | r z | t (+ the block sums' scratch); A | B | their flags | z = y = 0
  KZGX_TRY(kzgx::dev_alloc(c, (void**)&ws->var_scal, (2 * count + 1 + 256) * 32, &ws->var_scal_b));
  KZGX_TRY(kzgx::dev_alloc(c, (void**)&ws->var_pt, (2 * pw + 4 + 16) * 4, &ws->var_pt_b));
  uint32_t* A = ws->var_pt;
  uint32_t* B = A + pw;
  uint32_t* fl = B + pw;  // [A_inf, B_inf, -, -]
  uint32_t* zero = fl + 4;
  KZGX_TRY_HIP(hipMemsetAsync(zero, 0, 64, st));
  KZGX_TRY(kzgx::aggregate_scalars(c, (const uint32_t*)d_z, (const uint32_t*)d_y, (const uint32_t*)d_challenges, count,
                                   ws->var_scal, st));
  // A = sum r_k proof_k
  const kzgx::PointSeg sa{(const uint32_t*)d_proofs, (const uint32_t*)d_proof_inf, count};
  KZGX_TRY(kzgx::msm_points(c, *ws, &sa, 1, (const uint32_t*)d_challenges, A, fl, st));
  // B = sum r_k commit_k + sum r_k z_k proof_k - (sum r_k y_k) G1[0]
  const kzgx::PointSeg sb[3] = {{(const uint32_t*)d_commits, (const uint32_t*)d_commit_inf, count},
                                {(const uint32_t*)d_proofs, (const uint32_t*)d_proof_inf, count},
                                {ctx->d_srs_canon, nullptr, 1}};
  KZGX_TRY(kzgx::msm_points(c, *ws, sb, 3, ws->var_scal, B, fl + 1, st));
  // e(A, [tau]G2) == e(B, G2[0]): the single-opening check of proof = A,
  // commit = B at z = 0, y = 0
  return kzgx_verify_single_batch_device(ctx, B, fl + 1, A, fl, zero, zero + 8, 1, d_ok, stream);
}

// ---- batched point validation, prime-order subgroup checks (subgroup.hip) ---
namespace {
// the flags buffer of the workspace slot leased for this call's stream
int chk_scratch(kzgx_ctx* ctx, const kzgx::WsLease& ws, size_t words, uint32_t** out) {
  const size_t slot = (size_t)(ws.get() - ctx->c.ws);
  KZGX_TRY(kzgx::dev_alloc(&ctx->c, (void**)&ctx->d_chk[slot], words * 4, &ctx->chk_b[slot]));
  *out = ctx->d_chk[slot];
  return KZGX_OK;
}

int check_batch_host(kzgx_ctx* ctx, bool g2, const uint64_t* xy, const int* is_inf, size_t count, int subgroup,
                     int* ok) {
  KZGX_TRY(activate(ctx));
  if (count == 0) return KZGX_OK;
  if (!xy || !ok || count > KZGX_MSM_POINTS_MAX) return KZGX_ERR_ARG;
  const size_t pb = (g2 ? 2 : 1) * point_words(ctx) * 4;
  void *d_p, *d_f;
  KZGX_TRY(stage(ctx, 0, count * pb, &d_p));
  KZGX_TRY(stage(ctx, 1, count * 8, &d_f));
  hipStream_t st = ctx->c.stream;
  std::vector<uint32_t> f(count);
  KZGX_TRY_HIP(hipMemcpyAsync(d_p, xy, count * pb, hipMemcpyHostToDevice, st));
  if (is_inf) {
    for (size_t k = 0; k < count; k++) f[k] = (uint32_t)(is_inf[k] != 0);
    KZGX_TRY_HIP(hipMemcpyAsync(d_f, f.data(), count * 4, hipMemcpyHostToDevice, st));
  }
  uint32_t* d_ok = (uint32_t*)d_f + count;
  KZGX_TRY((g2 ? kzgx::g2_check : kzgx::g1_check)(&ctx->c, (const uint32_t*)d_p, is_inf ? (const uint32_t*)d_f : nullptr,
                                                  count, subgroup, d_ok, st));
  KZGX_TRY_HIP(hipMemcpyAsync(f.data(), d_ok, count * 4, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  for (size_t k = 0; k < count; k++) ok[k] = (int)f[k];
  return KZGX_OK;
}
}  // namespace

int kzgx_g1_check_batch_device(kzgx_ctx* ctx, const void* d_xy, const void* d_is_inf, size_t count, int subgroup,
                               void* d_ok, void* d_all_ok, void* stream) {
  KZGX_TRY(activate(ctx));
  if ((!d_ok && !d_all_ok) || (count > 0 && !d_xy) || count > KZGX_MSM_POINTS_MAX) return KZGX_ERR_ARG;
  hipStream_t st = pick(ctx, stream);
  if (count == 0) {
    if (d_all_ok) KZGX_TRY_HIP(hipMemsetD32Async((hipDeviceptr_t)d_all_ok, 1, 1, st));
    return KZGX_OK;
  }
  uint32_t* flags = (uint32_t*)d_ok;
  kzgx::WsLease ws = ctx->c.ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  if (!flags) KZGX_TRY(chk_scratch(ctx, ws, count, &flags));
  KZGX_TRY(kzgx::g1_check(&ctx->c, (const uint32_t*)d_xy, (const uint32_t*)d_is_inf, count, subgroup, flags, st));
  if (d_all_ok) KZGX_TRY(kzgx::flags_and(flags, count, (uint32_t*)d_all_ok, st));
  return KZGX_OK;
}

int kzgx_g1_check_batch(kzgx_ctx* ctx, const uint64_t* xy, const int* is_inf, size_t count, int subgroup, int* ok) {
  return check_batch_host(ctx, false, xy, is_inf, count, subgroup, ok);
}

int kzgx_g2_check_batch(kzgx_ctx* ctx, const uint64_t* xy, const int* is_inf, size_t count, int subgroup, int* ok) {
  return check_batch_host(ctx, true, xy, is_inf, count, subgroup, ok);
}

int kzgx_srs_check(kzgx_ctx* ctx, int subgroup, int* g1_ok, int* g2_ok) {
  KZGX_TRY(activate(ctx));
  if (!g1_ok || !g2_ok) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  hipStream_t st = ctx->c.stream;
  kzgx::WsLease ws = ctx->c.ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  const size_t n1 = ctx->c.n_srs, n2 = ctx->n_srs2, nmax = std::max(n1, n2);
  uint32_t* f;
  KZGX_TRY(chk_scratch(ctx, ws, nmax + 2, &f));
  uint32_t* all = f + nmax;  // [G1, G2]
  KZGX_TRY(kzgx::g1_check(&ctx->c, ctx->d_srs_canon, nullptr, n1, subgroup, f, st));
  KZGX_TRY(kzgx::flags_and(f, n1, all, st));
  KZGX_TRY(kzgx::g2_check(&ctx->c, ctx->d_srs2_canon, nullptr, n2, subgroup, f, st));
  KZGX_TRY(kzgx::flags_and(f, n2, all + 1, st));  // n2 == 0: 1
  uint32_t v[2] = {0, 0};
  KZGX_TRY_HIP(hipMemcpyAsync(v, all, 8, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  *g1_ok = v[0] ? 1 : 0;
  *g2_ok = v[1] ? 1 : 0;
  return KZGX_OK;
}

int kzgx_verify_aggregate_checked_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf,
                                         const void* d_proofs, const void* d_proof_inf, const void* d_z,
                                         const void* d_y, const void* d_challenges, size_t count, int subgroup,
                                         void* d_ok, void* stream) {
  KZGX_TRY(activate(ctx));
  if (!d_ok || !d_challenges) return KZGX_ERR_ARG;
  if (count > 0 && (!d_commits || !d_proofs || !d_z || !d_y)) return KZGX_ERR_ARG;
  if (2 * count + 1 > KZGX_MSM_POINTS_MAX) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0 || ctx->n_srs2 < 2) return KZGX_ERR_NO_SRS;
  hipStream_t st = pick(ctx, stream);
  if (count == 0) {
    KZGX_TRY_HIP(hipMemsetD32Async((hipDeviceptr_t)d_ok, 1, 1, st));
    return KZGX_OK;
  }
  kzgx::WsLease ws = ctx->c.ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  uint32_t* f;  // commit flags | proof flags | their AND
  KZGX_TRY(chk_scratch(ctx, ws, 2 * count + 1, &f));
  KZGX_TRY(kzgx::g1_check2(&ctx->c, (const uint32_t*)d_commits, (const uint32_t*)d_commit_inf, count,
                           (const uint32_t*)d_proofs, (const uint32_t*)d_proof_inf, count, subgroup, f, st));
  KZGX_TRY(kzgx::flags_and(f, 2 * count, f + 2 * count, st));
  KZGX_TRY(kzgx_verify_aggregate_device(ctx, d_commits, d_commit_inf, d_proofs, d_proof_inf, d_z, d_y, d_challenges,
                                        count, d_ok, stream));
  return kzgx::flag_gate((uint32_t*)d_ok, f + 2 * count, st);
}

// the host-pointer aggregate: kzgx_verify_aggregate (checked = false) and
// kzgx_verify_aggregate_checked share the staging and the drawn challenges
static int verify_aggregate_host(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf,
                                 const uint64_t* proofs_xy, const int* proof_inf, const uint64_t* zs,
                                 const uint64_t* ys, const uint64_t* challenges, size_t count, bool checked,
                                 int subgroup, int* ok) {
  KZGX_TRY(activate(ctx));
  if (!ok) return KZGX_ERR_ARG;
  if (count > 0 && (!commits_xy || !proofs_xy || !zs || !ys)) return KZGX_ERR_ARG;
  if (2 * count + 1 > KZGX_MSM_POINTS_MAX) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0 || ctx->n_srs2 < 2) return KZGX_ERR_NO_SRS;
  if (count == 0) {
    *ok = 1;
    return KZGX_OK;
  }
  // library-drawn challenges: independent 128-bit values, r_0 = 1
  std::vector<uint64_t> drawn;
  if (!challenges) {
    drawn.assign(count * 4, 0);
    std::random_device rd;
    for (size_t k = 0; k < count; k++)
      for (int j = 0; j < 2; j++) drawn[4 * k + j] = ((uint64_t)rd() << 32) | (uint64_t)rd();
    drawn[0] = 1;
    drawn[1] = 0;
    challenges = drawn.data();
  }
  const size_t pb = point_words(ctx) * 4;
  void *d_c, *d_p, *d_s, *d_f;
  KZGX_TRY(stage(ctx, 0, count * pb, &d_c));
  KZGX_TRY(stage(ctx, 1, count * pb, &d_p));
  KZGX_TRY(stage(ctx, 2, count * 96, &d_s));
  KZGX_TRY(stage(ctx, 3, count * 8 + 16, &d_f));
  std::vector<uint32_t> fl(2 * count);
  for (size_t k = 0; k < count; k++) {
    fl[k] = commit_inf ? (uint32_t)(commit_inf[k] != 0) : 0u;
    fl[count + k] = proof_inf ? (uint32_t)(proof_inf[k] != 0) : 0u;
  }
  hipStream_t st = ctx->c.stream;
  KZGX_TRY_HIP(hipMemcpyAsync(d_c, commits_xy, count * pb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_p, proofs_xy, count * pb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_s, zs, count * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync((char*)d_s + count * 32, ys, count * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync((char*)d_s + count * 64, challenges, count * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_f, fl.data(), count * 8, hipMemcpyHostToDevice, st));
  uint32_t* d_ok = (uint32_t*)d_f + 2 * count;
  if (checked)
    KZGX_TRY(kzgx_verify_aggregate_checked_device(ctx, d_c, d_f, d_p, (uint32_t*)d_f + count, d_s,
                                                  (char*)d_s + count * 32, (char*)d_s + count * 64, count, subgroup,
                                                  d_ok, nullptr));
  else
    KZGX_TRY(kzgx_verify_aggregate_device(ctx, d_c, d_f, d_p, (uint32_t*)d_f + count, d_s, (char*)d_s + count * 32,
                                          (char*)d_s + count * 64, count, d_ok, nullptr));
  uint32_t v = 0;
  KZGX_TRY_HIP(hipMemcpyAsync(&v, d_ok, 4, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  *ok = v ? 1 : 0;
  return KZGX_OK;
}

int kzgx_verify_aggregate(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf, const uint64_t* proofs_xy,
                          const int* proof_inf, const uint64_t* zs, const uint64_t* ys, const uint64_t* challenges,
                          size_t count, int* ok) {
  return verify_aggregate_host(ctx, commits_xy, commit_inf, proofs_xy, proof_inf, zs, ys, challenges, count, false, 0,
                               ok);
}

int kzgx_verify_aggregate_checked(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf,
                                  const uint64_t* proofs_xy, const int* proof_inf, const uint64_t* zs,
                                  const uint64_t* ys, const uint64_t* challenges, size_t count, int subgroup, int* ok) {
  return verify_aggregate_host(ctx, commits_xy, commit_inf, proofs_xy, proof_inf, zs, ys, challenges, count, true,
                               subgroup, ok);
}

// ---- evaluation form ------------------------------------------------------------
int kzgx_ntt_max_log2(int curve) { return kzgx::ntt_max_log2(curve); }

int kzgx_domain_root(int curve, unsigned log2n, uint64_t* root) {
  if (!root) return KZGX_ERR_ARG;
  const uint32_t* w = nullptr;
  if (curve == KZGX_CURVE_BN254 && log2n <= (unsigned)kzgx::BN254FrNtt::TWO_ADICITY)
    w = kzgx::BN254FrNtt::ROOT[log2n];
  else if (curve == KZGX_CURVE_BLS12381 && log2n <= (unsigned)kzgx::BLS12381FrNtt::TWO_ADICITY)
    w = kzgx::BLS12381FrNtt::ROOT[log2n];
  if (!w) return KZGX_ERR_ARG;
  for (int i = 0; i < 4; i++) root[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
  return KZGX_OK;
}

int kzgx_ntt_device(kzgx_ctx* ctx, const void* d_in, size_t in_stride, void* d_out, size_t out_stride,
                    unsigned log2n, size_t batch, int flags, void* stream) {
  KZGX_TRY(activate(ctx));
  if (batch == 0) return KZGX_OK;
  if ((flags & ~(KZGX_NTT_INVERSE | KZGX_NTT_BITREV)) || (int)log2n > kzgx::ntt_max_log2(ctx->c.curve))
    return KZGX_ERR_ARG;
  const size_t n = (size_t)1 << log2n;
  if (!d_in || !d_out || in_stride < n || out_stride < n || (d_in == d_out && in_stride != out_stride))
    return KZGX_ERR_ARG;
  return kzgx::ntt(&ctx->c, (const uint32_t*)d_in, in_stride, (uint32_t*)d_out, out_stride, log2n, batch,
                   (flags & KZGX_NTT_INVERSE) != 0, (flags & KZGX_NTT_BITREV) != 0, pick(ctx, stream));
}

int kzgx_ntt(kzgx_ctx* ctx, const uint64_t* in, unsigned log2n, size_t batch, int flags, uint64_t* out) {
  KZGX_TRY(activate(ctx));
  if (batch == 0) return KZGX_OK;
  if ((int)log2n > kzgx::ntt_max_log2(ctx->c.curve) || !in || !out) return KZGX_ERR_ARG;
  const size_t n = (size_t)1 << log2n, bytes = batch * n * 32;
  void* d = nullptr;
  KZGX_TRY(stage(ctx, 0, bytes, &d));
  hipStream_t st = ctx->c.stream;
  KZGX_TRY_HIP(hipMemcpyAsync(d, in, bytes, hipMemcpyHostToDevice, st));
  KZGX_TRY(kzgx_ntt_device(ctx, d, n, d, n, log2n, batch, flags, st));
  KZGX_TRY_HIP(hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  return KZGX_OK;
}

}  // extern "C"

namespace {
// the argument checks the commit and the prove entries share; *n = 2^log2n
int evals_args(kzgx_ctx* ctx, unsigned log2n, size_t eval_stride, bool stride0_ok, int flags, size_t* n) {
  if ((flags & ~KZGX_NTT_BITREV) || (int)log2n > kzgx::ntt_max_log2(ctx->c.curve)) return KZGX_ERR_ARG;
  *n = (size_t)1 << log2n;
  if (eval_stride < *n && !(stride0_ok && eval_stride == 0)) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  if (*n > ctx->c.n_srs) return KZGX_ERR_DEGREE;
  return KZGX_OK;
}

// inverse NTT of npolys evaluation vectors into the stream's coefficient
// workspace (n scalars apart); the caller's buffer is only read
int evals_to_coeffs(kzgx_ctx* ctx, const kzgx::WsLease& ws, const void* d_evals, size_t eval_stride, unsigned log2n,
                    size_t npolys, int flags, hipStream_t st) {
  const size_t n = (size_t)1 << log2n;
  KZGX_TRY(kzgx::dev_alloc(&ctx->c, (void**)&ws->ntt_coef, npolys * n * 32, &ws->ntt_coef_b));
  return kzgx::ntt(&ctx->c, (const uint32_t*)d_evals, eval_stride ? eval_stride : n, ws->ntt_coef, n, log2n, npolys,
                   true, (flags & KZGX_NTT_BITREV) != 0, st);
}
}  // namespace

extern "C" {

int kzgx_commit_evals_batch_device(kzgx_ctx* ctx, const void* d_evals, unsigned log2n, size_t batch,
                                   size_t eval_stride, int flags, void* d_out_xy, void* d_out_is_inf,
                                   void* stream) {
  KZGX_TRY(activate(ctx));
  if (batch == 0) return KZGX_OK;
  size_t n = 0;
  KZGX_TRY(evals_args(ctx, log2n, eval_stride, false, flags, &n));
  if (!d_evals || !d_out_xy || !d_out_is_inf || batch > 65535) return KZGX_ERR_ARG;
  hipStream_t st = pick(ctx, stream);
  kzgx::WsLease ws = ctx->c.ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  KZGX_TRY(evals_to_coeffs(ctx, ws, d_evals, eval_stride, log2n, batch, flags, st));
  return kzgx_msm_g1_batch_device(ctx, ws->ntt_coef, n, batch, n, d_out_xy, d_out_is_inf, st);
}

int kzgx_commit_evals_batch(kzgx_ctx* ctx, const uint64_t* evals, unsigned log2n, size_t batch, int flags,
                            uint64_t* out_xy, int* out_is_inf) {
  KZGX_TRY(activate(ctx));
  if (batch == 0) return KZGX_OK;
  size_t n = 0;
  KZGX_TRY(evals_args(ctx, log2n, (size_t)-1, false, flags, &n));  // rows are packed: no stride to check
  if (!evals || !out_xy || !out_is_inf) return KZGX_ERR_ARG;
  const size_t eb = batch * n * 32, ob = batch * point_words(ctx) * 4;
  void *d_e, *d_o;
  KZGX_TRY(stage(ctx, 0, eb, &d_e));
  KZGX_TRY(stage(ctx, 1, align256(ob) + batch * 4, &d_o));
  void* d_i = (char*)d_o + align256(ob);
  hipStream_t st = ctx->c.stream;
  KZGX_TRY_HIP(hipMemcpyAsync(d_e, evals, eb, hipMemcpyHostToDevice, st));
  KZGX_TRY(kzgx_commit_evals_batch_device(ctx, d_e, log2n, batch, n, flags, d_o, d_i, st));
  std::vector<uint32_t> inf(batch);
  KZGX_TRY_HIP(hipMemcpyAsync(out_xy, d_o, ob, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipMemcpyAsync(inf.data(), d_i, batch * 4, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  for (size_t b = 0; b < batch; b++) out_is_inf[b] = (int)inf[b];
  return KZGX_OK;
}

int kzgx_prove_evals_batch_device(kzgx_ctx* ctx, const void* d_evals, unsigned log2n, size_t eval_stride,
                                  const void* d_z, size_t batch, int flags, void* d_out_xy,
                                  void* d_out_is_inf, void* d_y, void* stream) {
  KZGX_TRY(activate(ctx));
  if (batch == 0) return KZGX_OK;
  size_t n = 0;
  KZGX_TRY(evals_args(ctx, log2n, eval_stride, true, flags, &n));
  if (!d_evals || !d_z || !d_out_xy || !d_out_is_inf || batch > 65535) return KZGX_ERR_ARG;
  hipStream_t st = pick(ctx, stream);
  kzgx::WsLease ws = ctx->c.ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  KZGX_TRY(evals_to_coeffs(ctx, ws, d_evals, eval_stride, log2n, eval_stride ? batch : 1, flags, st));
  return kzgx_prove_single_batch_device(ctx, ws->ntt_coef, n, eval_stride ? n : 0, d_z, batch, d_out_xy,
                                        d_out_is_inf, d_y, st);
}

int kzgx_prove_evals_batch(kzgx_ctx* ctx, const uint64_t* evals, unsigned log2n, size_t eval_stride,
                           const uint64_t* zs, size_t batch, int flags, uint64_t* out_xy, int* out_is_inf,
                           uint64_t* out_y) {
  KZGX_TRY(activate(ctx));
  if (batch == 0) return KZGX_OK;
  size_t n = 0;
  KZGX_TRY(evals_args(ctx, log2n, eval_stride, true, flags, &n));
  if (!evals || !zs || !out_xy || !out_is_inf) return KZGX_ERR_ARG;
  const size_t eb = (eval_stride ? (batch - 1) * eval_stride + n : n) * 32, ob = batch * point_words(ctx) * 4;
  const size_t i_off = align256(ob), y_off = i_off + align256(batch * 4);
  void *d_e, *d_z, *d_o;
  KZGX_TRY(stage(ctx, 0, eb, &d_e));
  KZGX_TRY(stage(ctx, 1, batch * 32, &d_z));
  KZGX_TRY(stage(ctx, 2, y_off + batch * 32, &d_o));
  hipStream_t st = ctx->c.stream;
  KZGX_TRY_HIP(hipMemcpyAsync(d_e, evals, eb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_z, zs, batch * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY(kzgx_prove_evals_batch_device(ctx, d_e, log2n, eval_stride, d_z, batch, flags, d_o, (char*)d_o + i_off,
                                         (char*)d_o + y_off, st));
  std::vector<uint32_t> inf(batch);
  KZGX_TRY_HIP(hipMemcpyAsync(out_xy, d_o, ob, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipMemcpyAsync(inf.data(), (char*)d_o + i_off, batch * 4, hipMemcpyDeviceToHost, st));
  if (out_y) KZGX_TRY_HIP(hipMemcpyAsync(out_y, (char*)d_o + y_off, batch * 32, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  for (size_t b = 0; b < batch; b++) out_is_inf[b] = (int)inf[b];
  return KZGX_OK;
}

// ---- G1 NTT, all-domain openings ------------------------------------------------------
int kzgx_g1_ntt_device(kzgx_ctx* ctx, const void* d_in_xy, const void* d_in_is_inf, void* d_out_xy,
                       void* d_out_is_inf, unsigned log2n, size_t batch, int flags, void* stream) {
  KZGX_TRY(activate(ctx));
  if (batch == 0) return KZGX_OK;
  if ((flags & ~(KZGX_NTT_INVERSE | KZGX_NTT_BITREV)) || (int)log2n > kzgx::ntt_max_log2(ctx->c.curve))
    return KZGX_ERR_ARG;
  if (!d_in_xy || !d_out_xy || !d_out_is_inf || d_in_xy == d_out_xy || batch > (SIZE_MAX >> 8 >> log2n))
    return KZGX_ERR_ARG;
  hipStream_t st = pick(ctx, stream);
  kzgx::WsLease ws = ctx->c.ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  return kzgx::g1_ntt(&ctx->c, *ws, (const uint32_t*)d_in_xy, (const uint32_t*)d_in_is_inf, (uint32_t*)d_out_xy,
                      (uint32_t*)d_out_is_inf, log2n, batch, (flags & KZGX_NTT_INVERSE) != 0,
                      (flags & KZGX_NTT_BITREV) != 0, st);
}

int kzgx_g1_ntt(kzgx_ctx* ctx, const uint64_t* in_xy, const int* in_is_inf, unsigned log2n, size_t batch, int flags,
                uint64_t* out_xy, int* out_is_inf) {
  KZGX_TRY(activate(ctx));
  if (batch == 0) return KZGX_OK;
  if ((flags & ~(KZGX_NTT_INVERSE | KZGX_NTT_BITREV)) || (int)log2n > kzgx::ntt_max_log2(ctx->c.curve))
    return KZGX_ERR_ARG;
  if (!in_xy || !out_xy || !out_is_inf || batch > (SIZE_MAX >> 8 >> log2n)) return KZGX_ERR_ARG;
  const size_t cnt = batch << log2n, pb = cnt * point_words(ctx) * 4;
  void *d_p, *d_f, *d_o;
  KZGX_TRY(stage(ctx, 0, pb, &d_p));
  KZGX_TRY(stage(ctx, 1, cnt * 4, &d_f));
  KZGX_TRY(stage(ctx, 2, align256(pb) + cnt * 4, &d_o));
  void* d_oi = (char*)d_o + align256(pb);
  hipStream_t st = ctx->c.stream;
  std::vector<uint32_t> f(cnt, 0u);
  if (in_is_inf)
    for (size_t i = 0; i < cnt; i++) f[i] = (uint32_t)(in_is_inf[i] != 0);
  KZGX_TRY_HIP(hipMemcpyAsync(d_p, in_xy, pb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_f, f.data(), cnt * 4, hipMemcpyHostToDevice, st));
  KZGX_TRY(kzgx_g1_ntt_device(ctx, d_p, d_f, d_o, d_oi, log2n, batch, flags, st));
  KZGX_TRY_HIP(hipMemcpyAsync(out_xy, d_o, pb, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipMemcpyAsync(f.data(), d_oi, cnt * 4, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  for (size_t i = 0; i < cnt; i++) out_is_inf[i] = (int)f[i];
  return KZGX_OK;
}

}  // extern "C"

namespace {
// the argument checks of the all-domain entries; *n = 2^log2n
int prove_all_args(kzgx_ctx* ctx, unsigned log2n, size_t in_stride, int flags, size_t* n) {
  if ((flags & ~(KZGX_NTT_BITREV | KZGX_PROVE_ALL_EVALS)) || (int)log2n + 1 > kzgx::ntt_max_log2(ctx->c.curve))
    return KZGX_ERR_ARG;
  *n = (size_t)1 << log2n;
  if (in_stride < *n) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  if (*n > ctx->c.n_srs) return KZGX_ERR_DEGREE;
  return KZGX_OK;
}
}  // namespace

extern "C" {

int kzgx_prove_all_prepare(kzgx_ctx* ctx, unsigned log2n) {
  KZGX_TRY(activate(ctx));
  size_t n = 0;
  KZGX_TRY(prove_all_args(ctx, log2n, (size_t)-1, 0, &n));
  hipStream_t st = ctx->c.stream;
  {
    kzgx::WsLease ws = ctx->c.ws_for(st);
    if (!ws) return KZGX_ERR_ARG;
    KZGX_TRY(kzgx::prove_all_setup(&ctx->c, *ws, ctx->d_srs_canon, log2n, st));
  }
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  return KZGX_OK;
}

int kzgx_prove_all_batch_device(kzgx_ctx* ctx, const void* d_in, unsigned log2n, size_t batch, size_t in_stride,
                                int flags, void* d_out_xy, void* d_out_is_inf, void* d_y, void* stream) {
  KZGX_TRY(activate(ctx));
  if (batch == 0) return KZGX_OK;
  size_t n = 0;
  KZGX_TRY(prove_all_args(ctx, log2n, in_stride, flags, &n));
  if (!d_in || !d_out_xy || !d_out_is_inf || batch > 0xffffffffu || batch > (SIZE_MAX >> 8 >> log2n))
    return KZGX_ERR_ARG;
  hipStream_t st = pick(ctx, stream);
  kzgx::WsLease ws = ctx->c.ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  const bool bitrev = (flags & KZGX_NTT_BITREV) != 0, evals = (flags & KZGX_PROVE_ALL_EVALS) != 0;
  // chunks of polynomials, so that every workspace of the call is bounded
  const size_t chunk = std::max<size_t>(1, kzgx::G1_NTT_CHUNK_RECORDS >> (log2n + 1)), pw = point_words(ctx);
  for (size_t b0 = 0; b0 < batch; b0 += chunk) {
    const size_t cb = std::min(chunk, batch - b0);
    const uint32_t* d_coef = (const uint32_t*)d_in + b0 * in_stride * 8;
    uint32_t* d_yc = d_y ? (uint32_t*)d_y + b0 * n * 8 : nullptr;
    size_t stride = in_stride;
    if (evals) {
      // the values are the y of every opening as they stand; the coefficients go to workspace
      if (d_yc)
        KZGX_TRY_HIP(hipMemcpy2DAsync(d_yc, n * 32, d_coef, in_stride * 32, n * 32, cb, hipMemcpyDeviceToDevice, st));
      KZGX_TRY(evals_to_coeffs(ctx, ws, d_coef, in_stride, log2n, cb, flags & KZGX_NTT_BITREV, st));
      d_coef = ws->ntt_coef;
      stride = n;
    } else if (d_yc) {
      KZGX_TRY(kzgx::ntt(&ctx->c, d_coef, stride, d_yc, n, log2n, cb, false, bitrev, st));
    }
    KZGX_TRY(kzgx::prove_all(&ctx->c, *ws, ctx->d_srs_canon, d_coef, stride, log2n, cb, bitrev,
                             (uint32_t*)d_out_xy + b0 * n * pw, (uint32_t*)d_out_is_inf + b0 * n, st));
  }
  return KZGX_OK;
}

int kzgx_prove_all_batch(kzgx_ctx* ctx, const uint64_t* in, unsigned log2n, size_t batch, int flags,
                         uint64_t* out_xy, int* out_is_inf, uint64_t* out_y) {
  KZGX_TRY(activate(ctx));
  if (batch == 0) return KZGX_OK;
  size_t n = 0;
  KZGX_TRY(prove_all_args(ctx, log2n, (size_t)-1, flags, &n));  // rows are packed: no stride to check
  if (!in || !out_xy || !out_is_inf || batch > (SIZE_MAX >> 8 >> log2n)) return KZGX_ERR_ARG;
  const size_t cnt = batch * n, sb = cnt * 32, ob = cnt * point_words(ctx) * 4;
  const size_t i_off = align256(ob), y_off = i_off + align256(cnt * 4);
  void *d_e, *d_o;
  KZGX_TRY(stage(ctx, 0, sb, &d_e));
  KZGX_TRY(stage(ctx, 1, y_off + sb, &d_o));
  hipStream_t st = ctx->c.stream;
  KZGX_TRY_HIP(hipMemcpyAsync(d_e, in, sb, hipMemcpyHostToDevice, st));
  KZGX_TRY(kzgx_prove_all_batch_device(ctx, d_e, log2n, batch, n, flags, d_o, (char*)d_o + i_off,
                                       out_y ? (char*)d_o + y_off : nullptr, st));
  std::vector<uint32_t> inf(cnt);
  KZGX_TRY_HIP(hipMemcpyAsync(out_xy, d_o, ob, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipMemcpyAsync(inf.data(), (char*)d_o + i_off, cnt * 4, hipMemcpyDeviceToHost, st));
  if (out_y) KZGX_TRY_HIP(hipMemcpyAsync(out_y, (char*)d_o + y_off, sb, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  for (size_t i = 0; i < cnt; i++) out_is_inf[i] = (int)inf[i];
  return KZGX_OK;
}

}  // extern "C"

namespace {
using kzgx::fr_host_mmul;  // fr_host.hpp

// xs[q] = the point of offset q in chunk `index` of y: w_D^(i + R j), with bitrev i = brev_R(index), j = brev_l(q)
template <class FR, class T>
void coset_points_host(unsigned kr, unsigned kl, bool bitrev, size_t index, uint64_t* xs) {
  const auto brev = [](size_t v, unsigned bits) {
    size_t r = 0;
    for (unsigned b = 0; b < bits; b++) r |= ((v >> b) & 1) << (bits - 1 - b);
    return r;
  };
  const size_t i = bitrev ? brev(index, kr) : index;
  uint32_t x[8], sq[8], step[8];
  const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  fr_host_mmul<FR>(T::ROOT[kr + kl], FR::R2, sq);  // Montgomery form of w_D
  std::copy(FR::ONE, FR::ONE + 8, x);
  for (unsigned b = 0; b < kr; b++) {  // x = w_D^i; sq ends as w_D^R, of order l
    if ((i >> b) & 1) fr_host_mmul<FR>(x, sq, x);
    fr_host_mmul<FR>(sq, sq, sq);
  }
  std::copy(sq, sq + 8, step);
  for (size_t j = 0; j < ((size_t)1 << kl); j++) {
    uint32_t c[8];
    fr_host_mmul<FR>(x, one, c);
    uint64_t* o = xs + 4 * (bitrev ? brev(j, kl) : j);
    for (int w = 0; w < 4; w++) o[w] = (uint64_t)c[2 * w] | ((uint64_t)c[2 * w + 1] << 32);
    fr_host_mmul<FR>(x, step, x);
  }
}

// the shapes of the coset entries: the size-2m and the size-D domains must exist
bool cosets_shape_ok(int curve, unsigned log2n, unsigned log2l, int flags) {
  const int mx = kzgx::ntt_max_log2(curve);
  if (mx < 0 || log2n > 31 || log2l > log2n) return false;
  if (flags & ~(KZGX_NTT_BITREV | KZGX_PROVE_ALL_EVALS | KZGX_PROVE_COSETS_EXTENDED)) return false;
  const int ext = (flags & KZGX_PROVE_COSETS_EXTENDED) ? 1 : 0;
  return (int)(log2n - log2l) + 1 <= mx && (int)log2n + ext <= mx;
}

// the argument checks of the coset entries; *n = 2^log2n
int prove_cosets_args(kzgx_ctx* ctx, unsigned log2n, unsigned log2l, size_t in_stride, int flags, size_t* n) {
  if (!cosets_shape_ok(ctx->c.curve, log2n, log2l, flags)) return KZGX_ERR_ARG;
  *n = (size_t)1 << log2n;
  if (in_stride < *n) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  if (*n > ctx->c.n_srs) return KZGX_ERR_DEGREE;
  return KZGX_OK;
}
}  // namespace

extern "C" {

// ---- coset openings -------------------------------------------------------------------------
int kzgx_coset_points(int curve, unsigned log2n, unsigned log2l, int flags, size_t index, uint64_t* xs) {
  if (!xs || !cosets_shape_ok(curve, log2n, log2l, flags)) return KZGX_ERR_ARG;
  const unsigned kr = log2n - log2l + ((flags & KZGX_PROVE_COSETS_EXTENDED) ? 1 : 0);
  if (index >> kr) return KZGX_ERR_ARG;
  const bool bitrev = (flags & KZGX_NTT_BITREV) != 0;
  if (curve == KZGX_CURVE_BN254)
    coset_points_host<kzgx::BN254Fr, kzgx::BN254FrNtt>(kr, log2l, bitrev, index, xs);
  else
    coset_points_host<kzgx::BLS12381Fr, kzgx::BLS12381FrNtt>(kr, log2l, bitrev, index, xs);
  return KZGX_OK;
}

int kzgx_prove_cosets_prepare(kzgx_ctx* ctx, unsigned log2n, unsigned log2l) {
  KZGX_TRY(activate(ctx));
  size_t n = 0;
  KZGX_TRY(prove_cosets_args(ctx, log2n, log2l, (size_t)-1, 0, &n));
  hipStream_t st = ctx->c.stream;
  {
    kzgx::WsLease ws = ctx->c.ws_for(st);
    if (!ws) return KZGX_ERR_ARG;
    KZGX_TRY(kzgx::prove_cosets_setup(&ctx->c, *ws, ctx->d_srs_canon, log2n, log2l, st));
  }
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  return KZGX_OK;
}

int kzgx_prove_cosets_batch_device(kzgx_ctx* ctx, const void* d_in, unsigned log2n, unsigned log2l, size_t batch,
                                   size_t in_stride, int flags, void* d_out_xy, void* d_out_is_inf, void* d_y,
                                   void* stream) {
  KZGX_TRY(activate(ctx));
  if (batch == 0) return KZGX_OK;
  size_t n = 0;
  KZGX_TRY(prove_cosets_args(ctx, log2n, log2l, in_stride, flags, &n));
  if (!d_in || !d_out_xy || !d_out_is_inf || batch > 0xffffffffu || batch > (SIZE_MAX >> 9 >> log2n))
    return KZGX_ERR_ARG;
  hipStream_t st = pick(ctx, stream);
  kzgx::WsLease ws = ctx->c.ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  const bool bitrev = (flags & KZGX_NTT_BITREV) != 0, evals = (flags & KZGX_PROVE_ALL_EVALS) != 0,
             ext = (flags & KZGX_PROVE_COSETS_EXTENDED) != 0;
  const size_t R = (size_t)1 << (log2n - log2l + (ext ? 1 : 0)), D = R << log2l;
  // chunks of polynomials, so that every workspace of the call is bounded
  const size_t chunk = std::max<size_t>(1, kzgx::G1_NTT_CHUNK_RECORDS >> (log2n + 1)), pw = point_words(ctx);
  for (size_t b0 = 0; b0 < batch; b0 += chunk) {
    const size_t cb = std::min(chunk, batch - b0);
    const uint32_t* d_coef = (const uint32_t*)d_in + b0 * in_stride * 8;
    size_t stride = in_stride;
    if (evals) {
      KZGX_TRY(evals_to_coeffs(ctx, ws, d_coef, in_stride, log2n, cb, flags & KZGX_NTT_BITREV, st));
      d_coef = ws->ntt_coef;
      stride = n;
    }
    KZGX_TRY(kzgx::prove_cosets(&ctx->c, *ws, ctx->d_srs_canon, d_coef, stride, log2n, log2l, cb, ext, bitrev,
                                (uint32_t*)d_out_xy + b0 * R * pw, (uint32_t*)d_out_is_inf + b0 * R,
                                d_y ? (uint32_t*)d_y + b0 * D * 8 : nullptr, st));
  }
  return KZGX_OK;
}

int kzgx_prove_cosets_batch(kzgx_ctx* ctx, const uint64_t* in, unsigned log2n, unsigned log2l, size_t batch,
                            int flags, uint64_t* out_xy, int* out_is_inf, uint64_t* out_y) {
  KZGX_TRY(activate(ctx));
  if (batch == 0) return KZGX_OK;
  size_t n = 0;
  KZGX_TRY(prove_cosets_args(ctx, log2n, log2l, (size_t)-1, flags, &n));  // rows are packed: no stride to check
  if (!in || !out_xy || !out_is_inf || batch > (SIZE_MAX >> 9 >> log2n)) return KZGX_ERR_ARG;
  const size_t R = (size_t)1 << (log2n - log2l + ((flags & KZGX_PROVE_COSETS_EXTENDED) ? 1 : 0));
  const size_t cnt = batch * R, sb = batch * n * 32, yb = (cnt << log2l) * 32, ob = cnt * point_words(ctx) * 4;
  const size_t i_off = align256(ob), y_off = i_off + align256(cnt * 4);
  void *d_e, *d_o;
  KZGX_TRY(stage(ctx, 0, sb, &d_e));
  KZGX_TRY(stage(ctx, 1, y_off + yb, &d_o));
  hipStream_t st = ctx->c.stream;
  KZGX_TRY_HIP(hipMemcpyAsync(d_e, in, sb, hipMemcpyHostToDevice, st));
  KZGX_TRY(kzgx_prove_cosets_batch_device(ctx, d_e, log2n, log2l, batch, n, flags, d_o, (char*)d_o + i_off,
                                          out_y ? (char*)d_o + y_off : nullptr, st));
  std::vector<uint32_t> inf(cnt);
  KZGX_TRY_HIP(hipMemcpyAsync(out_xy, d_o, ob, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipMemcpyAsync(inf.data(), (char*)d_o + i_off, cnt * 4, hipMemcpyDeviceToHost, st));
  if (out_y) KZGX_TRY_HIP(hipMemcpyAsync(out_y, (char*)d_o + y_off, yb, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  for (size_t i = 0; i < cnt; i++) out_is_inf[i] = (int)inf[i];
  return KZGX_OK;
}

}  // extern "C"

// ---- aggregated cell verification -----------------------------------------------------------
namespace {
struct CellsShape {
  unsigned kR, kD;  // log2 of the cosets and of the domain they partition
  size_t l;
  bool bitrev;
};

// the argument, limit and setup checks shared by the four entries
int cells_args(kzgx_ctx* ctx, size_t n_commits, size_t count, unsigned log2n, unsigned log2l, int flags,
               CellsShape* s) {
  const int mx = kzgx::ntt_max_log2(ctx->c.curve);
  if (flags & ~(KZGX_NTT_BITREV | KZGX_PROVE_COSETS_EXTENDED)) return KZGX_ERR_ARG;
  const int ext = (flags & KZGX_PROVE_COSETS_EXTENDED) ? 1 : 0;
  if (mx < 0 || log2n > 31 || log2l > log2n || (int)log2n + ext > mx) return KZGX_ERR_ARG;
  s->kR = log2n - log2l + ext;
  s->kD = log2n + ext;
  s->l = (size_t)1 << log2l;
  s->bitrev = (flags & KZGX_NTT_BITREV) != 0;
  if (n_commits > KZGX_MSM_POINTS_MAX || count > KZGX_MSM_POINTS_MAX ||
      n_commits + count + s->l > KZGX_MSM_POINTS_MAX)
    return KZGX_ERR_ARG;
  if ((count << log2l) > KZGX_VERIFY_CELLS_VALUES_MAX) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0 || ctx->n_srs2 < s->l + 1) return KZGX_ERR_NO_SRS;
  if (ctx->c.n_srs < s->l) return KZGX_ERR_DEGREE;
  return KZGX_OK;
}
}  // namespace

extern "C" {

int kzgx_verify_cells_aggregate_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf,
                                       size_t n_commits, const void* d_commit_index, const void* d_cell_index,
                                       const void* d_proofs, const void* d_proof_inf, const void* d_ys,
                                       const void* d_challenges, size_t count, unsigned log2n, unsigned log2l,
                                       int flags, void* d_ok, void* stream) {
  KZGX_TRY(activate(ctx));
  if (!d_ok || !d_challenges) return KZGX_ERR_ARG;
  if (count > 0 && (!d_commit_index || !d_cell_index || !d_proofs || !d_ys || (n_commits > 0 && !d_commits)))
    return KZGX_ERR_ARG;
  CellsShape sh;
  KZGX_TRY(cells_args(ctx, n_commits, count, log2n, log2l, flags, &sh));
  hipStream_t st = pick(ctx, stream);
  if (count == 0) {
    KZGX_TRY_HIP(hipMemsetD32Async((hipDeviceptr_t)d_ok, 1, 1, st));
    return KZGX_OK;
  }
  kzgx::Ctx* c = &ctx->c;
  kzgx::WsLease ws = c->ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  const size_t pw = point_words(ctx), l = sh.l, nsl = kzgx::cells_fold_slices(count, log2l);
  // the cells' interpolants; rho | s | -S (+ the fold's partials and flags);
  // A | B | their flags, the index gate | G2[l], G2[0] | the pairing's line tables
  KZGX_TRY(kzgx::dev_alloc(c, (void**)&ws->ntt_coef, count * l * 32, &ws->ntt_coef_b));
  KZGX_TRY(kzgx::dev_alloc(c, (void**)&ws->var_scal, (n_commits + count + l + nsl * l) * 32 + nsl * 4,
                           &ws->var_scal_b));
  const size_t o_q = 2 * pw + 8, o_ln = (o_q + 4 * pw + 63) & ~(size_t)63;
  KZGX_TRY(kzgx::dev_alloc(c, (void**)&ws->var_pt, o_ln * 4 + kzgx::pair2_wave_scratch_bytes(c->curve),
                           &ws->var_pt_b));
  uint32_t* A = ws->var_pt;
  uint32_t* B = A + pw;
  uint32_t* fl = B + pw;  // [A_inf, B_inf, -, -, gate]
  uint32_t* gate = fl + 4;
  uint32_t* q = A + o_q;
  // I_k's coefficients up to the coset shift: the size-l inverse transforms of the values
  KZGX_TRY(kzgx::ntt_twiddles(c, sh.kD, st));
  KZGX_TRY(kzgx::ntt(c, (const uint32_t*)d_ys, l, ws->ntt_coef, l, log2l, count, true, sh.bitrev, st));
  KZGX_TRY(kzgx::cells_scalars(c, ws->ntt_coef, (const uint32_t*)d_challenges, (const uint32_t*)d_cell_index,
                               (const uint32_t*)d_commit_index, count, n_commits, log2l, sh.kD, sh.bitrev,
                               ws->var_scal, gate, st));
  // A = sum r_k proof_k
  const kzgx::PointSeg sa{(const uint32_t*)d_proofs, (const uint32_t*)d_proof_inf, count};
  KZGX_TRY(kzgx::msm_points(c, *ws, &sa, 1, (const uint32_t*)d_challenges, A, fl, st));
  // B = sum rho_c commit_c + sum r_k a_k proof_k - sum S_t G1[t]
  const kzgx::PointSeg sb[3] = {{(const uint32_t*)d_commits, (const uint32_t*)d_commit_inf, n_commits},
                                {(const uint32_t*)d_proofs, (const uint32_t*)d_proof_inf, count},
                                {ctx->d_srs_canon, nullptr, l}};
  KZGX_TRY(kzgx::msm_points(c, *ws, sb, 3, ws->var_scal, B, fl + 1, st));
  // e(A, G2[l]) e(-B, G2[0]) == 1, every case decided on the device; then the index gate
  const size_t p2 = 2 * pw * 4;
  KZGX_TRY_HIP(hipMemcpyAsync(q, (const char*)ctx->d_srs2_canon + l * p2, p2, hipMemcpyDeviceToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync((char*)q + p2, ctx->d_srs2_canon, p2, hipMemcpyDeviceToDevice, st));
  KZGX_TRY(kzgx::pair2_wave(c, A, fl, q, nullptr, A + o_ln, (uint32_t*)d_ok, st));
  return kzgx::flag_gate((uint32_t*)d_ok, gate, st);
}

int kzgx_verify_cells_aggregate_checked_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf,
                                               size_t n_commits, const void* d_commit_index,
                                               const void* d_cell_index, const void* d_proofs,
                                               const void* d_proof_inf, const void* d_ys, const void* d_challenges,
                                               size_t count, unsigned log2n, unsigned log2l, int flags, int subgroup,
                                               void* d_ok, void* stream) {
  KZGX_TRY(activate(ctx));
  if (!d_ok || !d_challenges) return KZGX_ERR_ARG;
  if (count > 0 && (!d_commit_index || !d_cell_index || !d_proofs || !d_ys || (n_commits > 0 && !d_commits)))
    return KZGX_ERR_ARG;
  CellsShape sh;
  KZGX_TRY(cells_args(ctx, n_commits, count, log2n, log2l, flags, &sh));
  hipStream_t st = pick(ctx, stream);
  if (count == 0) {
    KZGX_TRY_HIP(hipMemsetD32Async((hipDeviceptr_t)d_ok, 1, 1, st));
    return KZGX_OK;
  }
  kzgx::WsLease ws = ctx->c.ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  const size_t np = n_commits + count;
  uint32_t* f;  // commit flags | proof flags | their AND
  KZGX_TRY(chk_scratch(ctx, ws, np + 1, &f));
  KZGX_TRY(kzgx::g1_check2(&ctx->c, (const uint32_t*)d_commits, (const uint32_t*)d_commit_inf, n_commits,
                           (const uint32_t*)d_proofs, (const uint32_t*)d_proof_inf, count, subgroup, f, st));
  KZGX_TRY(kzgx::flags_and(f, np, f + np, st));
  KZGX_TRY(kzgx_verify_cells_aggregate_device(ctx, d_commits, d_commit_inf, n_commits, d_commit_index, d_cell_index,
                                              d_proofs, d_proof_inf, d_ys, d_challenges, count, log2n, log2l, flags,
                                              d_ok, stream));
  return kzgx::flag_gate((uint32_t*)d_ok, f + np, st);
}

}  // extern "C"

// the host-pointer forms share the staging, the index checks and the drawn challenges
static int verify_cells_host(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf, size_t n_commits,
                             const uint32_t* commit_index, const uint32_t* cell_index, const uint64_t* proofs_xy,
                             const int* proof_inf, const uint64_t* ys, const uint64_t* challenges, size_t count,
                             unsigned log2n, unsigned log2l, int flags, bool checked, int subgroup, int* ok) {
  KZGX_TRY(activate(ctx));
  if (!ok) return KZGX_ERR_ARG;
  if (count > 0 && (!commit_index || !cell_index || !proofs_xy || !ys || (n_commits > 0 && !commits_xy)))
    return KZGX_ERR_ARG;
  CellsShape sh;
  KZGX_TRY(cells_args(ctx, n_commits, count, log2n, log2l, flags, &sh));
  if (count == 0) {
    *ok = 1;
    return KZGX_OK;
  }
  for (size_t k = 0; k < count; k++)
    if (commit_index[k] >= n_commits || (cell_index[k] >> sh.kR)) return KZGX_ERR_ARG;
  // library-drawn challenges: independent 128-bit values, r_0 = 1 (as kzgx_verify_aggregate)
  std::vector<uint64_t> drawn;
  if (!challenges) {
    drawn.assign(count * 4, 0);
    std::random_device rd;
    for (size_t k = 0; k < count; k++)
      for (int j = 0; j < 2; j++) drawn[4 * k + j] = ((uint64_t)rd() << 32) | (uint64_t)rd();
    drawn[0] = 1;
    drawn[1] = 0;
    challenges = drawn.data();
  }
  const size_t pb = point_words(ctx) * 4, yb = count * sh.l * 32, np = n_commits + count;
  void *d_c, *d_p, *d_s, *d_f;
  KZGX_TRY(stage(ctx, 0, n_commits * pb + 16, &d_c));
  KZGX_TRY(stage(ctx, 1, count * pb, &d_p));
  KZGX_TRY(stage(ctx, 2, yb + count * 32, &d_s));
  KZGX_TRY(stage(ctx, 3, (np + 2 * count) * 4 + 16, &d_f));
  // commit flags | proof flags | commit_index | cell_index | ok
  std::vector<uint32_t> fl(np + 2 * count);
  for (size_t k = 0; k < n_commits; k++) fl[k] = commit_inf ? (uint32_t)(commit_inf[k] != 0) : 0u;
  for (size_t k = 0; k < count; k++) {
    fl[n_commits + k] = proof_inf ? (uint32_t)(proof_inf[k] != 0) : 0u;
    fl[np + k] = commit_index[k];
    fl[np + count + k] = cell_index[k];
  }
  hipStream_t st = ctx->c.stream;
  KZGX_TRY_HIP(hipMemcpyAsync(d_c, commits_xy, n_commits * pb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_p, proofs_xy, count * pb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_s, ys, yb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync((char*)d_s + yb, challenges, count * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_f, fl.data(), fl.size() * 4, hipMemcpyHostToDevice, st));
  uint32_t* f = (uint32_t*)d_f;
  uint32_t* d_ok = f + np + 2 * count;
  if (checked)
    KZGX_TRY(kzgx_verify_cells_aggregate_checked_device(ctx, d_c, f, n_commits, f + np, f + np + count, d_p,
                                                        f + n_commits, d_s, (char*)d_s + yb, count, log2n, log2l,
                                                        flags, subgroup, d_ok, nullptr));
  else
    KZGX_TRY(kzgx_verify_cells_aggregate_device(ctx, d_c, f, n_commits, f + np, f + np + count, d_p, f + n_commits,
                                                d_s, (char*)d_s + yb, count, log2n, log2l, flags, d_ok, nullptr));
  uint32_t v = 0;
  KZGX_TRY_HIP(hipMemcpyAsync(&v, d_ok, 4, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  *ok = v ? 1 : 0;
  return KZGX_OK;
}

extern "C" {

int kzgx_verify_cells_aggregate(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf, size_t n_commits,
                                const uint32_t* commit_index, const uint32_t* cell_index, const uint64_t* proofs_xy,
                                const int* proof_inf, const uint64_t* ys, const uint64_t* challenges, size_t count,
                                unsigned log2n, unsigned log2l, int flags, int* ok) {
  return verify_cells_host(ctx, commits_xy, commit_inf, n_commits, commit_index, cell_index, proofs_xy, proof_inf, ys,
                           challenges, count, log2n, log2l, flags, false, 0, ok);
}

int kzgx_verify_cells_aggregate_checked(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf,
                                        size_t n_commits, const uint32_t* commit_index, const uint32_t* cell_index,
                                        const uint64_t* proofs_xy, const int* proof_inf, const uint64_t* ys,
                                        const uint64_t* challenges, size_t count, unsigned log2n, unsigned log2l,
                                        int flags, int subgroup, int* ok) {
  return verify_cells_host(ctx, commits_xy, commit_inf, n_commits, commit_index, cell_index, proofs_xy, proof_inf, ys,
                           challenges, count, log2n, log2l, flags, true, subgroup, ok);
}

}  // extern "C"

// ---- per-cell verdicts -------------------------------------------------------------------------
namespace {
// cells per chunk: the setter's value or the default, and at most
// KZGX_VERIFY_CELLS_EACH_CHUNK_VALUES scalars of transforms
size_t cells_each_chunk(const kzgx_ctx* ctx, unsigned log2l) {
  const size_t want = ctx->cells_chunk ? ctx->cells_chunk : (size_t)KZGX_VERIFY_CELLS_EACH_CHUNK;
  return std::max<size_t>(1, std::min(want, (size_t)KZGX_VERIFY_CELLS_EACH_CHUNK_VALUES >> log2l));
}

// the staged G2[0] || G2[l] and, for the wave path, its line tables
int cells_g2_ensure(kzgx_ctx* ctx, size_t l, bool wave, hipStream_t st, const kzgx_ctx::CellsG2** out) {
  kzgx_ctx::CellsG2& e = ctx->cells_g2[l];
  const size_t p2 = 2 * point_words(ctx) * 4;
  if (!e.d_q) {
    uint32_t* q = nullptr;
    KZGX_TRY_HIP(hipMalloc((void**)&q, 2 * p2));
    hipError_t r = hipMemcpyAsync(q, ctx->d_srs2_canon, p2, hipMemcpyDeviceToDevice, st);
    if (r == hipSuccess)
      r = hipMemcpyAsync((char*)q + p2, (const char*)ctx->d_srs2_canon + l * p2, p2, hipMemcpyDeviceToDevice, st);
    if (r == hipSuccess) r = hipStreamSynchronize(st);  // one-time; later calls may come on other streams
    if (r != hipSuccess) {
      (void)hipFree(q);
      return kzgx::hip_fail(r);
    }
    e.d_q = q;
  }
  if (wave && !e.d_vw) {
    uint32_t* b = nullptr;
    KZGX_TRY_HIP(hipMalloc((void**)&b, kzgx::verify_wave_bytes(ctx->c.curve)));
    kzgx::GenTables g;
    int r = kzgx::gen_tables_get(ctx->c.curve, ctx->c.device, st, &g);
    if (r == KZGX_OK) r = kzgx::verify_wave_prepare(&ctx->c, ctx->d_srs_canon, e.d_q, g.g1_comb, b, st);
    if (r == KZGX_OK && hipStreamSynchronize(st) != hipSuccess) r = KZGX_ERR_HIP;
    if (r != KZGX_OK) {
      (void)hipFree(b);
      return r;
    }
    e.d_vw = b;
  }
  *out = &e;
  return KZGX_OK;
}

// ok[k] = e(pi_k, G2[l]) == e(C_(c_k) - [I_k(tau)]G1 + [a_(i_k)]pi_k, G2[0]), in chunks of cells:
// inverse transforms, the interpolants' coefficients, one batched MSM over the SRS prefix,
// C' = C - [I(tau)]G1, then kzgx_verify_single_batch_device's two kernels on (C', pi, z = a, y = 0)
// against G2[0], G2[l]
int cells_each_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf, size_t n_commits,
                      const void* d_commit_index, const void* d_cell_index, const void* d_proofs,
                      const void* d_proof_inf, const void* d_ys, size_t count, unsigned log2n, unsigned log2l,
                      int flags, bool checked, int subgroup, void* d_ok, void* stream) {
  KZGX_TRY(activate(ctx));
  if (count > 0 &&
      (!d_ok || !d_commit_index || !d_cell_index || !d_proofs || !d_ys || (n_commits > 0 && !d_commits)))
    return KZGX_ERR_ARG;
  CellsShape sh;
  KZGX_TRY(cells_args(ctx, n_commits, count, log2n, log2l, flags, &sh));
  if (count == 0) return KZGX_OK;
  hipStream_t st = pick(ctx, stream);
  kzgx::Ctx* c = &ctx->c;
  const bool wave = count <= ctx->vw_max;
  const kzgx_ctx::CellsG2* g2;
  KZGX_TRY(cells_g2_ensure(ctx, sh.l, wave, st, &g2));
  kzgx::WsLease ws = c->ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  const size_t pw = point_words(ctx), l = sh.l, chunk = cells_each_chunk(ctx, log2l), cc = std::min(chunk, count);
  // the chunk's interpolants; a | y = 0; [I(tau)]G1 | C' | their flags | bad
  KZGX_TRY(kzgx::dev_alloc(c, (void**)&ws->ntt_coef, cc * l * 32, &ws->ntt_coef_b));
  KZGX_TRY(kzgx::dev_alloc(c, (void**)&ws->var_scal, 2 * cc * 32, &ws->var_scal_b));
  KZGX_TRY(kzgx::dev_alloc(c, (void**)&ws->var_pt, (2 * cc * pw + 3 * cc) * 4, &ws->var_pt_b));
  uint32_t* a = ws->var_scal;
  uint32_t* zero = a + cc * 8;
  uint32_t* I = ws->var_pt;
  uint32_t* D = I + cc * pw;
  uint32_t* I_inf = D + cc * pw;
  uint32_t* D_inf = I_inf + cc;
  uint32_t* bad = D_inf + cc;
  uint32_t* f = nullptr;  // commit flags | the chunk's proof flags
  if (checked) KZGX_TRY(chk_scratch(ctx, ws, n_commits + cc, &f));
  KZGX_TRY(kzgx::ntt_twiddles(c, sh.kD, st));
  KZGX_TRY_HIP(hipMemsetAsync(zero, 0, cc * 32, st));
  const uint32_t* cidx = (const uint32_t*)d_commit_index;
  const uint32_t* kidx = (const uint32_t*)d_cell_index;
  const uint32_t* pr = (const uint32_t*)d_proofs;
  const uint32_t* pf = (const uint32_t*)d_proof_inf;
  uint32_t* ok = (uint32_t*)d_ok;
  for (size_t k0 = 0; k0 < count; k0 += chunk) {
    const size_t m = std::min(chunk, count - k0);
    const uint32_t* pfk = pf ? pf + k0 : nullptr;
    if (checked)  // the commitments ride with the first chunk's proofs
      KZGX_TRY(kzgx::g1_check2(c, (const uint32_t*)d_commits, (const uint32_t*)d_commit_inf, k0 ? 0 : n_commits,
                               pr + k0 * pw, pfk, m, subgroup, k0 ? f + n_commits : f, st));
    {
      kzgx::ProfScope p(c, st, "cells_intt");
      KZGX_TRY(kzgx::ntt(c, (const uint32_t*)d_ys + k0 * l * 8, l, ws->ntt_coef, l, log2l, m, true, sh.bitrev, st));
    }
    KZGX_TRY(kzgx::cells_coeffs(c, ws->ntt_coef, kidx + k0, cidx + k0, m, n_commits, log2l, sh.kD, sh.bitrev, a, bad,
                                st));
    {
      kzgx::ProfScope p(c, st, "cells_msm");
      KZGX_TRY(kzgx::msm_batch(c, ws->ntt_coef, l, m, l * 8, I, I_inf, st));
    }
    KZGX_TRY(kzgx::cells_sub(c, (const uint32_t*)d_commits, (const uint32_t*)d_commit_inf, cidx + k0, bad, I, I_inf,
                             m, D, D_inf, st));
    if (wave)
      KZGX_TRY(kzgx::verify_wave_batch(c, D, D_inf, pr + k0 * pw, pfk, a, zero, m, ctx->d_srs_canon, g2->d_vw,
                                       ok + k0, st));
    else
      KZGX_TRY(kzgx::verify_single_batch(c, D, D_inf, pr + k0 * pw, pfk, a, zero, m, ctx->d_srs_canon, g2->d_q,
                                         ok + k0, st));
    KZGX_TRY(kzgx::cells_gate(ok + k0, bad, cidx + k0, f, f ? f + n_commits : nullptr, m, st));
  }
  return KZGX_OK;
}

// the host-pointer forms: staging and the index checks of verify_cells_host, count verdicts back
int cells_each_host(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf, size_t n_commits,
                    const uint32_t* commit_index, const uint32_t* cell_index, const uint64_t* proofs_xy,
                    const int* proof_inf, const uint64_t* ys, size_t count, unsigned log2n, unsigned log2l, int flags,
                    bool checked, int subgroup, int* ok) {
  KZGX_TRY(activate(ctx));
  if (count > 0 && (!ok || !commit_index || !cell_index || !proofs_xy || !ys || (n_commits > 0 && !commits_xy)))
    return KZGX_ERR_ARG;
  CellsShape sh;
  KZGX_TRY(cells_args(ctx, n_commits, count, log2n, log2l, flags, &sh));
  if (count == 0) return KZGX_OK;
  for (size_t k = 0; k < count; k++)
    if (commit_index[k] >= n_commits || (cell_index[k] >> sh.kR)) return KZGX_ERR_ARG;
  const size_t pb = point_words(ctx) * 4, yb = count * sh.l * 32, np = n_commits + count;
  void *d_c, *d_p, *d_s, *d_f;
  KZGX_TRY(stage(ctx, 0, n_commits * pb + 16, &d_c));
  KZGX_TRY(stage(ctx, 1, count * pb, &d_p));
  KZGX_TRY(stage(ctx, 2, yb, &d_s));
  KZGX_TRY(stage(ctx, 3, (np + 3 * count) * 4, &d_f));
  // commit flags | proof flags | commit_index | cell_index | ok
  std::vector<uint32_t> fl(np + 2 * count);
  for (size_t k = 0; k < n_commits; k++) fl[k] = commit_inf ? (uint32_t)(commit_inf[k] != 0) : 0u;
  for (size_t k = 0; k < count; k++) {
    fl[n_commits + k] = proof_inf ? (uint32_t)(proof_inf[k] != 0) : 0u;
    fl[np + k] = commit_index[k];
    fl[np + count + k] = cell_index[k];
  }
  hipStream_t st = ctx->c.stream;
  KZGX_TRY_HIP(hipMemcpyAsync(d_c, commits_xy, n_commits * pb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_p, proofs_xy, count * pb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_s, ys, yb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_f, fl.data(), fl.size() * 4, hipMemcpyHostToDevice, st));
  uint32_t* f = (uint32_t*)d_f;
  uint32_t* d_ok = f + np + 2 * count;
  KZGX_TRY(cells_each_device(ctx, d_c, f, n_commits, f + np, f + np + count, d_p, f + n_commits, d_s, count, log2n,
                             log2l, flags, checked, subgroup, d_ok, nullptr));
  std::vector<uint32_t> v(count);
  KZGX_TRY_HIP(hipMemcpyAsync(v.data(), d_ok, count * 4, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  for (size_t k = 0; k < count; k++) ok[k] = v[k] ? 1 : 0;
  return KZGX_OK;
}
}  // namespace

extern "C" {

int kzgx_verify_cells_each_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf, size_t n_commits,
                                  const void* d_commit_index, const void* d_cell_index, const void* d_proofs,
                                  const void* d_proof_inf, const void* d_ys, size_t count, unsigned log2n,
                                  unsigned log2l, int flags, void* d_ok, void* stream) {
  return cells_each_device(ctx, d_commits, d_commit_inf, n_commits, d_commit_index, d_cell_index, d_proofs,
                           d_proof_inf, d_ys, count, log2n, log2l, flags, false, 0, d_ok, stream);
}

int kzgx_verify_cells_each_checked_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf,
                                          size_t n_commits, const void* d_commit_index, const void* d_cell_index,
                                          const void* d_proofs, const void* d_proof_inf, const void* d_ys,
                                          size_t count, unsigned log2n, unsigned log2l, int flags, int subgroup,
                                          void* d_ok, void* stream) {
  return cells_each_device(ctx, d_commits, d_commit_inf, n_commits, d_commit_index, d_cell_index, d_proofs,
                           d_proof_inf, d_ys, count, log2n, log2l, flags, true, subgroup, d_ok, stream);
}

int kzgx_verify_cells_each(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf, size_t n_commits,
                           const uint32_t* commit_index, const uint32_t* cell_index, const uint64_t* proofs_xy,
                           const int* proof_inf, const uint64_t* ys, size_t count, unsigned log2n, unsigned log2l,
                           int flags, int* ok) {
  return cells_each_host(ctx, commits_xy, commit_inf, n_commits, commit_index, cell_index, proofs_xy, proof_inf, ys,
                         count, log2n, log2l, flags, false, 0, ok);
}

int kzgx_verify_cells_each_checked(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf,
                                   size_t n_commits, const uint32_t* commit_index, const uint32_t* cell_index,
                                   const uint64_t* proofs_xy, const int* proof_inf, const uint64_t* ys, size_t count,
                                   unsigned log2n, unsigned log2l, int flags, int subgroup, int* ok) {
  return cells_each_host(ctx, commits_xy, commit_inf, n_commits, commit_index, cell_index, proofs_xy, proof_inf, ys,
                         count, log2n, log2l, flags, true, subgroup, ok);
}

int kzgx_set_verify_cells_chunk(kzgx_ctx* ctx, size_t cells) {
  if (!ctx || cells > 65535) return KZGX_ERR_ARG;
  ctx->cells_chunk = cells;
  return KZGX_OK;
}

}  // extern "C"

// ---- compressed points (codec.hip) ------------------------------------------------------------
namespace {
// uint32 device flags -> the host's int flags (dst may be NULL)
void flags_out(const std::vector<uint32_t>& f, size_t off, size_t count, int* dst) {
  if (!dst) return;
  for (size_t k = 0; k < count; k++) dst[k] = (int)f[off + k];
}

// the host-pointer decompression of either group: records in, limbs | infinity flags | ok flags out
int decompress_host(kzgx_ctx* ctx, bool g2, const uint8_t* bytes, size_t count, int encoding, int subgroup,
                    uint64_t* out_xy, int* out_is_inf, int* ok) {
  KZGX_TRY(activate(ctx));
  const size_t rb = kzgx::point_bytes(ctx->c.curve, g2 ? 2 : 1, encoding);
  if (rb == 0) return KZGX_ERR_ARG;
  if (count == 0) return KZGX_OK;
  if (!bytes || !out_xy || !ok || count > KZGX_MSM_POINTS_MAX) return KZGX_ERR_ARG;
  const size_t pb = (g2 ? 2 : 1) * point_words(ctx) * 4;
  void *d_b, *d_p, *d_f;
  KZGX_TRY(stage(ctx, 0, count * rb, &d_b));
  KZGX_TRY(stage(ctx, 1, count * pb, &d_p));
  KZGX_TRY(stage(ctx, 2, count * 8, &d_f));
  hipStream_t st = ctx->c.stream;
  uint32_t* f = (uint32_t*)d_f;  // infinity flags | ok flags
  KZGX_TRY_HIP(hipMemcpyAsync(d_b, bytes, count * rb, hipMemcpyHostToDevice, st));
  if (g2)
    KZGX_TRY(kzgx::g2_decompress(&ctx->c, (const uint8_t*)d_b, count, subgroup, (uint32_t*)d_p, f, f + count, st));
  else
    KZGX_TRY(kzgx::g1_decompress2(&ctx->c, (const uint8_t*)d_b, count, nullptr, 0, encoding, subgroup,
                                  (uint32_t*)d_p, f, f + count, st));
  std::vector<uint32_t> h(2 * count);
  KZGX_TRY_HIP(hipMemcpyAsync(out_xy, d_p, count * pb, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipMemcpyAsync(h.data(), d_f, count * 8, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  flags_out(h, 0, count, out_is_inf);
  flags_out(h, count, count, ok);
  return KZGX_OK;
}

int compress_host(kzgx_ctx* ctx, bool g2, const uint64_t* xy, const int* is_inf, size_t count, int encoding,
                  uint8_t* out) {
  KZGX_TRY(activate(ctx));
  const size_t rb = kzgx::point_bytes(ctx->c.curve, g2 ? 2 : 1, encoding);
  if (rb == 0) return KZGX_ERR_ARG;
  if (count == 0) return KZGX_OK;
  if (!xy || !out || count > KZGX_MSM_POINTS_MAX) return KZGX_ERR_ARG;
  const size_t pb = (g2 ? 2 : 1) * point_words(ctx) * 4;
  void *d_p, *d_f, *d_b;
  KZGX_TRY(stage(ctx, 0, count * pb, &d_p));
  KZGX_TRY(stage(ctx, 1, count * 4, &d_f));
  KZGX_TRY(stage(ctx, 2, count * rb, &d_b));
  hipStream_t st = ctx->c.stream;
  std::vector<uint32_t> f;
  KZGX_TRY_HIP(hipMemcpyAsync(d_p, xy, count * pb, hipMemcpyHostToDevice, st));
  if (is_inf) {
    f.resize(count);
    for (size_t k = 0; k < count; k++) f[k] = (uint32_t)(is_inf[k] != 0);
    KZGX_TRY_HIP(hipMemcpyAsync(d_f, f.data(), count * 4, hipMemcpyHostToDevice, st));
  }
  const uint32_t* d_inf = is_inf ? (const uint32_t*)d_f : nullptr;
  if (g2)
    KZGX_TRY(kzgx::g2_compress(&ctx->c, (const uint32_t*)d_p, d_inf, count, (uint8_t*)d_b, st));
  else
    KZGX_TRY(kzgx::g1_compress(&ctx->c, (const uint32_t*)d_p, d_inf, count, encoding, (uint8_t*)d_b, st));
  KZGX_TRY_HIP(hipMemcpyAsync(out, d_b, count * rb, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  return KZGX_OK;
}
}  // namespace

extern "C" {

size_t kzgx_point_bytes(int curve, int group, int encoding) { return kzgx::point_bytes(curve, group, encoding); }

int kzgx_g1_decompress_batch(kzgx_ctx* ctx, const uint8_t* bytes, size_t count, int encoding, int subgroup,
                             uint64_t* out_xy, int* out_is_inf, int* ok) {
  return decompress_host(ctx, false, bytes, count, encoding, subgroup, out_xy, out_is_inf, ok);
}

int kzgx_g1_decompress_batch_device(kzgx_ctx* ctx, const void* d_bytes, size_t count, int encoding, int subgroup,
                                    void* d_out_xy, void* d_out_is_inf, void* d_ok, void* d_all_ok, void* stream) {
  KZGX_TRY(activate(ctx));
  if (kzgx::point_bytes(ctx->c.curve, 1, encoding) == 0) return KZGX_ERR_ARG;
  if ((!d_ok && !d_all_ok) || (count > 0 && (!d_bytes || !d_out_xy)) || count > KZGX_MSM_POINTS_MAX)
    return KZGX_ERR_ARG;
  hipStream_t st = pick(ctx, stream);
  if (count == 0) {
    if (d_all_ok) KZGX_TRY_HIP(hipMemsetD32Async((hipDeviceptr_t)d_all_ok, 1, 1, st));
    return KZGX_OK;
  }
  uint32_t* flags = (uint32_t*)d_ok;
  kzgx::WsLease ws = ctx->c.ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  if (!flags) KZGX_TRY(chk_scratch(ctx, ws, count, &flags));
  KZGX_TRY(kzgx::g1_decompress2(&ctx->c, (const uint8_t*)d_bytes, count, nullptr, 0, encoding, subgroup,
                                (uint32_t*)d_out_xy, (uint32_t*)d_out_is_inf, flags, st));
  if (d_all_ok) KZGX_TRY(kzgx::flags_and(flags, count, (uint32_t*)d_all_ok, st));
  return KZGX_OK;
}

int kzgx_g1_compress_batch(kzgx_ctx* ctx, const uint64_t* xy, const int* is_inf, size_t count, int encoding,
                           uint8_t* out) {
  return compress_host(ctx, false, xy, is_inf, count, encoding, out);
}

int kzgx_g1_compress_batch_device(kzgx_ctx* ctx, const void* d_xy, const void* d_is_inf, size_t count, int encoding,
                                  void* d_out, void* stream) {
  KZGX_TRY(activate(ctx));
  if (kzgx::point_bytes(ctx->c.curve, 1, encoding) == 0) return KZGX_ERR_ARG;
  if ((count > 0 && (!d_xy || !d_out)) || count > KZGX_MSM_POINTS_MAX) return KZGX_ERR_ARG;
  return kzgx::g1_compress(&ctx->c, (const uint32_t*)d_xy, (const uint32_t*)d_is_inf, count, encoding,
                           (uint8_t*)d_out, pick(ctx, stream));
}

int kzgx_g2_decompress_batch(kzgx_ctx* ctx, const uint8_t* bytes, size_t count, int subgroup, uint64_t* out_xy,
                             int* out_is_inf, int* ok) {
  return decompress_host(ctx, true, bytes, count, KZGX_ENC_ZCASH, subgroup, out_xy, out_is_inf, ok);
}

int kzgx_g2_compress_batch(kzgx_ctx* ctx, const uint64_t* xy, const int* is_inf, size_t count, uint8_t* out) {
  return compress_host(ctx, true, xy, is_inf, count, KZGX_ENC_ZCASH, out);
}

int kzgx_verify_cells_aggregate_bytes_device(kzgx_ctx* ctx, const void* d_commits_bytes, size_t n_commits,
                                             const void* d_commit_index, const void* d_cell_index,
                                             const void* d_proofs_bytes, const void* d_ys, const void* d_challenges,
                                             size_t count, unsigned log2n, unsigned log2l, int flags, int encoding,
                                             int subgroup, void* d_ok, void* stream) {
  KZGX_TRY(activate(ctx));
  if (kzgx::point_bytes(ctx->c.curve, 1, encoding) == 0) return KZGX_ERR_ARG;
  if (!d_ok || !d_challenges) return KZGX_ERR_ARG;
  if (count > 0 && (!d_commit_index || !d_cell_index || !d_proofs_bytes || !d_ys || (n_commits > 0 && !d_commits_bytes)))
    return KZGX_ERR_ARG;
  CellsShape sh;
  KZGX_TRY(cells_args(ctx, n_commits, count, log2n, log2l, flags, &sh));
  hipStream_t st = pick(ctx, stream);
  if (count == 0) {
    KZGX_TRY_HIP(hipMemsetD32Async((hipDeviceptr_t)d_ok, 1, 1, st));
    return KZGX_OK;
  }
  kzgx::WsLease ws = ctx->c.ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  const size_t np = n_commits + count, pw = point_words(ctx);
  uint32_t* xy;  // the recovered commits | proofs, their infinity flags, their ok flags, the AND
  KZGX_TRY(chk_scratch(ctx, ws, np * pw + 2 * np + 1, &xy));
  uint32_t* inf = xy + np * pw;
  uint32_t* okf = inf + np;
  KZGX_TRY(kzgx::g1_decompress2(&ctx->c, (const uint8_t*)d_commits_bytes, n_commits, (const uint8_t*)d_proofs_bytes,
                                count, encoding, subgroup, xy, inf, okf, st));
  KZGX_TRY(kzgx::flags_and(okf, np, okf + np, st));
  KZGX_TRY(kzgx_verify_cells_aggregate_device(ctx, xy, inf, n_commits, d_commit_index, d_cell_index,
                                              xy + n_commits * pw, inf + n_commits, d_ys, d_challenges, count, log2n,
                                              log2l, flags, d_ok, stream));
  return kzgx::flag_gate((uint32_t*)d_ok, okf + np, st);
}

int kzgx_verify_cells_aggregate_bytes(kzgx_ctx* ctx, const uint8_t* commits_bytes, size_t n_commits,
                                      const uint32_t* commit_index, const uint32_t* cell_index,
                                      const uint8_t* proofs_bytes, const uint64_t* ys, const uint64_t* challenges,
                                      size_t count, unsigned log2n, unsigned log2l, int flags, int encoding,
                                      int subgroup, int* ok) {
  KZGX_TRY(activate(ctx));
  const size_t rb = kzgx::point_bytes(ctx->c.curve, 1, encoding);
  if (rb == 0 || !ok) return KZGX_ERR_ARG;
  if (count > 0 && (!commit_index || !cell_index || !proofs_bytes || !ys || (n_commits > 0 && !commits_bytes)))
    return KZGX_ERR_ARG;
  CellsShape sh;
  KZGX_TRY(cells_args(ctx, n_commits, count, log2n, log2l, flags, &sh));
  if (count == 0) {
    *ok = 1;
    return KZGX_OK;
  }
  for (size_t k = 0; k < count; k++)
    if (commit_index[k] >= n_commits || (cell_index[k] >> sh.kR)) return KZGX_ERR_ARG;
  // library-drawn challenges: independent 128-bit values, r_0 = 1 (as kzgx_verify_cells_aggregate)
  std::vector<uint64_t> drawn;
  if (!challenges) {
    drawn.assign(count * 4, 0);
    std::random_device rd;
    for (size_t k = 0; k < count; k++)
      for (int j = 0; j < 2; j++) drawn[4 * k + j] = ((uint64_t)rd() << 32) | (uint64_t)rd();
    drawn[0] = 1;
    drawn[1] = 0;
    challenges = drawn.data();
  }
  const size_t cb = n_commits * rb, yb = count * sh.l * 32;
  void *d_b, *d_s, *d_f;
  KZGX_TRY(stage(ctx, 0, cb + count * rb, &d_b));  // commit records | proof records
  KZGX_TRY(stage(ctx, 2, yb + count * 32, &d_s));
  KZGX_TRY(stage(ctx, 3, 2 * count * 4 + 16, &d_f));  // commit_index | cell_index | ok
  hipStream_t st = ctx->c.stream;
  if (cb) KZGX_TRY_HIP(hipMemcpyAsync(d_b, commits_bytes, cb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync((char*)d_b + cb, proofs_bytes, count * rb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_s, ys, yb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync((char*)d_s + yb, challenges, count * 32, hipMemcpyHostToDevice, st));
  uint32_t* f = (uint32_t*)d_f;
  KZGX_TRY_HIP(hipMemcpyAsync(f, commit_index, count * 4, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(f + count, cell_index, count * 4, hipMemcpyHostToDevice, st));
  uint32_t* d_ok = f + 2 * count;
  KZGX_TRY(kzgx_verify_cells_aggregate_bytes_device(ctx, d_b, n_commits, f, f + count, (char*)d_b + cb, d_s,
                                                    (char*)d_s + yb, count, log2n, log2l, flags, encoding, subgroup,
                                                    d_ok, nullptr));
  uint32_t v = 0;
  KZGX_TRY_HIP(hipMemcpyAsync(&v, d_ok, 4, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  *ok = v ? 1 : 0;
  return KZGX_OK;
}

}  // extern "C"

// ---- cell recovery ----------------------------------------------------------------------------
namespace {
// the argument checks shared by the four entries (proofs: also the SRS the openings need)
int recover_args(kzgx_ctx* ctx, size_t count, size_t n_blobs, unsigned log2n, unsigned log2l, int flags, bool proofs) {
  const int mx = kzgx::ntt_max_log2(ctx->c.curve);
  if (flags & ~(KZGX_NTT_BITREV | KZGX_PROVE_COSETS_EXTENDED)) return KZGX_ERR_ARG;
  if (!(flags & KZGX_PROVE_COSETS_EXTENDED)) return KZGX_ERR_ARG;  // no redundancy to recover from
  if (mx < 0 || log2n > 31 || log2l > log2n || (int)log2n + 1 > mx) return KZGX_ERR_ARG;
  if (log2n + 1 - log2l > KZGX_RECOVER_MAX_LOG2_CELLS) return KZGX_ERR_ARG;
  if (count > 0xfffffffeu || n_blobs > 0xffffffffu || count > (SIZE_MAX >> 6 >> log2l) ||
      n_blobs > (SIZE_MAX >> 9 >> log2n))
    return KZGX_ERR_ARG;
  if (proofs) {
    size_t n = 0;
    KZGX_TRY(prove_cosets_args(ctx, log2n, log2l, (size_t)-1, flags, &n));
  }
  return KZGX_OK;
}

int recover_device(kzgx_ctx* ctx, const void* d_blob_index, const void* d_cell_index, const void* d_ys, size_t count,
                   size_t n_blobs, unsigned log2n, unsigned log2l, int flags, void* d_out_y, void* d_out_coeffs,
                   bool proofs, void* d_out_proofs_xy, void* d_out_proofs_is_inf, void* d_ok, void* stream) {
  KZGX_TRY(activate(ctx));
  if (n_blobs == 0) return KZGX_OK;
  KZGX_TRY(recover_args(ctx, count, n_blobs, log2n, log2l, flags, proofs));
  if (!d_ok || (count > 0 && (!d_blob_index || !d_cell_index || !d_ys))) return KZGX_ERR_ARG;
  if (proofs ? (!d_out_proofs_xy || !d_out_proofs_is_inf) : (!d_out_y && !d_out_coeffs)) return KZGX_ERR_ARG;
  hipStream_t st = pick(ctx, stream);
  kzgx::WsLease ws = ctx->c.ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  const size_t n = (size_t)1 << log2n, D = 2 * n, R = D >> log2l, pw = point_words(ctx);
  const bool bitrev = (flags & KZGX_NTT_BITREV) != 0;
  // chunks of blobs, so that every workspace of the call is bounded
  const size_t chunk = std::max<size_t>(1, kzgx::RECOVER_CHUNK_SCALARS >> (log2n + 1));
  for (size_t b0 = 0; b0 < n_blobs; b0 += chunk) {
    const size_t cb = std::min(chunk, n_blobs - b0);
    uint32_t* oc = d_out_coeffs ? (uint32_t*)d_out_coeffs + b0 * n * 8 : nullptr;
    KZGX_TRY(kzgx::recover_cells(&ctx->c, *ws, (const uint32_t*)d_blob_index, (const uint32_t*)d_cell_index,
                                 (const uint32_t*)d_ys, count, n_blobs, b0, cb, log2n, log2l, bitrev, proofs,
                                 d_out_y ? (uint32_t*)d_out_y + b0 * D * 8 : nullptr, oc, (uint32_t*)d_ok + b0, st));
    if (proofs)  // the coefficients stay on the device; a failed blob's are zero, its proofs infinity
      KZGX_TRY(kzgx_prove_cosets_batch_device(ctx, oc ? oc : ws->rec_coef, log2n, log2l, cb, n, flags,
                                              (uint32_t*)d_out_proofs_xy + b0 * R * pw,
                                              (uint32_t*)d_out_proofs_is_inf + b0 * R, nullptr, st));
  }
  return KZGX_OK;
}

int recover_host(kzgx_ctx* ctx, const uint32_t* blob_index, const uint32_t* cell_index, const uint64_t* ys,
                 size_t count, size_t n_blobs, unsigned log2n, unsigned log2l, int flags, uint64_t* out_y,
                 uint64_t* out_coeffs, bool proofs, uint64_t* out_proofs_xy, int* out_proofs_is_inf, int* ok) {
  KZGX_TRY(activate(ctx));
  if (n_blobs == 0) return KZGX_OK;
  KZGX_TRY(recover_args(ctx, count, n_blobs, log2n, log2l, flags, proofs));
  if (!ok || (count > 0 && (!blob_index || !cell_index || !ys))) return KZGX_ERR_ARG;
  if (proofs ? (!out_proofs_xy || !out_proofs_is_inf) : (!out_y && !out_coeffs)) return KZGX_ERR_ARG;
  const size_t n = (size_t)1 << log2n, D = 2 * n, R = D >> log2l;
  {  // every index in range, no (blob, cell) twice, at least R / 2 cells per blob
    std::vector<uint8_t> seen(n_blobs * R, 0);
    std::vector<uint32_t> cnt(n_blobs, 0);
    for (size_t k = 0; k < count; k++) {
      if (blob_index[k] >= n_blobs || cell_index[k] >= R) return KZGX_ERR_ARG;
      uint8_t& s = seen[(size_t)blob_index[k] * R + cell_index[k]];
      if (s) return KZGX_ERR_ARG;
      s = 1;
      cnt[blob_index[k]]++;
    }
    for (size_t b = 0; b < n_blobs; b++)
      if (cnt[b] < R / 2) return KZGX_ERR_ARG;
  }
  const size_t yb = (count << log2l) * 32, ib = align256(count * 4), oyb = out_y ? n_blobs * D * 32 : 0,
               ocb = out_coeffs ? n_blobs * n * 32 : 0, pb = proofs ? n_blobs * R * point_words(ctx) * 4 : 0,
               pfb = proofs ? n_blobs * R * 4 : 0;
  void *d_s, *d_i, *d_o, *d_p;
  KZGX_TRY(stage(ctx, 0, yb + 16, &d_s));
  KZGX_TRY(stage(ctx, 1, 2 * ib + n_blobs * 4, &d_i));  // blob_index | cell_index | ok
  KZGX_TRY(stage(ctx, 2, oyb + ocb + 16, &d_o));        // out_y | out_coeffs
  KZGX_TRY(stage(ctx, 3, align256(pb) + pfb + 16, &d_p));
  hipStream_t st = ctx->c.stream;
  KZGX_TRY_HIP(hipMemcpyAsync(d_s, ys, yb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_i, blob_index, count * 4, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync((char*)d_i + ib, cell_index, count * 4, hipMemcpyHostToDevice, st));
  void* d_ok = (char*)d_i + 2 * ib;
  void* d_oy = out_y ? d_o : nullptr;
  void* d_oc = out_coeffs ? (char*)d_o + oyb : nullptr;
  KZGX_TRY(recover_device(ctx, d_i, (char*)d_i + ib, d_s, count, n_blobs, log2n, log2l, flags, d_oy, d_oc, proofs, d_p,
                          (char*)d_p + align256(pb), d_ok, st));
  std::vector<uint32_t> okw(n_blobs), inf(proofs ? n_blobs * R : 0);
  if (out_y) KZGX_TRY_HIP(hipMemcpyAsync(out_y, d_oy, oyb, hipMemcpyDeviceToHost, st));
  if (out_coeffs) KZGX_TRY_HIP(hipMemcpyAsync(out_coeffs, d_oc, ocb, hipMemcpyDeviceToHost, st));
  if (proofs) {
    KZGX_TRY_HIP(hipMemcpyAsync(out_proofs_xy, d_p, pb, hipMemcpyDeviceToHost, st));
    KZGX_TRY_HIP(hipMemcpyAsync(inf.data(), (char*)d_p + align256(pb), pfb, hipMemcpyDeviceToHost, st));
  }
  KZGX_TRY_HIP(hipMemcpyAsync(okw.data(), d_ok, n_blobs * 4, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  for (size_t b = 0; b < n_blobs; b++) ok[b] = okw[b] ? 1 : 0;
  for (size_t i = 0; i < inf.size(); i++) out_proofs_is_inf[i] = (int)inf[i];
  return KZGX_OK;
}
}  // namespace

extern "C" {

int kzgx_recover_cells_device(kzgx_ctx* ctx, const void* d_blob_index, const void* d_cell_index, const void* d_ys,
                              size_t count, size_t n_blobs, unsigned log2n, unsigned log2l, int flags,
                              void* d_out_y, void* d_out_coeffs, void* d_ok, void* stream) {
  return recover_device(ctx, d_blob_index, d_cell_index, d_ys, count, n_blobs, log2n, log2l, flags, d_out_y,
                        d_out_coeffs, false, nullptr, nullptr, d_ok, stream);
}

int kzgx_recover_cells_and_proofs_device(kzgx_ctx* ctx, const void* d_blob_index, const void* d_cell_index,
                                         const void* d_ys, size_t count, size_t n_blobs, unsigned log2n,
                                         unsigned log2l, int flags, void* d_out_y, void* d_out_coeffs,
                                         void* d_out_proofs_xy, void* d_out_proofs_is_inf, void* d_ok,
                                         void* stream) {
  return recover_device(ctx, d_blob_index, d_cell_index, d_ys, count, n_blobs, log2n, log2l, flags, d_out_y,
                        d_out_coeffs, true, d_out_proofs_xy, d_out_proofs_is_inf, d_ok, stream);
}

int kzgx_recover_cells(kzgx_ctx* ctx, const uint32_t* blob_index, const uint32_t* cell_index, const uint64_t* ys,
                       size_t count, size_t n_blobs, unsigned log2n, unsigned log2l, int flags, uint64_t* out_y,
                       uint64_t* out_coeffs, int* ok) {
  return recover_host(ctx, blob_index, cell_index, ys, count, n_blobs, log2n, log2l, flags, out_y, out_coeffs, false,
                      nullptr, nullptr, ok);
}

int kzgx_recover_cells_and_proofs(kzgx_ctx* ctx, const uint32_t* blob_index, const uint32_t* cell_index,
                                  const uint64_t* ys, size_t count, size_t n_blobs, unsigned log2n, unsigned log2l,
                                  int flags, uint64_t* out_y, uint64_t* out_coeffs, uint64_t* out_proofs_xy,
                                  int* out_proofs_is_inf, int* ok) {
  return recover_host(ctx, blob_index, cell_index, ys, count, n_blobs, log2n, log2l, flags, out_y, out_coeffs, true,
                      out_proofs_xy, out_proofs_is_inf, ok);
}

}  // extern "C"

// ---- blob proofs (blob.hip) -------------------------------------------------------------------
namespace {
// the checks every blob entry starts with: the curve, the flag bits, the domain
int blob_args(int curve, unsigned log2n, int flags) {
  if (curve != KZGX_CURVE_BLS12381 || (flags & ~(KZGX_NTT_BITREV | KZGX_BLOB_BYTES))) return KZGX_ERR_ARG;
  return (int)log2n > kzgx::ntt_max_log2(curve) ? KZGX_ERR_ARG : KZGX_OK;
}
// scalar arrays are read and written 16 bytes at a time
bool misaligned16(const void* p) { return ((uintptr_t)p & 15u) != 0; }

// the blob entries' buffer of the workspace slot leased for this call's stream
int blob_scratch(kzgx_ctx* ctx, const kzgx::WsLease& ws, size_t bytes, uint8_t** out) {
  const size_t slot = (size_t)(ws.get() - ctx->c.ws);
  KZGX_TRY(kzgx::dev_alloc(&ctx->c, (void**)&ctx->d_blob[slot], bytes, &ctx->blob_b[slot]));
  *out = (uint8_t*)ctx->d_blob[slot];
  return KZGX_OK;
}

// library-drawn challenges: independent 128-bit values, r_0 = 1 (as kzgx_verify_aggregate)
void draw_challenges(std::vector<uint64_t>& drawn, size_t count) {
  drawn.assign(count * 4, 0);
  std::random_device rd;
  for (size_t k = 0; k < count; k++)
    for (int j = 0; j < 2; j++) drawn[4 * k + j] = ((uint64_t)rd() << 32) | (uint64_t)rd();
  drawn[0] = 1;
  drawn[1] = 0;
}

// What both verify entries start with, in the slot's buffer: z | y | the value kernel's fractions |
// the decoded commitments and proofs | their infinity flags | ok flags of the 2 count records and
// the count blobs
struct BlobFront {
  uint32_t *z, *y, *xy, *inf, *okf;
};
int blob_verify_args(kzgx_ctx* ctx, const void* blobs, unsigned log2n, size_t count, int flags, const void* crec,
                     const void* prec, const void* ok) {
  KZGX_TRY(blob_args(ctx->c.curve, log2n, flags));
  if (!ok || (count > 0 && (!blobs || !crec || !prec))) return KZGX_ERR_ARG;
  if (count > KZGX_MSM_POINTS_MAX / 2 - 1) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0 || ctx->n_srs2 < 2) return KZGX_ERR_NO_SRS;
  return KZGX_OK;
}
int blob_verify_front(kzgx_ctx* ctx, const kzgx::WsLease& ws, hipStream_t st, const void* d_blobs, unsigned log2n,
                      size_t count, int flags, const void* d_crec, const void* d_prec, int subgroup, BlobFront* f) {
  const size_t pw = point_words(ctx);
  uint8_t* buf;
  KZGX_TRY(blob_scratch(ctx, ws, count * (64 + kzgx::EVALS_AT_FRAC_BYTES + 2 * pw * 4 + 8 + 12) + 16, &buf));
  f->z = (uint32_t*)buf;
  f->y = f->z + count * 8;
  uint32_t* frac = f->y + count * 8;
  f->xy = frac + count * (kzgx::EVALS_AT_FRAC_BYTES / 4);
  f->inf = f->xy + 2 * count * pw;
  f->okf = f->inf + 2 * count;
  KZGX_TRY(kzgx::g1_decompress2(&ctx->c, (const uint8_t*)d_crec, count, (const uint8_t*)d_prec, count, KZGX_ENC_ZCASH,
                                subgroup, f->xy, f->inf, f->okf, st));
  KZGX_TRY(kzgx::blob_challenges(&ctx->c, d_blobs, log2n, count, (flags & KZGX_BLOB_BYTES) != 0,
                                 (const uint8_t*)d_crec, f->z, f->okf + 2 * count, st));
  return kzgx::evals_at(&ctx->c, d_blobs, log2n, (size_t)1 << log2n, (flags & KZGX_BLOB_BYTES) != 0,
                        (flags & KZGX_NTT_BITREV) != 0, f->z, count, f->y, frac, st);
}

// the host-pointer verify entries: blobs, records and challenges staged, one answer (each = false) or count
int blob_verify_host(kzgx_ctx* ctx, const void* blobs, unsigned log2n, size_t count, int flags, const uint8_t* crec,
                     const uint8_t* prec, const uint64_t* challenges, int subgroup, bool each, int* ok) {
  KZGX_TRY(activate(ctx));
  KZGX_TRY(blob_verify_args(ctx, blobs, log2n, count, flags, crec, prec, ok));
  if (count == 0) {
    if (!each) *ok = 1;
    return KZGX_OK;
  }
  std::vector<uint64_t> drawn;
  if (!each && !challenges) {
    draw_challenges(drawn, count);
    challenges = drawn.data();
  }
  const size_t bb = count * ((size_t)32 << log2n);
  void *d_b, *d_r, *d_s, *d_f;
  KZGX_TRY(stage(ctx, 0, bb, &d_b));
  KZGX_TRY(stage(ctx, 1, 2 * count * 48, &d_r));  // commit records | proof records
  KZGX_TRY(stage(ctx, 2, count * 32, &d_s));
  KZGX_TRY(stage(ctx, 3, count * 4 + 16, &d_f));
  hipStream_t st = ctx->c.stream;
  KZGX_TRY_HIP(hipMemcpyAsync(d_b, blobs, bb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_r, crec, count * 48, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync((char*)d_r + count * 48, prec, count * 48, hipMemcpyHostToDevice, st));
  std::vector<uint32_t> v(each ? count : 1);
  if (each) {
    KZGX_TRY(kzgx_verify_blobs_each_device(ctx, d_b, log2n, count, flags, d_r, (char*)d_r + count * 48, subgroup, d_f,
                                           nullptr));
  } else {
    KZGX_TRY_HIP(hipMemcpyAsync(d_s, challenges, count * 32, hipMemcpyHostToDevice, st));
    KZGX_TRY(kzgx_verify_blobs_batch_device(ctx, d_b, log2n, count, flags, d_r, (char*)d_r + count * 48, d_s, subgroup,
                                            d_f, nullptr));
  }
  KZGX_TRY_HIP(hipMemcpyAsync(v.data(), d_f, v.size() * 4, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  for (size_t k = 0; k < v.size(); k++) ok[k] = v[k] ? 1 : 0;
  return KZGX_OK;
}
}  // namespace

extern "C" {

int kzgx_sha256(const uint8_t* msg, size_t len, uint8_t out[32]) {
  if (!out || (len > 0 && !msg)) return KZGX_ERR_ARG;
  kzgx::sha256_host(msg, len, out);
  return KZGX_OK;
}

int kzgx_blob_challenge(int curve, const void* blob, unsigned log2n, int flags, const uint8_t* commit_record,
                        uint64_t* z_out, int* ok_out) {
  KZGX_TRY(blob_args(curve, log2n, flags));
  if (!blob || !commit_record || !z_out) return KZGX_ERR_ARG;
  kzgx::blob_challenge_host(blob, log2n, (flags & KZGX_BLOB_BYTES) != 0, commit_record, z_out, ok_out);
  return KZGX_OK;
}

int kzgx_blob_challenges_device(kzgx_ctx* ctx, const void* d_blobs, unsigned log2n, size_t count, int flags,
                                const void* d_commit_records, void* d_z, void* d_ok, void* stream) {
  KZGX_TRY(activate(ctx));
  KZGX_TRY(blob_args(ctx->c.curve, log2n, flags));
  if (count == 0) return KZGX_OK;
  if (!d_blobs || !d_commit_records || !d_z || misaligned16(d_blobs) || misaligned16(d_z)) return KZGX_ERR_ARG;
  return kzgx::blob_challenges(&ctx->c, d_blobs, log2n, count, (flags & KZGX_BLOB_BYTES) != 0,
                               (const uint8_t*)d_commit_records, (uint32_t*)d_z, (uint32_t*)d_ok, pick(ctx, stream));
}

int kzgx_blob_challenges(kzgx_ctx* ctx, const void* blobs, unsigned log2n, size_t count, int flags,
                         const uint8_t* commit_records, uint64_t* z_out, int* ok_out) {
  KZGX_TRY(activate(ctx));
  KZGX_TRY(blob_args(ctx->c.curve, log2n, flags));
  if (count == 0) return KZGX_OK;
  if (!blobs || !commit_records || !z_out || count > 0x7fffffffu) return KZGX_ERR_ARG;
  const size_t bb = count * ((size_t)32 << log2n);
  void *d_b, *d_r, *d_o;
  KZGX_TRY(stage(ctx, 0, bb, &d_b));
  KZGX_TRY(stage(ctx, 1, count * 48, &d_r));
  KZGX_TRY(stage(ctx, 2, count * 36, &d_o));  // z | ok
  hipStream_t st = ctx->c.stream;
  KZGX_TRY_HIP(hipMemcpyAsync(d_b, blobs, bb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_r, commit_records, count * 48, hipMemcpyHostToDevice, st));
  KZGX_TRY(kzgx_blob_challenges_device(ctx, d_b, log2n, count, flags, d_r, d_o, (char*)d_o + count * 32, st));
  std::vector<uint32_t> f(count);
  KZGX_TRY_HIP(hipMemcpyAsync(z_out, d_o, count * 32, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipMemcpyAsync(f.data(), (char*)d_o + count * 32, count * 4, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  flags_out(f, 0, count, ok_out);
  return KZGX_OK;
}

int kzgx_evals_at_batch_device(kzgx_ctx* ctx, const void* d_evals, unsigned log2n, size_t eval_stride,
                               const void* d_z, size_t count, int flags, void* d_y, void* stream) {
  KZGX_TRY(activate(ctx));
  KZGX_TRY(blob_args(ctx->c.curve, log2n, flags));
  if (eval_stride != 0 && eval_stride < ((size_t)1 << log2n)) return KZGX_ERR_ARG;
  if (count == 0) return KZGX_OK;
  if (!d_evals || !d_z || !d_y || misaligned16(d_evals) || misaligned16(d_z) || misaligned16(d_y) ||
      count > 0x7fffffffu)
    return KZGX_ERR_ARG;
  hipStream_t st = pick(ctx, stream);
  kzgx::WsLease ws = ctx->c.ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  uint8_t* frac;
  KZGX_TRY(blob_scratch(ctx, ws, count * kzgx::EVALS_AT_FRAC_BYTES, &frac));
  return kzgx::evals_at(&ctx->c, d_evals, log2n, eval_stride, (flags & KZGX_BLOB_BYTES) != 0,
                        (flags & KZGX_NTT_BITREV) != 0, (const uint32_t*)d_z, count, (uint32_t*)d_y, (uint32_t*)frac,
                        st);
}

int kzgx_evals_at_batch(kzgx_ctx* ctx, const void* evals, unsigned log2n, size_t eval_stride, const uint64_t* zs,
                        size_t count, int flags, uint64_t* ys) {
  KZGX_TRY(activate(ctx));
  KZGX_TRY(blob_args(ctx->c.curve, log2n, flags));
  const size_t n = (size_t)1 << log2n;
  if (eval_stride != 0 && eval_stride < n) return KZGX_ERR_ARG;
  if (count == 0) return KZGX_OK;
  if (!evals || !zs || !ys || count > 0x7fffffffu) return KZGX_ERR_ARG;
  const size_t eb = ((count - 1) * eval_stride + n) * 32;
  void *d_e, *d_s;
  KZGX_TRY(stage(ctx, 0, eb, &d_e));
  KZGX_TRY(stage(ctx, 1, count * 64, &d_s));  // z | y
  hipStream_t st = ctx->c.stream;
  KZGX_TRY_HIP(hipMemcpyAsync(d_e, evals, eb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_s, zs, count * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY(kzgx_evals_at_batch_device(ctx, d_e, log2n, eval_stride, d_s, count, flags, (char*)d_s + count * 32, st));
  KZGX_TRY_HIP(hipMemcpyAsync(ys, (char*)d_s + count * 32, count * 32, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  return KZGX_OK;
}

int kzgx_prove_blobs_batch_device(kzgx_ctx* ctx, const void* d_blobs, unsigned log2n, size_t count, int flags,
                                  void* d_commit_records, void* d_proof_records, void* d_z, void* d_y, void* d_ok,
                                  void* stream) {
  KZGX_TRY(activate(ctx));
  KZGX_TRY(blob_args(ctx->c.curve, log2n, flags));
  if (count == 0) return KZGX_OK;
  if (!d_blobs || !d_commit_records || !d_proof_records || misaligned16(d_blobs) || misaligned16(d_z) ||
      misaligned16(d_y) || count > 65535)
    return KZGX_ERR_ARG;
  const size_t n = (size_t)1 << log2n;
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  if (n > ctx->c.n_srs) return KZGX_ERR_DEGREE;
  hipStream_t st = pick(ctx, stream);
  kzgx::Ctx* c = &ctx->c;
  kzgx::WsLease ws = c->ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  const bool bytes = (flags & KZGX_BLOB_BYTES) != 0;
  const int nflags = flags & KZGX_NTT_BITREV;
  const size_t per = std::min(count, std::max<size_t>(1, kzgx::BLOB_CHUNK_SCALARS >> log2n)), pw = point_words(ctx);
  // a chunk's decoded limbs | its y | its points | their infinity flags | every blob's z | every blob's ok flag
  const size_t o_y = bytes ? per * n * 32 : 0, o_p = o_y + per * 32, o_i = o_p + per * pw * 4, o_z = o_i + per * 16,
               o_k = o_z + count * 32;
  uint8_t* buf;
  KZGX_TRY(blob_scratch(ctx, ws, o_k + count * 4, &buf));
  uint32_t* pts = (uint32_t*)(buf + o_p);
  uint32_t* inf = (uint32_t*)(buf + o_i);
  uint32_t* z = d_z ? (uint32_t*)d_z : (uint32_t*)(buf + o_z);
  uint32_t* okf = d_ok ? (uint32_t*)d_ok : (uint32_t*)(buf + o_k);
  // Two passes over the chunks with ONE challenge launch between them: the hash is a serial chain per lane
  // that takes as long for one blob as for thousands, so it is paid once per call, not once per chunk.
  // A call of several chunks decodes each chunk twice (a pass over its bytes) to keep the workspace bounded.
  for (int pass = 0; pass < 2; pass++) {
    for (size_t b0 = 0; b0 < count; b0 += per) {
      const size_t cb = std::min(per, count - b0);
      const uint8_t* src = (const uint8_t*)d_blobs + b0 * n * 32;
      const void* evals = src;
      if (bytes) {  // an invalid blob decodes to the zero polynomial: both records the identity
        if (pass == 0 || count > per) KZGX_TRY(kzgx::blob_decode(c, src, log2n, cb, (uint32_t*)buf, okf + b0, st));
        evals = buf;
      }
      uint8_t* rec = (uint8_t*)(pass == 0 ? d_commit_records : d_proof_records) + b0 * 48;
      if (pass == 0) {
        KZGX_TRY(kzgx_commit_evals_batch_device(ctx, evals, log2n, cb, n, nflags, pts, inf, st));
      } else {
        uint32_t* yp = d_y ? (uint32_t*)d_y + b0 * 8 : (uint32_t*)(buf + o_y);
        KZGX_TRY(kzgx_prove_evals_batch_device(ctx, evals, log2n, n, z + b0 * 8, cb, nflags, pts, inf, yp, st));
      }
      KZGX_TRY(kzgx::g1_compress(c, pts, inf, cb, KZGX_ENC_ZCASH, rec, st));
    }
    if (pass == 0)
      KZGX_TRY(kzgx::blob_challenges(c, d_blobs, log2n, count, bytes, (const uint8_t*)d_commit_records, z, okf, st));
  }
  return KZGX_OK;
}

int kzgx_prove_blobs_batch(kzgx_ctx* ctx, const void* blobs, unsigned log2n, size_t count, int flags,
                           uint8_t* commit_records, uint8_t* proof_records, uint64_t* z_out, uint64_t* y_out) {
  KZGX_TRY(activate(ctx));
  KZGX_TRY(blob_args(ctx->c.curve, log2n, flags));
  if (count == 0) return KZGX_OK;
  if (!blobs || !commit_records || !proof_records || count > 65535) return KZGX_ERR_ARG;
  const size_t bb = count * ((size_t)32 << log2n);
  const size_t o_p = count * 48, o_z = align256(2 * count * 48), o_y = o_z + count * 32, o_k = o_y + count * 32;
  void *d_b, *d_o;
  KZGX_TRY(stage(ctx, 0, bb, &d_b));
  KZGX_TRY(stage(ctx, 1, o_k + count * 4, &d_o));
  hipStream_t st = ctx->c.stream;
  char* o = (char*)d_o;
  KZGX_TRY_HIP(hipMemcpyAsync(d_b, blobs, bb, hipMemcpyHostToDevice, st));
  KZGX_TRY(kzgx_prove_blobs_batch_device(ctx, d_b, log2n, count, flags, o, o + o_p, o + o_z, o + o_y, o + o_k, st));
  std::vector<uint32_t> f(count);
  KZGX_TRY_HIP(hipMemcpyAsync(commit_records, o, count * 48, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipMemcpyAsync(proof_records, o + o_p, count * 48, hipMemcpyDeviceToHost, st));
  if (z_out) KZGX_TRY_HIP(hipMemcpyAsync(z_out, o + o_z, count * 32, hipMemcpyDeviceToHost, st));
  if (y_out) KZGX_TRY_HIP(hipMemcpyAsync(y_out, o + o_y, count * 32, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipMemcpyAsync(f.data(), o + o_k, count * 4, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  for (size_t b = 0; b < count; b++)
    if (!f[b]) return KZGX_ERR_ARG;  // an element >= r
  return KZGX_OK;
}

int kzgx_verify_blobs_batch_device(kzgx_ctx* ctx, const void* d_blobs, unsigned log2n, size_t count, int flags,
                                   const void* d_commit_records, const void* d_proof_records,
                                   const void* d_challenges, int subgroup, void* d_ok, void* stream) {
  KZGX_TRY(activate(ctx));
  KZGX_TRY(blob_verify_args(ctx, d_blobs, log2n, count, flags, d_commit_records, d_proof_records, d_ok));
  if (!d_challenges || misaligned16(d_blobs)) return KZGX_ERR_ARG;
  hipStream_t st = pick(ctx, stream);
  if (count == 0) {
    KZGX_TRY_HIP(hipMemsetD32Async((hipDeviceptr_t)d_ok, 1, 1, st));
    return KZGX_OK;
  }
  kzgx::WsLease ws = ctx->c.ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  BlobFront f;
  KZGX_TRY(blob_verify_front(ctx, ws, st, d_blobs, log2n, count, flags, d_commit_records, d_proof_records, subgroup,
                             &f));
  uint32_t* all = f.okf + 3 * count;  // every record decodes and every blob is canonical
  KZGX_TRY(kzgx::flags_and(f.okf, 3 * count, all, st));
  const size_t pw = point_words(ctx);
  KZGX_TRY(kzgx_verify_aggregate_device(ctx, f.xy, f.inf, f.xy + count * pw, f.inf + count, f.z, f.y, d_challenges,
                                        count, d_ok, stream));
  return kzgx::flag_gate((uint32_t*)d_ok, all, st);
}

int kzgx_verify_blobs_each_device(kzgx_ctx* ctx, const void* d_blobs, unsigned log2n, size_t count, int flags,
                                  const void* d_commit_records, const void* d_proof_records, int subgroup,
                                  void* d_ok, void* stream) {
  KZGX_TRY(activate(ctx));
  KZGX_TRY(blob_verify_args(ctx, d_blobs, log2n, count, flags, d_commit_records, d_proof_records, d_ok));
  if (misaligned16(d_blobs)) return KZGX_ERR_ARG;
  if (count == 0) return KZGX_OK;
  hipStream_t st = pick(ctx, stream);
  kzgx::WsLease ws = ctx->c.ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  BlobFront f;
  KZGX_TRY(blob_verify_front(ctx, ws, st, d_blobs, log2n, count, flags, d_commit_records, d_proof_records, subgroup,
                             &f));
  const size_t pw = point_words(ctx);
  KZGX_TRY(kzgx_verify_single_batch_device(ctx, f.xy, f.inf, f.xy + count * pw, f.inf + count, f.z, f.y, count, d_ok,
                                           stream));
  // a blob's own records and elements gate its verdict, nobody else's
  return kzgx::blob_gate((uint32_t*)d_ok, f.okf, f.okf + count, f.okf + 2 * count, count, st);
}

int kzgx_verify_blobs_batch(kzgx_ctx* ctx, const void* blobs, unsigned log2n, size_t count, int flags,
                            const uint8_t* commit_records, const uint8_t* proof_records, const uint64_t* challenges,
                            int subgroup, int* ok) {
  return blob_verify_host(ctx, blobs, log2n, count, flags, commit_records, proof_records, challenges, subgroup, false,
                          ok);
}

int kzgx_verify_blobs_each(kzgx_ctx* ctx, const void* blobs, unsigned log2n, size_t count, int flags,
                           const uint8_t* commit_records, const uint8_t* proof_records, int subgroup, int* ok) {
  return blob_verify_host(ctx, blobs, log2n, count, flags, commit_records, proof_records, nullptr, subgroup, true, ok);
}

}  // extern "C"

/* ---- setup ceremony -------------------------------------------------------------- */
namespace {
// v < r for a canonical 4 x 64-bit scalar; zero passes only with allow_zero
bool fr_in_range(int curve, const uint64_t* v, bool allow_zero) {
  const uint32_t* p = curve == KZGX_CURVE_BN254 ? kzgx::BN254Fr::P : kzgx::BLS12381Fr::P;
  if ((v[0] | v[1] | v[2] | v[3]) == 0) return allow_zero;
  for (int i = 3; i >= 0; i--) {
    const uint64_t r = (uint64_t)p[2 * i] | ((uint64_t)p[2 * i + 1] << 32);
    if (v[i] != r) return v[i] < r;
  }
  return false;  // v == r
}

bool all_zero(const uint8_t* p, size_t bytes) {
  return std::all_of(p, p + bytes, [](uint8_t b) { return b == 0; });
}
}  // namespace

extern "C" {

int kzgx_srs_update(kzgx_ctx* ctx, const uint64_t* s, size_t g1_start, size_t g2_start, uint64_t* witness_g2_xy) {
  KZGX_TRY(activate(ctx));
  if (!s || !fr_in_range(ctx->c.curve, s, false)) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  const size_t n = ctx->c.n_srs, m = ctx->n_srs2;
  if (n > 0x7fffffffu || m > 0x7fffffffu) return KZGX_ERR_ARG;
  hipStream_t st = ctx->c.stream;
  const int curve = ctx->c.curve;
  const size_t p1 = point_words(ctx) * 4, p2 = 2 * p1;
  // one staging block: s | witness
  void* d_blk;
  KZGX_TRY(stage(ctx, 0, 32 + p2, &d_blk));
  uint32_t* d_s = (uint32_t*)d_blk;
  uint32_t* d_wit = d_s + 8;
  // both halves go into fresh buffers and are installed together below: a
  // failure up to there leaves the old setup whole
  struct Fresh {
    uint32_t *g1 = nullptr, *g2 = nullptr;
    ~Fresh() {
      if (g1) (void)hipFree(g1);
      if (g2) (void)hipFree(g2);
    }
  } fresh;
  KZGX_TRY_HIP(hipMalloc((void**)&fresh.g1, n * p1));
  if (m) KZGX_TRY_HIP(hipMalloc((void**)&fresh.g2, m * p2));
  KZGX_TRY_HIP(hipMemcpyAsync(d_s, s, 32, hipMemcpyHostToDevice, st));
  // the G2 half (a few latency-bound waves; the witness [s] G2gen is one more
  // lane of its launch) forks onto the side stream, as verify_proof's does,
  // and runs beside the G1 half
  KZGX_TRY(side_ready(ctx));
  hipStream_t sd = ctx->side;
  KZGX_TRY_HIP(hipEventRecord(ctx->ev_fork, st));
  KZGX_TRY_HIP(hipStreamWaitEvent(sd, ctx->ev_fork, 0));
  const int rg2 = kzgx::srs_update_g2(curve, d_s, g2_start, m, ctx->d_srs2_canon, fresh.g2,
                                      witness_g2_xy ? d_wit : nullptr, sd);
  // (joined before any return below: the side work reads s and writes the fresh buffers)
  const hipError_t jr = hipEventRecord(ctx->ev_join, sd);
  if (rg2 != KZGX_OK || jr != hipSuccess) {
    (void)hipStreamSynchronize(sd);
    return rg2 != KZGX_OK ? rg2 : kzgx::hip_fail(jr);
  }
  const int rg1 = kzgx::srs_update_g1(curve, d_s, g1_start, n, ctx->d_srs_canon, fresh.g1, st);
  KZGX_TRY_HIP(hipStreamWaitEvent(st, ctx->ev_join, 0));
  if (rg1 != KZGX_OK) {
    (void)hipStreamSynchronize(st);
    return rg1;
  }
  if (witness_g2_xy) KZGX_TRY_HIP(hipMemcpyAsync(witness_g2_xy, d_wit, p2, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipMemsetAsync(d_s, 0, 32, st));  // the staged copy of the secret
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  // install, as kzgx_load_srs_g1 + kzgx_load_srs_g2 of the new points: every
  // derived table and cached setup is stale.  srs_upload releases this
  // context's reference to a shared default table and attaches to (or
  // builds) the table of the new points; a table other contexts hold is
  // never written.  hipFree waits for work that may still read the old points.
  ctx->vw_ready = false;
  cells_g2_drop(ctx);
  kzgx::prove_all_drop(&ctx->c);
  ctx->g2tab_n = 0;
  std::swap(ctx->d_srs_canon, fresh.g1);
  ctx->srs_canon_b = n * p1;
  if (m) {
    std::swap(ctx->d_srs2_canon, fresh.g2);
    ctx->srs2_canon_b = m * p2;
  }
  KZGX_TRY(kzgx::srs_upload(&ctx->c, ctx->d_srs_canon, n));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  return setup_finish(ctx);
}

int kzgx_srs_verify_structure(kzgx_ctx* ctx, const uint64_t* rho, const uint64_t* sigma, int flags, int* g1_ok,
                              int* g2_ok) {
  KZGX_TRY(activate(ctx));
  if (!g1_ok || !g2_ok || (flags & ~KZGX_SRS_STRUCT_GENERATORS)) return KZGX_ERR_ARG;
  const int curve = ctx->c.curve;
  if ((rho && !fr_in_range(curve, rho, true)) || (sigma && !fr_in_range(curve, sigma, true))) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0 || ctx->n_srs2 < 2) return KZGX_ERR_NO_SRS;
  const size_t n = ctx->c.n_srs, m = ctx->n_srs2;
  if (n > 0x7fffffffu || m > ((size_t)1 << 24)) return KZGX_ERR_ARG;  // (the G2 MSM's limit)
  // library-drawn challenges: independent 128-bit values
  uint64_t ch[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::random_device rd;
  for (int k = 0; k < 2; k++) {
    const uint64_t* given = k == 0 ? rho : sigma;
    for (int j = 0; j < 4; j++) ch[4 * k + j] = given ? given[j] : j < 2 ? ((uint64_t)rd() << 32) | (uint64_t)rd() : 0;
  }
  hipStream_t st = ctx->c.stream;
  const size_t p1 = point_words(ctx) * 4, p2 = 2 * p1, fb = 6 * p1;
  // the scalar rows (stage 0; the G2 rows reuse the G1 rows' place) and one
  // small block (stage 1):
  //   rho | sigma | generators | G1: A, B, P_1, P_0 | G2: Q_1, Q_0, A2, B2 | infinity flags | 4 Fp12
  const size_t o_gen = 64, o_g1 = o_gen + p1 + p2, o_g2 = o_g1 + 4 * p1, o_fl = o_g2 + 4 * p2, o_out = o_fl + 32,
               blk_b = o_out + 4 * fb;
  void *d_rows, *d_blk;
  KZGX_TRY(stage(ctx, 0, std::max(n, m) * 64, &d_rows));
  KZGX_TRY(stage(ctx, 1, blk_b, &d_blk));
  char* blk = (char*)d_blk;
  uint32_t* d_fl = (uint32_t*)(blk + o_fl);
  KZGX_TRY_HIP(hipMemsetAsync(blk + o_g1, 0, o_out - o_g1, st));
  KZGX_TRY_HIP(hipMemcpyAsync(blk, ch, 64, hipMemcpyHostToDevice, st));
  KZGX_TRY(kzgx::curve_generators(curve, (uint32_t*)(blk + o_gen), st));
  // G1: A = sum rho^i P_i and B = sum rho^i P_(i+1), one batch of two MSMs over the installed SRS
  if (n >= 2) {
    uint32_t* row0 = (uint32_t*)d_rows;
    KZGX_TRY(kzgx::fr_powers(curve, (const uint32_t*)blk, n - 1, row0, row0 + n * 8, st));
    KZGX_TRY(kzgx_msm_g1_batch_device(ctx, row0, n, 2, n, blk + o_g1, d_fl, nullptr));
    KZGX_TRY_HIP(hipMemcpyAsync(blk + o_g1 + 2 * p1, (const char*)ctx->d_srs_canon + p1, p1, hipMemcpyDeviceToDevice,
                                st));
  }
  KZGX_TRY_HIP(hipMemcpyAsync(blk + o_g1 + 3 * p1, ctx->d_srs_canon, p1, hipMemcpyDeviceToDevice, st));
  // G2: A2 = sum sigma^j Q_j and B2 = sum sigma^j Q_(j+1), the same two rows through the G2 MSM
  {
    uint32_t* row0 = (uint32_t*)d_rows;
    KZGX_TRY(kzgx::fr_powers(curve, (const uint32_t*)(blk + 32), m - 1, row0, row0 + m * 8, st));
    const uint32_t* tab = g2_table(ctx, m, st);
    KZGX_TRY(kzgx::msm_g2(&ctx->c, row0, ctx->d_srs2_canon, m, (uint32_t*)(blk + o_g2 + 2 * p2), d_fl + 6, st, tab));
    KZGX_TRY(kzgx::msm_g2(&ctx->c, row0 + m * 8, ctx->d_srs2_canon, m, (uint32_t*)(blk + o_g2 + 3 * p2), d_fl + 7, st,
                          tab));
    KZGX_TRY_HIP(hipMemcpyAsync(blk + o_g2, (const char*)ctx->d_srs2_canon + p2, p2, hipMemcpyDeviceToDevice, st));
    KZGX_TRY_HIP(hipMemcpyAsync(blk + o_g2 + p2, ctx->d_srs2_canon, p2, hipMemcpyDeviceToDevice, st));
  }
  // e(A, Q_1), e(B, Q_0), e(P_1, A2), e(P_0, B2): the pairing value is unique, so words compare
  KZGX_TRY(kzgx::pairing_batch(&ctx->c, (const uint32_t*)(blk + o_g1), d_fl, (const uint32_t*)(blk + o_g2), d_fl + 4, 4,
                               (uint32_t*)(blk + o_out), st));
  std::vector<uint8_t> h(blk_b);
  KZGX_TRY_HIP(hipMemcpyAsync(h.data() + o_gen, blk + o_gen, blk_b - o_gen, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  const uint8_t *P1 = h.data() + o_g1 + 2 * p1, *P0 = h.data() + o_g1 + 3 * p1, *Q0 = h.data() + o_g2 + p2;
  const uint8_t* out = h.data() + o_out;
  bool ok1 = std::memcmp(out, out + fb, fb) == 0 && !all_zero(P0, p1) && (n < 2 || !all_zero(P1, p1));
  // n = 1: there is no P_1 to test the G2 powers against
  bool ok2 = n >= 2 && std::memcmp(out + 2 * fb, out + 3 * fb, fb) == 0 && !all_zero(Q0, p2);
  if (flags & KZGX_SRS_STRUCT_GENERATORS) {
    const bool gens = std::memcmp(P0, h.data() + o_gen, p1) == 0 && std::memcmp(Q0, h.data() + o_gen + p1, p2) == 0;
    ok1 = ok1 && gens;
    ok2 = ok2 && gens;
  }
  *g1_ok = ok1 ? 1 : 0;
  *g2_ok = ok2 ? 1 : 0;
  return KZGX_OK;
}

int kzgx_srs_verify_update(kzgx_ctx* ctx, const uint64_t* prev_tau_g1_xy, const uint64_t* new_tau_g1_xy,
                           const uint64_t* witness_g2_xy, int* ok) {
  KZGX_TRY(activate(ctx));
  if (!prev_tau_g1_xy || !new_tau_g1_xy || !witness_g2_xy || !ok) return KZGX_ERR_ARG;
  hipStream_t st = ctx->c.stream;
  const size_t p1 = point_words(ctx) * 4, p2 = 2 * p1, fb = 6 * p1;
  // generators (G1, then G2) | G1: new, prev | G2: G2gen, W | 2 Fp12
  const size_t o_g1 = p1 + p2, o_g2 = o_g1 + 2 * p1, o_out = o_g2 + 2 * p2;
  void* d_blk;
  KZGX_TRY(stage(ctx, 1, o_out + 2 * fb, &d_blk));
  char* blk = (char*)d_blk;
  KZGX_TRY(kzgx::curve_generators(ctx->c.curve, (uint32_t*)blk, st));
  KZGX_TRY_HIP(hipMemcpyAsync(blk + o_g1, new_tau_g1_xy, p1, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(blk + o_g1 + p1, prev_tau_g1_xy, p1, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(blk + o_g2, blk + p1, p2, hipMemcpyDeviceToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(blk + o_g2 + p2, witness_g2_xy, p2, hipMemcpyHostToDevice, st));
  KZGX_TRY(kzgx::pairing_batch(&ctx->c, (const uint32_t*)(blk + o_g1), nullptr, (const uint32_t*)(blk + o_g2), nullptr, 2,
                               (uint32_t*)(blk + o_out), st));
  std::vector<uint8_t> out(2 * fb);
  KZGX_TRY_HIP(hipMemcpyAsync(out.data(), blk + o_out, 2 * fb, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  *ok = std::memcmp(out.data(), out.data() + fb, fb) == 0 && !all_zero((const uint8_t*)witness_g2_xy, p2) &&
                !all_zero((const uint8_t*)new_tau_g1_xy, p1)
            ? 1
            : 0;
  return KZGX_OK;
}

}  // extern "C"

// ---- batch openings: many polynomials at shared points, one proof each (multi_open.hip) ----------
namespace {
// the batch openings' buffer of the workspace slot leased for this call's stream
int multi_scratch(kzgx_ctx* ctx, const kzgx::WsLease& ws, size_t bytes, uint32_t** out) {
  const size_t slot = (size_t)(ws.get() - ctx->c.ws);
  KZGX_TRY(kzgx::dev_alloc(&ctx->c, (void**)&ctx->d_multi[slot], bytes, &ctx->multi_b[slot]));
  *out = ctx->d_multi[slot];
  return KZGX_OK;
}

// what the host can see of a call's shape, both sides (n_index: polynomials or commitments)
bool multi_shape_ok(size_t n_index, size_t n_groups, size_t count, int flags) {
  return (flags & ~KZGX_MULTI_WEIGHT_POWERS) == 0 && n_index <= 0xffffffffu && n_groups <= 0x7fffffffu &&
         count <= 0x7fffffffu && (n_groups > 0 || count == 0);
}

// the host entries' structure check: group_start non-decreasing from 0 to count, every index in range
bool multi_structure_ok(const uint32_t* index, size_t n_index, const uint32_t* group_start, size_t n_groups,
                        size_t count) {
  if (group_start[0] != 0 || group_start[n_groups] != count) return false;
  for (size_t g = 0; g < n_groups; g++)
    if (group_start[g] > group_start[g + 1]) return false;
  for (size_t k = 0; k < count; k++)
    if (index[k] >= n_index) return false;
  return true;
}

bool multi_canonical(int curve, const uint64_t* v, size_t m) {
  for (size_t i = 0; i < m; i++)
    if (!fr_in_range(curve, v + 4 * i, true)) return false;
  return true;
}

size_t align32(size_t b) { return (b + 31) & ~(size_t)31; }
}  // namespace

extern "C" {

int kzgx_set_multi_chunk(kzgx_ctx* ctx, size_t scalars) {
  if (!ctx) return KZGX_ERR_ARG;
  ctx->multi_chunk = scalars;
  return KZGX_OK;
}

int kzgx_prove_multi_batch_device(kzgx_ctx* ctx, const void* d_coeffs, size_t n, size_t coeff_stride, size_t n_polys,
                                  const void* d_poly_index, const void* d_group_start, size_t n_groups,
                                  const void* d_zs, const void* d_weights, size_t count, int flags, void* d_out_xy,
                                  void* d_out_is_inf, void* d_out_y, void* d_out_Y, void* d_ok, void* stream) {
  KZGX_TRY(activate(ctx));
  if (!multi_shape_ok(n_polys, n_groups, count, flags) || n == 0 || n > 0xffffffffu || coeff_stride < n)
    return KZGX_ERR_ARG;
  if (n_groups > 0 && (!d_coeffs || !d_group_start || !d_zs || !d_weights || !d_out_xy || !d_out_is_inf ||
                       (count > 0 && !d_poly_index)))
    return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  if (n - 1 > ctx->c.n_srs) return KZGX_ERR_DEGREE;
  hipStream_t st = pick(ctx, stream);
  if (n_groups == 0) {
    if (d_ok) KZGX_TRY_HIP(hipMemsetD32Async((hipDeviceptr_t)d_ok, 1, 1, st));
    return KZGX_OK;
  }
  kzgx::Ctx* c = &ctx->c;
  kzgx::WsLease ws = c->ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  const bool powers = (flags & KZGX_MULTI_WEIGHT_POWERS) != 0;
  const size_t chunk = ctx->multi_chunk ? ctx->multi_chunk : kzgx::MULTI_CHUNK_SCALARS;
  // groups per chunk (65535: the prove path's batch limit); claims per evaluation batch
  const size_t cg = std::min<size_t>({std::max<size_t>(1, chunk / n), 65535, n_groups});
  const uint32_t slice = kzgx::MULTI_EVAL_SLICE;
  const size_t nsl = n > slice ? (n + slice - 1) / slice : 0;
  const bool want_y = d_out_y && count > 0;
  const size_t ek = !want_y ? 0 : nsl ? std::min(std::max<size_t>(1, chunk / nsl), count) : count;
  const size_t part_sc = want_y ? kzgx::multi_eval_part_scalars(ek, n, slice) : 0;
  uint32_t* F;
  KZGX_TRY(multi_scratch(ctx, ws, (cg * n + part_sc) * 32, &F));
  uint32_t* part = F + cg * n * 8;
  const uint32_t* gs = (const uint32_t*)d_group_start;
  const uint32_t* pidx = (const uint32_t*)d_poly_index;
  if (d_ok) KZGX_TRY(kzgx::multi_check(c, pidx, n_polys, gs, n_groups, count, (uint32_t*)d_ok, st));
  const size_t pb = point_words(ctx) * 4;
  for (size_t g0 = 0; g0 < n_groups; g0 += cg) {
    const size_t ng = std::min(cg, n_groups - g0);
    KZGX_TRY(kzgx::multi_fold(c, (const uint32_t*)d_coeffs, n, coeff_stride * 8, n_polys, pidx, gs, g0, ng, count,
                              (const uint32_t*)d_weights, powers, F, st));
    KZGX_TRY(kzgx_prove_single_batch_device(ctx, F, n, n, (const char*)d_zs + g0 * 32, ng, (char*)d_out_xy + g0 * pb,
                                            (char*)d_out_is_inf + g0 * 4,
                                            d_out_Y ? (char*)d_out_Y + g0 * 32 : nullptr, st));
  }
  for (size_t k0 = 0; want_y && k0 < count; k0 += ek)
    KZGX_TRY(kzgx::multi_eval(c, (const uint32_t*)d_coeffs, n, coeff_stride * 8, n_polys, pidx, gs, n_groups,
                              (const uint32_t*)d_zs, k0, std::min(ek, count - k0), (uint32_t*)d_out_y, part, slice,
                              st));
  return KZGX_OK;
}

int kzgx_prove_multi_batch(kzgx_ctx* ctx, const uint64_t* coeffs, size_t n, size_t coeff_stride, size_t n_polys,
                           const uint32_t* poly_index, const uint32_t* group_start, size_t n_groups,
                           const uint64_t* zs, const uint64_t* weights, size_t count, int flags, uint64_t* out_xy,
                           int* out_is_inf, uint64_t* out_y, uint64_t* out_Y) {
  KZGX_TRY(activate(ctx));
  if (!multi_shape_ok(n_polys, n_groups, count, flags) || n == 0 || n > 0xffffffffu || coeff_stride < n)
    return KZGX_ERR_ARG;
  const size_t nw = (flags & KZGX_MULTI_WEIGHT_POWERS) ? n_groups : count;
  if (n_groups > 0) {
    if (!group_start || !zs || !weights || !out_xy || !out_is_inf || (count > 0 && !poly_index) ||
        (n_polys > 0 && !coeffs))
      return KZGX_ERR_ARG;
    if (!multi_structure_ok(poly_index, n_polys, group_start, n_groups, count) ||
        !multi_canonical(ctx->c.curve, zs, n_groups) || !multi_canonical(ctx->c.curve, weights, nw))
      return KZGX_ERR_ARG;
  }
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  if (n - 1 > ctx->c.n_srs) return KZGX_ERR_DEGREE;
  if (n_groups == 0) return KZGX_OK;
  const size_t pb = point_words(ctx) * 4;
  const size_t cb = n_polys ? ((n_polys - 1) * coeff_stride + n) * 32 : 32;
  // inputs: z | weights | poly_index | group_start; outputs: proofs | y | Y | flags
  const size_t i_w = n_groups * 32, i_p = i_w + nw * 32, i_g = i_p + align32(count * 4),
               i_end = i_g + (n_groups + 1) * 4;
  const size_t o_y = align32(n_groups * pb), o_Y = o_y + count * 32, o_f = o_Y + n_groups * 32,
               o_end = o_f + n_groups * 4;
  void *d_c, *d_i, *d_o;
  KZGX_TRY(stage(ctx, 0, cb, &d_c));
  KZGX_TRY(stage(ctx, 1, i_end, &d_i));
  KZGX_TRY(stage(ctx, 2, o_end, &d_o));
  hipStream_t st = ctx->c.stream;
  char *in = (char*)d_i, *out = (char*)d_o;
  if (n_polys) KZGX_TRY_HIP(hipMemcpyAsync(d_c, coeffs, cb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(in, zs, n_groups * 32, hipMemcpyHostToDevice, st));
  if (nw) KZGX_TRY_HIP(hipMemcpyAsync(in + i_w, weights, nw * 32, hipMemcpyHostToDevice, st));
  if (count) KZGX_TRY_HIP(hipMemcpyAsync(in + i_p, poly_index, count * 4, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(in + i_g, group_start, (n_groups + 1) * 4, hipMemcpyHostToDevice, st));
  KZGX_TRY(kzgx_prove_multi_batch_device(ctx, d_c, n, coeff_stride, n_polys, in + i_p, in + i_g, n_groups, in,
                                         in + i_w, count, flags, out, out + o_f, out_y ? out + o_y : nullptr,
                                         out_Y ? out + o_Y : nullptr, nullptr, nullptr));
  std::vector<uint32_t> inf(n_groups);
  KZGX_TRY_HIP(hipMemcpyAsync(out_xy, out, n_groups * pb, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipMemcpyAsync(inf.data(), out + o_f, n_groups * 4, hipMemcpyDeviceToHost, st));
  if (out_y && count) KZGX_TRY_HIP(hipMemcpyAsync(out_y, out + o_y, count * 32, hipMemcpyDeviceToHost, st));
  if (out_Y) KZGX_TRY_HIP(hipMemcpyAsync(out_Y, out + o_Y, n_groups * 32, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  for (size_t g = 0; g < n_groups; g++) out_is_inf[g] = (int)inf[g];
  return KZGX_OK;
}

}  // extern "C"

namespace {
// the device verify, with the point checks in front when checked
int verify_multi_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf, size_t n_commits,
                        const void* d_commit_index, const void* d_group_start, size_t n_groups, const void* d_zs,
                        const void* d_ys, const void* d_weights, const void* d_proofs, const void* d_proof_inf,
                        const void* d_challenges, size_t count, int flags, bool checked, int subgroup, void* d_ok,
                        void* stream) {
  KZGX_TRY(activate(ctx));
  if (!multi_shape_ok(n_commits, n_groups, count, flags) || !d_ok) return KZGX_ERR_ARG;
  if (n_groups > 0 && (!d_challenges || !d_weights || !d_group_start || !d_zs || !d_proofs ||
                       (n_commits > 0 && !d_commits) || (count > 0 && (!d_commit_index || !d_ys))))
    return KZGX_ERR_ARG;
  if (n_commits + n_groups + 1 > KZGX_MSM_POINTS_MAX) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0 || ctx->n_srs2 < 2) return KZGX_ERR_NO_SRS;
  hipStream_t st = pick(ctx, stream);
  if (n_groups == 0) {
    KZGX_TRY_HIP(hipMemsetD32Async((hipDeviceptr_t)d_ok, 1, 1, st));
    return KZGX_OK;
  }
  kzgx::Ctx* c = &ctx->c;
  kzgx::WsLease ws = c->ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  const size_t pw = point_words(ctx);
  uint32_t* f = nullptr;  // commit flags | proof flags | their AND
  if (checked) {
    KZGX_TRY(chk_scratch(ctx, ws, n_commits + n_groups + 1, &f));
    if (n_commits)
      KZGX_TRY(kzgx::g1_check2(c, (const uint32_t*)d_commits, (const uint32_t*)d_commit_inf, n_commits,
                               (const uint32_t*)d_proofs, (const uint32_t*)d_proof_inf, n_groups, subgroup, f, st));
    else
      KZGX_TRY(kzgx::g1_check(c, (const uint32_t*)d_proofs, (const uint32_t*)d_proof_inf, n_groups, subgroup, f, st));
    KZGX_TRY(kzgx::flags_and(f, n_commits + n_groups, f + n_commits + n_groups, st));
  }
  // scalars s_c | r_g z_g | -t (+ scratch); A | B | flags [A_inf, B_inf, gate, -] | z = y = 0
  KZGX_TRY(kzgx::dev_alloc(c, (void**)&ws->var_scal, kzgx::multi_scalars_words(n_commits, n_groups, count) * 4,
                           &ws->var_scal_b));
  KZGX_TRY(kzgx::dev_alloc(c, (void**)&ws->var_pt, (2 * pw + 4 + 16) * 4, &ws->var_pt_b));
  uint32_t* A = ws->var_pt;
  uint32_t* B = A + pw;
  uint32_t* fl = B + pw;
  uint32_t* zero = fl + 4;
  KZGX_TRY_HIP(hipMemsetAsync(zero, 0, 64, st));
  KZGX_TRY(kzgx::multi_check(c, (const uint32_t*)d_commit_index, n_commits, (const uint32_t*)d_group_start, n_groups,
                             count, fl + 2, st));
  KZGX_TRY(kzgx::multi_scalars(c, (const uint32_t*)d_commit_index, (const uint32_t*)d_group_start, n_groups,
                               (const uint32_t*)d_zs, (const uint32_t*)d_ys, (const uint32_t*)d_weights,
                               (flags & KZGX_MULTI_WEIGHT_POWERS) != 0, (const uint32_t*)d_challenges, count,
                               n_commits, ws->var_scal, st));
  // A = sum r_g proof_g
  const kzgx::PointSeg sa{(const uint32_t*)d_proofs, (const uint32_t*)d_proof_inf, n_groups};
  KZGX_TRY(kzgx::msm_points(c, *ws, &sa, 1, (const uint32_t*)d_challenges, A, fl, st));
  // B = sum s_c commit_c + sum r_g z_g proof_g - t G1[0]
  const kzgx::PointSeg sb[3] = {{(const uint32_t*)d_commits, (const uint32_t*)d_commit_inf, n_commits},
                                {(const uint32_t*)d_proofs, (const uint32_t*)d_proof_inf, n_groups},
                                {ctx->d_srs_canon, nullptr, 1}};
  const int skip = n_commits ? 0 : 1;  // no empty segment
  KZGX_TRY(kzgx::msm_points(c, *ws, sb + skip, 3 - skip, ws->var_scal, B, fl + 1, st));
  // e(A, [tau]G2) == e(B, G2[0]), as kzgx_verify_aggregate_device's tail
  KZGX_TRY(kzgx_verify_single_batch_device(ctx, B, fl + 1, A, fl, zero, zero + 8, 1, d_ok, stream));
  KZGX_TRY(kzgx::flag_gate((uint32_t*)d_ok, fl + 2, st));
  if (checked) KZGX_TRY(kzgx::flag_gate((uint32_t*)d_ok, f + n_commits + n_groups, st));
  return KZGX_OK;
}

int verify_multi_host(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf, size_t n_commits,
                      const uint32_t* commit_index, const uint32_t* group_start, size_t n_groups, const uint64_t* zs,
                      const uint64_t* ys, const uint64_t* weights, const uint64_t* proofs_xy, const int* proof_inf,
                      const uint64_t* challenges, size_t count, int flags, bool checked, int subgroup, int* ok) {
  KZGX_TRY(activate(ctx));
  if (!multi_shape_ok(n_commits, n_groups, count, flags) || !ok) return KZGX_ERR_ARG;
  const int curve = ctx->c.curve;
  const size_t nw = (flags & KZGX_MULTI_WEIGHT_POWERS) ? n_groups : count;
  if (n_groups > 0) {
    if (!weights || !group_start || !zs || !proofs_xy || (n_commits > 0 && !commits_xy) ||
        (count > 0 && (!commit_index || !ys)))
      return KZGX_ERR_ARG;
    if (!multi_structure_ok(commit_index, n_commits, group_start, n_groups, count) ||
        !multi_canonical(curve, zs, n_groups) || !multi_canonical(curve, weights, nw) || (challenges && !multi_canonical(curve, challenges, n_groups)))
      return KZGX_ERR_ARG;
  }
  if (n_commits + n_groups + 1 > KZGX_MSM_POINTS_MAX) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0 || ctx->n_srs2 < 2) return KZGX_ERR_NO_SRS;
  if (n_groups == 0) {
    *ok = 1;
    return KZGX_OK;
  }
  // library-drawn challenges: independent 128-bit values, r_0 = 1 (as kzgx_verify_aggregate)
  std::vector<uint64_t> drawn;
  if (!challenges) {
    drawn.assign(n_groups * 4, 0);
    std::random_device rd;
    for (size_t g = 0; g < n_groups; g++)
      for (int j = 0; j < 2; j++) drawn[4 * g + j] = ((uint64_t)rd() << 32) | (uint64_t)rd();
    drawn[0] = 1;
    drawn[1] = 0;
    challenges = drawn.data();
  }
  const size_t pb = point_words(ctx) * 4;
  // scalars: z | y | weights | challenges; words: commit_inf | proof_inf | commit_index | group_start | ok
  const size_t s_y = n_groups * 32, s_w = s_y + count * 32, s_r = s_w + nw * 32, s_end = s_r + n_groups * 32;
  const size_t w_p = n_commits, w_i = w_p + n_groups, w_g = w_i + count, w_ok = w_g + n_groups + 1;
  void *d_c, *d_p, *d_s, *d_w;
  KZGX_TRY(stage(ctx, 0, n_commits * pb, &d_c));
  KZGX_TRY(stage(ctx, 1, n_groups * pb, &d_p));
  KZGX_TRY(stage(ctx, 2, s_end, &d_s));
  KZGX_TRY(stage(ctx, 3, (w_ok + 1) * 4, &d_w));
  std::vector<uint32_t> w(w_ok, 0u);
  for (size_t i = 0; i < n_commits; i++) w[i] = commit_inf ? (uint32_t)(commit_inf[i] != 0) : 0u;
  for (size_t g = 0; g < n_groups; g++) w[w_p + g] = proof_inf ? (uint32_t)(proof_inf[g] != 0) : 0u;
  std::copy(commit_index, commit_index + count, w.begin() + w_i);
  std::copy(group_start, group_start + n_groups + 1, w.begin() + w_g);
  hipStream_t st = ctx->c.stream;
  char* sc = (char*)d_s;
  uint32_t* dw = (uint32_t*)d_w;
  if (n_commits) KZGX_TRY_HIP(hipMemcpyAsync(d_c, commits_xy, n_commits * pb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_p, proofs_xy, n_groups * pb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(sc, zs, n_groups * 32, hipMemcpyHostToDevice, st));
  if (count) KZGX_TRY_HIP(hipMemcpyAsync(sc + s_y, ys, count * 32, hipMemcpyHostToDevice, st));
  if (nw) KZGX_TRY_HIP(hipMemcpyAsync(sc + s_w, weights, nw * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(sc + s_r, challenges, n_groups * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(dw, w.data(), w_ok * 4, hipMemcpyHostToDevice, st));
  KZGX_TRY(verify_multi_device(ctx, d_c, dw, n_commits, dw + w_i, dw + w_g, n_groups, sc, sc + s_y, sc + s_w, d_p,
                               dw + w_p, sc + s_r, count, flags, checked, subgroup, dw + w_ok, nullptr));
  uint32_t v = 0;
  KZGX_TRY_HIP(hipMemcpyAsync(&v, dw + w_ok, 4, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  *ok = v ? 1 : 0;
  return KZGX_OK;
}
}  // namespace

extern "C" {

int kzgx_verify_multi_batch_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf, size_t n_commits,
                                   const void* d_commit_index, const void* d_group_start, size_t n_groups,
                                   const void* d_zs, const void* d_ys, const void* d_weights, const void* d_proofs,
                                   const void* d_proof_inf, const void* d_challenges, size_t count, int flags,
                                   void* d_ok, void* stream) {
  return verify_multi_device(ctx, d_commits, d_commit_inf, n_commits, d_commit_index, d_group_start, n_groups, d_zs,
                             d_ys, d_weights, d_proofs, d_proof_inf, d_challenges, count, flags, false, 0, d_ok,
                             stream);
}

int kzgx_verify_multi_batch_checked_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf,
                                           size_t n_commits, const void* d_commit_index, const void* d_group_start,
                                           size_t n_groups, const void* d_zs, const void* d_ys,
                                           const void* d_weights, const void* d_proofs, const void* d_proof_inf,
                                           const void* d_challenges, size_t count, int flags, int subgroup,
                                           void* d_ok, void* stream) {
  return verify_multi_device(ctx, d_commits, d_commit_inf, n_commits, d_commit_index, d_group_start, n_groups, d_zs,
                             d_ys, d_weights, d_proofs, d_proof_inf, d_challenges, count, flags, true, subgroup, d_ok,
                             stream);
}

int kzgx_verify_multi_batch(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf, size_t n_commits,
                            const uint32_t* commit_index, const uint32_t* group_start, size_t n_groups,
                            const uint64_t* zs, const uint64_t* ys, const uint64_t* weights,
                            const uint64_t* proofs_xy, const int* proof_inf, const uint64_t* challenges, size_t count,
                            int flags, int* ok) {
  return verify_multi_host(ctx, commits_xy, commit_inf, n_commits, commit_index, group_start, n_groups, zs, ys,
                           weights, proofs_xy, proof_inf, challenges, count, flags, false, 0, ok);
}

int kzgx_verify_multi_batch_checked(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf,
                                    size_t n_commits, const uint32_t* commit_index, const uint32_t* group_start,
                                    size_t n_groups, const uint64_t* zs, const uint64_t* ys, const uint64_t* weights,
                                    const uint64_t* proofs_xy, const int* proof_inf, const uint64_t* challenges,
                                    size_t count, int flags, int subgroup, int* ok) {
  return verify_multi_host(ctx, commits_xy, commit_inf, n_commits, commit_index, group_start, n_groups, zs, ys,
                           weights, proofs_xy, proof_inf, challenges, count, flags, true, subgroup, ok);
}

}  // extern "C"

// ---- Shplonk openings: many polynomials at different point sets, one two-point proof (shplonk.hip) ----
namespace {
// the Shplonk buffer of the workspace slot leased for this call's stream, carved front to back
struct ShpArena {
  char* p = nullptr;
  size_t used = 0;
  template <class T>
  T* take(size_t bytes) {
    T* r = (T*)(p + used);
    used += align32(bytes);
    return r;
  }
};
int shp_scratch(kzgx_ctx* ctx, const kzgx::WsLease& ws, size_t bytes, ShpArena* a) {
  const size_t slot = (size_t)(ws.get() - ctx->c.ws);
  KZGX_TRY(kzgx::dev_alloc(&ctx->c, (void**)&ctx->d_shp[slot], bytes, &ctx->shp_b[slot]));
  a->p = (char*)ctx->d_shp[slot];
  a->used = 0;
  return KZGX_OK;
}

// what the host can see of a call's shape, both sides (n_index: polynomials or commitments)
bool shp_shape_ok(size_t n_index, size_t n_points, size_t n_set_points, size_t n_sets, size_t count, size_t n_values,
                  int flags) {
  return (flags & ~KZGX_SHPLONK_WEIGHT_POWERS) == 0 && n_index <= 0xffffffffu && n_sets > 0 && n_sets < 65536 &&
         n_points > 0 && n_points <= KZGX_SHPLONK_POINTS_MAX && n_set_points > 0 &&
         n_set_points <= n_sets * KZGX_SHPLONK_SET_MAX && count <= 0x7fffffffu && n_values <= 0x7fffffffu;
}

kzgx::ShpTable shp_table(const void* d_points, size_t n_points, const void* d_sps, const void* d_sp,
                         size_t n_set_points, const void* d_cs, size_t n_sets, size_t count) {
  kzgx::ShpTable t;
  t.points = (const uint32_t*)d_points;
  t.set_point_start = (const uint32_t*)d_sps;
  t.set_points = (const uint32_t*)d_sp;
  t.claim_start = (const uint32_t*)d_cs;
  t.n_points = (uint32_t)n_points;
  t.n_set_points = (uint32_t)n_set_points;
  t.n_sets = (uint32_t)n_sets;
  t.count = (uint32_t)count;
  return t;
}

// the host entries' structure check (KZGX_ERR_ARG), then equal values inside one set (KZGX_ERR_DIV_ZERO).
// n_values == SIZE_MAX: the call has no values (kzgx_shplonk_open).
int shp_structure(int curve, const uint32_t* index, size_t n_index, const uint64_t* points, size_t n_points,
                  const uint32_t* sps, const uint32_t* sp, size_t n_set_points, const uint32_t* cs, size_t n_sets,
                  size_t count, size_t n_values) {
  if (sps[0] != 0 || sps[n_sets] != n_set_points || cs[0] != 0 || cs[n_sets] != count) return KZGX_ERR_ARG;
  uint64_t total = 0;
  for (size_t s = 0; s < n_sets; s++) {
    if (sps[s] >= sps[s + 1] || sps[s + 1] - sps[s] > KZGX_SHPLONK_SET_MAX || cs[s] > cs[s + 1]) return KZGX_ERR_ARG;
    total += (uint64_t)(sps[s + 1] - sps[s]) * (cs[s + 1] - cs[s]);
  }
  if (n_values != SIZE_MAX && total != n_values) return KZGX_ERR_ARG;
  for (size_t j = 0; j < n_set_points; j++)
    if (sp[j] >= n_points) return KZGX_ERR_ARG;
  for (size_t k = 0; k < count; k++)
    if (index[k] >= n_index) return KZGX_ERR_ARG;
  for (size_t s = 0; s < n_sets; s++)
    for (uint32_t a = sps[s]; a < sps[s + 1]; a++)
      for (uint32_t b = a + 1; b < sps[s + 1]; b++)
        if (sp[a] == sp[b]) return KZGX_ERR_ARG;
  if (!multi_canonical(curve, points, n_points)) return KZGX_ERR_ARG;
  for (size_t s = 0; s < n_sets; s++)
    for (uint32_t a = sps[s]; a < sps[s + 1]; a++)
      for (uint32_t b = a + 1; b < sps[s + 1]; b++)
        if (std::memcmp(points + 4 * (size_t)sp[a], points + 4 * (size_t)sp[b], 32) == 0) return KZGX_ERR_DIV_ZERO;
  return KZGX_OK;
}

// the index arrays of a host call in one staging block: set_point_start | set_points | claim_start | index
struct ShpIdx {
  size_t o_sps, o_sp, o_cs, o_ix, bytes;
};
ShpIdx shp_idx_layout(size_t n_set_points, size_t n_sets, size_t count) {
  ShpIdx l;
  l.o_sps = 0;
  l.o_sp = l.o_sps + align32((n_sets + 1) * 4);
  l.o_cs = l.o_sp + align32(n_set_points * 4);
  l.o_ix = l.o_cs + align32((n_sets + 1) * 4);
  l.bytes = l.o_ix + align32(count * 4);
  return l;
}
int shp_idx_copy(char* d, const ShpIdx& l, const uint32_t* sps, const uint32_t* sp, size_t n_set_points,
                 const uint32_t* cs, const uint32_t* index, size_t n_sets, size_t count, hipStream_t st) {
  KZGX_TRY_HIP(hipMemcpyAsync(d + l.o_sps, sps, (n_sets + 1) * 4, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d + l.o_sp, sp, n_set_points * 4, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d + l.o_cs, cs, (n_sets + 1) * 4, hipMemcpyHostToDevice, st));
  if (count) KZGX_TRY_HIP(hipMemcpyAsync(d + l.o_ix, index, count * 4, hipMemcpyHostToDevice, st));
  return KZGX_OK;
}
}  // namespace

extern "C" {

int kzgx_set_shplonk_chunk(kzgx_ctx* ctx, size_t scalars) {
  if (!ctx) return KZGX_ERR_ARG;
  ctx->shplonk_chunk = scalars;
  return KZGX_OK;
}

int kzgx_shplonk_commit_device(kzgx_ctx* ctx, const void* d_coeffs, size_t n, size_t coeff_stride, size_t n_polys,
                               const void* d_points, size_t n_points, const void* d_set_point_start,
                               const void* d_set_points, size_t n_set_points, const void* d_claim_start,
                               const void* d_poly_index, size_t n_sets, const void* d_weights, size_t count,
                               size_t n_values, int flags, void* d_out_xy, void* d_out_is_inf, void* d_out_h,
                               void* d_out_y, void* d_ok, void* stream) {
  KZGX_TRY(activate(ctx));
  if (!shp_shape_ok(n_polys, n_points, n_set_points, n_sets, count, n_values, flags) || n == 0 || n > 0xffffffffu ||
      coeff_stride < n)
    return KZGX_ERR_ARG;
  if (!d_coeffs || !d_points || !d_set_point_start || !d_set_points || !d_claim_start || !d_weights || !d_out_xy ||
      !d_out_is_inf || !d_out_h || (count > 0 && !d_poly_index))
    return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  if (n - 1 > ctx->c.n_srs) return KZGX_ERR_DEGREE;
  hipStream_t st = pick(ctx, stream);
  kzgx::Ctx* c = &ctx->c;
  kzgx::WsLease ws = c->ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  const bool powers = (flags & KZGX_SHPLONK_WEIGHT_POWERS) != 0;
  const size_t chunk = ctx->shplonk_chunk ? ctx->shplonk_chunk : kzgx::SHP_CHUNK_SCALARS;
  const size_t cs = std::min(std::max<size_t>(1, chunk / n), n_sets);  // sets per chunk (n_sets < 2^16)
  const size_t NT = kzgx::shp_tiles(n);
  // the values: as kzgx_prove_multi_batch_device's claims, over the (claim, point) list
  const uint32_t slice = kzgx::MULTI_EVAL_SLICE;
  const size_t nsl = n > slice ? (n + slice - 1) / slice : 0;
  const bool want_y = d_out_y && n_values > 0;
  const size_t ek = !want_y ? 0 : nsl ? std::min(std::max<size_t>(1, chunk / nsl), n_values) : n_values;
  const size_t part_sc = want_y ? kzgx::multi_eval_part_scalars(ek, n, slice) : 0;
  const size_t tot_sc = NT > 1 ? cs * kzgx::SHP_SET_MAX * NT * 2 : 0;
  ShpArena a;
  KZGX_TRY(shp_scratch(ctx, ws,
                       (n_set_points + (powers ? count : 0) + cs * n + tot_sc + (want_y ? n_values + part_sc : 0)) * 32 +
                           align32((n_sets + 1) * 8) + 32 + (want_y ? 2 * align32((n_values + 1) * 4) : 0) + 8 * 32,
                       &a));
  uint32_t* pc = a.take<uint32_t>(n_set_points * 32);
  uint32_t* wexp = a.take<uint32_t>(powers ? count * 32 : 0);
  uint32_t* F = a.take<uint32_t>(cs * n * 32);
  uint32_t* tot = a.take<uint32_t>(tot_sc * 32);
  uint64_t* voff = a.take<uint64_t>((n_sets + 1) * 8);
  uint32_t* gate = a.take<uint32_t>(32);
  const kzgx::ShpTable t =
      shp_table(d_points, n_points, d_set_point_start, d_set_points, n_set_points, d_claim_start, n_sets, count);
  const uint32_t* pidx = (const uint32_t*)d_poly_index;
  KZGX_TRY_HIP(hipMemsetD32Async((hipDeviceptr_t)gate, 1, 1, st));
  KZGX_TRY(kzgx::shp_check(t, pidx, n_polys, gate, st));
  KZGX_TRY(kzgx::shp_pairs(c, t, nullptr, pc, nullptr, gate, st));
  KZGX_TRY(kzgx::shp_offsets(t, voff, n_values, gate, st));
  const uint32_t* wts = (const uint32_t*)d_weights;
  if (powers) {
    KZGX_TRY(kzgx::shp_weight_powers(c, wts, count, wexp, st));
    wts = wexp;
  }
  for (size_t s0 = 0; s0 < n_sets; s0 += cs) {
    const size_t ns = std::min(cs, n_sets - s0);
    KZGX_TRY(kzgx::multi_fold(c, (const uint32_t*)d_coeffs, n, coeff_stride * 8, n_polys, pidx, t.claim_start, s0, ns,
                              count, wts, false, F, st));
    KZGX_TRY(kzgx::shp_quotient(c, t, F, n, s0, ns, pc, tot, (uint32_t*)d_out_h, s0 > 0, st));
  }
  // W = [h(tau)]G1 over the n - 1 scalars that can be non-zero
  KZGX_TRY(kzgx_msm_g1_batch_device(ctx, d_out_h, n - 1, 1, n - 1, d_out_xy, d_out_is_inf, st));
  if (want_y) {
    uint32_t* ezs = a.take<uint32_t>(n_values * 32);
    uint32_t* part = a.take<uint32_t>(part_sc * 32);
    uint32_t* epoly = a.take<uint32_t>((n_values + 1) * 4);
    uint32_t* egs = a.take<uint32_t>((n_values + 1) * 4);
    KZGX_TRY(kzgx::shp_expand(c, t, voff, pidx, n_values, epoly, ezs, egs, st));
    for (size_t k0 = 0; k0 < n_values; k0 += ek)
      KZGX_TRY(kzgx::multi_eval(c, (const uint32_t*)d_coeffs, n, coeff_stride * 8, n_polys, epoly, egs, n_values, ezs,
                                k0, std::min(ek, n_values - k0), (uint32_t*)d_out_y, part, slice, st));
  }
  if (d_ok) KZGX_TRY_HIP(hipMemcpyAsync(d_ok, gate, 4, hipMemcpyDeviceToDevice, st));
  return KZGX_OK;
}

int kzgx_shplonk_commit(kzgx_ctx* ctx, const uint64_t* coeffs, size_t n, size_t coeff_stride, size_t n_polys,
                        const uint64_t* points, size_t n_points, const uint32_t* set_point_start,
                        const uint32_t* set_points, size_t n_set_points, const uint32_t* claim_start,
                        const uint32_t* poly_index, size_t n_sets, const uint64_t* weights, size_t count,
                        size_t n_values, int flags, uint64_t* out_xy, int* out_is_inf, uint64_t* out_h,
                        uint64_t* out_y) {
  KZGX_TRY(activate(ctx));
  if (!shp_shape_ok(n_polys, n_points, n_set_points, n_sets, count, n_values, flags) || n == 0 || n > 0xffffffffu ||
      coeff_stride < n)
    return KZGX_ERR_ARG;
  if (!points || !set_point_start || !set_points || !claim_start || !weights || !out_xy || !out_is_inf || !out_h ||
      (count > 0 && !poly_index) || (n_polys > 0 && !coeffs))
    return KZGX_ERR_ARG;
  const size_t nw = (flags & KZGX_SHPLONK_WEIGHT_POWERS) ? 1 : count;
  if (!multi_canonical(ctx->c.curve, weights, nw)) return KZGX_ERR_ARG;
  KZGX_TRY(shp_structure(ctx->c.curve, poly_index, n_polys, points, n_points, set_point_start, set_points,
                         n_set_points, claim_start, n_sets, count, n_values));
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  if (n - 1 > ctx->c.n_srs) return KZGX_ERR_DEGREE;
  const size_t pb = point_words(ctx) * 4;
  const size_t cb = n_polys ? ((n_polys - 1) * coeff_stride + n) * 32 : 32;
  // inputs: points | weights | index arrays; outputs: W | flag | h | y
  const ShpIdx il = shp_idx_layout(n_set_points, n_sets, count);
  const size_t i_w = n_points * 32, i_x = i_w + std::max<size_t>(nw, 1) * 32, i_end = i_x + il.bytes;
  const size_t o_f = align32(pb), o_h = o_f + 32, o_y = o_h + n * 32, o_end = o_y + std::max<size_t>(n_values, 1) * 32;
  void *d_c, *d_i, *d_o;
  KZGX_TRY(stage(ctx, 0, cb, &d_c));
  KZGX_TRY(stage(ctx, 1, i_end, &d_i));
  KZGX_TRY(stage(ctx, 2, o_end, &d_o));
  hipStream_t st = ctx->c.stream;
  char *in = (char*)d_i, *out = (char*)d_o;
  if (n_polys) KZGX_TRY_HIP(hipMemcpyAsync(d_c, coeffs, cb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(in, points, n_points * 32, hipMemcpyHostToDevice, st));
  if (nw) KZGX_TRY_HIP(hipMemcpyAsync(in + i_w, weights, nw * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY(shp_idx_copy(in + i_x, il, set_point_start, set_points, n_set_points, claim_start, poly_index, n_sets, count,
                        st));
  KZGX_TRY(kzgx_shplonk_commit_device(ctx, d_c, n, coeff_stride, n_polys, in, n_points, in + i_x + il.o_sps,
                                      in + i_x + il.o_sp, n_set_points, in + i_x + il.o_cs, in + i_x + il.o_ix, n_sets,
                                      in + i_w, count, n_values, flags, out, out + o_f, out + o_h,
                                      out_y ? out + o_y : nullptr, nullptr, nullptr));
  uint32_t inf = 0;
  KZGX_TRY_HIP(hipMemcpyAsync(out_xy, out, pb, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipMemcpyAsync(&inf, out + o_f, 4, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipMemcpyAsync(out_h, out + o_h, n * 32, hipMemcpyDeviceToHost, st));
  if (out_y && n_values) KZGX_TRY_HIP(hipMemcpyAsync(out_y, out + o_y, n_values * 32, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  *out_is_inf = (int)inf;
  return KZGX_OK;
}

int kzgx_shplonk_open_device(kzgx_ctx* ctx, const void* d_coeffs, size_t n, size_t coeff_stride, size_t n_polys,
                             const void* d_points, size_t n_points, const void* d_set_point_start,
                             const void* d_set_points, size_t n_set_points, const void* d_claim_start,
                             const void* d_poly_index, size_t n_sets, const void* d_weights, size_t count, int flags,
                             const void* d_h, const void* d_z, void* d_out_xy, void* d_out_is_inf, void* d_out_Gz,
                             void* d_ok, void* stream) {
  KZGX_TRY(activate(ctx));
  if (!shp_shape_ok(n_polys, n_points, n_set_points, n_sets, count, 0, flags) || n == 0 || n > 0xffffffffu ||
      coeff_stride < n)
    return KZGX_ERR_ARG;
  if (!d_coeffs || !d_points || !d_set_point_start || !d_set_points || !d_claim_start || !d_weights || !d_h || !d_z ||
      !d_out_xy || !d_out_is_inf || (count > 0 && !d_poly_index))
    return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  if (n - 1 > ctx->c.n_srs) return KZGX_ERR_DEGREE;
  hipStream_t st = pick(ctx, stream);
  kzgx::Ctx* c = &ctx->c;
  kzgx::WsLease ws = c->ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  const bool powers = (flags & KZGX_SHPLONK_WEIGHT_POWERS) != 0;
  ShpArena a;
  KZGX_TRY(shp_scratch(ctx, ws, (n_sets + 1 + (powers ? count : 0) + count + n) * 32 + 2 * 32 + 8 * 32, &a));
  uint32_t* zeta = a.take<uint32_t>((n_sets + 1) * 32);
  uint32_t* wexp = a.take<uint32_t>(powers ? count * 32 : 0);
  uint32_t* cw = a.take<uint32_t>(count * 32);
  uint32_t* G = a.take<uint32_t>(n * 32);
  uint32_t* gs2 = a.take<uint32_t>(32);
  uint32_t* gate = a.take<uint32_t>(32);
  const kzgx::ShpTable t =
      shp_table(d_points, n_points, d_set_point_start, d_set_points, n_set_points, d_claim_start, n_sets, count);
  const uint32_t* pidx = (const uint32_t*)d_poly_index;
  KZGX_TRY_HIP(hipMemsetD32Async((hipDeviceptr_t)gate, 1, 1, st));
  KZGX_TRY(kzgx::shp_check(t, pidx, n_polys, gate, st));
  KZGX_TRY(kzgx::shp_zeta(c, t, (const uint32_t*)d_z, zeta, st));
  const uint32_t* wts = (const uint32_t*)d_weights;
  if (powers) {
    KZGX_TRY(kzgx::shp_weight_powers(c, wts, count, wexp, st));
    wts = wexp;
  }
  // G = sum_k zeta_(s(k)) w_k P_k - Z_T(z) h: one fold of all claims as one group, one axpy
  KZGX_TRY(kzgx::shp_claim_weights(c, t, zeta, wts, cw, gs2, st));
  KZGX_TRY(kzgx::multi_fold(c, (const uint32_t*)d_coeffs, n, coeff_stride * 8, n_polys, pidx, gs2, 0, 1, count, cw,
                            false, G, st));
  KZGX_TRY(kzgx::shp_axpy(c, G, (const uint32_t*)d_h, zeta + n_sets * 8, n, st));
  KZGX_TRY(kzgx_prove_single_batch_device(ctx, G, n, n, d_z, 1, d_out_xy, d_out_is_inf, d_out_Gz, st));
  if (d_ok) KZGX_TRY_HIP(hipMemcpyAsync(d_ok, gate, 4, hipMemcpyDeviceToDevice, st));
  return KZGX_OK;
}

int kzgx_shplonk_open(kzgx_ctx* ctx, const uint64_t* coeffs, size_t n, size_t coeff_stride, size_t n_polys,
                      const uint64_t* points, size_t n_points, const uint32_t* set_point_start,
                      const uint32_t* set_points, size_t n_set_points, const uint32_t* claim_start,
                      const uint32_t* poly_index, size_t n_sets, const uint64_t* weights, size_t count, int flags,
                      const uint64_t* h, const uint64_t* z, uint64_t* out_xy, int* out_is_inf, uint64_t* out_Gz) {
  KZGX_TRY(activate(ctx));
  if (!shp_shape_ok(n_polys, n_points, n_set_points, n_sets, count, 0, flags) || n == 0 || n > 0xffffffffu ||
      coeff_stride < n)
    return KZGX_ERR_ARG;
  if (!points || !set_point_start || !set_points || !claim_start || !weights || !h || !z || !out_xy || !out_is_inf ||
      (count > 0 && !poly_index) || (n_polys > 0 && !coeffs))
    return KZGX_ERR_ARG;
  const int curve = ctx->c.curve;
  const size_t nw = (flags & KZGX_SHPLONK_WEIGHT_POWERS) ? 1 : count;
  if (!multi_canonical(curve, weights, nw) || !multi_canonical(curve, z, 1) || !multi_canonical(curve, h, n))
    return KZGX_ERR_ARG;
  KZGX_TRY(shp_structure(curve, poly_index, n_polys, points, n_points, set_point_start, set_points, n_set_points,
                         claim_start, n_sets, count, SIZE_MAX));
  if (ctx->c.n_srs == 0) return KZGX_ERR_NO_SRS;
  if (n - 1 > ctx->c.n_srs) return KZGX_ERR_DEGREE;
  const size_t pb = point_words(ctx) * 4;
  const size_t cb = n_polys ? ((n_polys - 1) * coeff_stride + n) * 32 : 32;
  // inputs: points | weights | z | h | index arrays; outputs: W' | flag | G(z)
  const ShpIdx il = shp_idx_layout(n_set_points, n_sets, count);
  const size_t i_w = n_points * 32, i_z = i_w + std::max<size_t>(nw, 1) * 32, i_h = i_z + 32, i_x = i_h + n * 32,
               i_end = i_x + il.bytes;
  const size_t o_f = align32(pb), o_g = o_f + 32, o_end = o_g + 32;
  void *d_c, *d_i, *d_o;
  KZGX_TRY(stage(ctx, 0, cb, &d_c));
  KZGX_TRY(stage(ctx, 1, i_end, &d_i));
  KZGX_TRY(stage(ctx, 2, o_end, &d_o));
  hipStream_t st = ctx->c.stream;
  char *in = (char*)d_i, *out = (char*)d_o;
  if (n_polys) KZGX_TRY_HIP(hipMemcpyAsync(d_c, coeffs, cb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(in, points, n_points * 32, hipMemcpyHostToDevice, st));
  if (nw) KZGX_TRY_HIP(hipMemcpyAsync(in + i_w, weights, nw * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(in + i_z, z, 32, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(in + i_h, h, n * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY(shp_idx_copy(in + i_x, il, set_point_start, set_points, n_set_points, claim_start, poly_index, n_sets, count,
                        st));
  KZGX_TRY(kzgx_shplonk_open_device(ctx, d_c, n, coeff_stride, n_polys, in, n_points, in + i_x + il.o_sps,
                                    in + i_x + il.o_sp, n_set_points, in + i_x + il.o_cs, in + i_x + il.o_ix, n_sets,
                                    in + i_w, count, flags, in + i_h, in + i_z, out, out + o_f, out + o_g, nullptr,
                                    nullptr));
  uint32_t inf = 0;
  KZGX_TRY_HIP(hipMemcpyAsync(out_xy, out, pb, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipMemcpyAsync(&inf, out + o_f, 4, hipMemcpyDeviceToHost, st));
  if (out_Gz) KZGX_TRY_HIP(hipMemcpyAsync(out_Gz, out + o_g, 32, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  *out_is_inf = (int)inf;
  return KZGX_OK;
}

}  // extern "C"

namespace {
// the device verify, with the point checks in front when checked
int shp_verify_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf, size_t n_commits,
                      const void* d_commit_index, const void* d_points, size_t n_points,
                      const void* d_set_point_start, const void* d_set_points, size_t n_set_points,
                      const void* d_claim_start, size_t n_sets, const void* d_ys, size_t n_values,
                      const void* d_weights, size_t count, const void* d_z, const void* d_proof_xy,
                      const void* d_proof_inf, int flags, bool checked, int subgroup, void* d_ok, void* stream) {
  KZGX_TRY(activate(ctx));
  if (!shp_shape_ok(n_commits, n_points, n_set_points, n_sets, count, n_values, flags) || !d_ok) return KZGX_ERR_ARG;
  if (!d_points || !d_set_point_start || !d_set_points || !d_claim_start || !d_weights || !d_z || !d_proof_xy ||
      (n_commits > 0 && !d_commits) || (count > 0 && !d_commit_index) || (n_values > 0 && !d_ys))
    return KZGX_ERR_ARG;
  if (n_commits + 3 > KZGX_MSM_POINTS_MAX) return KZGX_ERR_ARG;
  if (ctx->c.n_srs == 0 || ctx->n_srs2 < 2) return KZGX_ERR_NO_SRS;
  hipStream_t st = pick(ctx, stream);
  kzgx::Ctx* c = &ctx->c;
  kzgx::WsLease ws = c->ws_for(st);
  if (!ws) return KZGX_ERR_ARG;
  const size_t pw = point_words(ctx);
  const bool powers = (flags & KZGX_SHPLONK_WEIGHT_POWERS) != 0;
  uint32_t* f = nullptr;  // commit flags | W, W' flags | their AND
  if (checked) {
    KZGX_TRY(chk_scratch(ctx, ws, n_commits + 2 + 1, &f));
    if (n_commits)
      KZGX_TRY(kzgx::g1_check2(c, (const uint32_t*)d_commits, (const uint32_t*)d_commit_inf, n_commits,
                               (const uint32_t*)d_proof_xy, (const uint32_t*)d_proof_inf, 2, subgroup, f, st));
    else
      KZGX_TRY(kzgx::g1_check(c, (const uint32_t*)d_proof_xy, (const uint32_t*)d_proof_inf, 2, subgroup, f, st));
    KZGX_TRY(kzgx::flags_and(f, n_commits + 2, f + n_commits + 2, st));
  }
  const size_t ms_words = kzgx::multi_scalars_words(n_commits, n_sets, count);
  ShpArena a;
  KZGX_TRY(shp_scratch(ctx, ws,
                       (2 * n_set_points + n_sets + 1 + (powers ? count : 0) + count + n_commits + 4) * 32 +
                           align32(ms_words * 4) + align32((n_sets + 1) * 8) + 32 + 10 * 32,
                       &a));
  uint32_t* pc = a.take<uint32_t>(n_set_points * 32);
  uint32_t* pl = a.take<uint32_t>(n_set_points * 32);
  uint32_t* zeta = a.take<uint32_t>((n_sets + 1) * 32);
  uint32_t* wexp = a.take<uint32_t>(powers ? count * 32 : 0);
  uint32_t* rk = a.take<uint32_t>(count * 32);
  uint32_t* ms = a.take<uint32_t>(ms_words * 4);
  uint32_t* sc = a.take<uint32_t>((n_commits + 4) * 32);
  uint64_t* voff = a.take<uint64_t>((n_sets + 1) * 8);
  uint32_t* gate = a.take<uint32_t>(32);
  // A | B | flags [A_inf, B_inf, -, -] | z = y = 0
  KZGX_TRY(kzgx::dev_alloc(c, (void**)&ws->var_pt, (2 * pw + 4 + 16) * 4, &ws->var_pt_b));
  uint32_t* A = ws->var_pt;
  uint32_t* B = A + pw;
  uint32_t* fl = B + pw;
  uint32_t* zero = fl + 4;
  KZGX_TRY_HIP(hipMemsetAsync(zero, 0, 64, st));
  const kzgx::ShpTable t =
      shp_table(d_points, n_points, d_set_point_start, d_set_points, n_set_points, d_claim_start, n_sets, count);
  const uint32_t* cidx = (const uint32_t*)d_commit_index;
  const uint32_t* zp = (const uint32_t*)d_z;
  KZGX_TRY_HIP(hipMemsetD32Async((hipDeviceptr_t)gate, 1, 1, st));
  KZGX_TRY(kzgx::shp_check(t, cidx, n_commits, gate, st));
  KZGX_TRY(kzgx::shp_pairs(c, t, zp, pc, pl, gate, st));
  KZGX_TRY(kzgx::shp_zeta(c, t, zp, zeta, st));
  KZGX_TRY(kzgx::shp_offsets(t, voff, n_values, gate, st));
  const uint32_t* wts = (const uint32_t*)d_weights;
  if (powers) {
    KZGX_TRY(kzgx::shp_weight_powers(c, wts, count, wexp, st));
    wts = wexp;
  }
  KZGX_TRY(kzgx::shp_interp(c, t, voff, (const uint32_t*)d_ys, n_values, pl, rk, st));
  // the batch openings' scalars with r_g := zeta_s and y_k := r_k(z): s_c and -t
  KZGX_TRY(kzgx::multi_scalars(c, cidx, t.claim_start, n_sets, zeta, rk, wts, false, zeta, count, n_commits, ms, st));
  KZGX_TRY(kzgx::shp_pack(c, ms, n_commits, n_sets, zeta, zp, sc, st));
  // A = W'
  const uint32_t* pinf = (const uint32_t*)d_proof_inf;
  const kzgx::PointSeg sa{(const uint32_t*)d_proof_xy + pw, pinf ? pinf + 1 : nullptr, 1};
  KZGX_TRY(kzgx::msm_points(c, *ws, &sa, 1, sc + (n_commits + 3) * 8, A, fl, st));
  // B = sum s_c C_c - t G1[0] - Z_T(z) W + z W'
  const kzgx::PointSeg sb[3] = {{(const uint32_t*)d_commits, (const uint32_t*)d_commit_inf, n_commits},
                                {ctx->d_srs_canon, nullptr, 1},
                                {(const uint32_t*)d_proof_xy, pinf, 2}};
  const int skip = n_commits ? 0 : 1;  // no empty segment
  KZGX_TRY(kzgx::msm_points(c, *ws, sb + skip, 3 - skip, sc, B, fl + 1, st));
  // e(A, [tau]G2) == e(B, G2[0]), as kzgx_verify_aggregate_device's tail
  KZGX_TRY(kzgx_verify_single_batch_device(ctx, B, fl + 1, A, fl, zero, zero + 8, 1, d_ok, stream));
  KZGX_TRY(kzgx::flag_gate((uint32_t*)d_ok, gate, st));
  if (checked) KZGX_TRY(kzgx::flag_gate((uint32_t*)d_ok, f + n_commits + 2, st));
  return KZGX_OK;
}

int shp_verify_host(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf, size_t n_commits,
                    const uint32_t* commit_index, const uint64_t* points, size_t n_points,
                    const uint32_t* set_point_start, const uint32_t* set_points, size_t n_set_points,
                    const uint32_t* claim_start, size_t n_sets, const uint64_t* ys, size_t n_values,
                    const uint64_t* weights, size_t count, const uint64_t* z, const uint64_t* proof_xy,
                    const int* proof_inf, int flags, bool checked, int subgroup, int* ok) {
  KZGX_TRY(activate(ctx));
  if (!shp_shape_ok(n_commits, n_points, n_set_points, n_sets, count, n_values, flags) || !ok) return KZGX_ERR_ARG;
  if (!points || !set_point_start || !set_points || !claim_start || !weights || !z || !proof_xy ||
      (n_commits > 0 && !commits_xy) || (count > 0 && !commit_index) || (n_values > 0 && !ys))
    return KZGX_ERR_ARG;
  if (n_commits + 3 > KZGX_MSM_POINTS_MAX) return KZGX_ERR_ARG;
  const int curve = ctx->c.curve;
  const size_t nw = (flags & KZGX_SHPLONK_WEIGHT_POWERS) ? 1 : count;
  if (!multi_canonical(curve, weights, nw) || !multi_canonical(curve, z, 1) || !multi_canonical(curve, ys, n_values))
    return KZGX_ERR_ARG;
  KZGX_TRY(shp_structure(curve, commit_index, n_commits, points, n_points, set_point_start, set_points, n_set_points,
                         claim_start, n_sets, count, n_values));
  if (ctx->c.n_srs == 0 || ctx->n_srs2 < 2) return KZGX_ERR_NO_SRS;
  const size_t pb = point_words(ctx) * 4;
  // scalars: points | y | weights | z; words: commit_inf | proof_inf (2) | index arrays | ok
  const ShpIdx il = shp_idx_layout(n_set_points, n_sets, count);
  const size_t s_y = n_points * 32, s_w = s_y + n_values * 32, s_z = s_w + std::max<size_t>(nw, 1) * 32, s_end = s_z + 32;
  const size_t w_p = align32(n_commits * 4), w_x = w_p + 32, w_ok = w_x + il.bytes, w_end = w_ok + 32;
  void *d_c, *d_p, *d_s, *d_w;
  KZGX_TRY(stage(ctx, 0, std::max<size_t>(n_commits, 1) * pb, &d_c));
  KZGX_TRY(stage(ctx, 1, 2 * pb, &d_p));
  KZGX_TRY(stage(ctx, 2, s_end, &d_s));
  KZGX_TRY(stage(ctx, 3, w_end, &d_w));
  std::vector<uint32_t> cf(n_commits + 2, 0u);
  for (size_t i = 0; i < n_commits; i++) cf[i] = commit_inf ? (uint32_t)(commit_inf[i] != 0) : 0u;
  for (size_t i = 0; i < 2; i++) cf[n_commits + i] = proof_inf ? (uint32_t)(proof_inf[i] != 0) : 0u;
  hipStream_t st = ctx->c.stream;
  char *sc = (char*)d_s, *dw = (char*)d_w;
  if (n_commits) {
    KZGX_TRY_HIP(hipMemcpyAsync(d_c, commits_xy, n_commits * pb, hipMemcpyHostToDevice, st));
    KZGX_TRY_HIP(hipMemcpyAsync(dw, cf.data(), n_commits * 4, hipMemcpyHostToDevice, st));
  }
  KZGX_TRY_HIP(hipMemcpyAsync(dw + w_p, cf.data() + n_commits, 8, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(d_p, proof_xy, 2 * pb, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(sc, points, n_points * 32, hipMemcpyHostToDevice, st));
  if (n_values) KZGX_TRY_HIP(hipMemcpyAsync(sc + s_y, ys, n_values * 32, hipMemcpyHostToDevice, st));
  if (nw) KZGX_TRY_HIP(hipMemcpyAsync(sc + s_w, weights, nw * 32, hipMemcpyHostToDevice, st));
  KZGX_TRY_HIP(hipMemcpyAsync(sc + s_z, z, 32, hipMemcpyHostToDevice, st));
  KZGX_TRY(shp_idx_copy(dw + w_x, il, set_point_start, set_points, n_set_points, claim_start, commit_index, n_sets,
                        count, st));
  // the flags are copied before the call below only reads them: the vector outlives the synchronisation
  KZGX_TRY(shp_verify_device(ctx, d_c, dw, n_commits, dw + w_x + il.o_ix, sc, n_points, dw + w_x + il.o_sps,
                             dw + w_x + il.o_sp, n_set_points, dw + w_x + il.o_cs, n_sets, sc + s_y, n_values,
                             sc + s_w, count, sc + s_z, d_p, dw + w_p, flags, checked, subgroup, dw + w_ok, nullptr));
  uint32_t v = 0;
  KZGX_TRY_HIP(hipMemcpyAsync(&v, dw + w_ok, 4, hipMemcpyDeviceToHost, st));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  *ok = v ? 1 : 0;
  return KZGX_OK;
}
}  // namespace

extern "C" {

int kzgx_shplonk_verify_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf, size_t n_commits,
                               const void* d_commit_index, const void* d_points, size_t n_points,
                               const void* d_set_point_start, const void* d_set_points, size_t n_set_points,
                               const void* d_claim_start, size_t n_sets, const void* d_ys, size_t n_values,
                               const void* d_weights, size_t count, const void* d_z, const void* d_proof_xy,
                               const void* d_proof_inf, int flags, void* d_ok, void* stream) {
  return shp_verify_device(ctx, d_commits, d_commit_inf, n_commits, d_commit_index, d_points, n_points,
                           d_set_point_start, d_set_points, n_set_points, d_claim_start, n_sets, d_ys, n_values,
                           d_weights, count, d_z, d_proof_xy, d_proof_inf, flags, false, 0, d_ok, stream);
}

int kzgx_shplonk_verify_checked_device(kzgx_ctx* ctx, const void* d_commits, const void* d_commit_inf,
                                       size_t n_commits, const void* d_commit_index, const void* d_points,
                                       size_t n_points, const void* d_set_point_start, const void* d_set_points,
                                       size_t n_set_points, const void* d_claim_start, size_t n_sets,
                                       const void* d_ys, size_t n_values, const void* d_weights, size_t count,
                                       const void* d_z, const void* d_proof_xy, const void* d_proof_inf, int flags,
                                       int subgroup, void* d_ok, void* stream) {
  return shp_verify_device(ctx, d_commits, d_commit_inf, n_commits, d_commit_index, d_points, n_points,
                           d_set_point_start, d_set_points, n_set_points, d_claim_start, n_sets, d_ys, n_values,
                           d_weights, count, d_z, d_proof_xy, d_proof_inf, flags, true, subgroup, d_ok, stream);
}

int kzgx_shplonk_verify(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf, size_t n_commits,
                        const uint32_t* commit_index, const uint64_t* points, size_t n_points,
                        const uint32_t* set_point_start, const uint32_t* set_points, size_t n_set_points,
                        const uint32_t* claim_start, size_t n_sets, const uint64_t* ys, size_t n_values,
                        const uint64_t* weights, size_t count, const uint64_t* z, const uint64_t* proof_xy,
                        const int* proof_inf, int flags, int* ok) {
  return shp_verify_host(ctx, commits_xy, commit_inf, n_commits, commit_index, points, n_points, set_point_start,
                         set_points, n_set_points, claim_start, n_sets, ys, n_values, weights, count, z, proof_xy,
                         proof_inf, flags, false, 0, ok);
}

int kzgx_shplonk_verify_checked(kzgx_ctx* ctx, const uint64_t* commits_xy, const int* commit_inf, size_t n_commits,
                                const uint32_t* commit_index, const uint64_t* points, size_t n_points,
                                const uint32_t* set_point_start, const uint32_t* set_points, size_t n_set_points,
                                const uint32_t* claim_start, size_t n_sets, const uint64_t* ys, size_t n_values,
                                const uint64_t* weights, size_t count, const uint64_t* z, const uint64_t* proof_xy,
                                const int* proof_inf, int flags, int subgroup, int* ok) {
  return shp_verify_host(ctx, commits_xy, commit_inf, n_commits, commit_index, points, n_points, set_point_start,
                         set_points, n_set_points, claim_start, n_sets, ys, n_values, weights, count, z, proof_xy,
                         proof_inf, flags, true, subgroup, ok);
}

}  // extern "C"

namespace {
// Once both SRS halves are present (the end of trusted_setup(int) or of a
// setup-file load): the verify tables (kzgx_verify_proof's [y]G table and the
// line tables of G2[0], G2[1]) and the call workspaces are made here, so the
// first commit / proof / verify on a new setup pays no allocation or table
// build (the reference's benchmark times each first call,
// benchmark/benchmark.cpp:40-66).  KZGX_LAZY_SETUP=1 leaves them to first use.
int setup_finish(kzgx_ctx* ctx) {
  static const bool lazy = kzgx::env_is_1("KZGX_LAZY_SETUP");
  if (lazy || ctx->c.n_srs == 0 || ctx->n_srs2 < 2) return KZGX_OK;
  hipStream_t st = ctx->c.stream;
  kzgx::GenTables g;
  KZGX_TRY(kzgx::gen_tables_get(ctx->c.curve, ctx->c.device, st, &g));
  KZGX_TRY(kzgx::dev_alloc(&ctx->c, (void**)&ctx->d_vw, kzgx::verify_wave_bytes(ctx->c.curve), &ctx->vw_b));
  KZGX_TRY(kzgx::verify_wave_prepare(&ctx->c, ctx->d_srs_canon, ctx->d_srs2_canon, g.g1_comb, ctx->d_vw, st));
  // staging of the host-pointer calls, sized for degree-4096 single calls
  KZGX_TRY(pin_stage(ctx, (size_t)1 << 20));
  void* d;
  for (int s = 0; s < 4; s++) KZGX_TRY(stage(ctx, s, (size_t)256 << 10, &d));
  KZGX_TRY_HIP(hipStreamSynchronize(st));
  ctx->vw_ready = true;
  // the multi-point verify's workspaces at the reference benchmark's largest
  // opening count (4096 points, benchmark/benchmark.cpp:85-99)
  {
    const size_t nv = std::min<size_t>(ctx->n_srs2 - 1, 4096);
    const size_t p1 = point_words(ctx) * 4, fb = 6 * p1;
    const size_t o_o = 3 * nv * 32 + (nv + 1) * 32 + 6 * p1 + 4 * 2 * p1 + 64;
    KZGX_TRY(stage(ctx, 3, ((o_o + 2 * fb + 255) & ~(size_t)255) + kzgx::pair2_wave_scratch_bytes(ctx->c.curve), &d));
    KZGX_TRY(kzgx::verify_ws_reserve(&ctx->c, nv));
  }
  // the single-call workspaces (quotient, latency partials, arrival
  // counters, Pippenger buffers): one zero proof at the largest default
  // degree and one at degree 128 size them
  const size_t nmax = std::min<size_t>(ctx->c.n_srs, 4097);
  std::vector<uint64_t> zc(4 * nmax, 0), zz(4, 0), xy(2 * point_words(ctx), 0), y(4, 0);
  int inf = 0;
  for (size_t n : {nmax, std::min<size_t>(nmax, 129)}) {
    KZGX_TRY(kzgx_prove_single_batch(ctx, zc.data(), n, 0, zz.data(), 1, xy.data(), &inf, y.data()));
    KZGX_TRY(kzgx_msm_g1(ctx, zc.data(), n, xy.data(), &inf));
  }
  return KZGX_OK;
}
}  // namespace

// Debug only (not part of include/kzg_gpu.h): copy a Pippenger workspace
// buffer of the context's default stream to the host, after a device sync.
// Looks the workspace up without binding or refreshing one.
extern "C" int kzgx_debug_ws_read(kzgx_ctx* ctx, const char* name, void* host, size_t bytes) {
  KZGX_TRY(activate(ctx));
  kzgx::MsmWs* w = ctx->c.ws_find(ctx->c.stream);
  if (!w || !name || !host) return KZGX_ERR_ARG;
  const void* src = nullptr;
  size_t cap = 0;
  const std::string s(name);
  if (s == "offsets") src = w->offsets, cap = w->offsets_b;
  else if (s == "entries") src = w->entries, cap = w->entries_b;
  else if (s == "bsum") src = w->bsum, cap = w->bsum_b;
  else if (s == "sstate") src = w->sstate, cap = w->sstate_b;
  else if (s == "tailk") src = w->tailk, cap = w->tailk_b;
  else if (s == "heads") src = w->heads, cap = w->heads_b;
  else if (s == "tails") src = w->tails, cap = w->tails_b;
  else if (s == "counts") src = w->counts, cap = w->counts_b;
  else if (s == "cursors") src = w->cursors, cap = w->cursors_b;
  else if (s == "gmeta") src = w->gmeta, cap = w->gmeta_b;
  else if (s == "gpart") src = w->gpart, cap = w->gpart_b;
  else if (s == "q") src = w->q, cap = w->q_b;
  if (!src || bytes > cap) return KZGX_ERR_ARG;
  KZGX_TRY_HIP(hipDeviceSynchronize());
  KZGX_TRY_HIP(hipMemcpy(host, src, bytes, hipMemcpyDeviceToHost));
  return KZGX_OK;
}

// debug: single-lane dependent-chain latency of one primitive (msm_fixed.hip
// k_debug_latency); res[0] = ns per operation, res[1] = core clocks
extern "C" int kzgx_debug_latency(kzgx_ctx* ctx, int op, unsigned iters, double* res) {
  KZGX_TRY(activate(ctx));
  if (!res) return KZGX_ERR_ARG;
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  return kzgx::debug_latency(&ctx->c, op, iters, res);
}

// debug: latency of one wave-wide Fp12 op of the verify path
// (verify_wave.hip k_vw_bench): res[0] = ns per op, res[1] = core clocks
namespace kzgx {
int coop_selftest(int curve, const uint32_t* d_tab, uint32_t n_pts, uint32_t* d_bad, hipStream_t st);  // latency.hip
}
// coop.hpp's cooperative point operations against the lone-lane forms on the
// loaded SRS (window 0 of the Pippenger table); *bad = bit mask of failing cases
extern "C" int kzgx_debug_coop_test(kzgx_ctx* ctx, unsigned* bad) {
  KZGX_TRY(activate(ctx));
  if (!bad || ctx->c.n_srs < 3) return KZGX_ERR_ARG;
  uint32_t* d_bad = nullptr;
  KZGX_TRY_HIP(hipMalloc((void**)&d_bad, 4));
  int rc = hipMemsetAsync(d_bad, 0, 4, ctx->c.stream) == hipSuccess ? KZGX_OK : KZGX_ERR_HIP;
  if (rc == KZGX_OK)
    rc = kzgx::coop_selftest(ctx->c.curve, ctx->c.d_table, (uint32_t)(ctx->c.n_srs < 3 * 4096 ? ctx->c.n_srs : 3 * 4096),
                             d_bad, ctx->c.stream);
  if (rc == KZGX_OK && hipMemcpyAsync(bad, d_bad, 4, hipMemcpyDeviceToHost, ctx->c.stream) != hipSuccess) rc = KZGX_ERR_HIP;
  if (rc == KZGX_OK && hipStreamSynchronize(ctx->c.stream) != hipSuccess) rc = KZGX_ERR_HIP;
  (void)hipFree(d_bad);
  return rc;
}

namespace kzgx {
int prim_selftest(int curve, int op, int mode, const uint32_t* in, size_t count, uint32_t* out, hipStream_t st);  // selftest.hip
}
// debug: one field / point primitive (selftest.hip PrimOp) on `count` tuples of
// raw limbs at `in`, the raw limbs of every result to `out`; `mode` picks the
// active lanes of the wave-uniform forms (0 = all, 1 = lanes 0-3, 2 = lane 0)
extern "C" int kzgx_debug_prim(kzgx_ctx* ctx, int op, int mode, const uint32_t* in, size_t count, uint32_t* out) {
  KZGX_TRY(activate(ctx));
  return kzgx::prim_selftest(ctx->c.curve, op, mode, in, count, out, ctx->c.stream);
}

// debug: the block table's endomorphism split of `count` scalars (8 words
// each, any 256-bit value) as the index pass forms it, 9 words per scalar to
// `out`: |k1| (4 words), |k2| (4 words), sign bits (bit 0: k1 < 0, bit 1: k2 < 0)
extern "C" int kzgx_debug_joint_glv(kzgx_ctx* ctx, const uint32_t* scalars, size_t count, uint32_t* out) {
  KZGX_TRY(activate(ctx));
  return kzgx::joint_glv_debug(&ctx->c, scalars, count, out);
}

extern "C" int kzgx_debug_vw_bench(kzgx_ctx* ctx, int op, unsigned iters, double* res) {
  KZGX_TRY(activate(ctx));
  if (!res || iters == 0) return KZGX_ERR_ARG;
  KZGX_TRY_HIP(hipStreamSynchronize(ctx->c.stream));
  return kzgx::vw_bench(ctx->c.curve, op, iters, &res[0], &res[1], ctx->c.stream);
}
