// Residency probe: how many one-wave workgroups a CU really holds at a given
// (unused) dynamic-LDS size, beside what the occupancy query answers -- the
// mechanism of the block table accumulation's residency reserve
// (msm_joint.hip).  Every workgroup spins for 200 us and stamps its start and
// end; the peak of workgroups in flight over the CU count is the residency.
// (At sizes that admit more than ~20 workgroups per CU the grid drains before
// the peak is reached.)  Output: profiles/accum_reserve_probe.txt.
//
//   hipcc -O2 --offload-arch=gfx950 scripts/probe_residency.hip -o scripts/probe_residency
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                                  \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      std::printf("error %s line %d\n", hipGetErrorString(e_), __LINE__);      \
      std::exit(1);                                                            \
    }                                                                          \
  } while (0)

__global__ __launch_bounds__(64) void k_spin(unsigned long long* out, unsigned long long ticks) {
  const unsigned long long t0 = wall_clock64();
  unsigned long long t1 = t0;
  for (int i = 0; i < 1000000 && t1 - t0 < ticks; i++) t1 = wall_clock64();
  if (threadIdx.x == 0) {
    out[2 * (size_t)blockIdx.x] = t0;
    out[2 * (size_t)blockIdx.x + 1] = t1;
  }
}

int main() {
  CK(hipSetDevice(0));
  hipDeviceProp_t p;
  CK(hipGetDeviceProperties(&p, 0));
  std::printf("CUs %d sharedMemPerBlock %zu sharedMemPerMultiprocessor %zu maxSharedMemoryPerMultiProcessor %zu\n",
              p.multiProcessorCount, p.sharedMemPerBlock, p.sharedMemPerMultiprocessor,
              p.maxSharedMemoryPerMultiProcessor);
  const int cus = p.multiProcessorCount;
  const unsigned grid = (unsigned)cus * 40;
  unsigned long long* d = nullptr;
  CK(hipMalloc((void**)&d, (size_t)grid * 16));
  std::vector<unsigned long long> h(2 * (size_t)grid);
  const size_t sizes[] = {0,     5120,  5632,  6144,  11776, 12288, 12800, 13312, 13824,
                          14080, 14336, 14848, 15360, 16384, 20480, 32768, 65536};
  for (size_t s : sizes) {
    int q = -1;
    CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, k_spin, 64, s));
    CK(hipMemset(d, 0, (size_t)grid * 16));
    hipLaunchKernelGGL(k_spin, dim3(grid), dim3(64), s, 0, d, 20000ull);  // 200 us at 100 MHz
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(h.data(), d, (size_t)grid * 16, hipMemcpyDeviceToHost));
    std::vector<std::pair<unsigned long long, int>> ev;
    for (unsigned i = 0; i < grid; i++) {
      ev.push_back({h[2 * i], +1});
      ev.push_back({h[2 * i + 1], -1});
    }
    std::sort(ev.begin(), ev.end());
    int cur = 0, peak = 0;
    for (auto& e : ev) {
      cur += e.second;
      peak = std::max(peak, cur);
    }
    std::printf("lds %6zu query %3d peak_resident %6d per_cu %.2f\n", s, q, peak, (double)peak / cus);
    std::fflush(stdout);
  }
  CK(hipFree(d));
  return 0;
}
