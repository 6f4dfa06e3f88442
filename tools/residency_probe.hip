// Residency probe (diagnostic, tools/gpu_residency.py): how many one-wave workgroups with N bytes of static LDS does one CU hold at a time?
// The compiler's occupancy remark does not say (it reports waves per SIMD from the registers) and the LDS allocation granule is not
// documented, so the device is asked: every workgroup finds its CU from the hardware id registers, raises that CU's counter on entry,
// records the counter's maximum, waits a bounded time so that the CU fills up, and lowers the counter on exit.
// Not part of the product library: built on its own by the tool, never loaded by the package, the tests or bench.py.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PROBE_KEYS 2048                 // (XCC_ID, 4 bits) << 8 | HW_ID[15:8] (CU_ID 11:8, SH_ID 12, SE_ID 15:13), of which 3 + 8 bits are used
#define PROBE_MAX_SLEEPS (1 << 14)      // second bound of the wait, should the clock not advance: 16 384 x s_sleep 64 (~2 us each)
#define HWREG(id, offset, size) ((id) | ((offset) << 6) | (((size) - 1) << 11))   // simm16 of s_getreg_b32
#define HWREG_HW_ID 4
#define HWREG_XCC_ID 20

template <int N>
__global__ __launch_bounds__(64) void residency_probe(unsigned* cur, unsigned* peak, unsigned* sink, unsigned long long ticks) {
  __shared__ unsigned pad[N / 4];
  const int lane = threadIdx.x;
  pad[(lane * 61 + blockIdx.x) % (N / 4)] = blockIdx.x;   // (the allocation is what is measured; touched so that it stays)
  const unsigned cu = __builtin_amdgcn_s_getreg(HWREG(HWREG_HW_ID, 8, 8));
  const unsigned xcc = __builtin_amdgcn_s_getreg(HWREG(HWREG_XCC_ID, 0, 4)) & 7u;
  const unsigned key = (xcc << 8) | cu;
  if (lane == 0) {
    const unsigned n = atomicAdd(&cur[key], 1u) + 1u;
    atomicMax(&peak[key], n);
    // the wait: bounded by the 100 MHz wall clock and by the iteration count; the other 63 lanes idle behind lane 0
    const unsigned long long t0 = wall_clock64();
    for (int it = 0; it < PROBE_MAX_SLEEPS && wall_clock64() - t0 < ticks; it++) __builtin_amdgcn_s_sleep(64);
    atomicSub(&cur[key], 1u);
  }
  if (pad[lane] == 0xffffffffu) sink[0] = 1u;
}

#define PROBE_SIZES(X) X(8192) X(12288) X(12688) X(12800) X(13312) X(13584) X(13824) X(14080) X(14848) X(16384)

static const char* g_err = "";
extern "C" const char* residency_last_error() { return g_err; }
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { g_err = hipGetErrorString(e_); return -1; } } while (0)

extern "C" int residency_sizes(int* out, int cap) {
  int n = 0;
#define X(N) if (n < cap) out[n] = N; n++;
  PROBE_SIZES(X)
#undef X
  return n;
}

// One launch of `nblocks` one-wave workgroups with `nbytes` of static LDS, each waiting `wait_us`; peak[PROBE_KEYS] (host memory) gets
// the largest number of workgroups seen at once on every CU (0: key not seen).  Returns 0, -1 on a HIP error, -2 on an unknown size.
extern "C" int residency_probe_run(int nbytes, int nblocks, double wait_us, unsigned* peak_host, float* ms_out) {
  if (wait_us < 0.0 || wait_us > 500.0 || nblocks < 1 || nblocks > (1 << 16)) { g_err = "wait_us in [0, 500], nblocks in [1, 65536]"; return -2; }
  unsigned *cur = nullptr, *peak = nullptr, *sink = nullptr;
  CHECK(hipMalloc(&cur, PROBE_KEYS * sizeof(unsigned)));
  CHECK(hipMalloc(&peak, PROBE_KEYS * sizeof(unsigned)));
  CHECK(hipMalloc(&sink, sizeof(unsigned)));
  CHECK(hipMemset(cur, 0, PROBE_KEYS * sizeof(unsigned)));
  CHECK(hipMemset(peak, 0, PROBE_KEYS * sizeof(unsigned)));
  CHECK(hipMemset(sink, 0, sizeof(unsigned)));
  const unsigned long long ticks = (unsigned long long)(wait_us * 100.0);   // wall_clock64 counts at 100 MHz
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  CHECK(hipEventRecord(e0, 0));
  bool known = false;
#define X(N) if (nbytes == N) { known = true; residency_probe<N><<<nblocks, 64, 0, 0>>>(cur, peak, sink, ticks); }
  PROBE_SIZES(X)
#undef X
  if (!known) { g_err = "no probe kernel of that LDS size (residency_sizes lists them)"; return -2; }
  CHECK(hipGetLastError());
  CHECK(hipEventRecord(e1, 0));
  CHECK(hipEventSynchronize(e1));
  if (ms_out) CHECK(hipEventElapsedTime(ms_out, e0, e1));
  CHECK(hipMemcpy(peak_host, peak, PROBE_KEYS * sizeof(unsigned), hipMemcpyDeviceToHost));
  CHECK(hipEventDestroy(e0)); CHECK(hipEventDestroy(e1));
  CHECK(hipFree(cur)); CHECK(hipFree(peak)); CHECK(hipFree(sink));
  return 0;
}

// What the runtime's occupancy calculator says for a kernel of another library (its handle: dlsym of the kernel's mangled name).
extern "C" int residency_occupancy(const void* kernel, int block, size_t dynamic_lds, int* blocks_per_cu) {
  CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, kernel, block, dynamic_lds));
  return 0;
}

extern "C" int residency_device(int* cus, int* lds_per_cu, int* lds_per_block) {
  hipDeviceProp_t p;
  CHECK(hipGetDeviceProperties(&p, 0));
  *cus = p.multiProcessorCount; *lds_per_cu = (int)p.maxSharedMemoryPerMultiProcessor; *lds_per_block = (int)p.sharedMemPerBlock;
  return 0;
}
