// tests/host/launch_check.cc -- TEST INFRASTRUCTURE: the one launch entry for kernels with dynamic LDS
// (jellyfish_amd/csrc/hip_launch.hpp) under the host emulation, which records every hipFuncSetAttribute and aborts a launch
// that asks for more than 64 KiB from a function whose limit was not raised.  A stand-alone program, built by
// tests/test_launch_emu.py with AddressSanitizer + UBSan and again with ThreadSanitizer, run as a plain child process.
//   launch_check            cases (a) - (f), prints "launch_check: ok"
// Under ThreadSanitizer the launches have an empty grid: the emulator's work-items are fibers on hand-switched stacks, which
// that tool does not follow; the limits, the call count and the locking under test are the same.
//   launch_check direct     case (g): a direct hipLaunchKernelGGL at 65 KiB with no attribute -- the emulator aborts
#include <hip/hip_runtime.h>
#include <algorithm>
#include <string>
#include <thread>
#include "../../include/jfgpu.h"

namespace {
thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if(e_ != hipSuccess) return fail(JFGPU_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while(0)
}  // namespace
#include "../../jellyfish_amd/csrc/hip_launch.hpp"

namespace {

// writes the first byte of its dynamic LDS and adds one to *n per block: the launch really ran
__global__ void first_kernel(unsigned long long* n) { hip_emu::dyn_lds()[0] = 1; if(threadIdx.x == 0) atomicAdd(n, 1ull); }
__global__ void second_kernel(unsigned long long* n, int by) { if(threadIdx.x == 0) atomicAdd(n, (unsigned long long)by); }

#ifdef __SANITIZE_THREAD__
constexpr unsigned kRun = 0;
#else
constexpr unsigned kRun = 1;
#endif
int failures = 0;
#define CHECK(cond) do { if(!(cond)) { fprintf(stderr, "launch_check: line %d: %s\n", __LINE__, #cond); ++failures; } } while(0)

const void* fn1() { return (const void*)first_kernel; }
const void* fn2() { return (const void*)second_kernel; }

}  // namespace

int main(int argc, char** argv) {
  unsigned long long* n = nullptr;
  if(hipMalloc(&n, sizeof *n) != hipSuccess) return 2;
  *n = 0;
  if(argc > 1 && std::string(argv[1]) == "direct") {                  // (g)
    hipLaunchKernelGGL(first_kernel, dim3(1), dim3(64), 65 << 10, nullptr, n);
    printf("launch_check: the direct launch was not refused\n");
    return 0;
  }
  using hip_emu::func_attr_calls; using hip_emu::func_lds_limit;
  const size_t L = 70 << 10;
  // (a) first launch at L: one call, with value L
  CHECK(launch_lds(first_kernel, dim3(2 * kRun), dim3(64), L, nullptr, n) == JFGPU_OK);
  CHECK(func_attr_calls() == 1 && func_lds_limit(fn1()) == L && *n == kRun * 2);
  // (b) the same kernel at <= L: no call
  CHECK(launch_lds(first_kernel, dim3(kRun), dim3(64), L, nullptr, n) == JFGPU_OK);
  CHECK(launch_lds(first_kernel, dim3(kRun), dim3(64), 1024, nullptr, n) == JFGPU_OK);
  CHECK(func_attr_calls() == 1 && func_lds_limit(fn1()) == L && *n == kRun * 4);
  // (c) the same kernel at a larger size: one call, the limit is the larger value
  CHECK(launch_lds(first_kernel, dim3(kRun), dim3(64), 2 * L, nullptr, n) == JFGPU_OK);
  CHECK(func_attr_calls() == 2 && func_lds_limit(fn1()) == 2 * L && *n == kRun * 5);
  // (d) a second kernel: independent of the first (a small size is set as well: the recorded value starts at 0)
  CHECK(func_lds_limit(fn2()) == 0);
  CHECK(launch_lds(second_kernel, dim3(kRun), dim3(64), 512, nullptr, n, 10) == JFGPU_OK);
  CHECK(func_attr_calls() == 3 && func_lds_limit(fn2()) == 512 && func_lds_limit(fn1()) == 2 * L && *n == kRun * 15);
  CHECK(launch_lds(second_kernel, dim3(kRun), dim3(64), 512, nullptr, n, 10) == JFGPU_OK);
  CHECK(func_attr_calls() == 3 && *n == kRun * 25);
  // (e) lds == 0: no call
  CHECK(launch_lds(second_kernel, dim3(kRun), dim3(64), 0, nullptr, n, 5) == JFGPU_OK);
  CHECK(func_attr_calls() == 3 && func_lds_limit(fn2()) == 512 && *n == kRun * 30);
  // (f) eight threads launch one kernel at mixed sizes: the limit ends at the largest, every launch ran, every call raised it
  {
    const long before = func_attr_calls();
    size_t top = 0;
    for(int i = 0; i < 8; ++i) for(int r = 0; r < 40; ++r) top = std::max(top, ((size_t)((i * 7 + r * 13) % 150) + 1) << 10);
    std::thread th[8];
    int bad[8] = {0};
    for(int i = 0; i < 8; ++i) th[i] = std::thread([&, i] {
      for(int r = 0; r < 40; ++r) {
        const size_t lds = ((size_t)((i * 7 + r * 13) % 150) + 1) << 10;      // 1 .. 150 KiB
        if(launch_lds(second_kernel, dim3(kRun), dim3(64), lds, nullptr, n, 1) != JFGPU_OK) ++bad[i];
        if(func_lds_limit(fn2()) < lds) ++bad[i];                               // never below what this thread has launched with
      }
    });
    for(auto& t : th) t.join();
    for(int b : bad) CHECK(b == 0);
    CHECK(func_lds_limit(fn2()) == top && *n == kRun * (30 + 8 * 40));
    const long calls = func_attr_calls() - before;
    CHECK(calls >= 1 && calls <= 150);                                          // only upwards: at most one call per distinct size
  }
  (void)hipFree(n);
  if(failures) return 1;
  printf("launch_check: ok\n");
  return 0;
}
