// jellyfish_amd/csrc/hip_launch.hpp -- the one launch entry for kernels that take dynamic LDS (host only; DESIGN.md, "Launches").
// A kernel's limit (hipFuncAttributeMaxDynamicSharedMemorySize) is raised by its launch: per device, only upwards, and to what
// the launch asks for, so there is no list of instantiations and sizes to keep in step with the launch sites.
// Included by jfgpu.hip after HIP_TRY and fail(): launch_lds returns the JFGPU_* code HIP_TRY would, and launches nothing then.
// It adds no synchronisation; what the launch itself reports stays with the caller's hipGetLastError.
#pragma once
#include <map>
#include <mutex>
#include <utility>

// The largest limit set so far for (device, kernel), 0 before the first launch: every kernel with dynamic LDS gets the
// attribute at least once.  The ABI is called from several threads with different handles, hence the mutex, held over the
// call so that a smaller request cannot land after a larger one.
static int raise_lds_limit(const void* kern, size_t lds) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, size_t> limit;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  size_t& have = limit[std::make_pair(dev, kern)];
  if(lds <= have) return JFGPU_OK;
  HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  have = lds;
  return JFGPU_OK;
}

// hipLaunchKernelGGL for a launch whose LDS argument is not the literal 0 (the handle's device is current: use()).
template <class... P, class... A>
int launch_lds(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A&... args) {
  if(lds) { const int rc = raise_lds_limit((const void*)kern, lds); if(rc) return rc; }
  hipLaunchKernelGGL(kern, grid, block, lds, stream, args...);
  return JFGPU_OK;
}
