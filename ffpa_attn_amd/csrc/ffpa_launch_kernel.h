// ffpa_launch_kernel.h — the one kernel launch of the attention kernels (included by the *_inst.hip translation units only): raise the kernel's dynamic LDS limit
// once per device, launch 256-lane workgroups, read the launch error.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

namespace ffpa {

// Returns 0, -1 (no current device), -2 (the LDS limit could not be raised) or the launch's hipError_t.  Keyed on the kernel ITSELF, not on its type: two kernels
// of one signature each keep their own per-device flags.
template <auto Kern, typename... Args>
static int launch_kernel(int total_wg, int lds_bytes, hipStream_t stream, const Args&... args) {
  static std::atomic<bool> attr_done[64];  // write-once per device (setting the attribute twice is harmless)
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  std::atomic<bool>* const done = (dev >= 0 && dev < 64) ? &attr_done[dev] : nullptr;
  if (done == nullptr || !done->load(std::memory_order_acquire)) {
    if (hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
      (void)hipGetLastError();
      return -2;
    }
    if (done != nullptr) done->store(true, std::memory_order_release);
  }
  hipLaunchKernelGGL(Kern, dim3((unsigned)total_wg), dim3(256), lds_bytes, stream, args...);
  return (int)hipGetLastError();
}

}  // namespace ffpa
