// Host helpers of the launch paths: the device's CU count, and a kernel's dynamic-LDS limit set once per device.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

// Compute units of the calling thread's current device (looked up once per device), or 0 if the runtime cannot say:
// each caller keeps its own fallback and rounding.
inline int device_cu_count() {
  static std::atomic<int> known[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  int n = known[dev & 63].load(std::memory_order_relaxed);
  if (n > 0) return n;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) return 0;
  known[dev & 63].store(n, std::memory_order_relaxed);
  return n;
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) for a kernel on the calling thread's current device, once per device
// (the attribute is per device: a process that moves to another GPU sets it there too; two threads racing here only
// repeat an idempotent call).  One instance per launch site: `static LdsAttrOnce attr; attr(fn, bytes)`.
struct LdsAttrOnce {
  std::atomic<unsigned long long> done{0};
  hipError_t operator()(const void* fn, int bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
    return e;
  }
};
