// v2v_launch.hpp -- host-side helpers the launchers share: the device's CU count and the dynamic-LDS limit of a kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

namespace v2v {

// CUs of the current device, cached per device; 256 when the query fails
inline int device_cus()
{
    static std::atomic<int> cached[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    int v = cached[dev].load(std::memory_order_relaxed);
    if (!v) {
        int cus = 0;
        v = (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) ? cus : 256;
        cached[dev].store(v, std::memory_order_relaxed);       // every thread computes the same value
    }
    return v;
}

// Dynamic LDS above the 64 KB a kernel gets by default: raise the kernel's limit once per device.  Kept out of the launch path so
// that a step (or a layer) captures into a hipGraph as a bare kernel node.  `raised` is the caller's static flag array of that kernel
// instance; the attribute call is idempotent (a benign repeat, but no data race), and an unknown device or one past the array sets it
// on every call.
inline hipError_t ensure_dynamic_lds(const void *kernel, int bytes, std::atomic<bool> (&raised)[64])
{
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;
    const bool known = dev >= 0 && dev < 64;
    if (known && raised[dev].load(std::memory_order_acquire)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && known) raised[dev].store(true, std::memory_order_release);
    return e;
}

}  // namespace v2v
