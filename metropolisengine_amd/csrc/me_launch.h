// The two per-device facts a host launcher asks for (me_per_device.h: per DEVICE of the process, not per process): a
// kernel's raised dynamic-LDS limit and the CU count.
#pragma once

#include <hip/hip_runtime.h>

#include "me_per_device.h"

namespace me {

// Allow `Kernel` dynamic LDS up to `bytes` (above 64 KiB a launch needs the function attribute) on the current device:
// set once per device and kernel instantiation, the runtime's answer handed out from then on.
template <auto Kernel>
inline hipError_t raise_lds_limit(size_t bytes) {
  static PerDevice<hipError_t> cache;
  int device = 0;
  if (hipError_t rc = hipGetDevice(&device); rc != hipSuccess) return rc;
  return cache.get(device, [bytes] {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  });
}

// compute units of `device`; 256 (an MI355X) where the query fails
inline int cu_count(int device) {
  static PerDevice<int> cache;
  return cache.get(device, [device] {
    int count = 0;
    if (hipDeviceGetAttribute(&count, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || count <= 0) return 256;
    return count;
  });
}
// ... of the current device
inline int cu_count() {
  int device = 0;
  return hipGetDevice(&device) == hipSuccess ? cu_count(device) : 256;
}

}  // namespace me
