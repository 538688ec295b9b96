// device.h -- what the launch planners ask the current device.
#pragma once
#include <hip/hip_runtime.h>

namespace tdnnf {

constexpr int kMaxDevices = 64;  // per-device state (the cache below, chain_den.hip's) is an array of this many

// Compute units of the current device, asked once per device (a process may drive several); -1 when the device does not say.
inline int device_cus_known() {
  static int cus_of[kMaxDevices];  // 0: not asked yet
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return -1;
  if (cus_of[dev] == 0) {
    hipDeviceProp_t prop;
    cus_of[dev] = hipGetDeviceProperties(&prop, dev) == hipSuccess ? prop.multiProcessorCount : -1;
    (void)hipGetLastError();
  }
  return cus_of[dev];
}
// the same for planners that must come up with a grid anyway: an MI355X's 256 when the device does not say
inline int device_cus() {
  const int cus = device_cus_known();
  return cus > 0 ? cus : 256;
}

// More than 64 KiB of dynamic LDS must be opted into, kernel by kernel.  A launch site does it once per instantiation:
//   static const bool opted = opt_in_lds(kernel<...>, bytes);
template <class Kernel>
bool opt_in_lds(Kernel *kernel, size_t bytes) {
  hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  return true;
}

}  // namespace tdnnf
