// host_util.hpp - what the two host units (diral_env.hip: the env handle; diral_agent.hip: the handle-free entry points)
// both use: the status of a handle-less call, the device guard, and the launch and dispatch helpers.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "common.hpp"

namespace diral {

inline int hip_status(hipError_t st) { return st == hipSuccess ? DIRAL_OK : DIRAL_ERR_HIP; }   // the handle-less entry points

// The handle-less entry points (diral_sps_*, diral_driver_shape, ...) take device pointers only: they run on the
// device that owns `p` (their first mandatory buffer), whatever device is current in the calling thread.
inline int device_of_ptr(const void* p) {
  hipPointerAttribute_t a;
  if (p && hipPointerGetAttributes(&a, p) == hipSuccess) return a.device;
  (void)hipGetLastError();
  return -1;
}

// Every entry point that touches the device runs with the handle's device current - or the device that owns a buffer -
// and restores the caller's (torch's) current device afterwards.
struct DeviceGuard {
  int prev = -1, dev;
  bool ok = true;
  explicit DeviceGuard(int d) : dev(d) {
    if (dev < 0) return;                                        // not a device allocation HIP knows: current device
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = (hipSetDevice(dev) == hipSuccess);
  }
  explicit DeviceGuard(const void* p) : DeviceGuard(device_of_ptr(p)) {}
  ~DeviceGuard() { if (dev >= 0 && prev >= 0 && prev != dev) (void)hipSetDevice(prev); }
};
#define DEVICE_ENTER(owner) \
  DeviceGuard guard(owner); \
  if (!guard.ok) return DIRAL_ERR_NO_DEVICE

inline int blocks(size_t total, int threads) { return (int)((total + threads - 1) / threads); }

// a launch and its status; launch_1d: one thread per item, in blocks of 256
template <auto Kernel, typename... Args>
hipError_t launch_k(dim3 grid, dim3 block, uint32_t lds, hipStream_t s, Args... args) {
  hipLaunchKernelGGL(Kernel, grid, block, lds, s, args...);
  return hipGetLastError();
}
template <auto Kernel, typename... Args>
hipError_t launch_1d(size_t total, hipStream_t s, Args... args) {
  return launch_k<Kernel>(dim3(blocks(total, 256)), dim3(256), 0, s, args...);
}
// run-time DIRAL_F32 / DIRAL_F64 -> the element type, handed to `f` as a value of it
template <typename F>
hipError_t by_dtype(int dtype, F&& f) { return dtype == DIRAL_F64 ? f(double{}) : f(float{}); }
template <typename F>
hipError_t by_vec(int vec, F&& f) {
  return vec == 4 ? f(std::integral_constant<int, 4>{}) : vec == 2 ? f(std::integral_constant<int, 2>{}) : f(std::integral_constant<int, 1>{});
}

}  // namespace diral
