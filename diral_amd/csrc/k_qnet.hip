// k_qnet.hip - qnet_forward_kernel (the dense Q-network chain, qnet_kernel.hpp) and its launcher.
#include "qnet_kernel.hpp"

namespace diral {

hipError_t launch_qnet(const QnetParams& p, hipStream_t s) {
  const uint32_t grid = (uint32_t)(((long long)p.rows + kQnetRows - 1) / kQnetRows);
  hipLaunchKernelGGL(qnet_forward_kernel, dim3(grid), dim3(kQnetThreads), 0, s, p);
  return hipGetLastError();
}

}  // namespace diral
