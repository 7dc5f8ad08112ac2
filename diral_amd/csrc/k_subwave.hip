// k_subwave.hip - the sub-wave step kernel (step_subwave.hpp): N <= 8, 4 or 8 lanes per env, DIRAL_PATH_SUBWAVE only.  That
// header also holds the slot's phases for the K-slot kernel of k_subwave_slots.hip.
#include "launch.hpp"
#include "step_subwave.hpp"

namespace diral {
namespace {
template <int G, bool OUT64>
hipError_t launch_sub(const StepParams& p, hipStream_t s) {
  constexpr int kEnvsPerBlock = kSubwaveThreads / G;
  const unsigned int grid = (unsigned int)((p.B + kEnvsPerBlock - 1) / kEnvsPerBlock);
  hipLaunchKernelGGL((step_subwave_kernel<G, OUT64>), dim3(grid), dim3(kSubwaveThreads), 0, s, p);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_subwave(const StepParams& p, hipStream_t s) {
  if (p.N < 1 || p.N > DIRAL_SUBWAVE_MAX_USERS || p.A < 1 || p.A > DIRAL_SUBWAVE_MAX_CHANNELS || p.K > DIRAL_SMALL_MAX_BINS ||
      p.B < 1)
    return hipErrorInvalidValue;                  // (diral_env_subwave_ok refuses these before a handle is pinned)
  if (p.N <= 4) return p.out_f64 ? launch_sub<4, true>(p, s) : launch_sub<4, false>(p, s);
  return p.out_f64 ? launch_sub<8, true>(p, s) : launch_sub<8, false>(p, s);
}
}  // namespace diral
