// k_subwave_slots.hip - K slots per launch of the sub-wave step (step_subwave_slots.hpp): N <= 8, 4 or 8 lanes per env,
// handles pinned to DIRAL_PATH_SUBWAVE with DIRAL_OPT_SUBWAVE_SLOTS.  The slot's phases are the one-slot kernel's
// (step_subwave.hpp); a translation unit of its own, so that the two kernels compile in parallel.
#include "launch.hpp"
#include "step_subwave_slots.hpp"

namespace diral {
namespace {
template <int G, bool OUT64>
hipError_t launch_sub_slots(const StepParams& p, const PolParams& q, hipStream_t s) {
  constexpr int kEnvsPerBlock = kSubwaveThreads / G;
  const unsigned int grid = (unsigned int)((p.B + kEnvsPerBlock - 1) / kEnvsPerBlock);
  // (the memory block, PolParams::mem_on: the MEM instantiations - the slots write rows of the caller's replay rings)
  if (q.mem_on) hipLaunchKernelGGL((step_subwave_slots_kernel<G, OUT64, true>), dim3(grid), dim3(kSubwaveThreads), 0, s, p, q);
  else hipLaunchKernelGGL((step_subwave_slots_kernel<G, OUT64, false>), dim3(grid), dim3(kSubwaveThreads), 0, s, p, q);
  return hipGetLastError();
}
}  // namespace

hipError_t launch_subwave_slots(const StepParams& p, const PolParams& q, hipStream_t s) {
  if (p.N < 1 || p.N > DIRAL_SUBWAVE_MAX_USERS || p.A < 1 || p.A > DIRAL_SUBWAVE_MAX_CHANNELS || p.K > DIRAL_SMALL_MAX_BINS ||
      p.B < 1 || q.K < 1)
    return hipErrorInvalidValue;                  // (diral_env_subwave_ok refuses these before a handle is pinned)
  if (q.prefill ? q.actions_out == nullptr : (q.rollout == 0 || q.actions_seq == nullptr)) return hipErrorInvalidValue;
  if (p.N <= 4) return p.out_f64 ? launch_sub_slots<4, true>(p, q, s) : launch_sub_slots<4, false>(p, q, s);
  return p.out_f64 ? launch_sub_slots<8, true>(p, q, s) : launch_sub_slots<8, false>(p, q, s);
}
}  // namespace diral
