// k_subwave_slots.hip - K slots per launch of the sub-wave step (step_subwave_slots.hpp): N <= 8, 4 or 8 lanes per env,
// handles pinned to DIRAL_PATH_SUBWAVE with DIRAL_OPT_SUBWAVE_SLOTS.  The slot's phases are the one-slot kernel's
// (step_subwave.hpp); a translation unit of its own, so that the two kernels compile in parallel.
#include "launch.hpp"
#include "step_subwave_slots.hpp"

namespace diral {
namespace {
// G lanes per env; by out dtype and memory block (PolParams::mem_on: the MEM instantiations - the slots write rows of the caller's replay rings)
template <int G>
struct LaunchSubSlots {
  const StepParams& p; const PolParams& q; hipStream_t s;
  template <bool OUT64, bool MEM>
  void operator()(std::integer_sequence<bool, OUT64, MEM>) const {
    const unsigned int grid = (unsigned int)((p.B + kSubwaveThreads / G - 1) / (kSubwaveThreads / G));   // kSubwaveThreads / G envs per block
    hipLaunchKernelGGL((step_subwave_slots_kernel<G, OUT64, MEM>), dim3(grid), dim3(kSubwaveThreads), 0, s, p, q);
  }
};
}  // namespace

hipError_t launch_subwave_slots(const StepParams& p, const PolParams& q, hipStream_t s) {
  if (p.N < 1 || p.N > DIRAL_SUBWAVE_MAX_USERS || p.A < 1 || p.A > DIRAL_SUBWAVE_MAX_CHANNELS || p.K > DIRAL_SMALL_MAX_BINS ||
      p.B < 1 || q.K < 1)
    return hipErrorInvalidValue;                  // (diral_env_subwave_ok refuses these before a handle is pinned)
  if (q.prefill ? q.actions_out == nullptr : (q.rollout == 0 || q.actions_seq == nullptr)) return hipErrorInvalidValue;
  if (p.N <= 4) bool_dispatch(LaunchSubSlots<4>{p, q, s}, std::integer_sequence<bool>{}, p.out_f64 != 0, q.mem_on != 0);
  else bool_dispatch(LaunchSubSlots<8>{p, q, s}, std::integer_sequence<bool>{}, p.out_f64 != 0, q.mem_on != 0);
  return hipGetLastError();
}
}  // namespace diral
