// k_wide_slots.hip - step_wide_slots_kernel: K slots per launch of the wide step (64 < N <= 256) with the policy epilogue
// (diral_env_step_policy, DiralSlotPolicy::slots > 1), the body of step_wide_kernel compiled with DIRAL_WIDE_KSLOTS.  Only
// what the fused path serves is instantiated: my_step without the run-time extras, RICH output tail, both table forms.
#include "launch.hpp"
#include "step_wide.hpp"

namespace diral {
#define DIRAL_WIDE_KERNEL step_wide_slots_kernel
#define DIRAL_WIDE_KSLOTS 1
#include "step_wide_body.inc"
#undef DIRAL_WIDE_KSLOTS
#undef DIRAL_WIDE_KERNEL

namespace {
template <int V>
struct LaunchWideSlots {
  const FastParams& f; const RichParams& r; const PolParams& q; dim3 g; uint32_t lds; hipStream_t s;
  template <bool O, bool F, bool P>
  void operator()(std::integer_sequence<bool, O, F, P>) const {
    hipLaunchKernelGGL((step_wide_slots_kernel<V, O, F, false, false, true, P>), g, dim3(64 * wide_waves(V)), lds, s, f, r, q);
  }
};
template <int V>
struct AttrWideSlots {
  int lds, lds_packed; hipError_t* st;
  template <bool O, bool F, bool P>
  void operator()(std::integer_sequence<bool, O, F, P>) const {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(step_wide_slots_kernel<V, O, F, false, false, true, P>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, P ? lds_packed : lds);
    if (e != hipSuccess) *st = e;
  }
};
}  // namespace

// blocks = envs in batch order (B): no slow-first listing over K slots
hipError_t launch_wide_slots(const FastParams& f, const RichParams& r, const PolParams& q, const KernelSel& k, int vpl, int B,
                             hipStream_t s) {
  if (vpl == 2) {
    const LaunchWideSlots<2> l{f, r, q, dim3(B), wide_lds_layout(2, f.A, f.K, k.packed).total, s};
    bool_dispatch(l, std::integer_sequence<bool>{}, k.out64, k.full, k.packed);
  } else {
    const LaunchWideSlots<4> l{f, r, q, dim3(B), wide_lds_layout(4, f.A, f.K, k.packed).total, s};
    bool_dispatch(l, std::integer_sequence<bool>{}, k.out64, k.full, k.packed);
  }
  return hipGetLastError();
}

hipError_t set_attr_wide_slots(int vpl, int A, int K) {
  hipError_t st = hipSuccess;
  for (int m = 0; m < 8; ++m) {
    if (vpl == 2) {
      const AttrWideSlots<2> a{(int)wide_lds_layout(2, A, K, false).total, (int)wide_lds_layout(2, A, K, true).total, &st};
      bool_dispatch(a, std::integer_sequence<bool>{}, (m & 1) != 0, (m & 2) != 0, (m & 4) != 0);
    } else {
      const AttrWideSlots<4> a{(int)wide_lds_layout(4, A, K, false).total, (int)wide_lds_layout(4, A, K, true).total, &st};
      bool_dispatch(a, std::integer_sequence<bool>{}, (m & 1) != 0, (m & 2) != 0, (m & 4) != 0);
    }
  }
  return st;
}
}  // namespace diral
