// k_fast64.hip - every instantiation of step_fast64_kernel and step_fast64_slots_kernel (N <= 64; one body, compiled twice) and their launchers.
#include "launch.hpp"
#include "step_fast64.hpp"

namespace diral {
#define DIRAL_FAST_KERNEL step_fast64_kernel
#include "step_fast64_body.inc"
#undef DIRAL_FAST_KERNEL
#define DIRAL_FAST_KERNEL step_fast64_slots_kernel
#define DIRAL_FAST_KSLOTS 1
#include "step_fast64_body.inc"
#undef DIRAL_FAST_KSLOTS
#undef DIRAL_FAST_KERNEL

namespace {
struct Fast64Args { const FastParams& f; const RichParams& r; const PolParams& q; dim3 g; uint32_t lds; hipStream_t s; };
template <bool POL>
struct LaunchFast64 {
  Fast64Args a;
  template <bool FL, bool O, bool C, bool X, bool R>
  void operator()(std::integer_sequence<bool, FL, O, C, X, R>) const {
    hipLaunchKernelGGL((step_fast64_kernel<FL, O, C, X, R, POL>), a.g, dim3(256), a.lds, a.s, a.f, a.r, a.q);
  }
};
// The slot loop's instantiations (FLAT, RICH, POL; no EXTRA switches): dispatched by recorded-mobility block (RP) and memory
// block (MEM), then chosen by step mode and information-age block - (CH, IA) has three legal values, not four - and out dtype
struct LaunchFast64Slots {
  Fast64Args a; bool ch, ia, out64;
  template <bool CH, bool IA, bool RP, bool MEM>
  void as() const {
    if (out64) hipLaunchKernelGGL((step_fast64_slots_kernel<true, true, CH, false, true, true, IA, RP, MEM>), a.g, dim3(256), a.lds, a.s, a.f, a.r, a.q);
    else hipLaunchKernelGGL((step_fast64_slots_kernel<true, false, CH, false, true, true, IA, RP, MEM>), a.g, dim3(256), a.lds, a.s, a.f, a.r, a.q);
  }
  template <bool RP, bool MEM>
  void operator()(std::integer_sequence<bool, RP, MEM>) const {
    if (ia) as<true, true, RP, MEM>();
    else if (ch) as<true, false, RP, MEM>();
    else as<false, false, RP, MEM>();
  }
};
}  // namespace

hipError_t launch_fast64(const FastParams& f, const RichParams& r, const KernelSel& k, int B, hipStream_t s) {
  static const PolParams no_policy{};
  const LaunchFast64<false> l{{f, r, no_policy, dim3(B), fast_lds_layout(f.K, f.A, k.rich, k.out64, k.flat, k.ch || k.extra).total, s}};
#ifdef DIRAL_FAST_BENCH_ONLY
  // tuning builds (profiles/build_variant.sh): only the instantiations the C2 / C4 bench lines run - seconds to compile
  if (!k.flat || k.out64 || k.ch || k.extra) return hipErrorInvalidValue;
  bool_dispatch(l, std::integer_sequence<bool, true, false, false, false>{}, k.rich);
#else
  bool_dispatch(l, std::integer_sequence<bool>{}, k.flat, k.out64, k.ch, k.extra, k.rich);
#endif
  return hipGetLastError();
}

// the one-slot POL instantiations (policy epilogue): the flat highway, my_step, no EXTRA switches, RICH
hipError_t launch_fast64_policy(const FastParams& f, const RichParams& r, const PolParams& q, bool out64, int B, hipStream_t s) {
  const LaunchFast64<true> l{{f, r, q, dim3(B), fast_lds_layout(f.K, f.A, true, out64, true, false).total, s}};
  if (out64) l(std::integer_sequence<bool, true, true, false, false, true>{});
  else l(std::integer_sequence<bool, true, false, false, false, true>{});
  return hipGetLastError();
}

// ... K slots per launch (PolParams::K > 1): step_fast64_slots_kernel, the same body with the env kept on the chip; `ch`:
// my_step_ch slots (the reception ratios of P1 in LDS next to the policy's arrays)
hipError_t launch_fast64_slots(const FastParams& f, const RichParams& r, const PolParams& q, bool ch, bool out64, int B, hipStream_t s) {
  const bool ia = ch && q.ia_on != 0;       // the information-age block: the IA instantiations (arrival stamps, histogram pass, term)
  const LaunchFast64Slots l{{f, r, q, dim3(B), fast_lds_layout(f.K, f.A, true, out64, true, ch, true, ia).total, s}, ch, ia, out64};
  // the RP instantiations: positions from the caller's sequence, the position log; MEM: the slots write rows of the caller's replay rings
  bool_dispatch(l, std::integer_sequence<bool>{}, q.rp_on != 0, q.mem_on != 0);
  return hipGetLastError();
}
}  // namespace diral
