// wave_ops.hpp - wave, lane and memory primitives shared by every kernel family; the reference's arithmetic is in
// ref_math.hpp.  (shfl_t stays in policy_device.hpp, next to its only callers, the NumPy-ordered row sums.)
#pragma once
#include "common.hpp"

namespace diral {

__device__ inline double readlane_f64(double v, int srclane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), srclane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), srclane);
  return __hiloint2double(hi, lo);
}
__device__ inline unsigned long long readlane_u64(unsigned long long v, int srclane) {
  const unsigned int lo = __builtin_amdgcn_readlane((unsigned int)v, srclane);
  const unsigned int hi = __builtin_amdgcn_readlane((unsigned int)(v >> 32), srclane);
  return ((unsigned long long)hi << 32) | lo;
}

// wave-uniform 64-bit value -> SGPR pair, so branches on it are scalar
__device__ inline unsigned long long uniform_u64(unsigned long long v) {
  const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)v);
  const unsigned int hi = __builtin_amdgcn_readfirstlane((unsigned int)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

// A wave-uniform row pointer pinned into an SGPR pair, typed as a GLOBAL
// (address_space(1)) pointer: loads/stores take the scalar-base + 32-bit lane offset
// form.  Without the pin the compiler hoists per-lane 64-bit addresses out of the column
// loops (16 VGPRs); without the address space a pointer rebuilt from integers is generic
// and every access becomes a FLAT instruction (which also counts on lgkmcnt).
template <typename T>
using global_ptr = __attribute__((address_space(1))) T*;
template <typename T>
__device__ inline global_ptr<T> uniform_ptr(T* base, size_t elem_off) {
  return (global_ptr<T>)uniform_u64((unsigned long long)(base + elem_off));
}

// Sum of a double over the 64 lanes of a wave with DPP moves (row_shr 8 / 4 / 2 / 1, then row_bcast 15 and 31): VALU only -
// `__shfl_down` compiles to ds_bpermute, an LDS round trip per level, and this sits on the critical path of the wave that
// does P2.  The total lands in lane 63 and is returned wave-uniform.  (The order differs from the shuffle tree: callers whose
// sums are compared bit for bit across kernels keep the tree.)
template <int CTRL, int ROW_MASK>
__device__ inline double dpp_add_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
  return v + __hiloint2double(hi, lo);
}
__device__ inline double wave_sum_f64(double v) {
  v = dpp_add_f64<0x118, 0xf>(v);      // row_shr:8 (lanes without a source add 0)
  v = dpp_add_f64<0x114, 0xf>(v);      // row_shr:4
  v = dpp_add_f64<0x112, 0xf>(v);      // row_shr:2
  v = dpp_add_f64<0x111, 0xf>(v);      // row_shr:1: lane 15 of every row holds the row's sum
  v = dpp_add_f64<0x142, 0xa>(v);      // row_bcast:15 into rows 1 and 3
  v = dpp_add_f64<0x143, 0xc>(v);      // row_bcast:31 into rows 2 and 3: lane 63 holds the total
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), 63);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
  return __hiloint2double(hi, lo);
}

// Orders this wave's LDS accesses for the COMPILER only.  The hardware already
// executes one wave's DS instructions in issue order, so a later ds_read sees an
// earlier ds_write of the same wave without any wait; a real fence would drain
// lgkmcnt at every merge step (measured: the dominant cost at N > 64).
__device__ inline void wave_lds_order() { asm volatile("" ::: "memory"); }

// Lane masks as values (a compare's result taken with __builtin_amdgcn_ballot_w64 while every lane of the wave is active):
// combined on the scalar side (and, andn2, or) and handed back to the vector side as the mask operand itself.
// x + 1 in the lanes of `m`, x elsewhere: ONE v_addc_co_u32 with the mask as its carry-in (from a bool the compiler makes
// v_cndmask_b32 0 / 1 and v_add)
__device__ inline unsigned int add_lane_mask(unsigned int x, unsigned long long m) {
  unsigned int r;
  unsigned long long carry_out;
  asm("v_addc_co_u32 %0, %1, 0, %2, %3" : "=v"(r), "=s"(carry_out) : "v"(x), "s"(m));
  return r;
}
// a in the lanes of `m`, b elsewhere
__device__ inline int select_lane_mask(unsigned long long m, int a, int b) {
  int r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(m));
  return r;
}

// the HIGH half of a (a >> 16) in the lanes of `m`, b elsewhere: the shift is the SDWA source selector of the select.  The
// SDWA form takes its mask from VCC (a scalar move: an asm operand cannot be bound to VCC); ONE vector instruction where the
// shift and v_cndmask_b32_e64 are two
__device__ inline int select_lane_mask_hi16(unsigned long long m, unsigned int a, int b) {
  int r;
  asm("s_mov_b64 vcc, %3\n\tv_cndmask_b32_sdwa %0, %1, %2, vcc dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1"
      : "=v"(r) : "v"(b), "v"(a), "s"(m) : "vcc");
  return r;
}

// An LDS object by its absolute byte address (register + compile-time constant: the constant goes
// into the DS instruction's immediate offset; going through the `extern __shared__` symbol instead
// leaves a relocated `+ 0` add in front of every access)
template <typename T>
__device__ inline const __attribute__((address_space(3))) T* lds_at(unsigned int byte_addr) {
  return (const __attribute__((address_space(3))) T*)(size_t)byte_addr;
}

// LDS byte address of a __shared__ object (what M0-relative DS instructions take)
__device__ inline unsigned int lds_addr(const void* p) {
  return (unsigned int)(size_t)(__attribute__((address_space(3))) const void*)p;
}

// Streaming (non-temporal) stores for the state vectors: they are the last thing a
// workgroup does and nothing on the chip reads them back, so they should neither claim L2
// lines nor hold the wave until a cached write is acknowledged (measured on C2: 98 -> 89 us
// per slot; on the table stores, which the barrier and P4 already overlap, it does not pay).
__device__ inline void stream_store(float* p, float v) { __builtin_nontemporal_store(v, p); }
__device__ inline void stream_store(double* p, double v) { __builtin_nontemporal_store(v, p); }
__device__ inline void stream_store4(float* p, float4 v) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  const f4 vv = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(vv, reinterpret_cast<f4*>(p));
}
__device__ inline void stream_store2(double* p, double2 v) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  const d2 vv = {v.x, v.y};
  __builtin_nontemporal_store(vv, reinterpret_cast<d2*>(p));
}

__device__ inline void store_out(void* base, size_t idx, double v, int f64) {
  if (f64) reinterpret_cast<double*>(base)[idx] = v;
  else reinterpret_cast<float*>(base)[idx] = (float)v;
}

// double -> int32, truncating, SATURATING, NaN -> 0 (the hardware conversion; a C cast is undefined out of range)
__device__ inline int cvt_i32_f32_sat(float x) {                   // truncating, saturating, NaN -> 0
  int r;
  asm("v_cvt_i32_f32 %0, %1" : "=v"(r) : "v"(x));
  return r;
}
__device__ inline int cvt_i32_f64_sat(double x) {
  int r;
  asm("v_cvt_i32_f64 %0, %1" : "=v"(r) : "v"(x));
  return r;
}

// Thermometer codes of table lags: c(lag) = (0xff << lag) & 0xff for lag 0..7, 0 = never heard.
// The codes form a chain under bit inclusion, so the code of the smaller lag (the fresher entry)
// is the bitwise OR, and the lag comes back as 8 - popcount.  Four lag bytes (0..7 exact, 12 =
// never heard) -> four codes with one v_perm_b32: selectors 0-7 pick bytes of the table
// {0xff, 0xfe, 0xfc, 0xf8, 0xf0, 0xe0, 0xc0, 0x80}, selector 12 yields 0x00.
__device__ inline unsigned int thermo_codes(unsigned int lag_bytes) {
  return __builtin_amdgcn_perm(0x80c0e0f0u, 0xf8fcfeffu, lag_bytes);
}

// Count of trailing zeros of byte BYTE of a word (-1 for a zero byte): one SDWA instruction.  The lag of a thermometer
// code (0xff << lag) & 0xff.
template <int BYTE>
__device__ inline int ffbl_byte(unsigned int w) {
  int r;
  static_assert(BYTE >= 0 && BYTE < 4, "byte select");
  if constexpr (BYTE == 0) asm("v_ffbl_b32_sdwa %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0" : "=v"(r) : "v"(w));
  if constexpr (BYTE == 1) asm("v_ffbl_b32_sdwa %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1" : "=v"(r) : "v"(w));
  if constexpr (BYTE == 2) asm("v_ffbl_b32_sdwa %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2" : "=v"(r) : "v"(w));
  if constexpr (BYTE == 3) asm("v_ffbl_b32_sdwa %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3" : "=v"(r) : "v"(w));
  return r;
}

}  // namespace diral
