// copy_envs_kernel.hpp - diral_env_copy_envs: whole envs from one handle to another (or within one) in their STORED
// form.  A handle keeps an env as one slab per state buffer; a copy is a gather of those slabs, `count`
// (source env, destination env) pairs in ONE launch - no conversion to the reference-shaped planes, no launch per buffer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace diral {

constexpr uint32_t kErrEnvIndex = 16u;   // sticky error bit: an env index outside its handle (DIRAL_ERR_ENV_INDEX)

constexpr int kCopyMaxSlabs = 16;
constexpr int kCopyThreads = 256;
constexpr int kCopyUnroll = 4;                                       // accesses a lane has in flight
constexpr uint32_t kCopyChunk = kCopyThreads * kCopyUnroll;          // units per workgroup: 16 KB of 16-byte slabs

// One state buffer of the two handles.  A unit is what one lane moves per access: 16 bytes where the env's slab is a
// multiple of 16 (the bases are hipMalloc's, so every env's slab is aligned too), else 4 (pos_x at N = 9: 72 bytes).
struct CopySlab {
  const char* src;
  char* dst;
  uint32_t bytes;    // per env
  uint32_t first;    // first unit of this slab in the env's concatenated slabs
};
struct CopyPlan {
  CopySlab slab[kCopyMaxSlabs];
  int32_t slabs;
  uint32_t units;    // of one env
};
inline uint32_t copy_units(uint32_t bytes) { return (bytes & 15u) ? bytes >> 2 : bytes >> 4; }

// (a use of the loaded value right behind the loads: without it the compiler sinks every load into the branch of its
// masked store, and a lane has one access in flight instead of kCopyUnroll)
__device__ __forceinline__ void copy_keep(const uint32_t& v) { asm volatile("" ::"v"(v)); }
__device__ __forceinline__ void copy_keep(const uint4& v) { asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w)); }

// units [lo, hi) of one slab, lo < hi <= lo + kCopyChunk: the loads of a lane are issued before its stores (source and
// destination are different envs: equal indices of one handle never get here).  A load past the span is clamped onto its
// last unit instead of predicated - unconditional loads stay in flight together - and only the stores are masked.
template <typename V>
__device__ __forceinline__ void copy_span(const V* __restrict__ s, V* __restrict__ d, uint32_t lo, uint32_t hi, uint32_t tid) {
  V r[kCopyUnroll];
#pragma unroll
  for (int k = 0; k < kCopyUnroll; ++k) r[k] = s[min(lo + tid + k * kCopyThreads, hi - 1u)];
#pragma unroll
  for (int k = 0; k < kCopyUnroll; ++k) copy_keep(r[k]);
#pragma unroll
  for (int k = 0; k < kCopyUnroll; ++k)
    if (lo + tid + k * kCopyThreads < hi) d[lo + tid + k * kCopyThreads] = r[k];
}

// grid: x = chunks of kCopyChunk units of an env's concatenated slabs, y = pairs (strided when count exceeds the grid's
// limit).  The pair's indices are uniform per workgroup; a pair with an index outside its handle is skipped and flagged.
__global__ __launch_bounds__(kCopyThreads) void copy_envs_kernel(CopyPlan plan, const int32_t* __restrict__ src_index,
                                                                 const int32_t* __restrict__ dst_index, int count, int B_src,
                                                                 int B_dst, int same, uint32_t* err) {
  const uint32_t tid = threadIdx.x;
  const uint32_t c_lo = blockIdx.x * kCopyChunk;
  const uint32_t c_hi = min(c_lo + kCopyChunk, plan.units);
  for (int i = blockIdx.y; i < count; i += gridDim.y) {
    const int si = src_index ? src_index[i] : i;
    const int di = dst_index ? dst_index[i] : i;
    if ((unsigned)si >= (unsigned)B_src || (unsigned)di >= (unsigned)B_dst) {
      if (blockIdx.x == 0 && tid == 0) atomicOr(err, kErrEnvIndex);
      continue;
    }
    if (same && si == di) continue;
    for (int e = 0; e < plan.slabs; ++e) {
      const CopySlab sl = plan.slab[e];
      const uint32_t n = (sl.bytes & 15u) ? sl.bytes >> 2 : sl.bytes >> 4;
      if (sl.first >= c_hi || sl.first + n <= c_lo) continue;
      const uint32_t lo = max(sl.first, c_lo) - sl.first, hi = min(sl.first + n, c_hi) - sl.first;
      const char* s = sl.src + (size_t)si * sl.bytes;
      char* d = sl.dst + (size_t)di * sl.bytes;
      if (sl.bytes & 15u) copy_span(reinterpret_cast<const uint32_t*>(s), reinterpret_cast<uint32_t*>(d), lo, hi, tid);
      else copy_span(reinterpret_cast<const uint4*>(s), reinterpret_cast<uint4*>(d), lo, hi, tid);
    }
  }
}

}  // namespace diral
