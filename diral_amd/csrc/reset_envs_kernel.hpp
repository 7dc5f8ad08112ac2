// reset_envs_kernel.hpp - diral_env_reset_envs: a chosen subset of a handle's envs back to what diral_env_reset leaves,
// in ONE launch over their slabs in the STORED form.  The envs come as an index list or as a device mask [B]; every slab
// diral_env_copy_envs would move (copy_envs_kernel.hpp) other than the positions is filled with its buffer's fill byte, and
// the positions and velocities are the given rows or the draws of reset_kernel (aux_kernels.hpp: reset_draw).  Stores
// only: nothing of the env is read, so duplicate entries write the same values.
#pragma once
#include "aux_kernels.hpp"
#include "copy_envs_kernel.hpp"

namespace diral {

// One state buffer of the handle; units as in CopySlab (16 bytes, or 4 where the env's slab is no multiple of 16).
struct ResetSlab {
  char* dst;
  uint32_t bytes;    // per env
  uint32_t first;    // first unit of this slab in the env's concatenated slabs
  uint32_t fill;     // the fill byte in all four bytes of a word
};
struct ResetPlan {
  ResetSlab slab[kCopyMaxSlabs];
  int32_t slabs;
  uint32_t units;    // of one env
};

// units [lo, hi) of one slab, lo < hi <= lo + kCopyChunk
template <typename V>
__device__ __forceinline__ void fill_span(V* __restrict__ d, const V v, uint32_t lo, uint32_t hi, uint32_t tid) {
#pragma unroll
  for (int k = 0; k < kCopyUnroll; ++k)
    if (lo + tid + k * kCopyThreads < hi) d[lo + tid + k * kCopyThreads] = v;
}

// grid: x = chunks of kCopyChunk units of an env's concatenated slabs, y = listed envs (strided when there are more than
// the grid's limit).  `mask` != NULL: entry i IS env i and `count` == B, a workgroup whose mask byte is 0 leaves after
// that one uniform load; else env index[i] (NULL: i).  An index outside the handle is skipped and flagged.  The
// workgroup of chunk 0 also writes the env's N positions and velocities: row b of x0 / y0 / v0, or the device draws at
// the env's GLOBAL vehicle index idx0 + b * N + u.
__global__ __launch_bounds__(kCopyThreads) void reset_envs_kernel(ResetPlan plan, const int32_t* __restrict__ index,
                                                                  const uint8_t* __restrict__ mask, int count, int B, int N,
                                                                  double L, int vary, uint64_t seed, uint64_t idx0,
                                                                  const double* __restrict__ x0, const double* __restrict__ y0,
                                                                  const double* __restrict__ v0, double* __restrict__ pos_x,
                                                                  double* __restrict__ pos_y, double* __restrict__ vel,
                                                                  uint32_t* err) {
  const uint32_t tid = threadIdx.x;
  const uint32_t c_lo = blockIdx.x * kCopyChunk;
  const uint32_t c_hi = min(c_lo + kCopyChunk, plan.units);
  for (int i = blockIdx.y; i < count; i += gridDim.y) {
    if (mask && mask[i] == 0) continue;
    const int b = index ? index[i] : i;                            // (the host refuses index and mask together)
    if ((unsigned)b >= (unsigned)B) {
      if (blockIdx.x == 0 && tid == 0) atomicOr(err, kErrEnvIndex);
      continue;
    }
    for (int e = 0; e < plan.slabs; ++e) {
      const ResetSlab sl = plan.slab[e];
      const uint32_t n = (sl.bytes & 15u) ? sl.bytes >> 2 : sl.bytes >> 4;
      if (sl.first >= c_hi || sl.first + n <= c_lo) continue;
      const uint32_t lo = max(sl.first, c_lo) - sl.first, hi = min(sl.first + n, c_hi) - sl.first;
      char* d = sl.dst + (size_t)b * sl.bytes;
      if (sl.bytes & 15u) fill_span(reinterpret_cast<uint32_t*>(d), sl.fill, lo, hi, tid);
      else fill_span(reinterpret_cast<uint4*>(d), make_uint4(sl.fill, sl.fill, sl.fill, sl.fill), lo, hi, tid);
    }
    if (blockIdx.x == 0) {
      for (uint32_t u = tid; u < (uint32_t)N; u += kCopyThreads) {
        const size_t j = (size_t)b * N + u;
        double x, y, v;
        reset_draw(L, vary, seed, idx0 + (uint64_t)j, j, x0, y0, v0, x, y, v);
        pos_x[j] = x; pos_y[j] = y; vel[j] = v;
      }
    }
  }
}

}  // namespace diral
