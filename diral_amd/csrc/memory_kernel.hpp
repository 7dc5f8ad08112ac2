// memory_kernel.hpp - diral_memory_add / diral_memory_sample / diral_memory_history: the DRQN agent's replay memory
// (utils/memory.py:162-194, a deque of (state, action, reward, next_state)) for B envs at once, the regrouping of a sampled
// batch (DRQN.get_states_user and the three like it, algorithms/drl_drqn.py:294-377) as ONE gather launch, and the acting
// window of the newest states (memory_history_kernel below) as another.
//
// Storage: three rings of C + 1 rows owned by the caller - states [C + 1][B][N][S], actions and rewards [C + 1][B][N].
// The driver always has state = next_state, so logical state j is stored once, in row j mod (C + 1); transition j keeps
// its action and reward in row j mod (C + 1).  With `count` transitions added the live ones are [count - len, count),
// len = min(count, C).
//
// Sample: a work item is (window m, state row s' of its step + 1): its source is ONE contiguous block of N * S values
// (ring row, env b), its destination N segments of S values, M * step * S apart, in `states` (s' < step) and / or
// `next_states` (s' >= 1) - every ring row of a window is read once.  An item belongs to a workgroup of 256 threads, or
// to a wave where N * S is small (four items per workgroup); the block is read with the widest loads N * S and the ring's
// address allow (VEC = 4 / 2 / 1 elements per lane), written with stores as wide when S is a multiple of VEC, else one
// element per lane - consecutive lanes still fill consecutive addresses of a segment.  No LDS.  The item's window - the
// injected pair, or the Feistel permutation below - is computed uniformly by the item's lanes; its first lane reports it.
#pragma once
#include "common.hpp"
#include "policy_device.hpp"
#include "select_kernel.hpp"   // bf16_bits

namespace diral {

constexpr int kMemBlock = 256;

template <typename T, int V>
struct alignas(sizeof(T) * V) MemVec { T v[V]; };

// the output's element from the ring's: one rounding to nearest even (float -> _Float16 / bf16, double -> float) or none
template <typename OT, typename RT>
__device__ __forceinline__ OT mem_cvt(RT v) { return (OT)v; }
template <>
__device__ __forceinline__ bf16_bits mem_cvt<bf16_bits, float>(float v) {
  const uint32_t u = __float_as_uint(v);
  if (v != v) return bf16_bits{(uint16_t)0x7fc0};
  return bf16_bits{(uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16)};
}
template <typename OT>
__device__ __forceinline__ OT mem_zero() { return (OT)0; }
template <>
__device__ __forceinline__ bf16_bits mem_zero<bf16_bits>() { return bf16_bits{(uint16_t)0}; }

__device__ __forceinline__ long long mem_mod(long long a, long long m) { const long long r = a % m; return r < 0 ? r + m : r; }

// P(x): a permutation of [0, R) - a 4-round Feistel network on 2 w bits, w = max(1, ceil(ceil_log2(R) / 2)), walked
// again while the value is outside [0, R) (a cycle walk: the network permutes [0, 2^(2w)), so the walk from x < R comes
// back inside, on average within 2^(2w) / R < 4 rounds).
__device__ inline uint64_t mem_permute(uint64_t x, uint64_t R, uint64_t seed) {
  const int cl = R <= 1 ? 0 : 64 - __builtin_clzll(R - 1);          // ceil_log2(R)
  const int w = cl <= 2 ? 1 : (cl + 1) >> 1;
  const uint64_t mask = (1ull << w) - 1ull;
  do {
    uint64_t l = x >> w, r = x & mask;
    for (int k = 0; k < 4; ++k) {
      const uint64_t nr = l ^ (rng_u64(seed, (uint64_t)k, r) & mask);
      l = r;
      r = nr;
    }
    x = (l << w) | r;
  } while (x >= R);
  return x;
}

struct MemSampleParams {
  const void* states;            // the rings
  const int32_t* actions;
  const void* rewards;
  int C, B, N, S;
  long long count;
  const long long* count_dev;    // null, or the count in device memory
  int M, step, last_only;
  const int32_t* idx;            // [M] injected starts, or null (drawn)
  const int32_t* env;            // [M]
  uint64_t seed;
  const long long* clock;
  long long clock_offset;
  void* states_out;              // [N * M][step][S] of OT, or null
  void* next_out;
  int32_t* actions_out;          // [N * M][step] ([N * M] with last_only), or null
  void* rewards_out;             // ... of RT
  int32_t* idx_out;              // [M] or null
  int32_t* env_out;
  int32_t* bad;                  // counter of the windows answered with zeros, or null
  int ushift;                    // log2 of the threads per item: 6 (a wave) or 8 (the workgroup)
  int vst;                       // S % VEC == 0 and the outputs aligned: VEC-wide stores
};

template <typename RT, typename OT, int VEC>
__global__ __launch_bounds__(kMemBlock) void memory_sample_kernel(MemSampleParams p) {
  const int U = 1 << p.ushift;
  const int t = threadIdx.x & (U - 1);
  const int rows = p.step + 1;
  const int N = p.N, S = p.S, M = p.M, step = p.step;
  // Workgroups are dealt to the eight XCDs in turn; the step + 1 items of a window write into the same N output rows
  // (step * S contiguous values each), so they go to ONE XCD, back to back - window m to XCD m mod 8 -, where its L2
  // puts their part-line stores together.  (Placement only changes the speed: any order gives the same batch.)
  const long long slot = (long long)(blockIdx.x >> 3) * (kMemBlock >> p.ushift) + (threadIdx.x >> p.ushift);
  const long long wq = slot / rows;
  const int sp = (int)(slot - wq * rows);
  const long long ml = wq * 8 + (blockIdx.x & 7);
  if (ml >= (long long)M) return;                                   // (whole waves: an item is a wave or the workgroup)
  const int m = (int)ml;

  // the window (uniform over the item)
  long long count = p.count_dev ? *p.count_dev : p.count;
  if (count < 0) count = 0;
  const long long len = count < (long long)p.C ? count : (long long)p.C;
  const long long L = len - step, R = L * (long long)p.B;
  bool ok = L > 0;
  long long b = 0, i = 0;
  if (p.idx) {
    i = p.idx[m];
    b = p.env[m];
    ok = ok && i >= 0 && i < L && b >= 0 && b < p.B;
  } else {
    ok = ok && (long long)M <= R;
    if (ok) {
      const uint64_t seed = p.seed + (p.clock ? (uint64_t)(p.clock_offset + *p.clock) : 0ull);
      const uint64_t v = mem_permute((uint64_t)m, (uint64_t)R, seed);
      b = (long long)(v % (uint64_t)p.B);
      i = (long long)(v / (uint64_t)p.B);
    } else {
      b = i = -1;
    }
  }
  if (sp == 0 && t == 0) {
    if (p.idx_out) p.idx_out[m] = (int32_t)i;
    if (p.env_out) p.env_out[m] = (int32_t)b;
    if (!ok && p.bad) atomicAdd(p.bad, 1);
  }
  if (!ok) b = i = 0;                                               // (nothing is read from the rings then)
  const long long r = mem_mod(count - len + i + sp, (long long)p.C + 1);   // ring row of logical state / transition
  const long long blk = r * p.B + b;

  // the state block: N * S values -> N segments of `states` (row s') and of `next_states` (row s' - 1)
  const RT* src = static_cast<const RT*>(p.states) + (size_t)blk * N * S;
  OT* so = (p.states_out && sp < step) ? static_cast<OT*>(p.states_out) + ((size_t)m * step + sp) * S : nullptr;
  OT* no = (p.next_out && sp >= 1) ? static_cast<OT*>(p.next_out) + ((size_t)m * step + (sp - 1)) * S : nullptr;
  const size_t ustride = (size_t)M * step * S;                      // from user n to user n + 1
  if (so || no) {
    const uint32_t nv = (uint32_t)(N * S) / VEC;
    for (uint32_t q = t; q < nv; q += U) {
      MemVec<RT, VEC> in;
      if (ok) in = *reinterpret_cast<const MemVec<RT, VEC>*>(src + (size_t)q * VEC);
      MemVec<OT, VEC> o;
#pragma unroll
      for (int k = 0; k < VEC; ++k) o.v[k] = ok ? mem_cvt<OT, RT>(in.v[k]) : mem_zero<OT>();
      const uint32_t e = q * VEC;
      if (VEC == 1 || p.vst) {
        const uint32_t n = e / (uint32_t)S, c = e - n * (uint32_t)S;
        const size_t d = (size_t)n * ustride + c;
        if (so) *reinterpret_cast<MemVec<OT, VEC>*>(so + d) = o;
        if (no) *reinterpret_cast<MemVec<OT, VEC>*>(no + d) = o;
      } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
          const uint32_t n = (e + k) / (uint32_t)S, c = (e + k) - n * (uint32_t)S;
          const size_t d = (size_t)n * ustride + c;
          if (so) so[d] = o.v[k];
          if (no) no[d] = o.v[k];
        }
      }
    }
  }

  // the transition's action and reward of every user
  if (sp < step && (!p.last_only || sp == step - 1)) {
    const int32_t* a_src = p.actions + (size_t)blk * N;
    const RT* r_src = static_cast<const RT*>(p.rewards) + (size_t)blk * N;
    for (int n = t; n < N; n += U) {
      const size_t d = p.last_only ? (size_t)n * M + m : ((size_t)n * M + m) * step + sp;
      if (p.actions_out) p.actions_out[d] = ok ? a_src[n] : 0;
      if (p.rewards_out) static_cast<RT*>(p.rewards_out)[d] = ok ? r_src[n] : (RT)0;
    }
  }
}

// The sample kernel's state-block loop as a function (the sample kernel keeps its own text: the register counts of its
// instantiations are on record).  The N * S values at `src` (one ring row of one env) -> N segments of S values, `ustride`
// apart, in `so` and / or `no`, by the item's U threads (`t` this one's place among them).  !ok: zeros, and nothing is read.
template <typename RT, typename OT, int VEC>
__device__ __forceinline__ void mem_scatter_block(const RT* src, bool ok, OT* so, OT* no, size_t ustride, int N, int S, int t,
                                                  int U, int vst) {
  const uint32_t nv = (uint32_t)(N * S) / VEC;
  for (uint32_t q = t; q < nv; q += U) {
    MemVec<RT, VEC> in;
    if (ok) in = *reinterpret_cast<const MemVec<RT, VEC>*>(src + (size_t)q * VEC);
    MemVec<OT, VEC> o;
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = ok ? mem_cvt<OT, RT>(in.v[k]) : mem_zero<OT>();
    const uint32_t e = q * VEC;
    if (VEC == 1 || vst) {
      const uint32_t n = e / (uint32_t)S, c = e - n * (uint32_t)S;
      const size_t d = (size_t)n * ustride + c;
      if (so) *reinterpret_cast<MemVec<OT, VEC>*>(so + d) = o;
      if (no) *reinterpret_cast<MemVec<OT, VEC>*>(no + d) = o;
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const uint32_t n = (e + k) / (uint32_t)S, c = (e + k) - n * (uint32_t)S;
        const size_t d = (size_t)n * ustride + c;
        if (so) so[d] = o.v[k];
        if (no) no[d] = o.v[k];
      }
    }
  }
}

struct MemHistoryParams {
  const void* states;            // the state ring
  int C, B, N, S;
  long long count;
  const long long* count_dev;
  int step;
  void* out;                     // [B * N][step][S] of OT
  int32_t* bad;                  // counter of the calls answered with zeros, or null
  int ushift, vst;               // as MemSampleParams'
};

// diral_memory_history: the acting window - np.array(deque(maxlen=step)) of the newest states, every agent's rows
// (state_vector[:, user], main_test.py:86, 125; drl_drqn.py:171-172).  The sample kernel's item with another destination:
// an item is (env b, window row s), its source the block of logical state count - step + 1 + s, its destination N segments
// of S values, step * S apart, from out[b * N][s] on - row b * N + n is env-major.  The step items of an env write into the
// same N rows and go to one XCD like a window's (above), env b to XCD b mod 8.  step > len + 1 reaches behind the live
// states [count - len, count]: the whole output is zeros then and the first item counts one in *bad.
template <typename RT, typename OT, int VEC>
__global__ __launch_bounds__(kMemBlock) void memory_history_kernel(MemHistoryParams p) {
  const int U = 1 << p.ushift;
  const int t = threadIdx.x & (U - 1);
  const int N = p.N, S = p.S, step = p.step;
  const long long slot = (long long)(blockIdx.x >> 3) * (kMemBlock >> p.ushift) + (threadIdx.x >> p.ushift);
  const long long bq = slot / step;
  const int sp = (int)(slot - bq * step);
  const long long b = bq * 8 + (blockIdx.x & 7);
  if (b >= (long long)p.B) return;                                  // (whole waves: an item is a wave or the workgroup)

  long long count = p.count_dev ? *p.count_dev : p.count;
  if (count < 0) count = 0;
  const long long len = count < (long long)p.C ? count : (long long)p.C;
  const bool ok = (long long)step <= len + 1;
  if (!ok && b == 0 && sp == 0 && t == 0 && p.bad) atomicAdd(p.bad, 1);
  const long long r = ok ? mem_mod(count - step + 1 + sp, (long long)p.C + 1) : 0;   // (nothing is read from the ring then)
  const RT* src = static_cast<const RT*>(p.states) + ((size_t)r * p.B + (size_t)b) * N * S;
  OT* dst = static_cast<OT*>(p.out) + ((size_t)b * N * step + sp) * S;
  mem_scatter_block<RT, OT, VEC>(src, ok, dst, nullptr, (size_t)step * S, N, S, t, U, p.vst);
}

struct MemAddParams {
  void* states;                  // the rings
  int32_t* actions;
  void* rewards;
  int C, K;
  long long BN, BNS;             // values per ring row
  long long count;
  const long long* count_dev;
  const void* next_states;       // [K][B][N][S] of ST
  const void* state0;            // [B][N][S] of ST or null
  const int32_t* a_in;           // [K][B][N]
  const void* r_in;              // [K][B][N] / [B][N], float64 (r_f64) or float32
  int r_f64, r_bcast;
};

// A strided copy with an optional convert.  grid.y walks the K slots (+ 1: state0); a ring row is contiguous on both sides.
template <typename ST, typename RT, int VEC>
__global__ __launch_bounds__(kMemBlock) void memory_add_kernel(MemAddParams p) {
  long long count = p.count_dev ? *p.count_dev : p.count;
  if (count < 0) count = 0;
  const long long rows = (long long)p.C + 1;
  const int ny = p.K + (p.state0 ? 1 : 0);
  const size_t gid = (size_t)blockIdx.x * kMemBlock + threadIdx.x, gstride = (size_t)gridDim.x * kMemBlock;
  const size_t nv = (size_t)p.BNS / VEC;
  for (int y = blockIdx.y; y < ny; y += gridDim.y) {
    const bool first = y == p.K;                                    // state0 -> state row `count`
    const ST* src = first ? static_cast<const ST*>(p.state0) : static_cast<const ST*>(p.next_states) + (size_t)y * p.BNS;
    RT* dst = static_cast<RT*>(p.states) + (size_t)mem_mod(first ? count : count + 1 + y, rows) * p.BNS;
    for (size_t q = gid; q < nv; q += gstride) {
      const MemVec<ST, VEC> in = *reinterpret_cast<const MemVec<ST, VEC>*>(src + q * VEC);
      MemVec<RT, VEC> o;
#pragma unroll
      for (int k = 0; k < VEC; ++k) o.v[k] = (RT)in.v[k];
      *reinterpret_cast<MemVec<RT, VEC>*>(dst + q * VEC) = o;
    }
    if (first) continue;
    const size_t tr = (size_t)mem_mod(count + y, rows) * p.BN;
    const size_t rs = p.r_bcast ? 0 : (size_t)y * p.BN;
    for (size_t e = gid; e < (size_t)p.BN; e += gstride) {
      p.actions[tr + e] = p.a_in[(size_t)y * p.BN + e];
      const double rv = p.r_f64 ? static_cast<const double*>(p.r_in)[rs + e] : (double)static_cast<const float*>(p.r_in)[rs + e];
      static_cast<RT*>(p.rewards)[tr + e] = (RT)rv;
    }
  }
}

}  // namespace diral
