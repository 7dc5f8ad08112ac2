// select_kernel.hpp - diral_policy_select: actions [agents] from Q-values [agents][A] in ONE launch - the exploration
// policies of algorithms/policies.py (GreedyPolicy :24-35, EpsilonGreedy :45-54, SoftmaxPolicy :92-112 with
// np.random.choice(p=), BoltzmanPolicy :144-178) for B x N agents at once.  Every Q-value is converted exactly to float64
// and all arithmetic is float64 in the order NumPy walks: np.argmax's tie and NaN rules, np.sum's pairwise order
// (policy_device.hpp), np.cumsum's sequential order, searchsorted(side="right").  The draws are injected or a function of
// (seed, stream, GLOBAL agent index), as diral_env_sample's.
//
// Two layouts.  A <= 64: one row per group of G lanes (G the power of two >= A, at least 4), one value per lane in a
// register, 64 / G rows per wave - at A = 32 and float32 a wave reads two rows as one 256-byte access; the reductions and
// the cumsum are lane shuffles inside the group.  A > 64 (up to 4096): one row per wave, lane l holds the elements
// l, l + 64, ...; the arg-max streams them through registers, SOFTMAX and BOLTZMANN - whose sums index the row in NumPy's
// order - stage the row in LDS (A doubles).
#pragma once
#include "common.hpp"
#include "policy_device.hpp"

namespace diral {

constexpr int kSelGreedy = 0, kSelEpsGreedy = 1, kSelSoftmax = 2, kSelBoltzmann = 3;   // DiralSelectKind
constexpr int kSelMaxA = 4096;
constexpr int kSelBlock = 256;                 // A <= 64: four waves of 64 / G rows each
constexpr uint64_t kSelStreamU = 10, kSelStreamA = 11;   // generator streams (1-9: reset, sample, velocity, SPS)

struct bf16_bits { uint16_t b; };              // a bfloat16 as stored: the upper half of a float32

template <typename QT>
__device__ __forceinline__ double q_to_f64(QT v) { return (double)v; }          // double, float, _Float16: exact
template <>
__device__ __forceinline__ double q_to_f64<bf16_bits>(bf16_bits v) { return (double)__uint_as_float((uint32_t)v.b << 16); }

struct SelParams {
  const void* q;                 // [agents][A] of QT
  int agents, N, A;
  int gshift;                    // A <= 64: log2 of the lanes per row
  double param;                  // the kind's parameter by value: eps / tmp / explore_p
  double beta, alpha;            // BOLTZMANN
  const double* param_dev;       // null, or the parameter in device memory: 1 value, or one per env (param_per_env)
  int param_per_env;
  const double* draw_u;          // [agents] injected draws in [0, 1), or null (device generator)
  const int32_t* draw_a;         // [agents] injected draws >= 0, used mod A, or null
  uint64_t seed, idx0;           // idx0: global index of agent 0 (DIRAL_OPT_ENV_OFFSET * N)
  const long long* clock;        // null, or a device counter: the launch draws with seed + clock_offset + *clock
  long long clock_offset;
  int32_t* actions_out;          // [agents]
  uint8_t* explored_out;         // [agents] or null
  int32_t* bad_rows;             // null, or a counter of the SOFTMAX rows answered by the GREEDY rule
};

// np.argmax's order: (v, i) comes before (w, j) when v is the greater value, a NaN is greater than any number, and the
// lower index wins between equals (-0.0 == +0.0) and between NaNs.  An empty slot is (-inf, INT_MAX): it loses to a real
// -inf at any index.
__device__ __forceinline__ bool arg_before(double v, int i, double w, int j) {
  const bool vn = v != v, wn = w != w;
  if (vn || wn) return vn && (!wn || i < j);
  return v > w || (v == w && i < j);
}
__device__ __forceinline__ void arg_take(double& bv, int& bi, double v, int i) {
  if (arg_before(v, i, bv, bi)) { bv = v; bi = i; }
}
// ... reduced over the 2^gshift lanes of a group with a butterfly: every lane of the group ends with the winner
__device__ __forceinline__ void arg_reduce(double& bv, int& bi, int lane, int gshift) {
  for (int m = (1 << gshift) >> 1; m > 0; m >>= 1) {
    const double ov = shfl_t(bv, lane ^ m);
    const int oi = __shfl(bi, lane ^ m);
    arg_take(bv, bi, ov, oi);
  }
}

// np.sum of the n <= 64 values a group holds one per lane (lane g0 + j holds a[j]) in NumPy's order - np_row_sum_wave's
// walk inside a group, and the sequential form for fewer than 8 elements.  Uniform over the group.
__device__ __forceinline__ double np_group_sum(double a, int n, int lane, int g0) {
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r = r + shfl_t(a, g0 + i);
    return r;
  }
  const int nb = n >> 3, j = (lane - g0) & 7;
  double r = a;
  for (int i = 1; i < nb; ++i) r = r + shfl_t(a, g0 + j + 8 * i);
  double t = r + shfl_t(r, (lane + 1) & 63);
  t = t + shfl_t(t, (lane + 2) & 63);
  t = t + shfl_t(t, (lane + 4) & 63);
  double sr = shfl_t(t, g0);
  for (int i = nb * 8; i < n; ++i) sr = sr + shfl_t(a, g0 + i);
  return sr;
}

// np.sum of a row of n <= kSelMaxA doubles in LDS by one wave, in NumPy's order.  pairwise_sum splits a block above 128
// elements at n / 2 rounded down to a multiple of 8, at most six times for n <= 4096 (the larger half is at most
// n / 2 + 8: 4096 -> ... -> below 80 behind six splits): bit 5 - d of the lane number says which half the lane follows at
// level d, so the 64 lanes reach every leaf; a block that does not split keeps the lane whose bit is 0.  Each owner sums
// its leaf (np_pairwise_sum's unsplit part), then the halves are added left + right from the deepest level up.
// Wave-uniform result.
__device__ __forceinline__ double np_wave_sum_lds(const double* a, int n, int lane) {
  int off = 0, len = n;
  unsigned int split = 0;
  bool own = true;
#pragma unroll
  for (int d = 0; d < 6; ++d) {
    const bool right = (lane >> (5 - d)) & 1;
    if (len > 128) {
      int n2 = len / 2;
      n2 -= n2 % 8;
      split |= 1u << d;
      if (right) { off += n2; len -= n2; } else len = n2;
    } else if (right) own = false;
  }
  double s = 0.0;
  if (own && len <= 128) s = np_pairwise_sum<double, 0>(a + off, len);
#pragma unroll
  for (int d = 5; d >= 0; --d) {
    const int bit = 1 << (5 - d);
    const double other = shfl_t(s, lane | bit);
    if (own && ((split >> d) & 1u) && (lane & (2 * bit - 1)) == 0) s = s + other;
  }
  return shfl_t(s, 0);
}

// the row's draws and parameter; `row` is the agent's place in this call, idx0 + row its global index
struct SelDraw { double u; int a; double par; };
template <int KIND>
__device__ __forceinline__ SelDraw sel_draw(const SelParams& p, long long row) {
  SelDraw d = {0.0, 0, p.param};
  if constexpr (KIND == kSelGreedy) return d;
  const uint64_t seed = p.seed + (p.clock ? (uint64_t)(p.clock_offset + *p.clock) : 0ull);
  const uint64_t gi = p.idx0 + (uint64_t)row;
  d.u = p.draw_u ? p.draw_u[row] : rng_unit(rng_u64(seed, kSelStreamU, gi));
  if constexpr (KIND != kSelSoftmax) {
    const uint64_t r = p.draw_a ? (uint64_t)(uint32_t)p.draw_a[row] : rng_u64(seed, kSelStreamA, gi);
    d.a = (int)(r % (uint64_t)p.A);
  }
  if (p.param_dev) d.par = p.param_dev[p.param_per_env ? row / p.N : 0];
  return d;
}

// A <= 64.  grid: blocks of four waves, wave w serves the rows w * (64 >> gshift) ...
template <typename QT, int KIND>
__global__ __launch_bounds__(kSelBlock) void select_actions_kernel(SelParams p) {
  const int lane = threadIdx.x & 63;
  const int A = p.A, gshift = p.gshift;
  const int g = lane & ((1 << gshift) - 1), g0 = lane - g;
  const long long wave = ((long long)blockIdx.x * kSelBlock + threadIdx.x) >> 6;
  const long long row = (wave << (6 - gshift)) + (lane >> gshift);
  const bool live = row < (long long)p.agents, have = live && g < A;
  const double ninf = -__builtin_inf();
  const double v = have ? q_to_f64(static_cast<const QT*>(p.q)[(size_t)row * A + g]) : ninf;
  SelDraw d = {0.0, 0, p.param};
  if (live) d = sel_draw<KIND>(p, row);

  int action = 0;
  bool explored = false, bad = false;
  if constexpr (KIND == kSelGreedy || KIND == kSelEpsGreedy || KIND == kSelSoftmax) {
    double bv = v;                                                  // np.argmax(Qs) (policies.py:30)
    int bi = have ? g : 0x7fffffff;
    arg_reduce(bv, bi, lane, gshift);
    action = bi;
  }
  if constexpr (KIND == kSelEpsGreedy) {
    explored = !(d.u > d.par);                                      // policies.py:50: draw > eps -> greedy
    if (explored) action = d.a;
  }
  if constexpr (KIND == kSelSoftmax) {
    const double x = v / d.par;                                     // policies.py:98
    double m = have ? x : ninf;                                     // x.max() (a NaN leaves through the sum below)
    for (int k = (1 << gshift) >> 1; k > 0; k >>= 1) m = fmax(m, shfl_t(m, lane ^ k));
    const double y = exp(x - m);                                    // :110-111
    const double S = np_group_sum(y, A, lane, g0);
    const double pr = y / S;                                        // :112
    // np.random.choice: cdf = p.cumsum() - sequentially -, cdf /= cdf[-1], searchsorted(u, side="right")
    double run = shfl_t(pr, g0), mine = run;
    for (int j = 1; j < A; ++j) {
      run = run + shfl_t(pr, g0 + j);
      if (g == j) mine = run;
    }
    const unsigned long long le = __ballot(have && mine / run <= d.u);
    const int cnt = __popcll((le >> g0) & ((~0ull) >> (64 - (1 << gshift))));
    bad = !(S > 0.0) || S == __builtin_inf();                       // a NaN, a +inf, nothing but -inf: choice() raises
    if (!bad) action = cnt < A - 1 ? cnt : A - 1;
  }
  if constexpr (KIND == kSelBoltzmann) {
    const double e = exp(p.beta * v);                               // policies.py:171-172
    const double S = np_group_sum(e, A, lane, g0);
    double bv = have ? ((1.0 - p.alpha) * e) / S + p.alpha / (double)A : ninf;
    int bi = have ? g : 0x7fffffff;
    arg_reduce(bv, bi, lane, gshift);                               // :175
    action = bi;
    explored = d.par > d.u;                                         // :162
    if (explored) action = d.a;
  }
  if (live && g == 0) {
    p.actions_out[row] = action;
    if (p.explored_out) p.explored_out[row] = explored ? 1 : 0;
  }
  if constexpr (KIND == kSelSoftmax) {
    const unsigned long long bm = __ballot(bad && live && g == 0);
    if (p.bad_rows && bm != 0ull && lane == 0) atomicAdd(p.bad_rows, (int)__popcll(bm));
  }
}

// A > 64.  grid: one wave (a block of 64 threads) per row; dynamic LDS: A doubles for SOFTMAX and BOLTZMANN, else none.
template <typename QT, int KIND>
__global__ __launch_bounds__(64) void select_actions_wide_kernel(SelParams p) {
  extern __shared__ double sel_row[];
  const int lane = threadIdx.x, A = p.A;
  const long long row = blockIdx.x;                                 // (the grid is `agents` blocks)
  const QT* q = static_cast<const QT*>(p.q) + (size_t)row * A;
  const double ninf = -__builtin_inf();
  const SelDraw d = sel_draw<KIND>(p, row);

  int action = 0;
  bool explored = false, bad = false;
  double bv = ninf;
  int bi = 0x7fffffff;
  if constexpr (KIND == kSelGreedy || KIND == kSelEpsGreedy) {
    for (int j = lane; j < A; j += 64) arg_take(bv, bi, q_to_f64(q[j]), j);
    arg_reduce(bv, bi, lane, 6);
    action = bi;
  }
  if constexpr (KIND == kSelEpsGreedy) {
    explored = !(d.u > d.par);
    if (explored) action = d.a;
  }
  if constexpr (KIND == kSelSoftmax) {
    double m = ninf;
    for (int j = lane; j < A; j += 64) {
      const double v = q_to_f64(q[j]);
      arg_take(bv, bi, v, j);
      const double x = v / d.par;
      sel_row[j] = x;
      m = fmax(m, x);
    }
    arg_reduce(bv, bi, lane, 6);
    for (int k = 32; k > 0; k >>= 1) m = fmax(m, shfl_t(m, lane ^ k));
    for (int j = lane; j < A; j += 64) sel_row[j] = exp(sel_row[j] - m);
    __syncthreads();
    const double S = np_wave_sum_lds(sel_row, A, lane);
    for (int j = lane; j < A; j += 64) sel_row[j] = sel_row[j] / S;
    __syncthreads();
    // the sequential cumsum, in place: every lane walks the row, the lane that holds element j keeps cdf[j]
    double run = sel_row[0];
    for (int j = 1; j < A; ++j) {
      run = run + sel_row[j];
      if ((j & 63) == lane) sel_row[j] = run;
    }
    __syncthreads();
    int cnt = 0;
    for (int j = lane; j < A; j += 64) cnt += (sel_row[j] / run <= d.u) ? 1 : 0;
    for (int k = 32; k > 0; k >>= 1) cnt += __shfl(cnt, lane ^ k);
    bad = !(S > 0.0) || S == __builtin_inf();
    action = bad ? bi : (cnt < A - 1 ? cnt : A - 1);
  }
  if constexpr (KIND == kSelBoltzmann) {
    for (int j = lane; j < A; j += 64) sel_row[j] = exp(p.beta * q_to_f64(q[j]));
    __syncthreads();
    const double S = np_wave_sum_lds(sel_row, A, lane);
    for (int j = lane; j < A; j += 64) arg_take(bv, bi, ((1.0 - p.alpha) * sel_row[j]) / S + p.alpha / (double)A, j);
    arg_reduce(bv, bi, lane, 6);
    action = bi;
    explored = d.par > d.u;
    if (explored) action = d.a;
  }
  if (lane == 0) {
    p.actions_out[row] = action;
    if (p.explored_out) p.explored_out[row] = explored ? 1 : 0;
    if (bad && p.bad_rows) atomicAdd(p.bad_rows, 1);
  }
}

}  // namespace diral
