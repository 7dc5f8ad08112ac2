// td_kernel.hpp - diral_td_head: the learning side's glue around a torch Q-network as ONE launch (+ one for the loss) -
// DRQN._calc_target (algorithms/drl_drqn.py:267-292) and the loss head (:76-80) with its gradient dL/dQ, for
// rows = N * batch rows of A Q-values.  Every Q-value is converted exactly to float32 (the reference's graph is float32)
// and a row is worked in this order:
//   1. j = np.argmax(index row) - the q_next_eval row (double DQN), or the q_next_target row - with np.argmax's tie and
//      NaN rules (arg_before, select_kernel.hpp);
//   2. nv = q_next_target[row][j].  In the plain case this is np.max of the row: a NaN row gives NaN as np.max does, and
//      a zero maximum carries the sign of the FIRST zero of the row where np.max may return another's - numerically equal;
//   3. target = (float)((double)r + (double)((float)gamma * nv)): NumPy multiplies the Python float into the float32
//      array in float32, adds the float64 rewards in float64, and the feed into the float32 placeholder rounds once.  The
//      conversion between the product and the sum keeps them two roundings (and the build has -ffp-contract=off);
//   4. Q = q[row][a], h = Q - target.  An action outside [0, A) gives Q = 0 and a zero gradient row - tf.one_hot's all-zero
//      row - and counts in *bad_rows; nothing is read out of bounds.  Q is GATHERED, where the reference forms
//      reduce_sum(q * one_hot): a non-finite value in a column that was not chosen does not poison the row (0 * inf = NaN
//      there), and a chosen -0.0 stays -0.0 (the sum's + 0.0 makes it +0.0 there).  Only that one element of q is read;
//   5. hl = (hysteretic && h < 0) ? h / 10.0f : h - a true division;
//   6. g = (2.0f * hl) / (float)rows, and g = g / 10.0f on the rows of the hysteretic branch: d mean(hl^2) / dQ.
// grad_q_out gets g in column a and zeros elsewhere, every element written by this launch (no memset), rounded once to
// the Q dtype.  The loss is a second launch of ONE workgroup over td_out in a fixed order - the kernel boundary is the
// hand-off, there is no ticket and no floating-point atomic, so two calls on the same input give the same bits.
//
// The select kernel's two layouts.  A <= 64: one row per group of G lanes (G the power of two >= A, at least 4), the index
// row one value per lane, 64 / G rows per wave, the arg-max a butterfly inside the group; no LDS.  64 < A <= 4096: one row
// per wave, lane l streams the elements l, l + 64, ... .  The loads are one element per lane, consecutive lanes on
// consecutive addresses (at A = 32 and float32 a wave reads two rows as one 256-byte access).
#pragma once
#include "common.hpp"
#include "memory_kernel.hpp"   // mem_cvt, mem_zero
#include "select_kernel.hpp"   // bf16_bits, q_to_f64, arg_take, arg_reduce

namespace diral {

constexpr int kTdMaxA = kSelMaxA;
constexpr int kTdMaxRows = 1 << 24;            // (float)rows is exact
constexpr int kTdBlock = 256;                  // A <= 64: four waves of 64 / G rows each; the loss: its one workgroup

struct TdParams {
  const void* q;                 // [rows][A] of QT, or null: targets only
  const void* qn_target;         // [rows][A]
  const void* qn_eval;           // [rows][A] or null (the plain DQN target)
  const int32_t* actions;        // [rows] (not read without q)
  const void* rewards;           // [rows] of RT
  int rows, A, gshift;
  float gamma;                   // (float)gamma
  float rows_f;                  // (float)rows
  int hysteretic;
  float* targets_out;            // [rows] or null
  float* td_out;                 // [rows] or null: hl
  int32_t* next_action_out;      // [rows] or null
  void* grad_q_out;              // [rows][A] of QT or null
  int32_t* bad_rows;             // null, or a counter of the rows whose action is outside [0, A)
};

template <typename QT>
__device__ __forceinline__ float q_to_f32(QT v) { return (float)q_to_f64(v); }   // exact: QT is float or narrower

// steps 2 and 3 of a row whose next action is j; uniform over the row's lanes
template <typename QT, typename RT>
__device__ __forceinline__ float td_target(const TdParams& p, long long row, int j) {
  const float nv = q_to_f32(static_cast<const QT*>(p.qn_target)[(size_t)row * p.A + j]);
  const float disc = p.gamma * nv;
  return (float)((double)static_cast<const RT*>(p.rewards)[row] + (double)disc);
}

// steps 4 to 6
struct TdRow { int a; bool inside; float hl, g; };
template <typename QT>
__device__ __forceinline__ TdRow td_error(const TdParams& p, long long row, float target) {
  TdRow r;
  r.a = p.actions[row];
  r.inside = r.a >= 0 && r.a < p.A;
  const float Q = r.inside ? q_to_f32(static_cast<const QT*>(p.q)[(size_t)row * p.A + r.a]) : 0.0f;
  const float h = Q - target;
  const bool damped = p.hysteretic && h < 0.0f;
  r.hl = damped ? h / 10.0f : h;
  r.g = (2.0f * r.hl) / p.rows_f;
  if (damped) r.g = r.g / 10.0f;
  return r;
}

// A <= 64.  grid: blocks of four waves, wave w serves the rows w * (64 >> gshift) ...
template <typename QT, typename RT>
__global__ __launch_bounds__(kTdBlock) void td_head_kernel(TdParams p) {
  const int lane = threadIdx.x & 63;
  const int A = p.A, gshift = p.gshift;
  const int g = lane & ((1 << gshift) - 1);
  const long long wave = ((long long)blockIdx.x * kTdBlock + threadIdx.x) >> 6;
  const long long row = (wave << (6 - gshift)) + (lane >> gshift);
  const bool live = row < (long long)p.rows, have = live && g < A;
  const size_t at = (size_t)row * A + g;
  const QT* index = static_cast<const QT*>(p.qn_eval ? p.qn_eval : p.qn_target);
  double bv = have ? q_to_f64(index[at]) : -__builtin_inf();
  int bi = have ? g : 0x7fffffff;
  arg_reduce(bv, bi, lane, gshift);                                 // np.argmax (drl_drqn.py:278; :284's np.max)
  float target = 0.0f;
  if (live) {
    target = td_target<QT, RT>(p, row, bi);
    if (g == 0) {
      if (p.targets_out) p.targets_out[row] = target;
      if (p.next_action_out) p.next_action_out[row] = bi;
    }
  }
  if (!p.q) return;
  bool bad = false;
  if (live) {
    const TdRow r = td_error<QT>(p, row, target);
    bad = !r.inside && g == 0;
    if (g == 0 && p.td_out) p.td_out[row] = r.hl;
    if (have && p.grad_q_out)
      static_cast<QT*>(p.grad_q_out)[at] = (r.inside && g == r.a) ? mem_cvt<QT, float>(r.g) : mem_zero<QT>();
  }
  const unsigned long long bm = __ballot(bad);
  if (p.bad_rows && bm != 0ull && lane == 0) atomicAdd(p.bad_rows, (int)__popcll(bm));
}

// A > 64.  grid: one wave (a block of 64 threads) per row.
template <typename QT, typename RT>
__global__ __launch_bounds__(64) void td_head_wide_kernel(TdParams p) {
  const int lane = threadIdx.x, A = p.A;
  const long long row = blockIdx.x;                                 // (the grid is `rows` blocks)
  const QT* index = static_cast<const QT*>(p.qn_eval ? p.qn_eval : p.qn_target) + (size_t)row * A;
  double bv = -__builtin_inf();
  int bi = 0x7fffffff;
  for (int j = lane; j < A; j += 64) arg_take(bv, bi, q_to_f64(index[j]), j);
  arg_reduce(bv, bi, lane, 6);
  const float target = td_target<QT, RT>(p, row, bi);
  if (lane == 0) {
    if (p.targets_out) p.targets_out[row] = target;
    if (p.next_action_out) p.next_action_out[row] = bi;
  }
  if (!p.q) return;
  const TdRow r = td_error<QT>(p, row, target);
  if (lane == 0) {
    if (p.td_out) p.td_out[row] = r.hl;
    if (!r.inside && p.bad_rows) atomicAdd(p.bad_rows, 1);
  }
  if (p.grad_q_out) {
    QT* grad = static_cast<QT*>(p.grad_q_out) + (size_t)row * A;
    for (int j = lane; j < A; j += 64) grad[j] = (r.inside && j == r.a) ? mem_cvt<QT, float>(r.g) : mem_zero<QT>();
  }
}

// mean(hl^2) behind the launch above.  grid: ONE workgroup.  Thread t adds the rows t, t + 256, ... one after the other
// in double (the square of a float32 is exact there), the 256 partial sums are added in index order, the loss is
// (float)(sum / rows).
__global__ __launch_bounds__(kTdBlock) void td_loss_kernel(const float* td, int rows, float* loss_out) {
  __shared__ double part[kTdBlock];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < rows; i += kTdBlock) {
    const double v = (double)td[i];
    const double sq = v * v;
    s = s + sq;
  }
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    double sum = 0.0;
    for (int k = 0; k < kTdBlock; ++k) sum = sum + part[k];
    *loss_out = (float)(sum / (double)rows);
  }
}

}  // namespace diral
