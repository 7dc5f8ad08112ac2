// ref_math.hpp - the reference's arithmetic, one copy each: Network.dist, Python's float `%`, np.histogram's bin, the
// value of a colliding resource (my_step), the reward from the reception ratio (my_step_ch).  Primitives: wave_ops.hpp.
#pragma once
#include "common.hpp"

namespace diral {

// Network.dist (network.py:318-332): sqrt(dx^2 + dy^2) with correctly rounded squares (DESIGN.md on the reference's pow()).
// All four forms rest on one argument: when dy == 0 - every pair in a random topology, where all y are 0 - sqrt(fl(dx*dx))
// == |dx| exactly in IEEE binary64 (no over/underflow for 2^-500 <= |dx| <= 2^500, and for dx == 0), so the sqrt is skipped.
// dist2d compares |dx| as a double; dist2d_leaf keeps the sqrt in line (leaf functions); fast_dist tests the exponent in the
// high word and compiles dy out when FLAT; pd_dist is the high-word test with the sqrt in line (unrolled sweeps).
__device__ DIRAL_OUTLINE double dist_general(double dx, double dy) {
  return __builtin_sqrt(dx * dx + dy * dy);
}
__device__ inline double dist2d(double x1, double y1, double x2, double y2) {
  const double dx = x2 - x1, dy = y2 - y1;
  const double ax = __builtin_fabs(dx);
  // (dx == 0 as well: sqrt(0) == 0 - a vehicle measured against itself, as the transmitter search does)
  if (dy == 0.0 && (ax == 0.0 || (ax >= 0x1p-500 && ax <= 0x1p500))) return ax;
  return dist_general(dx, dy);
}

// dist2d for the out-of-line reward functions: the IEEE sqrt is inlined so that they stay LEAF functions - a nested
// call makes the callee save its return address through a callee-saved VGPR in scratch memory, and a kernel that
// may reach such a callee carries a private segment (16 B / lane) for every wave it launches
__device__ inline double dist2d_leaf(double x1, double y1, double x2, double y2) {
  const double dx = x2 - x1, dy = y2 - y1;
  const double ax = __builtin_fabs(dx);
  if (dy == 0.0 && (ax == 0.0 || (ax >= 0x1p-500 && ax <= 0x1p500))) return ax;
  return __builtin_sqrt(dx * dx + dy * dy);
}

// Network.dist for the fast kernels: the exponent test is two integer ops.
template <bool FLAT>
__device__ inline double fast_dist(double x1, double y1, double x2, double y2) {
  const double dx = x2 - x1;
  const unsigned int hi = (unsigned int)__double2hiint(dx) & 0x7fffffffu;
  // The test is one-sided: beyond 2^500 the square overflows to inf in the reference while |dx| stays finite, but every
  // use of the result compares it with a finite range first - `d < Rc`, `d < Rb`, `d > Rc` - and agrees.  dx == 0 exactly
  // passes too (sqrt(0) == |dx| == 0): the search of P1 measures every transmitter against ITSELF, so without this case
  // each of its iterations pays the out-of-line call for that one lane.
  const bool in_range = hi >= 0x20b00000u || (hi | (unsigned int)__double2loint(dx)) == 0u;
  if (FLAT) {
    if (in_range) return __hiloint2double((int)hi, __double2loint(dx));
    return dist_general(dx, 0.0);
  } else {
    const double dy = y2 - y1;
    if (in_range && dy == 0.0) return __hiloint2double((int)hi, __double2loint(dx));
    return dist_general(dx, dy);
  }
}

// dist2d with the general case in line (the posdist kernels): a call inside an unrolled sweep would force the
// registers of the value array through the calling convention at every call site
__device__ inline double pd_dist(double x1, double y1, double x2, double y2) {
  const double dx = x2 - x1, dy = y2 - y1;
  // |dx| in [2^-500, 2^501) or dx == 0, and dy == 0: sqrt(dx * dx) == |dx| exactly (fast_dist's test on the high word)
  const unsigned int hi = (unsigned int)__double2hiint(dx) & 0x7fffffffu;
  const bool plain = (hi - 0x20b00000u <= 0x3e800000u) || (hi | (unsigned int)__double2loint(dx)) == 0u;
  if (dy == 0.0 && plain) return __hiloint2double((int)hi, __double2loint(dx));
  return __builtin_sqrt(dx * dx + dy * dy);
}

// Python float `%` for the position wrap (network.py:203): fast exact path when 0 <= s <= 2L (Sterbenz), generic fmod + sign fix-up otherwise.
__device__ DIRAL_OUTLINE double py_mod_general(double s, double L) {
  double m = fmod(s, L);
  if (m != 0.0) { if ((L < 0) != (m < 0)) m += L; } else { m = copysign(0.0, L); }
  return m;
}
__device__ inline double py_mod_pos(double s, double L) {
  if (s >= 0.0 && s < L) return s;
  if (s >= L && s <= 2.0 * L) {
    const double r = s - L;            // exact
    return (r >= L) ? r - L : r;       // s == 2L -> 0
  }
  return py_mod_general(s, L);
}

// np.histogram uniform-bin index (numpy/lib/_histograms_impl.py fast path).
// NumPy estimates the index with a division and then corrects it against the
// actual edges ("not guaranteed to give exactly consistent results within ~1
// ULP of the bin edges"), so its result is THE bin with edges[i] <= v <
// edges[i+1].  Any estimate followed by the same edge correction lands in the
// same bin; a reciprocal multiply replaces the f64 division.  `edges` are the
// exact np.linspace values (strictly increasing, checked at create).
__device__ inline int hist_bin(double v, double first, double inv_width, int K, const double* edges) {
  int idx = (int)((v - first) * inv_width);
  idx = idx < 0 ? 0 : (idx > K - 1 ? K - 1 : idx);
  while (idx > 0 && v < edges[idx]) --idx;
  while (idx < K - 1 && v >= edges[idx + 1]) ++idx;
  return idx;
}

// Bin of a value of the type-2 histogram, np.histogram(v, K, range=(-Rb, Rb)) (network.py:500): NumPy estimates the bin from
// (v - first) / (last - first) * K and corrects it by at most one step against the float edges.  The correction can
// only act when v lies within rounding distance of an edge.  With t = (v + Rb) * inv_w: t, the edges (linspace) and the
// comparisons are each within 2^-45 bin widths of their exact values (K <= 64), so if the fractional part of t lies in
// [2^-20, 1 - 2^-20] the value is safely inside bin floor(t) and the edges need not be read - one LDS round trip and two
// f64 compares less per table entry.  `unsafe` lanes (an exact hit of an edge: integer-valued positions) take the reads.
// Requires -Rb <= v < Rb (so 0 <= t <= K; t == K rounds in from below: fractional part 0, unsafe - the edge branch
// clamps the estimate to K - 1 first).
__device__ inline int hist_bin_estimate(double v, double Rb, double inv_w, int K, bool& unsafe) {
  const double t = (v + Rb) * inv_w;
  const int est = (int)t;                        // (t == K: fractional part 0 - the caller's edge branch clamps, hist_bin_clamp)
  const double fr = __builtin_amdgcn_fract(t);
  unsafe = !(__builtin_fabs(fr - 0.5) <= 0.5 - 0x1p-20);
  return est;
}
__device__ inline int hist_bin_clamp(int est, int K) { return est > K - 1 ? K - 1 : est; }

// Network.calculate_reward_weights (network.py:273-300) from the mean pair distance m of calculate_avg_distance: against
// calculate_norm (network.py:225-246) with the toy weights, else against Rc.  Positions in LDS (step_kernel, large_search_kernel).
__device__ inline int weight_from_mean(const StepParams& p, double m, const double* s_px, const double* s_py) {
  if (p.flags & DIRAL_F_TOY_WEIGHTS) {
    double x_min = p.L + 1, x_max = -p.L - 1;
    int umin = 0, umax = 0;
    for (int u = 0; u < p.N; ++u) {
      const double x = s_px[u];
      if (x < x_min) { x_min = x; umin = u; }
      if (x > x_max) { x_max = x; umax = u; }
    }
    return m == dist2d(s_px[umin], s_py[umin], s_px[umax], s_py[umax]);
  }
  return m > p.Rc;
}

// my_step: the value of a resource with c > 1 transmitters (test_env.py:163-199) from the reward design and that weight, which
// only the designs collision_uses_weight names read.  Called by large_search_kernel.  step_kernel, fast_collision_reward and
// wide_collision_reward spell the same statements out (with the call the tuned kernels compile to other code and the general
// kernel measured slower); the latter two also carry their own weight loops (lane broadcasts; LDS, all y == 0): change all.
__device__ inline bool collision_uses_weight(int rd, int c) { return rd == 1 || ((rd == 2 || rd == 5) && c == 2); }
__device__ inline double collision_value(int rd, int c, int wgt) {
  if (rd == 1) { const double R = (double)wgt / (double)c; return -1.0 * (1.0 - R); }
  if (rd == 2) return (c == 2) ? 2.0 * (double)wgt - (double)c : 0.0 - (double)c;
  if (rd == 3) { const double R = 1.0 / (double)c; return -1.0 * exp(1.0 - R); }
  if (rd == 4) return 1.0 / (double)c;
  return (c == 2 && wgt == 1) ? 0.0 : -1.0;
}

// my_step_ch reward of one transmitter (test_env.py:411-429) from its reception ratio
// R = received / in_range (1 for a sole transmitter).  Out of line: exp().
// (Designs other than 2, 3, 4: undefined in the reference, refused by the host - diral_env_step, diral_env_step_policy.)
__device__ DIRAL_OUTLINE double ch_reward(int rd, bool collided, double R) {
  if (collided) {
    if (rd == 3) return 1.0 - exp(1.0 - R);
    if (rd == 4) return -1.0 * exp(1.0 - R);
    return -1.0 * (1.0 - R);
  }
  if (rd == 4) return exp(1.0);
  return 1.0;
}

}  // namespace diral
