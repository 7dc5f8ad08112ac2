// step_fast64.hpp - the fused env-step kernel specialised for the headline
// configuration: N <= 64 vehicles (one wavefront lane per vehicle), A <= 64
// resources, the toy YAML's State flags (one-hot action + type-2 piggybacked
// positional histogram), my_step / my_step_ch / my_step_design + obtain_state,
// float32 or float64 outputs.
//
// Same semantics as step_kernel.hpp (which stays the general path and is what
// the parity tests compare this kernel against, bit for bit); what changes is
// the schedule.  Profiling on MI355X (profiles/) showed the general kernel
//   - LATENCY-bound on LDS round trips (63 % of wave cycles waiting),
//   - then instruction-ISSUE-bound (~7000 instructions per wave, 16 waves per
//     SIMD per launch), with ~90 KB of inlined rare-path code (sqrt/exp/fmod),
//   - with the gossip merge sitting on the CU-shared LDS pipe (a
//     ds_bpermute_b32 costs ~5.5 LDS cycles; one env-slot needs ~1800).
// So here:
//   * closest-transmitter search without LDS: lane = vehicle, a transmitter's
//     position is broadcast with v_readlane; each wave owns the groups of four
//     resources g == wave (mod 4), g = i / 4, and walks their transmitters in
//     ascending id with a strict '<' (the reference's lowest-id tie-break,
//     network.py:387-392);
//   * gossip merge key[u] = max(key[u], key[m_i(u)]): one ds_bpermute + max per
//     (resource, column PAIR): two columns travel as 16-bit (rank, source) keys in
//     one register (exactness argument and fallback at the merge loop);
//   * a compact parameter block, 32-bit table offsets, padded
//     viewer stride (NV = 64) so table loads/stores need no lane predicate;
//   * when every vehicle has y == 0 (any random topology, network.py:104) the
//     distance is |dx| exactly and the dy logic is compiled out (FLAT);
//   * branch-free histogram bin search; rare paths out of line.
// (No kernel in this header: the body, step_fast64_body.inc, is compiled by k_fast64.hip.)
#pragma once
#include "common.hpp"
#include "policy_device.hpp"
#include "ref_math.hpp"
#include "rich_out.hpp"
#include "step_params.hpp"
#include "wave_ops.hpp"

namespace diral {

#ifndef DIRAL_FAST_MINWAVES_KS
#define DIRAL_FAST_MINWAVES_KS 6        // step_fast64_slots_kernel (K slots per launch): <= 84 VGPRs, six workgroups per CU.  C2, 4096 envs,
                                        // K = 25, us per slot: 57.4 / 52.6 / 50.8 / 55.8 for 4 / 5 / 6 / 7 (the one-slot fused launch: 56.8)
#endif
#ifndef DIRAL_FAST_MINWAVES
#define DIRAL_FAST_MINWAVES 7           // <= 72 VGPRs, 7 waves/SIMD.  8 (64 VGPRs) was the optimum while the phases were latency-bound;
                                        // with the xpos ring (VALU-bound, 15 spilled registers at 64) 7 is 3 % faster, 6 no better
#endif

struct FastLds {
  uint32_t rv, edges, mask, act, hist, cnt, slow, inv, mtab, rtx, inr, px, py, npx, rew, stage, nact, kvel, ia, total;
};
// row stride (elements) of the channel-observation staging array [vehicle][resource] of the RICH
// instantiations: a multiple of 4 elements, so that the write-out reads a 16-byte piece of a row
// with ONE ds_read_b128 (f32) / ds_read_b128 of two doubles - and P1 (lane = vehicle) writes a group of
// four resources with one ds_write_b128 (fast_stage_store4); the 4 extra elements skew the rows over
// the banks
__host__ __device__ constexpr int fast_stage_stride(int A) { return (A <= 32 ? 32 : 64) + 4; }
// histogram row stride (words): odd (lane = row: conflict-free increments) and at least K + 1 - slot K of a row is a
// spare that takes the increments of entries that do not count (the column loop needs no exec-mask branch then)
__host__ __device__ constexpr int fast_hist_stride(int K) { return (K + 1) | 1; }
// gather-source table [vehicle][resource], one BYTE per entry (source lane * 4, the ds_bpermute address, <= 252): the
// merge reads the sources of FOUR consecutive resources with one ds_read_b32; the row stride of a32 + 4 bytes = 9 / 17
// words puts the 64 lanes' words - read by the merge, written by P1 a group at a time, lane = row - on distinct banks
__host__ __device__ constexpr int fast_mtab_stride(int A) { return (A <= 32 ? 32 : 64) + 4; }
// The order the slot loops (step_fast64_slots_kernel, `pol`) keep, K- and A-sized arrays in front: their text is the parent's
// (step_fast64_body.inc), and so is what they are compiled to.
__host__ __device__ inline FastLds fast_lds_layout_slots(int K, int A, bool rich, bool out64, bool flat, bool ratios, bool ia) {
  FastLds l;
  uint32_t o = 0;
  const uint32_t a32 = A <= 32 ? 32u : 64u;
  l.rv = o;    o += 8u * a32;
  l.edges = o; o += 8u * (K + 2);
  l.mask = o;  o += 8u * a32;
  l.act = o;   o += 4u * 64;
  l.hist = o;  o += 4u * fast_hist_stride(K) * 64;
  l.cnt = o;   o += 4u * 64;
  l.slow = o;  o += 16u;
  l.inv = o;   o += out64 ? 0u : 8u * 64;
  l.mtab = o;  o += 64u * fast_mtab_stride(A);
  l.rtx = o;   o += ratios ? 8u * 64 : 0u;
  l.inr = o;   o += ratios ? 4u * 64 : 0u;
  l.px = l.py = l.npx = l.rew = l.stage = o;
  if (!rich) { l.px = o; o += 8u * 64; }
  if (rich) {
    l.px = o;  o += 8u * 64;
    l.py = o;  o += flat ? 0u : 8u * 64;
    l.npx = o; o += 8u * 64;
    l.rew = o; o += 8u * 64;
    o = align_up(o, 16);
    l.stage = o; o += (out64 ? 8u : 4u) * 64 * fast_stage_stride(A);
  }
  l.nact = o;  o += 4u * 64;
  o = align_up(o, 8);
  l.kvel = o;  o += 8u * 64;
  l.ia = o;    o += ia ? 8u + 4u * 100 : 0u;
  l.total = align_up(o, 16);
  return l;
}
__host__ __device__ inline FastLds fast_lds_layout(int K, int A, bool rich, bool out64, bool flat, bool ratios = true, bool pol = false,
                                                     bool ia = false) {
  // The arrays whose size depends on neither K nor A come FIRST: their offsets are compile-time constants of an
  // instantiation (every flag below is a template parameter there) and ride in the DS instructions' immediate offsets.
  // Behind them the arrays sized by A (32 or 64 columns), whose offsets are constants plus multiples of one value, and
  // last the two sized by K.  With the K- and A-sized arrays in front, as they were, every offset was a run-time sum that
  // the kernel kept in an SGPR from P0 to P4 - ten of the one-slot kernel's sixteen spilled SGPRs.
  if (pol) return fast_lds_layout_slots(K, A, rich, out64, flat, ratios, ia);
  FastLds l;
  uint32_t o = 0;
  const uint32_t a32 = A <= 32 ? 32u : 64u;
  l.act = o;   o += 4u * 64;
  l.cnt = o;   o += 4u * 64;
  l.slow = o;  o += 16u;                     // the workgroup holds a quad flagged for the keyed path of the next slot
  l.inv = o;   o += out64 ? 0u : 8u * 64;   // float32 outputs: 1.0 / n for the 64 possible neighbour counts (P4), staged in P0
  // (CH and EXTRA instantiations only - `ratios`: without them the RICH workgroup of A <= 32 stays at 20 KB, eight per CU)
  l.rtx = o;   o += ratios ? 8u * 64 : 0u;  // my_step_ch: reception ratio R per transmitter
  l.inr = o;   o += ratios ? 4u * 64 : 0u;  // my_step_ch: receivers in range per transmitter
  l.px = l.py = l.npx = l.rew = l.stage = o;
  if (!rich) { l.px = o; o += 8u * 64; }     // the pre-move positions, for P2 behind the last barrier (RICH: part of the tail below)
  if (rich) {                               // RICH output tail (rich_out.hpp): per-vehicle values by index
    l.px = o;  o += 8u * 64;
    l.py = o;  o += flat ? 0u : 8u * 64;    // every pos_y == 0: not staged (keeps 8 workgroups per CU at A <= 32)
    l.npx = o; o += 8u * 64;
    l.rew = o; o += 8u * 64;
  }
  l.nact = l.kvel = l.ia = o;               // (the slot loops' arrays: above)
  o = align_up(o, 16);
  // -- sized by A
  l.mask = o;  o += 8u * a32;
  l.rv = o;    o += 8u * a32;
  l.mtab = o;  o += 64u * fast_mtab_stride(A);      // [vehicle][resource] gather source lane * 4 (bpermute address), bytes
  if (rich) {                               // (16-byte aligned: everything above is a multiple of 16)
    l.stage = o; o += (out64 ? 8u : 4u) * 64 * fast_stage_stride(A);   // channel observation [vehicle][resource]
  }
  // -- sized by K
  l.edges = o; o += 8u * (K + 2);
  o = align_up(o, 16);                      // (the histogram is zeroed with 16-byte stores: P0)
  l.hist = o;  o += 4u * fast_hist_stride(K) * 64;
  l.total = align_up(o, 16);
  return l;
}

// Reward of a colliding resource (test_env.py:163-199) incl.
// Network.calculate_reward_weights (network.py:273-300); wave-uniform, positions
// broadcast from lanes.  Out of line: runs ~once per colliding resource.
__device__ DIRAL_OUTLINE double fast_collision_reward(int rd, uint32_t flags, double L, double Rc, int N,
                                                                  unsigned long long mk, int c, double mypx,
                                                                  double mypy) {
  int wgt = 0;
  if (rd == 1 || ((rd == 2 || rd == 5) && c == 2)) {
    double s = 0.0;                    // calculate_avg_distance (network.py:307-316)
    int cnt = 0;
    unsigned long long ma = mk;
    while (ma) {
      const int a = __builtin_ctzll(ma);
      ma &= ma - 1;
      const double xa = readlane_f64(mypx, a), ya = readlane_f64(mypy, a);
      unsigned long long mb = ma;
      while (mb) {
        const int b = __builtin_ctzll(mb);
        mb &= mb - 1;
        s = s + dist2d_leaf(xa, ya, readlane_f64(mypx, b), readlane_f64(mypy, b));
        ++cnt;
      }
    }
    const double m = (cnt == 1) ? s : s / (double)cnt;       // s/1 == s exactly
    if (flags & DIRAL_F_TOY_WEIGHTS) {
      double x_min = L + 1, x_max = -L - 1;      // calculate_norm (network.py:225-246)
      int umin = 0, umax = 0;
      for (int u = 0; u < N; ++u) {
        const double x = readlane_f64(mypx, u);
        if (x < x_min) { x_min = x; umin = u; }
        if (x > x_max) { x_max = x; umax = u; }
      }
      wgt = (m == dist2d_leaf(readlane_f64(mypx, umin), readlane_f64(mypy, umin), readlane_f64(mypx, umax),
                         readlane_f64(mypy, umax)));
    } else {
      wgt = (m > Rc);
    }
  }
  // (collision_value, spelled out: see ref_math.hpp)
  if (rd == 1) { const double R = (double)wgt / (double)c; return -1.0 * (1.0 - R); }
  if (rd == 2) return (c == 2) ? 2.0 * (double)wgt - (double)c : 0.0 - (double)c;
  if (rd == 3) { const double R = 1.0 / (double)c; return -1.0 * exp(1.0 - R); }
  if (rd == 4) return 1.0 / (double)c;
  return (c == 2 && wgt == 1) ? 0.0 : -1.0;
}

// The SPS agents of one env decide from the channel observation staged in LDS (POL instantiations): what
// sps_step_wave_kernel<1, T, true> does with the rows it loads from HBM, for the 64 lanes = vehicles of this wave.
// `stage`: [vehicle][SA] of out dtype, as written to chobs_out; `own`: this slot's action of the lane's vehicle.
// Out of line: log10 and the candidate ranking stay out of the step kernel's register allocation; runs once per env.
template <typename T>
__device__ DIRAL_OUTLINE void fast_sps_decide(const T* stage, int SA, int A, int N, size_t bN, int lane, int own,
                                              int& action, int& cnt, const PolParams* q, int ks = 0, bool last = true) {
  // (`action`, `cnt`: the agent's prev_action and reselection counter, loaded by the caller ahead of P3 and kept in its
  // registers from slot to slot of a K-slot launch; slot `ks` draws with seed + ks: what K single-slot calls are given)
  const uint64_t seed = q->seed + (uint64_t)ks + (q->clock ? (uint64_t)*q->clock : 0ull);
  const int i = (int)bN + lane;
  const bool live = lane < N;
  const bool resel = live && sps_advance(i, cnt, q->keep_prob, q->draw_counter, q->draw_keep, seed);
  unsigned int r = 0;
  if (resel) r = q->draw_choice ? (unsigned int)q->draw_choice[i] : (unsigned int)(rng_u64(seed, 9, (uint64_t)i) >> 33);
  unsigned long long todo = __ballot(resel);
  while (todo) {
    const int j = __builtin_ctzll(todo);
    todo &= todo - 1;
    const int prev_j = __builtin_amdgcn_readlane(action, j);
    const int own_j = __builtin_amdgcn_readlane(own, j);
    const unsigned int r_j = (unsigned int)__builtin_amdgcn_readlane((int)r, j);
    double d[1];
    d[0] = lane < A ? (double)stage[j * SA + lane] : 0.0;
    const int ch = sps_choose_chobs_wave<1>(d, lane, A, prev_j, own_j, q->threshold, q->inc_db, r_j);
    if (lane == j) action = ch;
  }
  // (prev_action only ever changes to the action chosen - v2x_sps.py:98 -, so behind the last slot of the launch the
  // agent's action IS its prev_action, whichever slot chose it)
  if (live && last) {
    q->sps_prev[i] = action;
    q->sps_counter[i] = cnt;
    q->actions_out[i] = action;
  }
}

// Four consecutive staged observations of one vehicle (P1, a group of four resources) into its row of the staging
// array: one ds_write_b128 (float), two (double).  `row4` is 16-byte aligned (fast_stage_stride: a multiple of 4).
__device__ __forceinline__ void fast_stage_store4(float* row4, const float (&v)[4]) {
  *reinterpret_cast<float4*>(row4) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void fast_stage_store4(double* row4, const double (&v)[4]) {
  *reinterpret_cast<double2*>(row4) = make_double2(v[0], v[1]);
  *reinterpret_cast<double2*>(row4 + 2) = make_double2(v[2], v[3]);
}

#ifdef DIRAL_TIMING
#define DIRAL_FSTAMP(i) do { if (lane == 0 && p.dbg && !listed) { p.dbg[((size_t)b * 4 + wave) * 8 + (i)] = __builtin_amdgcn_s_memtime(); \
    if ((i) == 7) { __builtin_amdgcn_s_waitcnt(0); atomicMax(&p.dbg[(size_t)p.B * 40 + (((size_t)(p.t & 1) * gridDim.x + b) * 2) + 1], (unsigned long long)__builtin_amdgcn_s_memrealtime()); } } } while (0)
#else
#define DIRAL_FSTAMP(i) do {} while (0)
#endif

// The template parameters of the kernels in step_fast64_body.inc:
// CH: my_step_ch (test_env.py:351-443) instead of my_step: the reward of a transmitter is
// built from its reception ratio (PRR) instead of the collision count; the gossip, the
// move and the observation are the same.
// EXTRA: the rarely used run-time switches (my_step_design, arrival stamps) are compiled in;
// the plain instantiations stay free of them (they cost the headline kernel 4 spilled VGPRs).
// RICH: the output tail of rich_out.hpp (channel observation output, the cheap State flags)
// instead of the fixed [one-hot | histogram] state; `r` is only read by these instantiations.
// POL: the policy epilogue (PolParams: reward shaping + the SPS agents' decisions for the next slot) - RICH instantiations
// of my_step only (step_fast64_slots_kernel: of my_step_ch too - K slots per launch and the enable_channel prefill); `q` is
// only read by these.
}  // namespace diral
