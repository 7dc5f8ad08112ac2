// step_subwave.hpp - the env step for toy-size envs: G = 4 or 8 lanes per env, 16 or 8 envs per wavefront.
//
// The reference ships one family of configurations, configs/4ue_3r_toy (4 vehicles, 3 resources).  step_kernel.hpp and
// step_fast64.hpp give such an env a 256-thread workgroup with 4 live lanes per wave; here lane g * G + u of a wave is
// viewer u of the wave's g-th env, a 256-thread block holds 256 / G envs and the grid is ceil(B / (256 / G)).
//
// This header holds ONE copy of every phase of a slot, as __forceinline__ functions (values in, values out), and the
// one-slot kernel built from them; step_subwave_slots.hpp runs the same phases inside its slot loop.  What differs
// between the two kernels stays in the kernels: where per-vehicle state is loaded from, what is stored behind a slot and
// what behind the launch, how the metric columns are accumulated.
//
// One launch of step_subwave_kernel does what step_kernel<1, false> does for one slot (my_step / my_step_ch /
// my_step_design with every run-time switch of StepParams), on the same planes tkey[b][k][u] / tx[b][k][u]: it is that
// kernel's statement with "wave" read as "lane group".  A lane keeps its viewer's N <= 8 table entries (key + xpos) in
// registers across the slot; an env's positions are staged in the group's 2 x G doubles of LDS (written and read by one
// wave: no workgroup barrier anywhere).
//
// The rules that keep these kernels from hanging or faulting.  Every cross-lane operation of the family - the ballots
// masked to the group, the __shfl of width G - is in this header (the slot loop adds the shaping sum's shuffles only), so
// this is where they are stated, and they bind the phase functions and their callers alike:
//   * config and mode are uniform over the launch, per-env data (who transmits, who is in range, who is closest) is not.
//     Every __ballot and __shfl sits in control flow whose trip counts are N, A, K (slots or bins) or the compile-time G,
//     or in a branch on a launch-uniform switch; nothing cross-lane inside a branch or a loop that depends on env data,
//     and no phase function is called from one;
//   * anything that depends on env data is predicated BY VALUE; groups past B and lanes u >= N run the same instruction
//     stream with their loads clamped to env 0 / vehicle 0 and their stores predicated off; there is no early return
//     and no workgroup barrier;
//   * the group's LDS positions are written and read by one wave: wave_lds_order() stands between the write and the
//     reads, and - where a kernel rewrites them slot after slot - between a slot's last read and the next write.
// The phases take and give plain scalars and register arrays; an aggregate holding an array, passed by reference, left a
// stack object (48 B/lane of scratch), which is why the histogram travels as four words and a count.
#pragma once
#include "common.hpp"
#include "ref_math.hpp"
#include "rich_out.hpp"
#include "wave_ops.hpp"

namespace diral {

constexpr int kSubwaveThreads = 256;

// Network.calculate_reward_weights (network.py:273-300) for the transmitter set `mk` of one env: calculate_avg_distance
// in combinations order, serial sum (network.py:307-316).  gx / gy: the env's positions (LDS).
__device__ inline int subwave_reward_weight(const StepParams& p, unsigned int mk, const double* gx, const double* gy) {
  double s = 0.0;
  int cnt = 0;
  unsigned int ma = mk;
  while (ma) {
    const int a = __builtin_ctz(ma);
    ma &= ma - 1;
    unsigned int mb = ma;
    while (mb) {
      const int b = __builtin_ctz(mb);
      mb &= mb - 1;
      s = s + dist2d(gx[a], gy[a], gx[b], gy[b]);
      ++cnt;
    }
  }
  const double m = s / (double)cnt;
  return weight_from_mean(p, m, gx, gy);
}

// A lane's place in the launch and the launch-uniform switches the phases share (scalars only).
struct SubwaveLane {
  int u, uc;                 // viewer; clamped to vehicle 0 where the lane is not valid
  int gbase;                 // first lane of the group in its wave
  bool valid;                // env < B and u < N
  size_t b, bN, bR;          // env (clamped to 0: every load stays inside the handle's buffers), b * N, b * NR
  bool piggy, track_la, want_prr, mobile;
  double *gx, *gy;           // the env's positions in LDS, one wave writes and reads them
};

template <int G>
__device__ __forceinline__ SubwaveLane subwave_lane(const StepParams& p, double* s_px, double* s_py) {
  static_assert(G == 4 || G == 8, "lanes per env");
  const int tid = threadIdx.x;
  const long long benv = (long long)blockIdx.x * (kSubwaveThreads / G) + (tid / G);
  SubwaveLane L;
  L.u = tid & (G - 1);
  L.gbase = (tid & 63) & ~(G - 1);
  L.valid = benv < (long long)p.B && L.u < p.N;
  L.b = L.valid ? (size_t)benv : 0;
  L.uc = L.valid ? L.u : 0;
  L.bN = L.b * p.N;
  L.bR = L.b * p.NR;
  L.piggy = (p.flags & DIRAL_F_ADD_POSDIST_PIGGY) != 0;
  L.track_la = (p.flags & DIRAL_F_TRACK_ARRIVAL) && p.la != nullptr;
  L.want_prr = p.mode == DIRAL_STEP_MY_STEP_CH || (p.mode == DIRAL_STEP_MY_STEP && (p.flags & DIRAL_F_TRACK_PRR));
  L.mobile = (p.flags & DIRAL_F_MOBILITY) != 0;
  L.gx = s_px + (tid - L.u);
  L.gy = s_py + (tid - L.u);
  return L;
}

// The viewer's table entries tkey[b][k][u] / tx[b][k][u], k < N, into registers; 0 elsewhere.
template <int G>
__device__ __forceinline__ void subwave_load_entries(const StepParams& p, const SubwaveLane& L, unsigned int (&w1)[G],
                                                     double (&xo)[G]) {
#pragma unroll
  for (int k = 0; k < G; ++k) {
    const bool ok = L.valid && k < p.N;
    const size_t idx = (L.bR + (ok ? k : 0)) * p.NV + L.uc;
    const unsigned int w = p.tkey[idx];
    const double x = p.tx[idx];
    w1[k] = ok ? w : 0u;
    xo[k] = ok ? x : 0.0;
  }
}

// P0: the action a lane runs with (-1: no vehicle, or an action outside 0 ... A - 1, which raises kErrAction) ...
__device__ __forceinline__ int subwave_action(const StepParams& p, const SubwaveLane& L, int a) {
  const bool bad = a < 0 || a >= p.A;
  if (L.valid && bad) atomicOr(p.err, kErrAction);
  return (L.valid && !bad) ? a : -1;
}
// ... and the post-move x of a vehicle at x with velocity v
__device__ __forceinline__ double subwave_move(const StepParams& p, const SubwaveLane& L, long long slot, double x, double v) {
  double nx = x;
  if (L.mobile) {
    if (p.trace) {                                                   // replay branch, network.py:194-199
      long long tt = slot % p.trace_len;
      if (tt < 0) tt += p.trace_len;
      const size_t base = p.trace_per_env ? L.b * p.trace_len : 0;
      nx = p.trace[(base + (size_t)tt) * p.N + L.uc];
    } else {
      nx = py_mod_pos(x + v + p.L, p.L);                             // network.py:203
    }
  }
  return nx;
}

// P1: per resource: tx set, closest in-range tx per viewer, the collision value.  Reads the group's LDS positions (the
// caller has written them and ordered the write).  Writes the channel observation - `chobs_out` (null in the slot loop)
// and the section of state row `row` of `state_out` (null where no state leaves) - and the arrival stamps.
struct SubwaveSearch {
  unsigned long long mtab;   // 4 bits per resource: the gather source m_i(u) of the merge
  unsigned int my_mk;        // the transmitter set of this vehicle's resource
  double my_rtx, my_rv;      // received / in range of a colliding transmitter; its resource's collision value
};
template <int G, bool OUT64>
__device__ __forceinline__ SubwaveSearch subwave_search(const StepParams& p, const SubwaveLane& L, int myact, double mypx,
                                                        double mypy, long long slot, void* chobs_out, void* state_out,
                                                        size_t row) {
  constexpr unsigned int GM = (1u << G) - 1u;
  const int u = L.u, N = p.N, A = p.A, mode = p.mode;
  const bool valid = L.valid, track_la = L.track_la;
  const size_t bN = L.bN;
  if (p.off_chobs < 0) state_out = nullptr;                          // (a row without the section)
  // distance of this viewer to every vehicle of its env, once for all resources
  double dist[G];
  unsigned int inr_bits = 0u;
#pragma unroll
  for (int w = 0; w < G; ++w) {
    dist[w] = dist2d(L.gx[w], L.gy[w], mypx, mypy);
    inr_bits |= (dist[w] < p.Rc ? 1u : 0u) << w;
  }
  SubwaveSearch s = {0ull, 0u, 1.0, 0.0};
  for (int i = 0; i < A; ++i) {
    const bool is_tx = myact == i;
    const unsigned int mk = (unsigned int)(__ballot(is_tx) >> L.gbase) & GM;
    const int c = __popc(mk);
    const bool rx = valid && !is_tx;
    double best = 100000.0;                                          // network.py:385-386
    int bid = -1;
    // Network.find_closest_tx (network.py:378-398), ascending tx id, strict <
#pragma unroll
    for (int w = 0; w < G; ++w) {
      const bool tx_w = (mk >> w) & 1u;
      const bool inr = (inr_bits >> w) & 1u;
      if (tx_w && inr && dist[w] < best) { best = dist[w]; bid = w; }
      if (track_la && tx_w && rx && !inr) p.la[(bN + w) * N + u] = -1;   // network.py:394
    }
    const bool got = rx && bid >= 0;
    s.mtab |= (unsigned long long)(got ? bid : u) << (4 * i);
    if (L.want_prr) {
      // received[tx] / in_range[tx] of a colliding transmitter (test_env.py:395-405); the ballots are unconditional
      int n_in = 0, n_rec = 0;
#pragma unroll
      for (int w = 0; w < G; ++w) {
        const bool tx_w = (mk >> w) & 1u;
        const unsigned int m_in = (unsigned int)(__ballot(rx && tx_w && ((inr_bits >> w) & 1u)) >> L.gbase) & GM;
        const unsigned int m_rec = (unsigned int)(__ballot(rx && bid == w) >> L.gbase) & GM;
        if (w == u) { n_in = __popc(m_in); n_rec = __popc(m_rec); }
      }
      if (is_tx && c > 1) s.my_rtx = n_in > 0 ? (double)n_rec / (double)n_in : 1.0;
    }
    if (valid) {
      // channel observation of the reference step (`obs[user][i]`)
      if (chobs_out || state_out) {
        double ob = 0.0;
        if (!is_tx && c > 0) {
          if (mode == DIRAL_STEP_MY_STEP && p.state_type == 2) ob = best;          // test_env.py:240
          else ob = 1.0;                                                            // :228, :306, :432
        }
        if (chobs_out) rich_store<OUT64>(chobs_out, (bN + u) * A + i, ob);
        if (state_out) rich_store<OUT64>(state_out, row * p.S + p.off_chobs + i, ob);
      }
      if (track_la && mode == DIRAL_STEP_MY_STEP_CH && got) p.la[(bN + bid) * N + u] = (int32_t)slot;   // test_env.py:436
    }
    if (is_tx) {
      s.my_mk = mk;
      if (mode == DIRAL_STEP_MY_STEP && c > 1) {
        // test_env.py:163-199, one value per resource (every transmitter of it computes the same one)
        const int rd = p.reward_design;
        const int wgt = collision_uses_weight(rd, c) ? subwave_reward_weight(p, mk, L.gx, L.gy) : 0;
        s.my_rv = collision_value(rd, c, wgt);
      }
    }
  }
  return s;
}

// P2: reward per transmitter.  `pfc`: the vehicle's proportional-fair counter, in and out (used where `pf_on`).
struct SubwaveReward {
  double r, prr;
  int sole, coll;
};
__device__ __forceinline__ SubwaveReward subwave_reward(const StepParams& p, const SubwaveLane& L, int myact,
                                                        const SubwaveSearch& s, double mypx, double mypy, bool pf_on, int& pfc) {
  SubwaveReward o = {0.0, 0.0, 0, 0};
  if (L.valid && myact >= 0) {
    const int c = __popc(s.my_mk);
    if (p.mode == DIRAL_STEP_MY_STEP) {                                         // test_env.py:211-222
      if (c > 1) {
        o.r = s.my_rv;
        if (pf_on) {
          if (pfc > p.pf_threshold) o.r = p.pf_penalty;
          pfc = pfc + 1;
        }
        o.coll = 1; o.prr = s.my_rtx;
      } else {
        o.r = 1.0;
        if (pf_on) pfc = 0;
        o.sole = 1; o.prr = 1.0;
      }
    } else if (p.mode == DIRAL_STEP_MY_STEP_CH) {                               // test_env.py:411-429
      const double R = (c > 1) ? s.my_rtx : 1.0;
      o.r = ch_reward(p.reward_design, c > 1, R);
      if (c > 1) o.coll = 1; else o.sole = 1;
      o.prr = R;
    } else {                                                                    // test_env.py:297-301, 319-349
      if (c == 1) { o.r = 1.0; o.sole = 1; }
      else {
        int n = 1;
        double dlast = 0.0;
        unsigned int m = s.my_mk & ~(1u << L.u);
        while (m) {
          const int v = __builtin_ctz(m);
          m &= m - 1;
          const double d = dist2d(mypx, mypy, L.gx[v], L.gy[v]);
          if (d < 2.0 * p.Rc) { if (n == 1) dlast = d; ++n; }                   // network.py:122-133
        }
        if (n == 1) o.r = 1.0;
        else if (n == 2) o.r = ((dlast / 1.0) > p.Rc * 2.0) ? 0.0 : -2.0;        // network.py:135-157
        else o.r = -(double)n;
        o.coll = 1;
      }
    }
  }
  return o;
}

// The env's metric sums of a slot (prr counted where `want_prr`): a tree over the group, every lane taking part.
template <int G>
__device__ __forceinline__ SubwaveReward subwave_group_sums(const SubwaveReward& v, bool want_prr) {
  SubwaveReward s = {v.r, want_prr ? v.prr : 0.0, v.sole, v.coll};
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
    s.r += __shfl_xor(s.r, off, G);
    s.prr += __shfl_xor(s.prr, off, G);
    s.sole += __shfl_xor(s.sole, off, G);
    s.coll += __shfl_xor(s.coll, off, G);
  }
  return s;
}

// P3: neighbour-table stamp + gossip merge + observation histogram on the viewer's entries w1[k] / xo[k], which come out
// updated.  STORE: tkey of every valid entry and tx of every changed one go to the planes here (the one-slot kernel; the
// slot loop keeps them in registers and writes them behind its last slot).  The histogram (where `want_hist`) is 4 bits
// per bin in h0 ... h3 - K <= 64 bins, at most N - 1 <= 7 entries per viewer - and their number in cnt.
template <int G, bool STORE>
__device__ __forceinline__ void subwave_merge(const StepParams& p, const SubwaveLane& L, unsigned long long mtab, double mypx,
                                              double mynpx, double mypy, bool want_hist, unsigned int (&w1)[G], double (&xo)[G],
                                              unsigned long long& h0, unsigned long long& h1, unsigned long long& h2,
                                              unsigned long long& h3, unsigned int& cnt) {
  const int u = L.u, N = p.N;
  const bool valid = L.valid;
  bool seq_ovf = false;
  unsigned int key[G];
  h0 = h1 = h2 = h3 = 0ull;
  cnt = 0u;
  // Vehicle.periodic_update (vehicle.py:56-70), branch-free
#pragma unroll
  for (int k = 0; k < G; ++k) {
    const bool own = valid && u == k;
    const unsigned int w = w1[k];
    const unsigned int seq = (w >> 8) + (own ? 1u : 0u);
    const unsigned int a0 = w & 255u;
    const unsigned int age = own ? 0u : (a0 + (a0 < 255u ? 1u : 0u));
    seq_ovf = seq_ovf || (own && seq >= (1u << 24) - 1u);
    w1[k] = (valid && k < N) ? ((seq << 8) | age) : 0u;
    key[k] = (w1[k] & ~255u) | (unsigned int)u;
    if (own) xo[k] = mypx;                                            // own stamp (vehicle.py:63)
  }
  // Vehicle.received_update as the column statement of step_kernel.hpp: key[u] = max(key[u], key[m_i(u)]) on
  // (sequence number, source) for resources in order; m_i(u) == u where viewer u receives nothing on i
  for (int i = 0; i < p.A; ++i) {
    const int m = (int)((mtab >> (4 * i)) & 15ull);
#pragma unroll
    for (int k = 0; k < G; ++k) {
      const unsigned int v = (unsigned int)__shfl((int)key[k], m, G);
      key[k] = max(key[k], v);
    }
  }
  // xpos follows the winning sequence number from the recorded source, age resets on change (an entry that is not
  // valid has sequence number 0 on every lane of the group: it never changes and stays 0 / 0.0)
#pragma unroll
  for (int k = 0; k < G; ++k) {
    const unsigned int kf = key[k], w = w1[k];
    const int src = (int)(kf & 255u);
    const bool upd = ((kf ^ w) >> 8) != 0u;
    const double xg = __shfl(xo[k], src, G);
    const double xn = upd ? xg : xo[k];
    const unsigned int wn = upd ? (kf & ~255u) : w;
    w1[k] = wn;
    xo[k] = xn;
    if (valid && k < N) {
      if constexpr (STORE) {
        p.tkey[(L.bR + k) * p.NV + u] = wn;
        if (upd || u == k) p.tx[(L.bR + k) * p.NV + u] = xn;
      }
      // Network.dist_piggy + get_positional_dist_2_piggy (network.py:538-558, 473-513)
      const int age = (int)(wn & 255u);
      if (want_hist && u != k && age < p.age_limit) {
        const double x1 = xn;
        const double y1 = ((wn >> 8) > 0u) ? L.gy[k] : 0.0;
        const double d = dist2d(x1, y1, mynpx, mypy);
        if (d < p.Rb) {
          const double v = (x1 - mynpx > 0.0) ? d : -d;
          const int bin = hist_bin(v, -p.Rb, p.hist_inv_width, p.K, p.edges);
          const unsigned long long one = 1ull << (4 * (bin & 15));
          const int hw = bin >> 4;
          h0 += hw == 0 ? one : 0ull; h1 += hw == 1 ? one : 0ull;
          h2 += hw == 2 ? one : 0ull; h3 += hw == 3 ? one : 0ull;
          cnt += 1u;
        }
      }
    }
  }
  if (seq_ovf) atomicOr(p.err, kErrSeq);
}

// A launch-uniform int in a scalar register of its own.  The section offsets of StepParams arrive as one 8-dword scalar
// load; where that tuple is spilled, every branch of the row loop below reloads all of it (72 v_readlane per row element
// in the slot loop against 8 with the offsets apart: the loop is most of a slot whose state leaves).
__device__ __forceinline__ int own_sgpr(int v) {
  asm("" : "+s"(v));
  return v;
}

// The viewer's own state row `row` of `state_out`, section by section (test_env.py:527-583); the channel observation
// was written in P1, the sorted distances and the type-1 histogram belong to posdist_kernel.hpp.  `rcol`: the reward
// column; myvel: the velocity the slot ran with.
template <bool OUT64>
__device__ __forceinline__ void subwave_state_row(const StepParams& p, void* state_out, size_t row, int u, int myact,
                                                  unsigned long long h0, unsigned long long h1, unsigned long long h2,
                                                  unsigned long long h3, unsigned int cnt, double rcol, double mynpx,
                                                  double mypy, double myvel) {
  const int S = p.S, A = p.A;
  const int off_act = own_sgpr(p.off_act), off_chobs = own_sgpr(p.off_chobs), off_hist = own_sgpr(p.off_hist),
            off_posdist = own_sgpr(p.off_posdist), off_rew = own_sgpr(p.off_rew), off_idx = own_sgpr(p.off_idx),
            off_pos = own_sgpr(p.off_pos), off_vel = own_sgpr(p.off_vel), off_fp = own_sgpr(p.off_fp);
  const bool real = (p.flags & DIRAL_F_ACTION_REAL) != 0;
  for (int s = 0; s < S; ++s) {
    double val = 0.0;
    bool write = true;
    if (off_act >= 0 && s >= off_act && s < off_act + (real ? 1 : A)) {
      val = real ? (double)myact : ((myact == s - off_act) ? 1.0 : 0.0);     // test_env.py:585-595
    } else if (off_chobs >= 0 && s >= off_chobs && s < off_chobs + A) {
      write = false;
    } else if (off_hist >= 0 && s >= off_hist && s < off_hist + p.K) {
      if (p.posdist_type != 2) write = false;
      const int bin = s - off_hist, hw = bin >> 4;
      const unsigned long long word = hw == 0 ? h0 : (hw == 1 ? h1 : (hw == 2 ? h2 : h3));
      const unsigned int h = (unsigned int)(word >> (4 * (bin & 15))) & 15u;
      val = cnt ? (double)h / (double)cnt : 0.0;                                // network.py:501
    } else if (off_posdist >= 0 && s >= off_posdist && s < off_posdist + p.N - 1) {
      write = false;
    } else if (s == off_rew) {
      val = rcol;
    } else if (s == off_idx) {
      val = (double)(u + 1);
    } else if (off_pos >= 0 && s == off_pos) {
      val = mynpx / p.L;                                                        // network.py:403-407
    } else if (off_pos >= 0 && s == off_pos + 1) {
      val = mypy / p.H;
    } else if (s == off_vel) {
      val = myvel;
    } else if (off_fp >= 0 && s == off_fp) {
      val = p.episode;
    } else if (off_fp >= 0 && s == off_fp + 1) {
      val = p.eps;
    }
    if (write) rich_store<OUT64>(state_out, row * S + s, val);
  }
}

// One slot per launch.  The second launch bound is waves per SIMD: the 4 (G = 4, 128 VGPRs) and 3 (G = 8) this kernel ran
// at before its phases became functions; without it the allocation ends one wave lower, with it nothing spills.
template <int G, bool OUT64>
__global__ __launch_bounds__(kSubwaveThreads, G == 4 ? 4 : 3) void step_subwave_kernel(const StepParams p) {
  __shared__ double s_px[kSubwaveThreads];
  __shared__ double s_py[kSubwaveThreads];
  const SubwaveLane L = subwave_lane<G>(p, s_px, s_py);
  const int u = L.u;
  const bool valid = L.valid;
  const size_t b = L.b, bN = L.bN;
  const bool want_hist = L.piggy && p.posdist_type == 2 && p.state_out != nullptr && p.off_hist >= 0;
  const bool pf_on = (p.flags & DIRAL_F_PROPORTIONAL_FAIR) && p.mode == DIRAL_STEP_MY_STEP;
  const long long slot = p.t + (p.t_dev ? *p.t_dev : 0ll);

  // ---- the viewer's table entries, issued before any compute ----------------
  unsigned int w1[G];
  double xo[G];
  if (L.piggy) subwave_load_entries<G>(p, L, w1, xo);

  // ---- P0: per-vehicle state, the post-move position ------------------------
  const int a = p.actions[bN + L.uc];
  const double x = p.pos_x[bN + L.uc], y = p.pos_y[bN + L.uc], v = p.vel[bN + L.uc];
  const double nx = subwave_move(p, L, slot, x, v);
  const int myact = subwave_action(p, L, a);
  const double mypx = valid ? x : 0.0, mypy = valid ? y : 0.0, myvel = valid ? v : 0.0, mynpx = valid ? nx : 0.0;
  L.gx[u] = mypx; L.gy[u] = mypy;
  wave_lds_order();

  // ---- P1, P2 and the env's metric sums --------------------------------------
  const SubwaveSearch found = subwave_search<G, OUT64>(p, L, myact, mypx, mypy, slot, p.chobs_out, p.state_out, bN + u);
  const bool tx = valid && myact >= 0;
  int pfc = 0;
  if (pf_on && tx) pfc = p.pf[bN + u];
  const SubwaveReward rw = subwave_reward(p, L, myact, found, mypx, mypy, pf_on, pfc);
  if (pf_on && tx) p.pf[bN + u] = pfc;
  if (tx && p.rew_out) rich_store<OUT64>(p.rew_out, bN + u, rw.r);
  const SubwaveReward sum = subwave_group_sums<G>(rw, L.want_prr);

  // ---- P3: the entries go back to the planes from inside the merge -----------
  unsigned long long h0 = 0ull, h1 = 0ull, h2 = 0ull, h3 = 0ull;
  unsigned int cnt = 0u;
  if (L.piggy) subwave_merge<G, true>(p, L, found.mtab, mypx, mynpx, mypy, want_hist, w1, xo, h0, h1, h2, h3, cnt);

  // ---- P4: write-back: positions, done flag, metrics, state vectors ----------
  if (valid) {
    p.pos_x[bN + u] = mynpx;
    if (u == 0) {
      if (p.done_out) p.done_out[b] = (uint8_t)((slot % p.episode_interval) == p.episode_interval - 1);
      double* mt = p.metrics + b * DIRAL_M_COLUMNS;
      mt[DIRAL_M_SLOTS] += 1.0;
      mt[DIRAL_M_SUM_REWARD] += sum.r;
      mt[DIRAL_M_TX_SOLE] += (double)sum.sole;
      mt[DIRAL_M_TX_COLLIDED] += (double)sum.coll;
      if (L.want_prr) { mt[DIRAL_M_PRR_SUM] += sum.prr; mt[DIRAL_M_PRR_CNT] += (double)sum.sole + (double)sum.coll; }
    }
    if (p.state_out) subwave_state_row<OUT64>(p, p.state_out, bN + u, u, myact, h0, h1, h2, h3, cnt, rw.r, mynpx, mypy, myvel);
  }
}

}  // namespace diral
