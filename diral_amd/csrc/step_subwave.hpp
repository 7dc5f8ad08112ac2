// step_subwave.hpp - the env step for toy-size envs: G = 4 or 8 lanes per env, 16 or 8 envs per wavefront.
//
// The reference ships one family of configurations, configs/4ue_3r_toy (4 vehicles, 3 resources).  step_kernel.hpp and
// step_fast64.hpp give such an env a 256-thread workgroup with 4 live lanes per wave; here lane g * G + u of a wave is
// viewer u of the wave's g-th env, a 256-thread block holds 256 / G envs and the grid is ceil(B / (256 / G)).
//
// One launch does what step_kernel<1, false> does for one slot (my_step / my_step_ch / my_step_design with every run-time
// switch of StepParams), on the same planes tkey[b][k][u] / tx[b][k][u]: it is that kernel's statement with "wave" read
// as "lane group".  A lane keeps its viewer's N <= 8 table entries (key + xpos) in registers across the slot; an env's
// positions are staged in the group's 2 x G doubles of LDS (written and read by one wave: no workgroup barrier anywhere).
//
// The rule that keeps it from faulting: config and mode are uniform over the launch, per-env data (who transmits, who is
// in range, who is closest) is not.  Every cross-lane operation - the ballots masked to the group, the __shfl of width G
// - therefore sits in control flow whose trip counts are N, A, K or the compile-time G, and is predicated BY VALUE: no
// ballot or shuffle inside a branch or a loop that depends on env data.  Groups past B and lanes u >= N run the same
// instruction stream with their loads clamped to env 0 / vehicle 0 and their stores predicated off; there is no early
// return.
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

template <int G, bool OUT64>
__global__ __launch_bounds__(kSubwaveThreads) void step_subwave_kernel(const StepParams p) {
  static_assert(G == 4 || G == 8, "lanes per env");
  constexpr unsigned int GM = (1u << G) - 1u;
  __shared__ double s_px[kSubwaveThreads];
  __shared__ double s_py[kSubwaveThreads];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int u = tid & (G - 1);                     // viewer
  const int gbase = lane & ~(G - 1);               // first lane of the group in its wave
  const int N = p.N, A = p.A, K = p.K, NV = p.NV;
  const long long benv = (long long)blockIdx.x * (kSubwaveThreads / G) + (tid / G);
  const bool valid = benv < (long long)p.B && u < N;
  const size_t b = valid ? (size_t)benv : 0;       // clamped: every load stays inside the handle's buffers
  const int uc = valid ? u : 0;
  const int mode = p.mode;
  const bool piggy = (p.flags & DIRAL_F_ADD_POSDIST_PIGGY) != 0;
  const bool want_hist = piggy && p.posdist_type == 2 && p.state_out != nullptr && p.off_hist >= 0;
  const bool track_la = (p.flags & DIRAL_F_TRACK_ARRIVAL) && p.la != nullptr;
  const bool want_prr = mode == DIRAL_STEP_MY_STEP_CH || (mode == DIRAL_STEP_MY_STEP && (p.flags & DIRAL_F_TRACK_PRR));
  const bool mobile = (p.flags & DIRAL_F_MOBILITY) != 0;
  const bool use_pf = (p.flags & DIRAL_F_PROPORTIONAL_FAIR) != 0;
  const size_t bN = b * N;
  const size_t bR = b * p.NR;
  const long long slot = p.t + (p.t_dev ? *p.t_dev : 0ll);

  // ---- the viewer's table entries, issued before any compute ----------------
  unsigned int w1[G];
  double xo[G];
  if (piggy) {
#pragma unroll
    for (int k = 0; k < G; ++k) {
      const bool ok = valid && k < N;
      const size_t idx = (bR + (ok ? k : 0)) * NV + uc;
      const unsigned int w = p.tkey[idx];
      const double x = p.tx[idx];
      w1[k] = ok ? w : 0u;
      xo[k] = ok ? x : 0.0;
    }
  }

  // ---- P0: per-vehicle state, the post-move position ------------------------
  int myact = -1;
  double mypx = 0.0, mypy = 0.0, myvel = 0.0, mynpx = 0.0;
  {
    const int a = p.actions[bN + uc];
    const double x = p.pos_x[bN + uc], y = p.pos_y[bN + uc], v = p.vel[bN + uc];
    double nx = x;
    if (mobile) {
      if (p.trace) {                                                 // replay branch, network.py:194-199
        long long tt = slot % p.trace_len;
        if (tt < 0) tt += p.trace_len;
        const size_t base = p.trace_per_env ? b * p.trace_len : 0;
        nx = p.trace[(base + (size_t)tt) * N + uc];
      } else {
        nx = py_mod_pos(x + v + p.L, p.L);                           // network.py:203
      }
    }
    if (valid) {
      myact = a;
      if (a < 0 || a >= A) { atomicOr(p.err, kErrAction); myact = -1; }
      mypx = x; mypy = y; myvel = v; mynpx = nx;
    }
  }
  double* const gx = s_px + (tid - u);             // the env's positions, one wave writes and reads them
  double* const gy = s_py + (tid - u);
  gx[u] = mypx; gy[u] = mypy;
  wave_lds_order();

  // distance of this viewer to every vehicle of its env, once for all resources
  double dist[G];
  unsigned int inr_bits = 0u;
#pragma unroll
  for (int w = 0; w < G; ++w) {
    dist[w] = dist2d(gx[w], gy[w], mypx, mypy);
    inr_bits |= (dist[w] < p.Rc ? 1u : 0u) << w;
  }

  // ---- P1: per resource: tx set, closest in-range tx per viewer, rewards -----
  unsigned long long mtab = 0ull;                  // 4 bits per resource: the gather source m_i(u) of the merge
  unsigned int my_mk = 0u;                         // the transmitter set of this vehicle's resource
  double my_rtx = 1.0, my_rv = 0.0;
  for (int i = 0; i < A; ++i) {
    const bool is_tx = myact == i;
    const unsigned int mk = (unsigned int)(__ballot(is_tx) >> gbase) & GM;
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
    mtab |= (unsigned long long)(got ? bid : u) << (4 * i);
    if (want_prr) {
      // received[tx] / in_range[tx] of a colliding transmitter (test_env.py:395-405); the ballots are unconditional
      int n_in = 0, n_rec = 0;
#pragma unroll
      for (int w = 0; w < G; ++w) {
        const bool tx_w = (mk >> w) & 1u;
        const unsigned int m_in = (unsigned int)(__ballot(rx && tx_w && ((inr_bits >> w) & 1u)) >> gbase) & GM;
        const unsigned int m_rec = (unsigned int)(__ballot(rx && bid == w) >> gbase) & GM;
        if (w == u) { n_in = __popc(m_in); n_rec = __popc(m_rec); }
      }
      if (is_tx && c > 1) my_rtx = n_in > 0 ? (double)n_rec / (double)n_in : 1.0;
    }
    if (valid) {
      // channel observation of the reference step (`obs[user][i]`)
      double ob = 0.0;
      if (!is_tx && c > 0) {
        if (mode == DIRAL_STEP_MY_STEP && p.state_type == 2) ob = best;          // test_env.py:240
        else ob = 1.0;                                                            // :228, :306, :432
      }
      if (p.chobs_out) rich_store<OUT64>(p.chobs_out, (bN + u) * A + i, ob);
      if (p.state_out && p.off_chobs >= 0) rich_store<OUT64>(p.state_out, (bN + u) * p.S + p.off_chobs + i, ob);
      if (track_la && mode == DIRAL_STEP_MY_STEP_CH && got) p.la[(bN + bid) * N + u] = (int32_t)slot;   // test_env.py:436
    }
    if (is_tx) {
      my_mk = mk;
      if (mode == DIRAL_STEP_MY_STEP && c > 1) {
        // test_env.py:163-199, one value per resource (every transmitter of it computes the same one)
        const int rd = p.reward_design;
        const int wgt = collision_uses_weight(rd, c) ? subwave_reward_weight(p, mk, gx, gy) : 0;
        my_rv = collision_value(rd, c, wgt);
      }
    }
  }

  // ---- P2: reward per transmitter -------------------------------------------
  double r = 0.0, prr = 0.0;
  int sole = 0, coll = 0;
  if (valid && myact >= 0) {
    const int c = __popc(my_mk);
    if (mode == DIRAL_STEP_MY_STEP) {                                           // test_env.py:211-222
      if (c > 1) {
        r = my_rv;
        if (use_pf) {
          const int pc = p.pf[bN + u];
          if (pc > p.pf_threshold) r = p.pf_penalty;
          p.pf[bN + u] = pc + 1;
        }
        coll = 1; prr = my_rtx;
      } else {
        r = 1.0;
        if (use_pf) p.pf[bN + u] = 0;
        sole = 1; prr = 1.0;
      }
    } else if (mode == DIRAL_STEP_MY_STEP_CH) {                                 // test_env.py:411-429
      const double R = (c > 1) ? my_rtx : 1.0;
      r = ch_reward(p.reward_design, c > 1, R);
      if (c > 1) coll = 1; else sole = 1;
      prr = R;
    } else {                                                                    // test_env.py:297-301, 319-349
      if (c == 1) { r = 1.0; sole = 1; }
      else {
        int n = 1;
        double dlast = 0.0;
        unsigned int m = my_mk & ~(1u << u);
        while (m) {
          const int o = __builtin_ctz(m);
          m &= m - 1;
          const double d = dist2d(mypx, mypy, gx[o], gy[o]);
          if (d < 2.0 * p.Rc) { if (n == 1) dlast = d; ++n; }                   // network.py:122-133
        }
        if (n == 1) r = 1.0;
        else if (n == 2) r = ((dlast / 1.0) > p.Rc * 2.0) ? 0.0 : -2.0;          // network.py:135-157
        else r = -(double)n;
        coll = 1;
      }
    }
    if (p.rew_out) rich_store<OUT64>(p.rew_out, bN + u, r);
  }
  // the env's metric sums: a tree over the group, every lane taking part
  double vr = r, vp = want_prr ? prr : 0.0;
  int vs = sole, vc = coll;
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) {
    vr += __shfl_xor(vr, off, G);
    vp += __shfl_xor(vp, off, G);
    vs += __shfl_xor(vs, off, G);
    vc += __shfl_xor(vc, off, G);
  }

  // ---- P3: neighbour-table stamp + gossip merge + observation histogram ------
  unsigned long long hist[4] = {0ull, 0ull, 0ull, 0ull};   // K <= 64 bins of 4 bits: at most N - 1 <= 7 entries per viewer
  unsigned int mycnt = 0u;
  if (piggy) {
    bool seq_ovf = false;
    unsigned int key[G];
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
      if (own) xo[k] = mypx;                                          // own stamp (vehicle.py:63)
    }
    // Vehicle.received_update as the column statement of step_kernel.hpp: key[u] = max(key[u], key[m_i(u)]) on
    // (sequence number, source) for resources in order; m_i(u) == u where viewer u receives nothing on i
    for (int i = 0; i < A; ++i) {
      const int m = (int)((mtab >> (4 * i)) & 15ull);
#pragma unroll
      for (int k = 0; k < G; ++k) {
        const unsigned int v = (unsigned int)__shfl((int)key[k], m, G);
        key[k] = max(key[k], v);
      }
    }
    // xpos follows the winning sequence number from the recorded source, age resets on change
#pragma unroll
    for (int k = 0; k < G; ++k) {
      const unsigned int kf = key[k], w = w1[k];
      const int src = (int)(kf & 255u);
      const bool upd = ((kf ^ w) >> 8) != 0u;
      const double xg = __shfl(xo[k], src, G);
      const double xn = upd ? xg : xo[k];
      const unsigned int wn = upd ? (kf & ~255u) : w;
      if (valid && k < N) {
        p.tkey[(bR + k) * NV + u] = wn;
        if (upd || u == k) p.tx[(bR + k) * NV + u] = xn;
        // Network.dist_piggy + get_positional_dist_2_piggy (network.py:538-558, 473-513)
        const int age = (int)(wn & 255u);
        if (want_hist && u != k && age < p.age_limit) {
          const double x1 = xn;
          const double y1 = ((wn >> 8) > 0u) ? gy[k] : 0.0;
          const double d = dist2d(x1, y1, mynpx, mypy);
          if (d < p.Rb) {
            const double v = (x1 - mynpx > 0.0) ? d : -d;
            const int bin = hist_bin(v, -p.Rb, p.hist_inv_width, K, p.edges);
            const unsigned long long one = 1ull << (4 * (bin & 15));
            const int hw = bin >> 4;
            hist[0] += hw == 0 ? one : 0ull; hist[1] += hw == 1 ? one : 0ull;
            hist[2] += hw == 2 ? one : 0ull; hist[3] += hw == 3 ? one : 0ull;
            mycnt += 1u;
          }
        }
      }
    }
    if (seq_ovf) atomicOr(p.err, kErrSeq);
  }

  // ---- P4: write-back: positions, state vectors, done flag, metrics ----------
  if (valid) {
    p.pos_x[bN + u] = mynpx;
    if (u == 0) {
      if (p.done_out) p.done_out[b] = (uint8_t)((slot % p.episode_interval) == p.episode_interval - 1);
      double* mt = p.metrics + b * DIRAL_M_COLUMNS;
      mt[DIRAL_M_SLOTS] += 1.0;
      mt[DIRAL_M_SUM_REWARD] += vr;
      mt[DIRAL_M_TX_SOLE] += (double)vs;
      mt[DIRAL_M_TX_COLLIDED] += (double)vc;
      if (want_prr) { mt[DIRAL_M_PRR_SUM] += vp; mt[DIRAL_M_PRR_CNT] += (double)vs + (double)vc; }
    }
    if (p.state_out) {
      // the viewer's own row, section by section (test_env.py:527-583); the channel observation was written in P1, the
      // sorted distances and the type-1 histogram belong to posdist_kernel.hpp
      const int S = p.S;
      const bool real = (p.flags & DIRAL_F_ACTION_REAL) != 0;
      const size_t row = (bN + u) * S;
      for (int s = 0; s < S; ++s) {
        double val = 0.0;
        bool write = true;
        if (p.off_act >= 0 && s >= p.off_act && s < p.off_act + (real ? 1 : A)) {
          val = real ? (double)myact : ((myact == s - p.off_act) ? 1.0 : 0.0);   // test_env.py:585-595
        } else if (p.off_chobs >= 0 && s >= p.off_chobs && s < p.off_chobs + A) {
          write = false;
        } else if (p.off_hist >= 0 && s >= p.off_hist && s < p.off_hist + K) {
          if (p.posdist_type != 2) write = false;
          const int bin = s - p.off_hist, hw = bin >> 4;
          const unsigned long long word = hw == 0 ? hist[0] : (hw == 1 ? hist[1] : (hw == 2 ? hist[2] : hist[3]));
          const unsigned int h = (unsigned int)(word >> (4 * (bin & 15))) & 15u;
          val = mycnt ? (double)h / (double)mycnt : 0.0;                          // network.py:501
        } else if (p.off_posdist >= 0 && s >= p.off_posdist && s < p.off_posdist + N - 1) {
          write = false;
        } else if (s == p.off_rew) {
          val = r;
        } else if (s == p.off_idx) {
          val = (double)(u + 1);
        } else if (p.off_pos >= 0 && s == p.off_pos) {
          val = mynpx / p.L;                                                      // network.py:403-407
        } else if (p.off_pos >= 0 && s == p.off_pos + 1) {
          val = mypy / p.H;
        } else if (s == p.off_vel) {
          val = myvel;
        } else if (p.off_fp >= 0 && s == p.off_fp) {
          val = p.episode;
        } else if (p.off_fp >= 0 && s == p.off_fp + 1) {
          val = p.eps;
        }
        if (write) rich_store<OUT64>(p.state_out, row + s, val);
      }
    }
  }
}

}  // namespace diral
