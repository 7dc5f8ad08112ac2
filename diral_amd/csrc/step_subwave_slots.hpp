// step_subwave_slots.hpp - K slots per launch of the sub-wave step (step_subwave.hpp): diral_env_rollout and the random
// prefill on a handle pinned to DIRAL_PATH_SUBWAVE with DIRAL_OPT_SUBWAVE_SLOTS.
//
// The mapping is step_subwave_kernel's: G = 4 or 8 lanes per env, lane g * G + u of a wave is viewer u of the wave's g-th
// env, 64 or 32 envs per 256-thread block, grid = ceil(B / (256 / G)).  One slot is that kernel's statement (restated here
// on ref_math.hpp, so the one-slot kernel keeps its code and its registers); around it runs `for ks in 0 ... q.K - 1`, a
// loop whose trip count is uniform over the launch.  From slot to slot a lane keeps, in registers:
//   * its viewer's N <= 8 table entries w1[k] / xo[k] - read once in front of slot 0, EVERY valid entry written once
//     behind slot K - 1 (an entry no slot changed is written back as it was read: the one-slot kernel's `upd || u == k`
//     then holds over the whole launch);
//   * its position (this slot's post-move position is the next slot's position), its velocity, its proportional-fair
//     counter and its stuck-penalty state (one owner lane each);
//   * the env's metric columns, summed in slot order from the loaded value: the doubles of K load-add-store launches.
// Arrival stamps (`la`) stay plain stores with the slot number t + ks (+ clock): a (tx, rx) pair has one owner lane.
//
// Where the actions come from: a rollout (q.rollout) runs actions_seq[ks][b][u], the load of slot ks + 1 issued at the
// top of slot ks; the prefill (q.prefill) runs p.actions in slot 0 and TestEnv.sample's draw with seed + ks + 1 behind
// slot ks (what diral_env_sample(seed + ks + 1) writes), every prefill slot with slot number 0.
//
// The rules of step_subwave.hpp hold here as well:
//   * every ballot and every __shfl sits in control flow whose trip counts are K (slots or bins), N, A or the
//     compile-time G, or in a branch on a launch-uniform switch; nothing cross-lane inside a branch or loop that depends
//     on env data;
//   * anything that depends on env data is predicated BY VALUE; groups past B and lanes u >= N run the same instruction
//     stream with their loads clamped to env 0 / vehicle 0 and their stores predicated off; no early return, no
//     workgroup barrier;
//   * the group's LDS positions are rewritten every slot by the one wave that reads them: wave_lds_order() stands
//     between a slot's last read and the next slot's write, and again between the write and the reads.
#pragma once
#include <type_traits>

#include "policy_device.hpp"
#include "step_subwave.hpp"

namespace diral {

template <int G, bool OUT64>
__global__ __launch_bounds__(kSubwaveThreads) void step_subwave_slots_kernel(const StepParams p, const PolParams q) {
  static_assert(G == 4 || G == 8, "lanes per env");
  using out_t = typename std::conditional<OUT64, double, float>::type;
  constexpr unsigned int GM = (1u << G) - 1u;
  __shared__ double s_px[kSubwaveThreads];
  __shared__ double s_py[kSubwaveThreads];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int u = tid & (G - 1);                     // viewer
  const int gbase = lane & ~(G - 1);               // first lane of the group in its wave
  const int N = p.N, A = p.A, K = p.K, NV = p.NV;
  const int KS = q.K;
  const long long benv = (long long)blockIdx.x * (kSubwaveThreads / G) + (tid / G);
  const bool valid = benv < (long long)p.B && u < N;
  const size_t b = valid ? (size_t)benv : 0;       // clamped: every load stays inside the handle's buffers
  const int uc = valid ? u : 0;
  const int mode = p.mode;
  const bool prefill = q.prefill != 0;
  const bool rollout = q.rollout != 0;
  const bool every = prefill || (q.rollout & 2) != 0;   // every slot's state vector leaves ([K][B][N][S])
  const bool piggy = (p.flags & DIRAL_F_ADD_POSDIST_PIGGY) != 0;
  const bool hist_cfg = piggy && p.posdist_type == 2 && p.off_hist >= 0;
  const bool track_la = (p.flags & DIRAL_F_TRACK_ARRIVAL) && p.la != nullptr;
  const bool want_prr = mode == DIRAL_STEP_MY_STEP_CH || (mode == DIRAL_STEP_MY_STEP && (p.flags & DIRAL_F_TRACK_PRR));
  const bool mobile = (p.flags & DIRAL_F_MOBILITY) != 0;
  const bool pf_on = (p.flags & DIRAL_F_PROPORTIONAL_FAIR) && mode == DIRAL_STEP_MY_STEP && p.pf != nullptr;
  const bool shaping = q.shaped_out != nullptr;
  const bool pen_on = shaping && (q.shape_flags & 4) != 0;
  const size_t bN = b * N;
  const size_t bR = b * p.NR;
  const size_t BN = (size_t)p.B * (size_t)N;
  const long long clock = p.t_dev ? *p.t_dev : 0ll;

  // ---- in front of slot 0: everything the slots keep in registers -----------
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
  double mypx = 0.0, mypy = 0.0, myvel = 0.0;
  {
    const double x = p.pos_x[bN + uc], y = p.pos_y[bN + uc], v = p.vel[bN + uc];
    if (valid) { mypx = x; mypy = y; myvel = v; }
  }
  int pfc = 0, penc = 0, penp = 0;
  if (pf_on) pfc = p.pf[bN + uc];
  if (pen_on) { penc = q.pen_counter[bN + uc]; penp = q.pen_prev[bN + uc]; }
  // the env's metric columns (every lane of the group holds the same sums; lane 0 of the group writes them back)
  const double* const mt_in = p.metrics + b * DIRAL_M_COLUMNS;
  double m_slots = mt_in[DIRAL_M_SLOTS], m_rew = mt_in[DIRAL_M_SUM_REWARD], m_sole = mt_in[DIRAL_M_TX_SOLE],
         m_coll = mt_in[DIRAL_M_TX_COLLIDED], m_prr = mt_in[DIRAL_M_PRR_SUM], m_cnt = mt_in[DIRAL_M_PRR_CNT];
  // slot 0's actions: the head of the sequence (p.actions IS actions_seq for a rollout) or the caller's draw (prefill)
  int act_next = p.actions[bN + uc];
  double* const gx = s_px + (tid - u);             // the env's positions, one wave writes and reads them
  double* const gy = s_py + (tid - u);

  for (int ks = 0; ks < KS; ++ks) {
    const bool last = ks == KS - 1;
    const int a = act_next;
    // (the next slot's actions, asked for here: the round trip runs under this slot)
    if (rollout && !last) act_next = q.actions_seq[(size_t)(ks + 1) * BN + bN + uc];
    const long long slot = p.t + (prefill ? 0 : ks) + clock;
    // where this slot's state vector goes, if it leaves
    void* const state_out = (p.state_out && (last || every)) ? p.state_out : nullptr;
    const size_t srow0 = every ? (size_t)ks * BN : 0;
    const bool want_hist = hist_cfg && state_out != nullptr;

    // ---- P0: the action, the post-move position --------------------------------
    int myact = -1;
    double mynpx = 0.0;
    {
      double nx = mypx;
      if (mobile) {
        if (p.trace) {                                                 // replay branch, network.py:194-199
          long long tt = slot % p.trace_len;
          if (tt < 0) tt += p.trace_len;
          const size_t base = p.trace_per_env ? b * p.trace_len : 0;
          nx = p.trace[(base + (size_t)tt) * N + uc];
        } else {
          nx = py_mod_pos(mypx + myvel + p.L, p.L);                    // network.py:203
        }
      }
      if (valid) {
        myact = a;
        if (a < 0 || a >= A) { atomicOr(p.err, kErrAction); myact = -1; }
        mynpx = nx;
        if (prefill && q.actions_all) q.actions_all[(size_t)ks * BN + bN + u] = a;   // the actions this slot runs with
      }
    }
    wave_lds_order();                              // (behind the last read of the slot before)
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
    unsigned long long mtab = 0ull;                // 4 bits per resource: the gather source m_i(u) of the merge
    unsigned int my_mk = 0u;                       // the transmitter set of this vehicle's resource
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
        // the channel-observation section of a rich state row (`obs[user][i]`); chobs_out is no output of a slot call
        if (state_out && p.off_chobs >= 0) {
          double ob = 0.0;
          if (!is_tx && c > 0) {
            if (mode == DIRAL_STEP_MY_STEP && p.state_type == 2) ob = best;          // test_env.py:240
            else ob = 1.0;                                                            // :228, :306, :432
          }
          rich_store<OUT64>(state_out, (srow0 + bN + u) * p.S + p.off_chobs + i, ob);
        }
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
          if (pf_on) {
            if (pfc > p.pf_threshold) r = p.pf_penalty;
            pfc = pfc + 1;
          }
          coll = 1; prr = my_rtx;
        } else {
          r = 1.0;
          if (pf_on) pfc = 0;
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
      if (p.rew_out && last) rich_store<OUT64>(p.rew_out, bN + u, r);
    }
    // the env's metric sums: a tree over the group, every lane taking part; added in slot order
    {
      double vr = r, vp = want_prr ? prr : 0.0;
      int vs = sole, vc = coll;
#pragma unroll
      for (int off = G / 2; off > 0; off >>= 1) {
        vr += __shfl_xor(vr, off, G);
        vp += __shfl_xor(vp, off, G);
        vs += __shfl_xor(vs, off, G);
        vc += __shfl_xor(vc, off, G);
      }
      m_slots += 1.0;
      m_rew += vr;
      m_sole += (double)vs;
      m_coll += (double)vc;
      if (want_prr) { m_prr += vp; m_cnt += (double)vs + (double)vc; }
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
      // xpos follows the winning sequence number from the recorded source, age resets on change; the entry stays in
      // its registers for the next slot
#pragma unroll
      for (int k = 0; k < G; ++k) {
        const unsigned int kf = key[k], w = w1[k];
        const int src = (int)(kf & 255u);
        const bool ok = valid && k < N;
        const bool upd = ok && ((kf ^ w) >> 8) != 0u;
        const double xg = __shfl(xo[k], src, G);
        const double xn = upd ? xg : xo[k];
        const unsigned int wn = upd ? (kf & ~255u) : w;
        w1[k] = wn;
        xo[k] = xn;
        if (ok) {
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

    // ---- P4: the done flag and the state vector of a slot whose state leaves ----
    if (valid) {
      if (u == 0 && p.done_out && last) p.done_out[b] = (uint8_t)((slot % p.episode_interval) == p.episode_interval - 1);
      if (state_out) {
        // the viewer's own row, section by section (test_env.py:527-583); the channel observation was written in P1
        const int S = p.S;
        const bool real = (p.flags & DIRAL_F_ACTION_REAL) != 0;
        const size_t row = (srow0 + bN + u) * S;
        // (prefill: obtain_state is handed the bootstrap step's rewards, main_test.py:110)
        const double rcol = q.rew_in ? q.rew_in[bN + u] : r;
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
            val = rcol;
          } else if (s == p.off_idx) {
            val = (double)(u + 1);
          } else if (p.off_pos >= 0 && s == p.off_pos) {
            val = mynpx / p.L;                                                      // network.py:403-407
          } else if (p.off_pos >= 0 && s == p.off_pos + 1) {
            val = mypy / p.H;
          } else if (s == p.off_vel) {
            val = myvel;                                                            // the velocity this slot ran with
          } else if (p.off_fp >= 0 && s == p.off_fp) {
            val = p.episode;
          } else if (p.off_fp >= 0 && s == p.off_fp + 1) {
            val = p.eps;
          }
          if (write) rich_store<OUT64>(state_out, row + s, val);
        }
      }
    }

    // ---- the driver's reward shaping (main_test.py:171, 178, 194-206): driver_shape_wave_kernel's statement in the
    //      output dtype, np.sum in NumPy's order ------------------------------------
    if (shaping) {                                                     // (launch-uniform)
      const out_t ar = valid ? (out_t)r : (out_t)0;
      out_t sr;
      if (N < 8) {
        // fewer than 8 elements: sequentially from 0, ((0 + a0) + a1) + ...
        sr = (out_t)0;
        for (int i = 0; i < N; ++i) sr = sr + __shfl(ar, i, G);
      } else {
        // ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)): the xor butterfly of width 8 gives it on every lane
        sr = ar;
#pragma unroll
        for (int off = 1; off < G; off <<= 1) sr = sr + __shfl_xor(sr, off, G);
      }
      if (valid) {
        const size_t sB = (size_t)ks * (size_t)p.B;
        if (u == 0) {
          if (q.sum_r_out) static_cast<out_t*>(q.sum_r_out)[sB + b] = sr;
          if (q.coll_out) static_cast<out_t*>(q.coll_out)[sB + b] = (out_t)A - sr;
        }
        out_t rr = ar;
        if (pen_on) {
          const bool stuck = (rr < (out_t)1) && (a == penp);
          penc = stuck ? penc + 1 : 0;
          if (penc > q.pen_threshold) rr = (out_t)q.pen_value;
          penp = a;
        }
        if (q.shape_flags & 1) rr = rr + sr / (out_t)N;
        static_cast<out_t*>(q.shaped_out)[sB * N + bN + u] = rr;
      }
    }

    // ---- what the next slot takes over ------------------------------------------
    if (valid) mypx = mynpx;
    if (q.vel_vary) {
      // Network.update_velocity (network.py:208-223) behind a slot that ends an episode, as velocity_kernel draws it:
      // diral_env_update_velocity(env, NULL, vel_seed + episode)
      const long long tt = p.t + ks + clock;
      if ((unsigned int)tt % (unsigned int)p.episode_interval == (unsigned int)p.episode_interval - 1u) {
        const uint64_t vseed = q.vel_seed + (uint64_t)((unsigned int)tt / (unsigned int)p.episode_interval);
        myvel = valid ? velocity_draw(myvel, vseed, q.idx0 + (uint64_t)bN + (uint64_t)u) : 0.0;
      }
    }
    if (prefill) {
      // TestEnv.sample (test_env.py:116-122) for the next slot, as sample_kernel draws it with seed + ks + 1
      act_next = (int)(rng_u64(q.seed + (uint64_t)ks + 1ull, 3, q.idx0 + (uint64_t)bN + (uint64_t)uc) % (uint64_t)A);
      if (last && valid) q.actions_out[bN + u] = act_next;
    }
  }

  // ---- behind slot K - 1: the registers go back ---------------------------------
  if (valid) {
    if (piggy) {
#pragma unroll
      for (int k = 0; k < G; ++k) {
        if (k < N) {
          p.tkey[(bR + k) * NV + u] = w1[k];
          p.tx[(bR + k) * NV + u] = xo[k];
        }
      }
    }
    p.pos_x[bN + u] = mypx;
    if (q.vel_vary) q.vel_w[bN + u] = myvel;
    if (pf_on) p.pf[bN + u] = pfc;
    if (pen_on) { q.pen_counter[bN + u] = penc; q.pen_prev[bN + u] = penp; }
    if (u == 0) {
      double* mt = p.metrics + b * DIRAL_M_COLUMNS;
      mt[DIRAL_M_SLOTS] = m_slots;
      mt[DIRAL_M_SUM_REWARD] = m_rew;
      mt[DIRAL_M_TX_SOLE] = m_sole;
      mt[DIRAL_M_TX_COLLIDED] = m_coll;
      if (want_prr) { mt[DIRAL_M_PRR_SUM] = m_prr; mt[DIRAL_M_PRR_CNT] = m_cnt; }
    }
  }
}

}  // namespace diral
