// step_subwave_slots.hpp - K slots per launch of the sub-wave step (step_subwave.hpp): diral_env_rollout and the random
// prefill on a handle pinned to DIRAL_PATH_SUBWAVE with DIRAL_OPT_SUBWAVE_SLOTS.
//
// The mapping is step_subwave_kernel's: G = 4 or 8 lanes per env, lane g * G + u of a wave is viewer u of the wave's g-th
// env, 64 or 32 envs per 256-thread block, grid = ceil(B / (256 / G)).  One slot is the phase functions of
// step_subwave.hpp, the ones the one-slot kernel is made of; around them runs `for ks in 0 ... q.K - 1`, a loop whose trip
// count is uniform over the launch.  From slot to slot a lane keeps, in registers:
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
// The rules in the header of step_subwave.hpp bind this kernel as a caller of the phases: they are called from the slot
// loop and from branches on launch-uniform switches only, the group's LDS positions are rewritten every slot between two
// wave_lds_order(), and the one cross-lane code of its own, the shaping sum, sits under `shaping` and the trip counts N
// and G.
#pragma once
#include <type_traits>

#include "policy_device.hpp"
#include "step_subwave.hpp"

namespace diral {

// MEM: the launch carries the memory block (PolParams::mem_on).  An instantiation of its own: as a run-time switch the block
// cost every launch without it 3 to 7 % (profiles/rollout_memory/).
template <int G, bool OUT64, bool MEM = false>
__global__ __launch_bounds__(kSubwaveThreads) void step_subwave_slots_kernel(const StepParams p, const PolParams q) {
  using out_t = typename std::conditional<OUT64, double, float>::type;
  __shared__ double s_px[kSubwaveThreads];
  __shared__ double s_py[kSubwaveThreads];
  const SubwaveLane L = subwave_lane<G>(p, s_px, s_py);
  const int u = L.u, uc = L.uc;
  const bool valid = L.valid;
  const size_t b = L.b, bN = L.bN;
  const int N = p.N, A = p.A;
  const int KS = q.K;
  const bool prefill = q.prefill != 0;
  const bool rollout = q.rollout != 0;
  const bool every = prefill || (q.rollout & 2) != 0;   // every slot's state vector leaves ([K][B][N][S])
  const bool hist_cfg = L.piggy && p.posdist_type == 2 && p.off_hist >= 0;
  const bool pf_on = (p.flags & DIRAL_F_PROPORTIONAL_FAIR) && p.mode == DIRAL_STEP_MY_STEP && p.pf != nullptr;
  const bool shaping = q.shaped_out != nullptr;
  const bool pen_on = shaping && (q.shape_flags & 4) != 0;
  const size_t BN = (size_t)p.B * (size_t)N;
  const long long clock = p.t_dev ? *p.t_dev : 0ll;
  // the memory block (MEM): slot ks writes ring rows instead of [K]-major scratch - p.state_out is the state ring, `mem_row`
  // the row of the slot's actions and reward, the row behind it the one of its state vector; launch-uniform
  constexpr bool mem = MEM;
  int mem_row = 0;
  if constexpr (MEM) mem_row = mem_row_head(q);

  // ---- in front of slot 0: everything the slots keep in registers -----------
  unsigned int w1[G];
  double xo[G];
  if (L.piggy) subwave_load_entries<G>(p, L, w1, xo);
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

  for (int ks = 0; ks < KS; ++ks) {
    const bool last = ks == KS - 1;
    const int a = act_next;
    // (the next slot's actions, asked for here: the round trip runs under this slot)
    if (rollout && !last) act_next = q.actions_seq[(size_t)(ks + 1) * BN + bN + uc];
    const long long slot = p.t + (prefill ? 0 : ks) + clock;
    // where this slot's state vector goes, if it leaves
    void* const state_out = (p.state_out && (last || every)) ? p.state_out : nullptr;
    const size_t srow0 = mem ? (size_t)mem_row_next(mem_row, q.mem_rows) * BN : (every ? (size_t)ks * BN : 0);
    const bool want_hist = hist_cfg && state_out != nullptr;

    // ---- P0: the action, the post-move position --------------------------------
    const int myact = subwave_action(p, L, a);
    const double mynpx = valid ? subwave_move(p, L, slot, mypx, myvel) : 0.0;
    if (valid && prefill && q.actions_all) q.actions_all[(size_t)ks * BN + bN + u] = a;   // the actions this slot runs with
    if constexpr (MEM) if (valid) {
      // ... into the action ring, and a prefill's stale bootstrap rewards into the reward ring (add_prefill's rows)
      q.mem_actions[(size_t)mem_row * BN + bN + u] = a;
      if (prefill) static_cast<out_t*>(q.mem_rewards)[(size_t)mem_row * BN + bN + u] = (out_t)q.rew_in[bN + u];
    }
    wave_lds_order();                              // (behind the last read of the slot before)
    L.gx[u] = mypx; L.gy[u] = mypy;
    wave_lds_order();

    // ---- P1, P2; chobs_out is no output of a slot call, rew_out one of the last slot ----
    const SubwaveSearch found = subwave_search<G, OUT64>(p, L, myact, mypx, mypy, slot, nullptr, state_out, srow0 + bN + u);
    const SubwaveReward rw = subwave_reward(p, L, myact, found, mypx, mypy, pf_on, pfc);
    const double r = rw.r;
    if (valid && myact >= 0 && p.rew_out && last) rich_store<OUT64>(p.rew_out, bN + u, r);
    // the env's metric sums, added in slot order
    {
      const SubwaveReward sum = subwave_group_sums<G>(rw, L.want_prr);
      m_slots += 1.0;
      m_rew += sum.r;
      m_sole += (double)sum.sole;
      m_coll += (double)sum.coll;
      if (L.want_prr) { m_prr += sum.prr; m_cnt += (double)sum.sole + (double)sum.coll; }
    }

    // ---- P3: the entries stay in their registers for the next slot --------------
    unsigned long long h0 = 0ull, h1 = 0ull, h2 = 0ull, h3 = 0ull;
    unsigned int cnt = 0u;
    if (L.piggy) subwave_merge<G, false>(p, L, found.mtab, mypx, mynpx, mypy, want_hist, w1, xo, h0, h1, h2, h3, cnt);

    // ---- P4: the done flag and the state vector of a slot whose state leaves ----
    if (valid) {
      if (u == 0 && p.done_out && last) p.done_out[b] = (uint8_t)((slot % p.episode_interval) == p.episode_interval - 1);
      // (prefill: obtain_state is handed the bootstrap step's rewards, main_test.py:110)
      if (state_out)
        subwave_state_row<OUT64>(p, state_out, srow0 + bN + u, u, myact, h0, h1, h2, h3, cnt, q.rew_in ? q.rew_in[bN + u] : r,
                                 mynpx, mypy, myvel);
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
        static_cast<out_t*>(q.shaped_out)[(mem ? (size_t)mem_row * (size_t)p.B : sB) * N + bN + u] = rr;   // (the block: the reward ring's row)
      }
    }

    // ---- what the next slot takes over ------------------------------------------
    if (valid) mypx = mynpx;
    if constexpr (MEM) mem_row = mem_row_next(mem_row, q.mem_rows);
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
    if (L.piggy) {
#pragma unroll
      for (int k = 0; k < G; ++k) {
        if (k < N) {
          p.tkey[(L.bR + k) * p.NV + u] = w1[k];
          p.tx[(L.bR + k) * p.NV + u] = xo[k];
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
      if (L.want_prr) { mt[DIRAL_M_PRR_SUM] = m_prr; mt[DIRAL_M_PRR_CNT] = m_cnt; }
    }
  }
}

}  // namespace diral