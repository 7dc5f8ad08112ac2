#!/usr/bin/env python3
"""Generate golden input/output vectors by IMPORTING the reference env.

Runs ONLY in the build container (needs /root/reference, which does not exist
on the GPU box).  The reference is imported, driven with seeded inputs, and its
inputs + outputs are recorded as small .npz fixtures under tests/golden/.
Nothing of the reference's source is stored - only data.

Reference entry points exercised (all under /root/reference/envs):
  TestEnv.my_step            test_env.py:124-266
  TestEnv.my_step_design     test_env.py:269-349
  TestEnv.my_step_ch         test_env.py:351-443
  TestEnv.obtain_state       test_env.py:527-583
  TestEnv.reset_mobility_env test_env.py:479-484
  Network.update_velocity    network.py:208-223
  Network.get_information_age network.py:560-574

  SemiPersistentScheduling   algorithms/v2x_sps.py:8-104   (`sps` fixtures)

  Vehicle (a static N-vehicle topology)  vehicle.py:9-33, network.py:302-305, 545
  Network.dist with pos_y != 0            network.py:318-332   (off-lane fixtures)
  Network.get_positional_dist / _piggy    network.py:409-471   (at 64 / 80 vehicles)
  Network.get_information_age, t < last arrival   network.py:566-574 (negative list index)

Usage:  python tests/golden/gen_golden.py        (rewrites tests/golden/*.npz)
        python tests/golden/gen_golden.py curated | driver | sps | trace | piggyback   (one family)
        python tests/golden/gen_golden.py fuzz [n_cases [first_seed]]
            the seeded differential sweep: draw_ref_case(i) for i in first_seed .. first_seed + n_cases - 1
            (default 320 from 0), each recorded from the reference into a temporary directory, replayed through
            Oracle(sq_mode=SQ_POW) under the comparison of test_oracle_reproduces_reference_bit_exact, and
            written as one table row into tests/golden/FUZZ_SWEEP.md.  Nothing is kept but the report.
"""
import contextlib
import hashlib
import io
import json
import os
import sys
import tempfile
import time
from unittest import mock

import numpy as np

REF = "/root/reference/envs"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
sys.path.insert(0, REF)
with contextlib.redirect_stdout(io.StringIO()):
    from test_env import TestEnv  # noqa: E402  (the reference)
    import network as ref_network  # noqa: E402
sys.path.insert(0, ROOT)
from tests.golden_util import OUT_KEYS, out_sha  # noqa: E402  (the per-slot hash the replays recompute)


# The `EnvironmentTest` block of configs/4ue_3r_toy/*_b20_*_dis_07.yaml:45-71,
# restated as data (values only).
TOY = dict(
    congestion_test=True, load_positions=False, num_channels=3, num_users=4,
    mobility=True, mobility_vary=False, highway_length=100,
    enable_fingerprint=False, reward_design=2, communication_range=250,
    State=dict(type=2, add_action=True, add_reward=False, add_index=False,
               add_velocity=False, action_index="binary", piggybacking=False,
               add_position=False, add_positional_dist=False,
               add_positional_dist_piggy=True, add_positional_dist_type=2,
               add_channel_obs=False, num_bins=20),
)


def cfg_with(base=None, state=None, **kw):
    c = json.loads(json.dumps(base or TOY))
    c.update(kw)
    if state:
        c["State"].update(state)
    return c


def big_cfg(N, A, L, **kw):
    return cfg_with(num_users=N, num_channels=A, highway_length=L,
                    congestion_test=False, **kw)


def make_env(cfg):
    with contextlib.redirect_stdout(io.StringIO()):
        return TestEnv(**json.loads(json.dumps(cfg)))


def make_static_env(cfg):
    """mobility False + enable_design_topology True with num_users vehicles.  The reference's constructor builds
    the six vehicles of its design test whatever num_users is (network.py:59-60, 69-79), so the N-vehicle static
    topology is its own mobile network (network.py:54-58, 92-112: N Vehicle objects with N-entry tables) with the
    two attributes the run-time code reads set to what this config gives them: `mobility` False (update_mobility
    does nothing, network.py:302-305) and `enable_design_topology_net` True (dist_piggy, network.py:545)."""
    env = make_env(cfg_with(cfg, mobility=True, enable_design_topology=False))
    env.mobility = env.network.mobility = False
    env.enable_design_topology = env.network.enable_design_topology_net = True
    return env


def set_init(env, x0, y0, v0):
    """Overwrite the random topology (network.py:92-119) with recorded values,
    keeping the reference's own scalar types (np.int64 positions, float v)."""
    for u, veh in enumerate(env.network.vehicles):
        veh.pos_x = np.int64(x0[u]) if float(x0[u]).is_integer() else float(x0[u])
        veh.pos_y = np.int64(y0[u]) if float(y0[u]).is_integer() else float(y0[u])
        veh.pos = [veh.pos_x, veh.pos_y]
        veh.velocity = float(v0[u])


def tables(env):
    N = env.NUM_USERS
    seq = np.zeros((N, N), np.int64)
    age = np.zeros((N, N), np.int64)
    tx = np.zeros((N, N), np.float64)
    ty = np.zeros((N, N), np.float64)
    for u, veh in enumerate(env.network.vehicles):
        for k in range(N):
            e = veh.pos_of_neighbors[k]
            seq[u, k] = e["seq_number"]
            age[u, k] = e["last_updated"]
            tx[u, k] = e["xpos"]
            ty[u, k] = e["ypos"]
    return seq, age, tx, ty


def last_arrival(env):
    N = env.NUM_USERS
    la = np.zeros((N, N), np.int64)
    for t in range(N):
        for r in range(N):
            la[t, r] = env.network.last_arrival_time[t][r]
    return la


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(name, cfg, init, steps, vel_updates=None, table_every=1,
             full_tables=True, episode_eps=None, trace=None, trace_after=None, extra=None,
             record_every=1, out_dir=None, quiet=False):
    """steps: list of (mode, actions, t).  vel_updates: {step_index: draws[N]}
    applied AFTER that step (main_test.py:226-233 order).  record_every > 1 thins the fixture: the full per-slot
    outputs (OUT_KEYS) are kept at every record_every-th slot and the last (`rec_step` lists them), their hashes
    (`out_sha`) at every slot, like `table_sha`."""
    if trace is not None:
        # trace replay (network.py:171-178): the reference np.load()s `load_file_pos`
        tpath = os.path.join(out_dir or tempfile.gettempdir(), "diral_golden_trace_%s.npy" % name)
        np.save(tpath, np.asarray(trace, dtype=np.float64))
        cfg = cfg_with(cfg, load_positions=True, load_file_pos="/tmp/diral_golden_trace_%s.npy" % name)
    static = not cfg["mobility"] and cfg.get("enable_design_topology") and not isinstance(init, str)
    env = make_static_env(cfg) if static else make_env(cfg)
    if trace is not None:
        env.load_file_positions = tpath
    N, A = env.NUM_USERS, env.NUM_CHANNELS
    if isinstance(init, str) and init == "fixed4":
        env.reset_mobility_env()
    elif isinstance(init, str) and init == "design6":
        pass  # enable_design_topology builds it in the constructor
    else:
        set_init(env, *init)
    x0 = np.array([float(v.pos_x) for v in env.network.vehicles])
    y0 = np.array([float(v.pos_y) for v in env.network.vehicles])
    v0 = np.array([float(v.velocity) for v in env.network.vehicles])

    rec = dict(rews=[], chobs=[], state=[], pos_x=[], vel=[], ia=[])
    tab = dict(step=[], seq=[], age=[], x=[], y=[], la=[])
    tab_sha = []
    o_sha, rec_step = [], []
    vel_updates = vel_updates or {}
    for si, (mode, acts, t) in enumerate(steps):
        acts = np.asarray(acts, dtype=np.int32)
        t = int(t)
        with contextlib.redirect_stdout(io.StringIO()):
            if mode == "step":
                obs, rews = env.my_step(acts, t)
            elif mode == "ch":
                obs, rews = env.my_step_ch(acts, t)
            elif mode == "design":
                obs, rews = env.my_step_design(acts, t)
            else:
                raise ValueError(mode)
            ep, eps = (episode_eps[si] if episode_eps else (0, 1))
            st = env.obtain_state(obs, acts, list(rews), ep, eps)
        now = dict(rews=np.array(rews, dtype=np.float64),
                   chobs=np.array([obs[u] for u in range(N)], dtype=np.float64),
                   # (action_index "real" alone leaves each agent's state a scalar, test_env.py:543: one column)
                   state=np.array([np.asarray(s, dtype=np.float64).reshape(-1) for s in st]).reshape(N, -1)
                   if np.size(st[0]) else np.zeros((N, 0)),
                   pos_x=np.array([float(v.pos_x) for v in env.network.vehicles]),
                   ia=np.array(env.network.get_information_age(t), dtype=np.int64))
        if si in vel_updates:
            draws = list(vel_updates[si])
            with mock.patch.object(ref_network.random, "randrange",
                                   side_effect=lambda a, b: draws.pop(0)):
                env.update_velocity()
        now["vel"] = np.array([float(v.velocity) for v in env.network.vehicles])
        o_sha.append([out_sha(now[k]) for k in OUT_KEYS])
        if si % record_every == 0 or si == len(steps) - 1:
            rec_step.append(si)
            for k in OUT_KEYS:
                rec[k].append(now[k])
        if trace is not None and si == trace_after:
            with contextlib.redirect_stdout(io.StringIO()):
                env.load_saved_positions()                      # main_test.py:118
        seq, age, tx, ty = tables(env)
        la = last_arrival(env)
        tab_sha.append([sha(seq), sha(age), sha(tx), sha(ty), sha(la)])
        if full_tables and (si % table_every == 0 or si == len(steps) - 1):
            tab["step"].append(si)
            tab["seq"].append(seq)
            tab["age"].append(age)
            tab["x"].append(tx)
            tab["y"].append(ty)
            tab["la"].append(la)

    out = dict(
        cfg=np.array(json.dumps(cfg)),
        x0=x0, y0=y0, v0=v0,
        modes=np.array([s[0] for s in steps]),
        actions=np.array([s[1] for s in steps], dtype=np.int32),
        tsteps=np.array([s[2] for s in steps], dtype=np.int64),
        vel_update_steps=np.array(sorted(vel_updates), dtype=np.int64),
        vel_update_draws=np.array([vel_updates[k] for k in sorted(vel_updates)],
                                  dtype=np.uint8).reshape(len(vel_updates), N),
        episode_eps=np.array(episode_eps if episode_eps else
                             [(0, 1)] * len(steps), dtype=np.float64),
        state_space=np.int64(env.get_state_space()),
        table_sha=np.array(tab_sha),
        trace=np.asarray(trace if trace is not None else np.zeros((0, N)), dtype=np.float64),
        trace_after=np.int64(-1 if trace_after is None else trace_after),
    )
    for k, v in rec.items():
        out[k] = np.array(v)
    for k, v in tab.items():
        out["tab_" + k] = np.array(v)
    if getattr(env, "piggybacking", False):
        # TestEnv.prev_obs after the last step (test_env.py:260-261): dict user -> ndarray[A]
        out["prev_obs"] = np.array([env.prev_obs[u] for u in range(N)], dtype=np.float64)
    if record_every > 1:
        out["rec_step"] = np.array(rec_step, dtype=np.int64)
        out["out_sha"] = np.array(o_sha)
    for k, v in (extra or {}).items():
        out[k] = np.asarray(v)
    path = os.path.join(out_dir or OUT, name + ".npz")
    np.savez_compressed(path, **out)
    if not quiet:
        print("%-28s N=%-3d A=%-2d steps=%-3d  %7.1f KB" % (
            name, N, A, len(steps), os.path.getsize(path) / 1024))
    return path


def run_driver_case(name, cfg, init, n_prefill, T, enable_channel, global_reward_avg, ia_averaging,
                    episode_interval, seed, ia_penalty_enable=False, ia_penalty_threshold=5, ia_penalty_value=-10):
    """The env-facing call sequence of main_test.marl_test (main_test.py:86-236)
    with the TF agent replaced by recorded random actions: bootstrap, prefill with
    my_step_design (or my_step_ch), slot loop with information age, reward shaping,
    episode boundaries.  utils/misc.calculate_ia_penalty is the reference's own."""
    sys.path.insert(0, "/root/reference")
    from utils.misc import calculate_ia_penalty
    rng = np.random.default_rng(seed)
    env = make_env(cfg)
    N, A = env.NUM_USERS, env.NUM_CHANNELS
    if isinstance(init, str) and init == "fixed4":
        env.reset_mobility_env()
    else:
        set_init(env, *init)
    x0 = np.array([float(v.pos_x) for v in env.network.vehicles])
    y0 = np.array([float(v.pos_y) for v in env.network.vehicles])
    v0 = np.array([float(v.velocity) for v in env.network.vehicles])
    rec = dict(boot_action=None, boot_state=None, pre_actions=[], pre_states=[], actions=[], states=[],
               raw_reward=[], shaped_reward=[], sum_r=[], collision=[], ia=[], ia_sum=[], ia_pen=[],
               episode_end=[], vel_draws=[], episode=[], eps=[])
    with contextlib.redirect_stdout(io.StringIO()):
        action = rng.integers(0, A, size=N).astype(np.int32)           # env.sample() (main_test.py:89)
        obs, rews = env.my_step(action, 0)                               # :92
        rews = list(rews)
        state = env.obtain_state(obs, action, rews)                      # :94
        rec["boot_action"], rec["boot_state"] = action, np.array(state, dtype=np.float64)
        for ii in range(n_prefill):                                      # :99-114
            action = rng.integers(0, A, size=N).astype(np.int32)
            if enable_channel:
                obs, reward = env.my_step_ch(action, 0)
            else:
                obs, reward = env.my_step_design(action, 0)
            next_state = env.obtain_state(obs, action, rews)             # stale `rews` (main_test.py:110)
            rec["pre_actions"].append(action)
            rec["pre_states"].append(np.array(next_state, dtype=np.float64))
        episode, eps, sum_ia_prev = 0, 0.99, 0
        pen_counter = np.zeros(N, int)
        prev_actions = -np.ones(N, int)
        for time_step in range(T):                                       # :119
            action = rng.integers(0, A, size=N).astype(np.int32)
            if enable_channel:
                obs, reward = env.my_step_ch(action, time_step)          # :144
            else:
                obs, reward = env.my_step(action, time_step)             # :146
            raw = np.array(reward, dtype=np.float64)
            ia = env.network.get_information_age(time_step)             # :150
            ia_sum = calculate_ia_penalty(ia)                            # :151
            ia_penalty = 0
            if ia_averaging:                                             # :153-160
                if ia_sum > sum_ia_prev:
                    ia_penalty = -1
                elif ia_sum < sum_ia_prev:
                    ia_penalty = 1
                sum_ia_prev = ia_sum
            next_state = env.obtain_state(obs, action, reward, episode, eps)   # :164
            sum_r = np.sum(reward)                                       # :171
            collision = A - sum_r                                        # :178
            for i in range(len(reward)):                                 # :188-206
                if ia_averaging:
                    reward[i] += ia_penalty
                if ia_penalty_enable:
                    if reward[i] < 1 and action[i] == prev_actions[i]:
                        pen_counter[i] += 1
                    else:
                        pen_counter[i] = 0
                    if pen_counter[i] > ia_penalty_threshold:
                        reward[i] = ia_penalty_value
                    prev_actions[i] = action[i]
                if global_reward_avg:
                    reward[i] = reward[i] + sum_r / len(reward)
            end = (time_step % episode_interval == episode_interval - 1)  # :226
            draws = np.zeros(N, np.uint8)
            if end:
                episode += 1
                eps = max(eps * 0.9992, 0.001)
                draws = rng.integers(1, 4, size=N).astype(np.uint8)
                dl = list(draws)
                with mock.patch.object(ref_network.random, "randrange", side_effect=lambda a, b: dl.pop(0)):
                    env.update_velocity()                                # :233
            for k, v in (("actions", action), ("states", np.array(next_state, dtype=np.float64)),
                         ("raw_reward", raw), ("shaped_reward", np.array(reward, dtype=np.float64)),
                         ("sum_r", sum_r), ("collision", collision), ("ia", np.array(ia)), ("ia_sum", ia_sum),
                         ("ia_pen", ia_penalty), ("episode_end", end), ("vel_draws", draws),
                         ("episode", episode), ("eps", eps)):
                rec[k].append(v)
    seq, age, tx, ty = tables(env)
    out = dict(cfg=np.array(json.dumps(cfg)), x0=x0, y0=y0, v0=v0,
               opts=np.array(json.dumps(dict(n_prefill=n_prefill, T=T, enable_channel=enable_channel,
                                             global_reward_avg=global_reward_avg, ia_averaging=ia_averaging,
                                             episode_interval=episode_interval, ia_penalty_enable=ia_penalty_enable,
                                             ia_penalty_threshold=ia_penalty_threshold,
                                             ia_penalty_value=ia_penalty_value))),
               final_seq=seq, final_age=age, final_x=tx,
               final_pos=np.array([float(v.pos_x) for v in env.network.vehicles]),
               final_vel=np.array([float(v.velocity) for v in env.network.vehicles]))
    for k, v in rec.items():
        out[k] = np.array(v)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print("%-28s N=%-3d A=%-2d slots=%-3d  %7.1f KB" % (name, N, A, T, os.path.getsize(path) / 1024))


def rand_init(rng, N, L, vary):
    # network.py:103-110: x=randint(0,L) (integer valued), y=randint(0,1)=0,
    # v = 1.7 if mobility_vary else uniform(1.1, 2.7)
    x0 = rng.integers(0, L, size=N).astype(np.float64)
    y0 = np.zeros(N)
    v0 = np.full(N, 1.7) if vary else rng.uniform(1.1, 2.7, size=N)
    return x0, y0, v0


def rand_steps(rng, mode, T, N, A, sticky=0.0):
    acts = rng.integers(0, A, size=N)
    steps = []
    for t in range(T):
        new = rng.integers(0, A, size=N)
        keep = rng.random(N) < sticky
        acts = np.where(keep, acts, new)
        steps.append((mode, acts.copy(), t))
    return steps


def main():
    toy_actions = [[0, 1, 2, 0], [0, 0, 0, 0], [1, 1, 2, 2], [2, 2, 2, 1]]

    # ---- G1: fixed 4-UE topology, every reward design, both step kinds -----
    for rd in (1, 2, 3, 4, 5):
        run_case("g1_step_rd%d" % rd, cfg_with(reward_design=rd), "fixed4",
                 [("step", a, t) for t, a in enumerate(toy_actions)])
    for rd in (2, 3, 4):
        run_case("g1_ch_rd%d" % rd, cfg_with(reward_design=rd), "fixed4",
                 [("ch", a, t) for t, a in enumerate(toy_actions)])
    run_case("g1_design", cfg_with(), "fixed4",
             [("design", a, 0) for a in toy_actions])
    for nb in (10, 40):
        run_case("g1_step_rd2_b%d" % nb, cfg_with(state=dict(num_bins=nb)),
                 "fixed4", [("step", a, t) for t, a in enumerate(toy_actions)])
    # longer toy run past the ghost-entry phase (19 slots)
    rng = np.random.default_rng(11)
    run_case("g1_step_rd2_long", cfg_with(), "fixed4",
             rand_steps(rng, "step", 60, 4, 3), table_every=10)
    # non-toy weights branch (network.py:291-295) on the toy topology
    run_case("g1_step_rd1_nontoy", cfg_with(reward_design=1, congestion_test=False,
                                            communication_range=1),
             "fixed4", [("step", a, t) for t, a in enumerate(toy_actions)])

    # ---- state-vector flag coverage (test_env.py:49-85, 527-583) -----------
    allflags = dict(add_reward=True, add_index=True, add_velocity=True,
                    add_position=True, add_channel_obs=True)
    run_case("g1_flags_all", cfg_with(state=allflags, enable_fingerprint=True),
             "fixed4", [("step", a, t) for t, a in enumerate(toy_actions)],
             episode_eps=[(0, 1.0), (0, 0.99), (1, 0.98), (1, 0.5)])
    run_case("g1_flags_real_type1",
             cfg_with(state=dict(action_index="real", type=1, add_channel_obs=True)),
             "fixed4", [("step", a, t) for t, a in enumerate(toy_actions)])
    run_case("g1_flags_nopiggy",
             cfg_with(state=dict(add_positional_dist_piggy=False, add_channel_obs=True)),
             "fixed4", [("step", a, t) for t, a in enumerate(toy_actions)])
    run_case("g1_pf", cfg_with(proportional_fair=True), "fixed4",
             [("step", [0, 0, 1, 2], t) for t in range(14)] +
             [("step", [0, 1, 1, 2], 14), ("step", [0, 0, 1, 2], 15)],
             table_every=8)
    # secondary observation modes
    run_case("g1_posdist_full", cfg_with(state=dict(add_positional_dist=True)),
             "fixed4", [("step", a, t) for t, a in enumerate(toy_actions)])
    run_case("g1_posdist_type1", cfg_with(state=dict(add_positional_dist_type=1)),
             "fixed4", [("step", a, t) for t, a in enumerate(toy_actions)])

    # ---- G2: 3-UE line, multi-hop ordering ----------------------
    line = cfg_with(num_users=3, num_channels=3, highway_length=1000,
                    congestion_test=False)
    init3 = (np.array([0., 200., 400.]), np.zeros(3), np.array([1.5, 1.5, 1.5]))
    run_case("g2_line_012", line, init3, [("step", [0, 1, 2], 0), ("step", [0, 1, 2], 1)])
    run_case("g2_line_210", line, init3, [("step", [2, 1, 0], 0), ("step", [2, 1, 0], 1)])

    # ---- G3: 6-UE design topology, two communication ranges ----------------
    for rc in (100, 250):
        d6 = cfg_with(num_users=6, num_channels=4, highway_length=2000,
                      congestion_test=False, enable_design_topology=True,
                      communication_range=rc)
        rng = np.random.default_rng(30 + rc)
        st = rand_steps(rng, "design", 6, 6, 4) + rand_steps(rng, "step", 6, 6, 4) \
            + rand_steps(rng, "ch", 6, 6, 4)
        run_case("g3_design6_rc%d" % rc, d6, "design6", st, table_every=6)

    # ---- G4: C2-shaped 64 UE / 32 res --------------------------------------
    rng = np.random.default_rng(1234)
    c2 = big_cfg(64, 32, 2000)
    run_case("g4_c2_step", c2, rand_init(rng, 64, 2000, False),
             rand_steps(rng, "step", 40, 64, 32), table_every=39, full_tables=True)
    rng = np.random.default_rng(1235)
    run_case("g4_c2_ch", c2, rand_init(rng, 64, 2000, False),
             rand_steps(rng, "ch", 24, 64, 32, sticky=0.5), full_tables=False)
    rng = np.random.default_rng(1236)
    c2v = big_cfg(64, 32, 2000, mobility_vary=True, reward_design=1,
                  state=dict(add_channel_obs=True, add_reward=True))
    run_case("g4_c2_vary_rd1", c2v, rand_init(rng, 64, 2000, True),
             rand_steps(rng, "step", 30, 64, 32, sticky=0.8),
             vel_updates={24: rng.integers(1, 4, size=64)}, full_tables=False)
    rng = np.random.default_rng(1237)
    run_case("g4_c2_design", c2, rand_init(rng, 64, 2000, False),
             rand_steps(rng, "design", 8, 64, 32), full_tables=False)

    # ---- G5: C3-shaped 256 UE / 64 res, congested --------------------------
    rng = np.random.default_rng(2345)
    run_case("g5_c3_step", big_cfg(256, 64, 4000),
             rand_init(rng, 256, 4000, False),
             rand_steps(rng, "step", 5, 256, 64), full_tables=False)

    # ---- G6: C5-shaped 128 UE / 64 res, mobility_vary ----------------------
    rng = np.random.default_rng(3456)
    run_case("g6_c5_vary", big_cfg(128, 64, 4000, mobility_vary=True),
             rand_init(rng, 128, 4000, True),
             rand_steps(rng, "step", 30, 128, 64),
             vel_updates={24: rng.integers(1, 4, size=128)}, full_tables=False)

    # ---- odd sizes: N not a multiple of 64, A > N, A = 1 -------------------
    rng = np.random.default_rng(4567)
    run_case("g8_n70_a5", big_cfg(70, 5, 1500), rand_init(rng, 70, 1500, False),
             rand_steps(rng, "step", 12, 70, 5), full_tables=False)
    rng = np.random.default_rng(4568)
    run_case("g8_n5_a9_ch", big_cfg(5, 9, 300, reward_design=3, communication_range=120),
             rand_init(rng, 5, 300, False),
             rand_steps(rng, "ch", 25, 5, 9), table_every=24)
    rng = np.random.default_rng(4569)
    run_case("g8_n33_a1", big_cfg(33, 1, 800), rand_init(rng, 33, 800, False),
             rand_steps(rng, "step", 4, 33, 1), full_tables=False)


def main_piggyback():
    # ---- P: State.piggybacking (test_env.py:71-79, 241-254, 260-264): my_step returns each agent's observation
    # with the previous observation of every resource's closest transmitter np.insert-ed at the resource's index -
    # A * A values, the channel-observation section of the state vector; defined while every receiver hears a
    # transmitter on every used resource (communication_range >= highway_length), a KeyError otherwise
    toy_actions = [[0, 1, 2, 0], [0, 0, 0, 0], [1, 1, 2, 2], [2, 2, 2, 1]]
    pb = dict(piggybacking=True, add_channel_obs=True)
    rng = np.random.default_rng(501)
    run_case("g1_piggyback", cfg_with(state=pb), "fixed4",
             [("step", a, t) for t, a in enumerate(toy_actions)] +
             [("step", rng.integers(0, 3, size=4), t) for t in range(4, 30)], table_every=29)
    rng = np.random.default_rng(502)
    run_case("g1_piggyback_flags",
             cfg_with(state=dict(pb, add_reward=True, add_index=True, add_position=True, add_velocity=True,
                                 add_positional_dist=True), reward_design=3, enable_fingerprint=True),
             "fixed4", rand_steps(rng, "step", 12, 4, 3, sticky=0.4), table_every=11,
             episode_eps=[(t // 5, 0.99 ** t) for t in range(12)])
    rng = np.random.default_rng(503)
    run_case("g8_piggyback_n6_a4", big_cfg(6, 4, 400, communication_range=500, state=dict(pb, num_bins=10)),
             rand_init(rng, 6, 400, False), rand_steps(rng, "step", 25, 6, 4), table_every=24)
    rng = np.random.default_rng(504)
    run_case("g8_piggyback_n9_a5_type1hist",
             big_cfg(9, 5, 300, communication_range=300, mobility_vary=True,
                     state=dict(pb, add_positional_dist_type=1, num_bins=8)),
             rand_init(rng, 9, 300, True), rand_steps(rng, "step", 30, 9, 5, sticky=0.5),
             vel_updates={24: rng.integers(1, 4, size=9)}, table_every=29)
    # a highway longer than the communication range: the slot in which a receiver hears nobody on a used
    # resource raises KeyError (`self.prev_obs[None]`, test_env.py:243).  Recorded: the slots before it, and the
    # actions of the slot that raised
    rng = np.random.default_rng(505)
    cfg = big_cfg(8, 3, 1000, communication_range=250, state=pb)
    # (the vehicles start within range of one another just short of the end of the highway; the first to wrap
    # around to x = 0 (network.py:189-206) is 900 m from the rest: network.py:318-332 has no ring distance)
    init = (np.arange(8) * 7.0 + 930.0, np.zeros(8), rng.uniform(1.1, 2.7, size=8))
    steps = rand_steps(rng, "step", 40, 8, 3)
    env = make_env(cfg)
    set_init(env, *init)
    raised_at = -1
    for si, (_, acts, t) in enumerate(steps):
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                env.my_step(np.asarray(acts, dtype=np.int32), t)
        except KeyError as ex:
            assert ex.args == (None,)
            raised_at = si
            break
    assert raised_at >= 0
    run_case("g8_piggyback_keyerror", cfg, init, steps[:raised_at], table_every=max(raised_at - 1, 1),
             extra=dict(keyerror_actions=np.asarray(steps[raised_at][1], dtype=np.int32),
                        keyerror_t=np.int64(steps[raised_at][2])))


def main_trace():
    # ---- T: trace replay (load_positions, network.py:171-178, 194-199) ----------
    rng = np.random.default_rng(91)
    N, A, L = 12, 5, 500
    tr = np.sort(rng.uniform(0, L, size=(7, N)), axis=1) + rng.normal(0, 3, size=(7, N))
    run_case("g9_trace_replay", big_cfg(N, A, L, communication_range=140), rand_init(rng, N, L, False),
             rand_steps(rng, "step", 6, N, A) + [("step", rng.integers(0, A, size=N), t) for t in (6, 7, 13, 20, 3)]
             + rand_steps(rng, "ch", 4, N, A), trace=tr, trace_after=2, table_every=5)


def main_driver():
    # ---- D: driver-loop fixtures -------------------
    run_driver_case("d1_driver_toy", cfg_with(), "fixed4", n_prefill=12, T=60, enable_channel=False,
                    global_reward_avg=True, ia_averaging=False, episode_interval=25, seed=71)
    rng = np.random.default_rng(72)
    run_driver_case("d2_driver_ch_vary", big_cfg(16, 6, 600, mobility_vary=True, reward_design=3,
                                                 communication_range=150),
                    rand_init(rng, 16, 600, True), n_prefill=8, T=80, enable_channel=True,
                    global_reward_avg=True, ia_averaging=True, episode_interval=25, seed=73,
                    ia_penalty_enable=True, ia_penalty_threshold=2)
    # d3: the headline size (64 vehicles / 32 resources) with `enable_channel`: 25 prefill slots of my_step_ch, two
    # episode ends; no information-age term in the rewards, so that the loop also replays without arrival stamps
    rng = np.random.default_rng(74)
    run_driver_case("d3_driver_ch_c2", big_cfg(64, 32, 2000, mobility_vary=True, reward_design=3),
                    rand_init(rng, 64, 2000, True), n_prefill=25, T=52, enable_channel=True,
                    global_reward_avg=True, ia_averaging=False, episode_interval=25, seed=75,
                    ia_penalty_enable=True, ia_penalty_threshold=2)
    # d4: 100 vehicles (step_wide), information-age averaging and the stuck-action penalty
    rng = np.random.default_rng(76)
    run_driver_case("d4_driver_ch_n100", big_cfg(100, 10, 2500, mobility_vary=True, reward_design=2,
                                                 communication_range=200),
                    rand_init(rng, 100, 2500, True), n_prefill=6, T=32, enable_channel=True,
                    global_reward_avg=False, ia_averaging=True, episode_interval=10, seed=77,
                    ia_penalty_enable=True, ia_penalty_threshold=1)



def lanes(rng, N):
    # off-lane vehicles: y in {0, 1, 2} across the highway's height (network.py:31, 104 draws only 0)
    return rng.integers(0, 3, size=N).astype(np.float64)


def sparse_case(name, N, A, seed, T, record_every=1, state=None, y=False, **kw):
    """A highway that breaks apart and re-merges: about one vehicle per communication range, speeds spread by a
    velocity update every 10 slots (network.py:208-223), the first vehicles wrapping at the end of the highway
    (network.py:203) while clusters form, split and merge."""
    rng = np.random.default_rng(seed)
    Rc = 40
    L = N * Rc
    cfg = big_cfg(N, A, L, mobility_vary=True, communication_range=Rc, state=state, **kw)
    x0, y0, v0 = rand_init(rng, N, L, True)
    x0[: max(2, N // 8)] = L - 1 - rng.integers(0, 60, size=max(2, N // 8))     # these wrap within the first slots
    if y:
        y0 = lanes(rng, N)
    steps = rand_steps(rng, "step", T, N, A, sticky=0.3)
    vu = {si: rng.integers(1, 4, size=N) for si in range(0, T - 1, 10)}
    run_case(name, cfg, (x0, y0, v0), steps, vel_updates=vu, table_every=T // 3, record_every=record_every)


RICH = dict(add_reward=True, add_index=True, add_velocity=True, add_position=True, add_channel_obs=True)


def main_curated():
    """g10+: the cells tests/test_fixture_coverage.py counts, chosen by coverage (65 to 256 vehicles in every step
    kind and reward design, sparse highways, off-lane vehicles, > 64 resources, > 256 vehicles, saturated table
    ages, the secondary observation modes, odd histograms, static topology, slot numbers that jump)."""
    # ---- 65 to 256 vehicles, my_step_ch, reward designs 2 / 3 / 4, >= 20 slots ----
    rng = np.random.default_rng(1001)
    run_case("g10_ch_rd2_n96", big_cfg(96, 12, 2400, reward_design=2), rand_init(rng, 96, 2400, False),
             rand_steps(rng, "ch", 22, 96, 12, sticky=0.5), full_tables=False)
    rng = np.random.default_rng(1002)
    run_case("g10_ch_rd3_n130_rich", big_cfg(130, 6, 5200, reward_design=3, communication_range=120,
                                              enable_fingerprint=True, state=RICH),
             rand_init(rng, 130, 5200, False), rand_steps(rng, "ch", 20, 130, 6, sticky=0.6), full_tables=False,
             episode_eps=[(t // 7, 0.99 ** t) for t in range(20)])
    rng = np.random.default_rng(1003)
    run_case("g10_ch_rd4_n256", big_cfg(256, 20, 6000, reward_design=4), rand_init(rng, 256, 6000, False),
             rand_steps(rng, "ch", 20, 256, 20, sticky=0.4), full_tables=False)
    # ---- my_step_design ----
    rng = np.random.default_rng(1004)
    run_case("g10_design_n150", big_cfg(150, 9, 3000, communication_range=150), rand_init(rng, 150, 3000, False),
             rand_steps(rng, "design", 8, 150, 9), full_tables=False)
    # ---- my_step, reward designs 1 / 3 / 4 / 5 ----
    for rd, N, A, seed in ((1, 65, 4, 1011), (3, 128, 6, 1013), (4, 255, 5, 1014), (5, 256, 7, 1015)):
        rng = np.random.default_rng(seed)
        run_case("g10_step_rd%d_n%d" % (rd, N), big_cfg(N, A, 12 * N, reward_design=rd, communication_range=200),
                 rand_init(rng, N, 12 * N, False), rand_steps(rng, "step", 6, N, A), full_tables=False)
    # ---- rich State flags beyond 64 vehicles: State.type 1 + "real" (every receiver hears every transmitter, or
    #      test_env.py:230-232 passes tx_id None on), and type 2 (g10_ch_rd3_n130_rich above) ----
    rng = np.random.default_rng(1020)
    run_case("g10_rich_type1_n70", big_cfg(70, 5, 600, reward_design=1, communication_range=700,
                                           enable_fingerprint=True, state=dict(RICH, type=1, action_index="real")),
             rand_init(rng, 70, 600, False), rand_steps(rng, "step", 8, 70, 5, sticky=0.5), full_tables=False,
             episode_eps=[(t // 3, 0.9 ** t) for t in range(8)])

    # ---- sparse highways that split and re-merge, velocity updates, wrap-around, >= 150 slots ----
    sparse_case("g11_sparse_n48", 48, 3, 1101, 150)
    sparse_case("g11_sparse_n100", 100, 2, 1102, 150, record_every=10)
    sparse_case("g11_sparse_n200", 200, 2, 1103, 150, record_every=25, state=dict(num_bins=8))

    # ---- table ages past 255 (the device's age byte saturates): my_step_ch so that the information age counts,
    #      checkpoints at slots 270 and 299, readouts at every slot in between ----
    rng = np.random.default_rng(1201)
    run_case("g12_age_past_255", big_cfg(12, 3, 3000, communication_range=60, reward_design=3),
             rand_init(rng, 12, 3000, False), rand_steps(rng, "ch", 300, 12, 3), table_every=90)

    # ---- off-lane vehicles, with bin_range != 500 and odd bin counts ----
    rng = np.random.default_rng(1301)
    x0, _, v0 = rand_init(rng, 40, 900, False)
    run_case("g13_offlane_n40", big_cfg(40, 5, 900, communication_range=90, bin_range=123.456,
                                        state=dict(num_bins=7, add_channel_obs=True)),
             (x0, lanes(rng, 40), v0), rand_steps(rng, "step", 30, 40, 5), table_every=29)
    rng = np.random.default_rng(1302)
    x0, _, v0 = rand_init(rng, 90, 1500, False)
    run_case("g13_offlane_n90", big_cfg(90, 4, 1500, communication_range=120, bin_range=250,
                                        state=dict(num_bins=33, add_position=True)),
             (x0, lanes(rng, 90), v0), rand_steps(rng, "step", 12, 90, 4) + rand_steps(rng, "ch", 6, 90, 4),
             full_tables=False)

    # ---- more than 64 resources (the general kernel) ----
    rng = np.random.default_rng(1401)
    run_case("g14_a80_step", big_cfg(20, 80, 700), rand_init(rng, 20, 700, False),
             rand_steps(rng, "step", 10, 20, 80, sticky=0.5), table_every=9)
    rng = np.random.default_rng(1402)
    run_case("g14_a100_ch", big_cfg(30, 100, 900, reward_design=2, communication_range=200),
             rand_init(rng, 30, 900, False), rand_steps(rng, "ch", 8, 30, 100, sticky=0.5), full_tables=False)

    # ---- more than 256 vehicles (csrc/step_large.hpp): 300 and 512, all three step kinds ----
    rng = np.random.default_rng(1501)
    run_case("g15_n300_step_design", big_cfg(300, 8, 6000, reward_design=5), rand_init(rng, 300, 6000, False),
             rand_steps(rng, "step", 3, 300, 8) + rand_steps(rng, "design", 2, 300, 8), full_tables=False)
    rng = np.random.default_rng(1502)
    run_case("g15_n512_ch", big_cfg(512, 40, 9000, reward_design=3), rand_init(rng, 512, 9000, False),
             rand_steps(rng, "ch", 3, 512, 40), full_tables=False)

    # ---- the secondary observation modes at 64 / 80 vehicles ----
    rng = np.random.default_rng(1601)
    run_case("g16_posdist_n64", big_cfg(64, 4, 1600, state=dict(add_positional_dist=True)),
             rand_init(rng, 64, 1600, False), rand_steps(rng, "step", 5, 64, 4), full_tables=False)
    rng = np.random.default_rng(1602)
    run_case("g16_type1hist_n80", big_cfg(80, 6, 1600, mobility_vary=True,
                                          state=dict(add_positional_dist_type=1, num_bins=12)),
             rand_init(rng, 80, 1600, True), rand_steps(rng, "step", 8, 80, 6),
             vel_updates={3: rng.integers(1, 4, size=80)}, full_tables=False)

    # ---- proportional_fair: sticky actions, so that the counters pass pf_threshold (test_env.py:215-222) ----
    rng = np.random.default_rng(1701)
    run_case("g17_pf_n32", big_cfg(32, 4, 800, proportional_fair=True), rand_init(rng, 32, 800, False),
             rand_steps(rng, "step", 36, 32, 4, sticky=0.97), table_every=35)

    # ---- static topology (mobility False, enable_design_topology True: make_static_env) ----
    rng = np.random.default_rng(1801)
    run_case("g18_static_n32", big_cfg(32, 5, 900, mobility=False, enable_design_topology=True,
                                       communication_range=150),
             rand_init(rng, 32, 900, False),
             rand_steps(rng, "design", 5, 32, 5) + rand_steps(rng, "step", 5, 32, 5) + rand_steps(rng, "ch", 5, 32, 5),
             table_every=14)

    # ---- congestion_test weights beyond the toy (network.py:284-290: m == norm) ----
    rng = np.random.default_rng(1901)
    run_case("g19_toyweights_n9", cfg_with(num_users=9, num_channels=5, highway_length=300, reward_design=1),
             rand_init(rng, 9, 300, False), rand_steps(rng, "step", 20, 9, 5), table_every=19)

    # ---- trace replay at 70 vehicles ----
    rng = np.random.default_rng(2001)
    N, A, L = 70, 4, 1400
    tr = np.sort(rng.uniform(0, L, size=(5, N)), axis=1) + rng.normal(0, 3, size=(5, N))
    run_case("g20_trace_n70", big_cfg(N, A, L, communication_range=140), rand_init(rng, N, L, False),
             rand_steps(rng, "step", 4, N, A) + [("step", rng.integers(0, A, size=N), t) for t in (4, 9, 17, 2)]
             + rand_steps(rng, "ch", 3, N, A), trace=tr, trace_after=1, full_tables=False)

    # ---- State.piggybacking with 16 resources (A * A = 256 observation columns) ----
    rng = np.random.default_rng(2101)
    run_case("g21_piggyback_a16", big_cfg(6, 16, 200, communication_range=300,
                                          state=dict(piggybacking=True, add_channel_obs=True)),
             rand_init(rng, 6, 200, False), rand_steps(rng, "step", 10, 6, 16, sticky=0.4), table_every=9)

    # ---- slot numbers: a start beyond 10^6 and a sequence that jumps forwards and back (the information age of
    #      a slot before the last arrival is a negative list index, network.py:571-573) ----
    rng = np.random.default_rng(2201)
    ts = 1_000_000 + np.array([0, 1, 2, 3, 10, 11, 5, 6, 40, 41, 42, 20, 21, 22, 23, 24])
    run_case("g22_tjump_n20", big_cfg(20, 4, 500, reward_design=2, communication_range=150),
             rand_init(rng, 20, 500, False),
             [("ch", rng.integers(0, 4, size=20), int(t)) for t in ts], table_every=15)


# ---- the seeded differential sweep (`fuzz`) ------------------------------------------------

FUZZ_BUDGET = 2.5e7          # dictionary operations of the reference per case: ~10 s of CPU


def draw_ref_case(i):
    """Case i of the sweep: a configuration both the reference and EnvConfig.validate() accept, its topology,
    its steps.  Combinations the reference cannot run are remapped; each remap names the reference line."""
    rng = np.random.default_rng(50000 + i)
    N = int(rng.choice([63, 64, 65, 128, 255, 256, 257]) if rng.random() < 0.4 else
            rng.choice([rng.integers(1, 9), rng.integers(9, 65), rng.integers(65, 257), rng.integers(257, 601)]))
    A = int(rng.choice([rng.integers(1, 9), rng.integers(9, 65), rng.integers(65, 131)], p=[0.4, 0.4, 0.2]))
    K = int(rng.integers(1, 65))
    kind = str(rng.choice(["step", "step", "ch", "design", "mixed"]))
    rd = int(rng.choice([2, 3, 4])) if kind in ("ch", "mixed") else int(rng.integers(1, 6))
    #   (my_step_ch with reward design 1 or 5 only prints "This is not defined", test_env.py:419-420, 428-429)
    L = int(rng.choice([4, 10, 25, 40]) * N + rng.integers(20, 200))
    Rc = float(rng.choice([L + 10.0, 250.0, 120.0, 3.0 * L / N, 1.2 * L / N]))
    st = dict(type=int(rng.choice([1, 2])), add_reward=bool(rng.random() < 0.3), add_action=bool(rng.random() < 0.8),
              add_index=bool(rng.random() < 0.3), add_velocity=bool(rng.random() < 0.3),
              action_index=str(rng.choice(["binary", "real"])), piggybacking=False,
              add_position=bool(rng.random() < 0.3), add_positional_dist=bool(rng.random() < 0.2),
              add_positional_dist_piggy=bool(rng.random() < 0.8), add_positional_dist_type=int(rng.choice([1, 2, 2])),
              add_channel_obs=bool(rng.random() < 0.4), num_bins=K)
    mobility = bool(rng.random() < 0.85)
    offlane = bool(rng.random() < 0.25)
    if st["type"] == 1 and st["add_positional_dist_piggy"] and Rc * Rc <= (L * L + 4.0):
        # test_env.py:230-232 hands tx_id None to received_update when no transmitter is in range
        # (network.py:583: self.vehicles[None], TypeError) - SURVEY Q9
        st["type"] = 2
    if kind == "step" and rng.random() < 0.1 and A <= 20:
        # State.piggybacking: type 2 with add_channel_obs (EnvConfig.validate: no fixed state vector otherwise),
        # my_step only (my_step_ch / my_step_design return A columns where get_state_space counts A * A,
        # test_env.py:71-72, 316, 443), and every receiver in range of a transmitter (prev_obs[None], test_env.py:243)
        st.update(piggybacking=True, type=2, add_channel_obs=True)
        Rc = L + 10.0
    if not mobility and st["add_positional_dist"]:
        st["add_positional_dist"] = False      # network.py:341-344: dist_sign reads pos_of_nodes, which is empty
    if st["add_positional_dist"] and N < 3:
        st["add_positional_dist"] = False      # network.py:429: two vehicles on one spot divide by max_dist 0
    vary = bool(rng.random() < 0.4)
    cfg = cfg_with(num_users=N, num_channels=A, highway_length=L,
                   reward_design=rd, mobility=mobility, enable_design_topology=not mobility, mobility_vary=vary,
                   enable_fingerprint=bool(rng.random() < 0.3), proportional_fair=bool(rng.random() < 0.2),
                   congestion_test=bool(rng.random() < 0.2), communication_range=Rc,
                   bin_range=float(rng.choice([50.0, 123.456, 250.0, 500.0, 1000.0])), state=st)
    # the reference's cost per slot: tables N * N, received_update N * N * min(A, N); my_step_ch adds N^3 / A
    per_slot = float(N) * N * (4 + min(A, N)) + (float(N) ** 3 / A if kind in ("ch", "mixed") else 0.0)
    T = int(max(2, min(40, FUZZ_BUDGET // per_slot)))
    x0, y0, v0 = rand_init(rng, N, L, vary)
    if offlane:
        y0 = lanes(rng, N)
    sticky = float(rng.choice([0.0, 0.5, 0.9]))
    acts = rng.integers(0, A, size=N)
    t = int(rng.choice([0, 0, 7, 10 ** 6]))
    steps = []
    for si in range(T):
        acts = np.where(rng.random(N) < sticky, acts, rng.integers(0, A, size=N))
        mode = kind if kind != "mixed" else str(rng.choice(["step", "ch", "design"]))
        steps.append((mode, acts.copy(), t))
        # mostly t + 1; now and then a jump forwards or back (back by < 100: network.py:571-573 indexes a list
        # of 100 with t - last_arrival)
        t = max(0, t + (1 if rng.random() < 0.85 else int(rng.integers(-30, 60))))
    vu = {si: rng.integers(1, 4, size=N) for si in range(4, T, 5)} if vary else None
    trace = trace_after = None
    if mobility and rng.random() < 0.1:
        trace = np.sort(rng.uniform(0, L, size=(int(rng.integers(1, 6)), N)), axis=1) + rng.normal(0, 3, size=(1, N))
        trace_after = int(rng.integers(0, T))
    eps = [(si // 3, 0.97 ** si) for si in range(T)]
    return dict(cfg=cfg, init=(x0, y0, v0), steps=steps, vel_updates=vu, trace=trace, trace_after=trace_after,
                episode_eps=eps, kind=kind, offlane=offlane)


def fuzz_one(i):
    """One sweep case -> its report row (a dict)."""
    import traceback
    from tests.golden_util import Golden, compare_with_reference
    c = draw_ref_case(i)
    cfg, st = c["cfg"], c["cfg"]["State"]
    flags = [k[4:] for k in ("add_reward", "add_index", "add_velocity", "add_position", "add_positional_dist",
                             "add_channel_obs") if st[k]]
    flags += ["type%d" % st["type"], st["action_index"] if st["add_action"] else "noaction",
              ("hist%d" % st["add_positional_dist_type"]) if st["add_positional_dist_piggy"] else "notables"]
    flags += [k for k in ("mobility_vary", "enable_fingerprint", "proportional_fair", "congestion_test") if cfg[k]]
    flags += (["piggybacking"] if st["piggybacking"] else []) + (["static"] if not cfg["mobility"] else []) \
        + (["offlane"] if c["offlane"] else []) + (["trace"] if c["trace"] is not None else [])
    row = dict(seed=i, N=cfg["num_users"], A=cfg["num_channels"], K=st["num_bins"], T=len(c["steps"]), mode=c["kind"],
               rd=cfg["reward_design"], Rc=cfg["communication_range"], L=cfg["highway_length"],
               bin_range=cfg["bin_range"], t0=c["steps"][0][2], flags=" ".join(flags))
    t0 = time.time()
    with tempfile.TemporaryDirectory() as tmp:
        try:
            path = run_case("fuzz%d" % i, cfg, c["init"], c["steps"], vel_updates=c["vel_updates"], trace=c["trace"],
                            trace_after=c["trace_after"], episode_eps=c["episode_eps"],
                            table_every=max(1, len(c["steps"]) - 1), out_dir=tmp, quiet=True)
        except Exception as ex:                  # a finding, written down with the reference's own line
            tb = traceback.extract_tb(ex.__traceback__)
            where = [f for f in tb if f.filename.startswith(REF)]
            row["verdict"] = "REFERENCE RAISED %s at %s" % (type(ex).__name__, "%s:%d" % (
                os.path.basename(where[-1].filename), where[-1].lineno) if where else "generator")
            row["seconds"] = time.time() - t0
            return row
        row["ref_s"] = time.time() - t0
        try:
            compare_with_reference(Golden("fuzz%d" % i, path=path))
            row["verdict"] = "ok"
        except AssertionError as ex:
            a = ex.args[0] if ex.args else ("?", -1)
            row["verdict"] = "MISMATCH %s %s" % (a[0], a[1]) if isinstance(a, tuple) else "MISMATCH %s" % (a,)
    # what the device build says to this configuration without a GPU: diral_env_validate's documented refusals
    try:
        import ctypes
        from diral_amd import _lib
        from diral_amd.config import EnvConfig
        rc = _lib.load().diral_env_validate(ctypes.byref(EnvConfig.from_dict(cfg).to_c()))
        row["device"] = {0: "ok", -3: "DIRAL_ERR_UNSUPPORTED"}.get(rc, "status %d" % rc)
    except Exception as ex:
        row["device"] = "validate() raised %s" % type(ex).__name__
    row["seconds"] = time.time() - t0
    return row


def main_fuzz(n=320, first=0, procs=None):
    import multiprocessing
    t0 = time.time()
    with multiprocessing.Pool(procs or min(8, os.cpu_count() or 1)) as pool:
        rows = pool.map(fuzz_one, range(first, first + n), chunksize=1)
    bad = [r for r in rows if r["verdict"].startswith("MISMATCH")]
    raised = [r for r in rows if r["verdict"].startswith("REFERENCE")]
    refused = [r for r in rows if r.get("device", "ok") != "ok"]
    cols = ("seed", "N", "A", "K", "T", "mode", "rd", "L", "Rc", "bin_range", "t0", "flags", "seconds", "device",
            "verdict")
    lines = ["# Differential sweep: the reference against the CPU oracle", "",
             "Written by `python tests/golden/gen_golden.py fuzz %d %d`; do not edit by hand." % (n, first), "",
             "Each row is `draw_ref_case(seed)`: recorded from the reference with `run_case`, replayed through",
             "`Oracle(sq_mode=SQ_POW)` and compared like `test_oracle_reproduces_reference_bit_exact` (every output",
             "of every slot bit for bit, the table planes by hash at every slot and in full at the first and last).",
             "`device` is what `diral_env_validate` answers to the configuration (no GPU takes part in the sweep).",
             "The `seconds` column is the only one that changes from run to run.", "",
             "## Summary", "",
             "- seeds %d to %d: %d cases, %d ok, %d MISMATCH, %d REFERENCE RAISED (%.1f %%; the cap is 5 %%)" % (
                 first, first + n - 1, n, n - len(bad) - len(raised), len(bad), len(raised), 100.0 * len(raised) / n),
             "- sizes: N %d to %d (%d cases beyond 64 vehicles, %d beyond 256), A %d to %d (%d beyond 64 resources)" % (
                 min(r["N"] for r in rows), max(r["N"] for r in rows), sum(r["N"] > 64 for r in rows),
                 sum(r["N"] > 256 for r in rows), min(r["A"] for r in rows), max(r["A"] for r in rows),
                 sum(r["A"] > 64 for r in rows)),
             "- step kinds: " + ", ".join("%s %d" % (k, sum(r["mode"] == k for r in rows))
                                          for k in ("step", "ch", "design", "mixed")),
             "- configurations the device build refuses (documented `DIRAL_ERR_UNSUPPORTED`): " +
             (", ".join("seed %d (N=%d A=%d K=%d %s)" % (r["seed"], r["N"], r["A"], r["K"], r["device"])
                        for r in refused) or "none"),
             "- mismatches: " + (", ".join("seed %d: %s" % (r["seed"], r["verdict"]) for r in bad) or "none"),
             "- reference exceptions: " + (", ".join("seed %d: %s" % (r["seed"], r["verdict"]) for r in raised) or "none"),
             "", "## Cases", "", "| " + " | ".join(cols) + " |", "|" + "---|" * len(cols)]
    for r in rows:
        lines.append("| " + " | ".join(("%.1f" % r[c]) if c == "seconds" else ("%g" % r[c]) if isinstance(r.get(c), float)
                                       else str(r.get(c, "-")) for c in cols) + " |")
    with open(os.path.join(OUT, "FUZZ_SWEEP.md"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("%d cases in %.0f s: %d mismatches, %d reference exceptions" % (n, time.time() - t0, len(bad), len(raised)))


def run_sps_case(name, n_agents, A, T, threshold, seed, level_lo, level_hi, tie_step, keep_lo=0.0):
    """The reference's SPS agent (algorithms/v2x_sps.py) itself, one object per agent, fed
    recorded selection windows; its three global-RNG calls are mocked with recorded draws:
      random.randint(a, b)  -> the recorded counter / initial values
      random.random()       -> the recorded keep draw
      random.choice(sB)     -> sB[draw % len(sB)] with the recorded draw
    Recorded: initial (prev_action, counter), per step and agent the window (as integer
    codes: window = code * tie_step, exact in float64), the three draws, and the decisions
    (action, reselection_counter, prev_action after the step) plus how often the threshold
    was raised (len of the while loop, v2x_sps.py:41-50) for the fixture's own statistics."""
    sys.path.insert(0, "/root/reference/algorithms")
    import v2x_sps as ref_sps
    rng = np.random.default_rng(seed)
    cur = {}
    ref_sps.random = mock.MagicMock()

    def fake_randint(a, b):
        if (a, b) == (5, 16):
            return int(cur["counter"])
        raise AssertionError((a, b))
    ref_sps.random.randint.side_effect = fake_randint
    ref_sps.random.random.side_effect = lambda: float(cur["keep"])
    ref_sps.random.choice.side_effect = lambda seq: seq[int(cur["choice"]) % len(seq)]

    init_prev = rng.integers(0, A, size=n_agents)           # randint(0, selection_window) with window = A - 1
    init_cnt = rng.integers(5, 16, size=n_agents)            # randint(5, 15)
    agents = []
    for u in range(n_agents):
        draws = [int(init_prev[u]), int(init_cnt[u])]
        ref_sps.random.randint.side_effect = lambda a, b, d=draws: d.pop(0)
        ag = ref_sps.SemiPersistentScheduling(u, A - 1, threshold)
        assert ag.prev_action == init_prev[u] and ag.reselection_counter == init_cnt[u]
        agents.append(ag)
    ref_sps.random.randint.side_effect = fake_randint

    codes = np.zeros((T, n_agents, A), np.int16)
    d_counter = rng.integers(5, 17, size=(T, n_agents)).astype(np.int32)
    d_keep = keep_lo + (1.0 - keep_lo) * rng.random((T, n_agents))   # keep_lo > 0: more re-selections per recorded step
    d_choice = rng.integers(0, 1 << 20, size=(T, n_agents)).astype(np.int32)
    actions = np.zeros((T, n_agents), np.int32)
    counters = np.zeros((T, n_agents), np.int32)
    prevs = np.zeros((T, n_agents), np.int32)
    for t in range(T):
        for u, ag in enumerate(agents):
            # windows: mostly a busy band around the threshold (ties by quantisation), sometimes
            # everything far above it (several 3 dB raises), sometimes nearly all free
            r = rng.random()
            if r < 0.2:
                c = rng.integers(level_hi, level_hi + 40, size=A)
            elif r < 0.35:
                c = rng.integers(level_lo - 60, level_lo, size=A)
            else:
                c = rng.integers(level_lo, level_hi, size=A)
            codes[t, u] = c
            win = [float(v) * tie_step for v in c]
            cur.update(counter=d_counter[t, u], keep=d_keep[t, u], choice=d_choice[t, u])
            actions[t, u] = ag.step(win)
            counters[t, u] = ag.reselection_counter
            prevs[t, u] = ag.prev_action
    n_resel = ref_sps.random.choice.call_count
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, A=np.int64(A), threshold=np.float64(threshold), tie_step=np.float64(tie_step),
                        init_prev=init_prev.astype(np.int32), init_counter=init_cnt.astype(np.int32),
                        codes=codes, draw_counter=d_counter, draw_keep=d_keep, draw_choice=d_choice,
                        actions=actions, counters=counters, prev_actions=prevs, reselections=np.int64(n_resel))
    print("%-28s agents=%-3d A=%-2d steps=%-3d reselections=%d  %7.1f KB" % (
        name, n_agents, A, T, n_resel, os.path.getsize(path) / 1024))


def main_sps():
    # ---- S: the SPS baseline, recorded from algorithms/v2x_sps.py ----
    # integer-dB windows around an integer threshold: ties, threshold raises
    run_sps_case("s1_sps_int_threshold", n_agents=40, A=12, T=140, threshold=-110.0, seed=81,
                 level_lo=-125, level_hi=-95, tie_step=1.0)
    # non-integer threshold and quarter-dB windows: `tmp_threshold += 3` accumulates roundings
    # ((thr + 3) - 3 != thr), boundary subframes sit within an ulp of the threshold sequence
    run_sps_case("s2_sps_frac_threshold", n_agents=40, A=20, T=140, threshold=-110.3, seed=82,
                 level_lo=-500, level_hi=-380, tie_step=0.25)
    # tiny window (A = 3: min_sA = 0.6) and A = 1 (the only subframe is the previous action:
    # sA stays empty while len(sA) < 0.2 ... the reference loops forever there, so A >= 2)
    run_sps_case("s3_sps_small_window", n_agents=24, A=3, T=200, threshold=-110.0, seed=83,
                 level_lo=-120, level_hi=-100, tie_step=0.5)
    # wide windows: exactly one wavefront of subframes, then 2 and 4 subframes per lane of the
    # wave-cooperative kernel (csrc/agent_kernels.hpp), then beyond it (one thread per agent)
    run_sps_case("s4_sps_window64", n_agents=70, A=64, T=40, threshold=-110.0, seed=84,
                 level_lo=-125, level_hi=-95, tie_step=1.0, keep_lo=0.7)
    run_sps_case("s5_sps_window100", n_agents=30, A=100, T=60, threshold=-110.3, seed=85,
                 level_lo=-460, level_hi=-400, tie_step=0.25, keep_lo=0.7)
    run_sps_case("s6_sps_window200", n_agents=20, A=200, T=60, threshold=-110.0, seed=86,
                 level_lo=-118, level_hi=-102, tie_step=1.0, keep_lo=0.7)
    run_sps_case("s7_sps_window300", n_agents=12, A=300, T=70, threshold=-110.0, seed=87,
                 level_lo=-240, level_hi=-200, tie_step=0.5, keep_lo=0.7)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "driver":
        main_driver()
    elif len(sys.argv) > 1 and sys.argv[1] == "sps":
        main_sps()
    elif len(sys.argv) > 1 and sys.argv[1] == "trace":
        main_trace()
    elif len(sys.argv) > 1 and sys.argv[1] == "piggyback":
        main_piggyback()
    elif len(sys.argv) > 1 and sys.argv[1] == "curated":
        main_curated()
    elif len(sys.argv) > 1 and sys.argv[1] == "fuzz":
        main_fuzz(*[int(a) for a in sys.argv[2:4]])
    else:
        main()
        main_curated()
        main_piggyback()
        main_trace()
        main_driver()
        main_sps()
