"""What the K-slots-per-launch GPU tests share: the two comparisons the family rests on, each stated once.

Open loop (`VecV2VEnv.rollout` and its information-age / replay blocks): `slot_loop` is the loop a launch stands for -
K x [`_step`, optionally `info_age`, `diral_driver_shape`, `update_velocity` behind an episode end] on a twin handle -,
`as_rollout` cuts its result to what one launch returns, `assert_same` / `assert_same_envs` / `go_on_alike` compare.

Closed loop (`step_policy(slots=K)`): `closed_loop_twins` runs the same slots as K one-slot calls on one handle and as one
K-slot launch on another, `compare_closed_loop` compares the two sides.

The comparators take any tensors (tests/test_kslots_harness.py runs them on the CPU); everything that makes a handle needs
a GPU."""
from types import SimpleNamespace

import numpy as np
import torch

from diral_amd.config import KERNEL_CH, KERNEL_FAST64, KERNEL_POLICY, STEP_MY_STEP, STEP_MY_STEP_CH, bench_config
from diral_amd.vec_env import driver_shape

DEV = "cuda:0"
RICH = dict(add_channel_obs=True, add_reward=True, add_index=True, add_velocity=True, add_position=True)
MODES = {"my_step": STEP_MY_STEP, "my_step_ch": STEP_MY_STEP_CH}
VEL_SEED = 4242
PEN_THR, PEN_VAL = 2, -10.0


# ---- the handles -------------------------------------------------------------------------------------------------------
def chain_cfg(N, A, rd=2, vary=False, rich=False, track=False, L=None, Rc=120.0):
    """L = 30 N + 50 with a communication range of 120 (tests/test_driver_loop.py): some pairs are out of range."""
    kw = dict(reward_design=rd, communication_range=Rc, mobility_vary=vary)
    if rich:
        kw["State"] = RICH
    cfg = bench_config(N, A, 30.0 * N + 50 if L is None else L, **kw)
    return cfg.replace(track_arrival=True) if track else cfg


def start(cfg, B, seed, x0=None):
    """(x0, v0) of B envs: one generator, the positions drawn first (none where `x0` is given), then the velocities."""
    rng = np.random.default_rng(seed)
    if x0 is None:
        x0 = rng.integers(0, int(cfg.highway_length), size=(B, cfg.num_users)).astype(np.float64)
    v0 = np.full((B, cfg.num_users), 1.7) if cfg.mobility_vary else rng.uniform(1.1, 2.7, size=(B, cfg.num_users))
    return x0, v0


def twins(cfg, B, dtype, start, n=2):
    from diral_amd.vec_env import VecV2VEnv
    envs = []
    for _ in range(n):
        env = VecV2VEnv(cfg, batch=B, device=DEV, out_dtype=dtype)
        env.reset_topology(start[0], 0.0, start[1])
        envs.append(env)
    return envs


def stuck_penalty_state(B, N):
    """`stuck_penalty=` of rollout / step_policy: (threshold, value, counter, previous actions)."""
    return (PEN_THR, PEN_VAL, torch.zeros((B, N), dtype=torch.int32, device=DEV), torch.full((B, N), -1, dtype=torch.int32, device=DEV))


# ---- the open loop -----------------------------------------------------------------------------------------------------
def slot_loop(env, seq, t, mode, *, avg=True, pen=None, ia_prev=None, want_ia=False, stop=None, want_obs=True, want_xpos=False):
    """The loop the launches stand for, on `env` (which carries the trace, if any): K x [step, info_age, diral_driver_shape,
    update_velocity behind an episode end] - everything of every slot, stacked [K, ...].  `states` is None where no slot
    builds a state vector (`want_obs=False`, or a config without one); `xpos` (get_x_pos() behind every slot) on request."""
    K, B, N = seq.shape[0], env.B, env.N
    ei = env.cfg.episode_interval
    o = dict(dtype=env.out_dtype, device=env.device)
    shaped, sum_r, coll = torch.empty((K, B, N), **o), torch.empty((K, B), **o), torch.empty((K, B), **o)
    if want_ia:
        ia_all = torch.empty((K, B, 100), dtype=torch.int32, device=env.device)
        ia_sum = torch.empty((K, B), dtype=torch.int64, device=env.device)
    if ia_prev is not None:
        ia_pen = torch.zeros((K, B), dtype=torch.int32, device=env.device)
    keep_obs = want_obs and env.S > 0
    states, rews, dones, xpos = [], [], [], []
    thr, val, cnt, pa = pen if pen is not None else (0, 0.0, None, None)
    for k in range(K):
        a = seq[k].contiguous()
        obs, rew, done = env._step(MODES[mode], a, t + k, want_obs=want_obs)
        env.t = t + k + 1
        if want_ia:
            ia_all[k] = env.info_age(t + k)
        driver_shape(env, rew, a, shaped=shaped[k], sum_r=sum_r[k], collision=coll[k], global_reward_avg=avg,
                     ia=ia_all[k] if want_ia else None, sum_ia_prev=ia_prev, ia_sum=ia_sum[k] if want_ia else None,
                     ia_penalty=ia_pen[k] if ia_prev is not None else None, pen_counter=cnt, prev_actions=pa,
                     pen_threshold=thr, pen_value=val)
        rews.append(rew.clone()); dones.append(done.clone())
        if keep_obs:
            states.append(obs.clone())
        if want_xpos:
            xpos.append(env.get_x_pos().clone())
        if (t + k) % ei == ei - 1:
            env.update_velocity(seed=VEL_SEED + (t + k) // ei)
        if stop is not None and k == stop[0]:
            stop[1](env)
    out = dict(states=torch.stack(states) if keep_obs else None, reward=torch.stack(rews), done=torch.stack(dones),
               shaped=shaped, sum_r=sum_r, collision=coll)
    if want_xpos:
        out["xpos"] = torch.stack(xpos)
    if want_ia:
        out.update(ia=ia_all, ia_sum=ia_sum)
    if ia_prev is not None:
        out["ia_penalty"] = ia_pen
    return out


def as_rollout(stacked, states, log=False):
    """What ONE launch over all the slots of `stacked` returns (VecV2VEnv.rollout): reward and done of the last slot,
    `states` "last" / "all" / None, the per-slot outputs as they are; `xpos` only where the launch logs positions."""
    out = {k: v for k, v in stacked.items() if k not in ("states", "reward", "done", "xpos")}
    st = stacked["states"]
    out["states"] = None if (states is None or st is None) else (st if states == "all" else st[-1])
    out["reward"], out["done"] = stacked["reward"][-1], stacked["done"][-1]
    if log:
        out["xpos"] = stacked["xpos"]
    return out


def assert_equal(want, got, what):
    """Two tensors: shape, dtype and every element; the first differing indices in the message."""
    assert want.shape == got.shape and want.dtype == got.dtype, (what, want.shape, got.shape, want.dtype, got.dtype)
    assert torch.equal(want, got), (what, (want != got).nonzero()[:5])


def assert_same(want, got, what):
    """Two result dicts: the same keys, None where the other has None, and equal tensors (`assert_equal`)."""
    assert set(want) == set(got), (what, sorted(want), sorted(got))
    for key in want:
        assert (want[key] is None) == (got[key] is None), (what, key)
        if want[key] is not None:
            assert_equal(want[key], got[key], (what, key))


def assert_same_envs(e1, e2, entries=True):
    """Positions, velocities, the tables in every stored form (planes, packed words, ring as export_entries reads them),
    arrival stamps where tracked, the metrics with the PRR columns.  Returns the exported state."""
    s1, s2 = e1.export_state(), e2.export_state()
    assert set(s1) == set(s2)
    for key in s1:
        assert torch.equal(s1[key], s2[key]), key
    if entries:
        assert torch.equal(e1.export_entries(), e2.export_entries())
    m1, m2 = e1.metrics(), e2.metrics()
    assert torch.equal(m1, m2), (m1 != m2).nonzero()[:4]
    return s1


def go_on_alike(e_loop, e_one, mode, t, info_age=False):
    """Both handles go on alike: three further one-slot steps, then the sticky error flags."""
    for k in range(3):
        a = e_loop.sample(900 + k)
        o1, r1, d1 = e_loop._step(MODES[mode], a, t + k)
        o2, r2, d2 = e_one._step(MODES[mode], a, t + k)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
        if info_age:
            assert torch.equal(e_loop.info_age(t + k), e_one.info_age(t + k))
    e_loop.check(); e_one.check()


def check_rollout(cfg, B, dtype, K, mode="my_step", states="last", t0=0, warm=0, avg=True, pen=False, constant=False, reps=2,
                  x0=None, family=KERNEL_FAST64, seed=31):
    """`reps` plain rollout launches of K slots, the second continuing the first, against the loop on a twin env; then the
    exported state, the metrics, three further ordinary steps and env.check().  Returns (state, penalty tensors, env) of
    the launches' side."""
    e_loop, e_one = twins(cfg, B, dtype, start(cfg, B, seed, x0))
    N = cfg.num_users
    pens = [stuck_penalty_state(B, N) if pen else None for _ in range(2)]
    for w in range(warm):                                            # ordinary steps on both sides first
        a = e_loop.sample(500 + w)
        for env in (e_loop, e_one):
            env._step(MODES[mode], a, w)
    t = t0
    for rep in range(reps):
        if constant:
            seq = e_loop.sample(9000 + rep).unsqueeze(0).expand(K, B, N).contiguous()
        else:
            seq = torch.stack([e_loop.sample(7000 + 100 * rep + k) for k in range(K)])
        want = as_rollout(slot_loop(e_loop, seq, t, mode, avg=avg, pen=pens[0], want_obs=states is not None), states)
        got = e_one.rollout(seq, t, mode=mode, states=states, global_reward_avg=avg, stuck_penalty=pens[1], vel_seed=VEL_SEED)
        torch.cuda.synchronize()
        lk = e_one.last_kernel()
        assert (lk & 15) == family and (lk & KERNEL_POLICY), lk
        assert bool(lk & KERNEL_CH) == (mode == "my_step_ch")
        assert_same(want, got, rep)
        assert e_one.t == t + K == e_loop.t
        t += K
    s = assert_same_envs(e_loop, e_one)
    if pen:
        assert torch.equal(pens[0][2], pens[1][2]) and torch.equal(pens[0][3], pens[1][3])
    go_on_alike(e_loop, e_one, mode, t)
    return s, pens[1], e_one


# ---- the closed loop ---------------------------------------------------------------------------------------------------
def closed_loop_twins(cfg, B, dt, K, t0, *, topo, pol_seed, keep, mode=None, want_obs=True, one_slot_obs=None, want_chobs=False,
                      vel_seed=0, clock=False, pen=False, reps=2, prep=None, tail_slot=False, want_start=False,
                      expect_one=None, expect_fused=None):
    """The same slots on two envs: K one-slot `step_policy` calls (side 0) and one K-slot launch (side 1), `reps` times, behind
    `t0` one-slot calls on both sides; with `tail_slot` one more one-slot call on both behind them.

    `topo`: a seed for reset_topology, or its positional arguments.  `one_slot_obs`: `want_obs` of the one-slot calls where it
    differs from the launch's.  `clock`: a device SlotClock carries the slot number.  `prep(env, policy)` runs before the
    first slot.  `expect_one` / `expect_fused`: what `last_kernel()` must satisfy behind each one-slot call / the launch.
    `want_start`: keep (positions, actions) behind the warm-up.

    Returns the two sides: env, pol, outs (one dict per launch: every slot's shaped / sum_r / coll, the last slot's obs / rew /
    done / chobs, the next actions), pen (the penalty tensors), last (the actions behind the tail slot), start."""
    from diral_amd.rollout import SlotClock
    from diral_amd.sps import SpsPolicy
    from diral_amd.vec_env import VecV2VEnv
    N, A = cfg.num_users, cfg.num_channels
    ei = cfg.episode_interval
    one_obs = want_obs if one_slot_obs is None else one_slot_obs
    o = dict(dtype=dt, device=DEV)
    sides = []
    for fused in (False, True):
        env = VecV2VEnv(cfg, batch=B, device=DEV, out_dtype=dt)
        if isinstance(topo, int):
            env.reset_topology(seed=topo)
        else:
            env.reset_topology(*topo)
        pol = SpsPolicy(B, N, A, device=DEV, seed=pol_seed)
        pol.keep_prob = keep
        if prep is not None:
            prep(env, pol)
        clk = SlotClock(DEV, 0) if clock else None
        if clk is not None:
            env.set_clock(clk.t)
        pn = stuck_penalty_state(B, N) if pen else None
        a = pol.prev_action.clone()
        nxt = torch.empty_like(a)
        t = 0

        def one(sh=None, sr=None, co=None):
            nonlocal a, nxt, t
            # (with a device clock the by-value slot number is an offset: 0)
            env.step_policy(a, 0 if clk is not None else t, pol, nxt, shaped_out=sh, sum_r_out=sr, collision_out=co, clock=clk,
                            seed_offset=0, mode=mode, want_chobs=want_chobs, want_obs=one_obs,
                            stuck_penalty=pn if sh is not None else None)
            if expect_one is not None:
                assert expect_one(env.last_kernel()), env.last_kernel()
            if cfg.mobility_vary and t % ei == ei - 1:
                env.update_velocity(seed=vel_seed + t // ei)
            if clk is not None:
                env.lib.diral_clock_add(clk.ptr(), 1, env._stream())
            a, nxt = nxt, a
            t += 1
        sh0 = torch.zeros((B, N), **o) if pen else None
        for _ in range(t0):                                       # warm-up, one slot per call on both sides
            one(sh0)
        begin = (env.export_state()["pos_x"].cpu().numpy(), a.cpu().numpy()) if want_start else None
        outs = []
        for rep in range(reps):
            sh, sr, co = torch.zeros((K, B, N), **o), torch.zeros((K, B), **o), torch.zeros((K, B), **o)
            if fused:
                env.step_policy(a, 0 if clk is not None else t, pol, nxt, shaped_out=sh, sum_r_out=sr, collision_out=co, slots=K,
                                vel_seed=vel_seed, clock=clk, seed_offset=0, mode=mode, want_chobs=want_chobs, want_obs=want_obs,
                                stuck_penalty=pn)
                if expect_fused is not None:
                    assert expect_fused(env.last_kernel()), env.last_kernel()
                if clk is not None:
                    env.lib.diral_clock_add(clk.ptr(), K, env._stream())
                a, nxt = nxt, a
                t += K
            else:
                for k in range(K):
                    one(sh[k], sr[k], co[k])
            outs.append(dict(shaped=sh, sum_r=sr, coll=co, obs=env._obs.clone() if (want_obs or one_obs) else None,
                             rew=env._rew.clone(), done=env._done.clone(), actions=a.clone(),
                             chobs=env._chobs.clone() if want_chobs else None))
        if tail_slot:
            one()                                                 # a one-slot call behind the K-slot ones
        torch.cuda.synchronize()
        sides.append(SimpleNamespace(env=env, pol=pol, outs=outs, pen=pn, last=a.clone() if tail_slot else None, start=begin))
    return sides


def compare_closed_loop(runs, *, want_obs=True, want_chobs=False, check=True):
    """The two sides of `closed_loop_twins`: every launch's outputs, the tail slot's actions and reward, the policy state,
    the exported state, the metrics, the penalty tensors and - unless the caller goes on stepping and checks behind that -
    the sticky error flags.  Returns the exported state."""
    s1, s2 = runs
    for rep, (o1, o2) in enumerate(zip(s1.outs, s2.outs)):
        for k in ("shaped", "sum_r", "coll", "rew", "done", "actions") + (("obs",) if want_obs else ()) + (("chobs",) if want_chobs else ()):
            assert_equal(o1[k], o2[k], (rep, k))
    if s1.last is not None:
        assert torch.equal(s1.last, s2.last) and torch.equal(s1.env._rew, s2.env._rew)
    assert torch.equal(s1.pol.prev_action, s2.pol.prev_action) and torch.equal(s1.pol.counter, s2.pol.counter)
    state = assert_same_envs(s1.env, s2.env, entries=False)
    if s1.pen is not None:
        assert torch.equal(s1.pen[2], s2.pen[2]) and torch.equal(s1.pen[3], s2.pen[3])
    if check:
        s1.env.check(); s2.env.check()
    return state
