"""K slots per launch at 64 < N <= 256 vehicles (step_wide_slots_kernel, k_wide_slots.hip): `diral_env_step_policy` with
DiralSlotPolicy::slots = K > 1 against K one-slot calls - at these sizes each of those is three launches (the step with the
channel observation, diral_driver_shape, diral_sps_step_chobs) - bit for bit."""
import numpy as np
import pytest
import torch

from diral_amd.config import (KERNEL_PACKED, KERNEL_POLICY, KERNEL_RICH, KERNEL_WIDE, STEP_MY_STEP_CH, ERR_UNSUPPORTED,
                              bench_config)

pytestmark = pytest.mark.gpu


def _pair(cfg, B, dt, K, t0, *, want_obs=True, want_chobs=False, keep=0.8, vary=False, vel_seed=0, clock=False, pen=False,
          x0=None, reps=2, prep=None, form=None, monkeypatch=None):
    """Runs the same slots on two envs: K one-slot calls (side 0) and one K-slot launch (side 1), `reps` times, then one
    one-slot call on both sides.  Returns the two sides' (env, policy, per-launch outputs, penalty tensors)."""
    from diral_amd.rollout import SlotClock
    from diral_amd.sps import SpsPolicy
    from diral_amd.vec_env import VecV2VEnv
    if form is not None:
        monkeypatch.setenv("DIRAL_TABLE_FORM", form)
    N, A = cfg.num_users, cfg.num_channels
    runs = []
    for fused_k in (False, True):
        env = VecV2VEnv(cfg, batch=B, device="cuda:0", out_dtype=dt)
        if x0 is not None:
            env.reset_topology(x0, None, np.full(x0.shape, 1.7))
        else:
            env.reset_topology(seed=21)
        pol = SpsPolicy(B, N, A, device="cuda:0", seed=3)
        pol.keep_prob = keep
        if prep is not None:
            prep(env, pol)
        clk = SlotClock("cuda:0", 0) if clock else None
        if clk is not None:
            env.set_clock(clk.t)
        pn = None
        if pen:
            pn = (2, -10.0, torch.zeros((B, N), dtype=torch.int32, device="cuda:0"),
                  torch.full((B, N), -1, dtype=torch.int32, device="cuda:0"))
        a = pol.prev_action.clone()
        nxt = torch.empty_like(a)
        t = 0

        def one(sh=None, sr=None, co=None):
            nonlocal a, nxt, t
            env.step_policy(a, 0 if clk is not None else t, pol, nxt, shaped_out=sh, sum_r_out=sr, collision_out=co,
                            clock=clk, seed_offset=0, want_chobs=want_chobs, want_obs=want_obs,
                            stuck_penalty=pn if sh is not None else None)
            assert env.last_kernel() & KERNEL_POLICY == 0
            if vary and t % cfg.episode_interval == cfg.episode_interval - 1:
                env.update_velocity(seed=vel_seed + t // cfg.episode_interval)
            if clk is not None:
                env.lib.diral_clock_add(clk.ptr(), 1, env._stream())
            a, nxt = nxt, a
            t += 1
        sh0 = torch.zeros((B, N), dtype=dt, device="cuda:0")
        for _ in range(t0):                                       # warm-up, one slot per call on both sides
            one(sh0 if pen else None)
        outs = []
        for rep in range(reps):
            sh = torch.zeros((K, B, N), dtype=dt, device="cuda:0")
            sr = torch.zeros((K, B), dtype=dt, device="cuda:0")
            co = torch.zeros((K, B), dtype=dt, device="cuda:0")
            if fused_k:
                env.step_policy(a, 0 if clk is not None else t, pol, nxt, shaped_out=sh, sum_r_out=sr, collision_out=co,
                                slots=K, vel_seed=vel_seed, clock=clk, seed_offset=0, want_chobs=want_chobs,
                                want_obs=want_obs, stuck_penalty=pn)
                lk = env.last_kernel()
                assert lk & (15 | KERNEL_POLICY | KERNEL_RICH) == KERNEL_WIDE | KERNEL_POLICY | KERNEL_RICH, lk
                if clk is not None:
                    env.lib.diral_clock_add(clk.ptr(), K, env._stream())
                a, nxt = nxt, a
                t += K
            else:
                for k in range(K):
                    one(sh[k], sr[k], co[k])
            outs.append(dict(shaped=sh, sum_r=sr, coll=co, obs=env._obs.clone() if want_obs else None, rew=env._rew.clone(),
                             done=env._done.clone(), actions=a.clone(), chobs=env._chobs.clone() if want_chobs else None))
        one()                                                     # a one-slot call behind the K-slot ones
        torch.cuda.synchronize()
        runs.append((env, pol, outs, pn, a.clone()))
    return runs


def _compare(runs, want_obs=True, want_chobs=False):
    (e1, p1, o1, pn1, a1), (e2, p2, o2, pn2, a2) = runs
    for rep in range(len(o1)):
        for k in ("shaped", "sum_r", "coll", "rew", "done", "actions"):
            assert torch.equal(o1[rep][k], o2[rep][k]), (rep, k, (o1[rep][k] != o2[rep][k]).nonzero()[:4])
        if want_obs:
            assert torch.equal(o1[rep]["obs"], o2[rep]["obs"]), (rep, (o1[rep]["obs"] != o2[rep]["obs"]).nonzero()[:4])
        if want_chobs:
            assert torch.equal(o1[rep]["chobs"], o2[rep]["chobs"]), rep
    assert torch.equal(a1, a2) and torch.equal(e1._rew, e2._rew)
    assert torch.equal(p1.prev_action, p2.prev_action) and torch.equal(p1.counter, p2.counter)
    sa, sb = e1.export_state(), e2.export_state()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(e1.metrics(), e2.metrics())
    if pn1 is not None:
        assert torch.equal(pn1[2], pn2[2]) and torch.equal(pn1[3], pn2[3])
    e1.check()
    e2.check()
    return sa


@pytest.mark.parametrize("N,A,form,dt,K,want_obs", [
    (65, 7, "packed", torch.float32, 6, True),
    (65, 7, "plane", torch.float64, 2, False),
    (96, 48, "plane", torch.float32, 25, True),
    (96, 48, "packed", torch.float64, 6, True),
    (128, 64, "packed", torch.float32, 25, False),
    (128, 64, "plane", torch.float64, 6, True),
    (200, 33, "packed", torch.float64, 2, True),
    (200, 33, "plane", torch.float32, 6, False),
    (250, 40, "packed", torch.float32, 6, True),      # 249 <= N <= 255: np.sum's pairwise order splits twice
    (255, 64, "plane", torch.float64, 6, False),
    (256, 64, "packed", torch.float32, 6, True),
    (256, 64, "plane", torch.float64, 25, True),
])
def test_wide_k_slots_equal_k_one_slot_calls(N, A, form, dt, K, want_obs, monkeypatch):
    """K slots in one launch at 64 < N <= 256 equal K one-slot calls (three launches each), in both table forms and both
    output dtypes: per-slot shaped rewards / sums / collisions, the last slot's state, reward, done and channel
    observation, the next actions, the policy state, the exported tables, positions, velocities and the metrics."""
    cfg = bench_config(N, A, 10.0 * N + 400, reward_design=2)
    B = 24
    runs = _pair(cfg, B, dt, K, 5, want_obs=want_obs, want_chobs=True, form=form, monkeypatch=monkeypatch)
    packed = runs[1][0].last_kernel() & KERNEL_PACKED
    assert bool(packed) == (form == "packed")
    _compare(runs, want_obs=want_obs, want_chobs=True)


@pytest.mark.parametrize("N", [128, 256])
@pytest.mark.parametrize("case", ["vary_inside", "vary_last", "rich_vel", "stuck_penalty", "prop_fair", "slot_clock",
                                  "sorted_distances"])
def test_wide_k_slots_on_the_other_code_paths_of_the_slot_loop(case, N):
    """The slot loop's other paths at N = 128 and 256: mobility_vary with an episode end inside the launch and on its last
    slot, the RICH state columns (the velocity column shows the velocities the in-launch update left), the stuck-action
    penalty, proportional fair, the device slot clock, and sorted distances launched behind the K-slot step."""
    A, B, dt, K, t0, vary, kw = 32, 16, torch.float32, 6, 21, False, {}
    if case in ("vary_inside", "vary_last", "rich_vel"):
        vary = True
        K = 4 if case == "vary_last" else 6                       # the episode ends at t = 24: inside / on the last slot
    if case == "rich_vel":
        kw = dict(State=dict(add_velocity=True, add_reward=True, add_position=True, add_index=True, add_channel_obs=True))
    elif case == "prop_fair":
        kw = dict(proportional_fair=True)
    elif case == "sorted_distances":
        kw = dict(State=dict(add_positional_dist=True))
    cfg = bench_config(N, A, 10.0 * N + 400, reward_design=2, mobility_vary=vary, **kw)
    runs = _pair(cfg, B, dt, K, t0, want_chobs=case == "rich_vel", keep=0.95 if case in ("stuck_penalty", "prop_fair") else 0.8,
                 vary=vary, vel_seed=4242, clock=case == "slot_clock", pen=case == "stuck_penalty")
    sa = _compare(runs, want_chobs=case == "rich_vel")
    if vary:
        assert not torch.equal(sa["vel"], torch.full_like(sa["vel"], 1.7))
    if case == "rich_vel":
        o = runs[1][2]
        vcol = cfg.state_space - 1                                # add_velocity: the last column
        assert not torch.equal(o[0]["obs"][:, :, vcol], torch.full_like(o[0]["obs"][:, :, vcol], 1.7))
    if case == "stuck_penalty":
        assert int(runs[1][3][2].max()) > 2


def test_wide_k_slots_when_every_agent_reselects():
    """keep_prob = 0 and every counter at 0: every agent of every env re-selects in slot 0 (and many later) - N = 256,
    A = 64, float64 - against the three-launch loop."""
    N, A = 256, 64
    cfg = bench_config(N, A, 10.0 * N + 400, reward_design=2)

    def prep(env, pol):
        pol.counter.zero_()
    runs = _pair(cfg, 8, torch.float64, 6, 0, keep=0.0, want_chobs=True, prep=prep)
    _compare(runs, want_chobs=True)


def test_wide_k_slots_on_a_highway_that_breaks_apart(monkeypatch):
    """A sparse 128-vehicle packed highway with mobility_vary, long enough that entries fall beyond the codes inside the
    K-slot launches (flagged passes, the far-entry guard): K-slot launches against the three-launch loop."""
    N, A, L, B = 128, 16, 4000.0, 6
    cfg = bench_config(N, A, L, mobility_vary=True)
    rng = np.random.default_rng(N + A)
    x0 = rng.integers(0, int(L), size=(B, N)).astype(np.float64)
    x0[0] = np.concatenate([rng.integers(0, 1200, size=N // 2), rng.integers(2400, 3600, size=N - N // 2)])
    runs = _pair(cfg, B, torch.float64, 25, 100, keep=0.9, vary=True, vel_seed=99, x0=x0, reps=8, form="packed",
                 monkeypatch=monkeypatch)
    sa = _compare(runs)
    seq = sa["seq"]
    own = torch.diagonal(seq, dim1=1, dim2=2).unsqueeze(1)
    assert bool(((own - seq >= 8) & (seq > 0)).any()), "no entry fell beyond the codes"


def _refusal_envs():
    from diral_amd.vec_env import VecV2VEnv
    cases = []
    base = dict(reward_design=2)
    cases.append(("my_step_ch", bench_config(128, 32, 1700.0, **base), dict(mode=STEP_MY_STEP_CH)))
    cases.append(("arrival_stamps", bench_config(128, 32, 1700.0, track_arrival=True, **base), {}))
    cases.append(("prr", bench_config(128, 32, 1700.0, track_prr=True, **base), {}))
    cases.append(("static", bench_config(128, 32, 1700.0, mobility=False, enable_design_topology=True, **base), {}))
    cases.append(("no_tables", bench_config(128, 32, 1700.0, State=dict(add_positional_dist_piggy=False, num_bins=0), **base), {}))
    cases.append(("off_lane", bench_config(128, 32, 1700.0, **base), {}))
    cases.append(("a_gt_64", bench_config(128, 65, 1700.0, **base), {}))
    cases.append(("large", bench_config(257, 32, 3000.0, **base), {}))
    cases.append(("piggybacking", bench_config(96, 8, 1400.0, State=dict(piggybacking=True, add_channel_obs=True), **base), {}))
    return VecV2VEnv, cases


def test_wide_k_slots_refusals_leave_the_env_untouched():
    """Configurations the K-slot kernel does not take raise DIRAL_ERR_UNSUPPORTED with nothing launched: my_step_ch, the
    run-time extras (arrival stamps, PRR tracking, a static topology, no piggybacked tables), vehicles off the y = 0 lane,
    A > 64, the large path (N > 256), State.piggybacking.  export_state() is unchanged by the refused call."""
    from diral_amd.sps import SpsPolicy
    from diral_amd.vec_env import DiralError
    VecV2VEnv, cases = _refusal_envs()
    B = 4
    for name, cfg, kw in cases:
        try:
            env = VecV2VEnv(cfg, batch=B, device="cuda:0")
        except (ValueError, DiralError) as ex:                    # (a configuration the env itself refuses is no K-slot case)
            pytest.fail("%s: %s" % (name, ex))
        N, A = cfg.num_users, cfg.num_channels
        if name == "off_lane":
            rng = np.random.default_rng(1)
            env.reset_topology(rng.integers(0, 1700, size=(B, N)).astype(np.float64), rng.uniform(0, 5, size=(B, N)),
                               np.full((B, N), 1.7))
        else:
            env.reset_topology(seed=2)
        pol = SpsPolicy(B, N, A, device="cuda:0", seed=1)
        a = pol.prev_action.clone()
        nxt = torch.empty_like(a)
        before = {k: v.clone() for k, v in env.export_state().items()}
        prev, cnt = pol.prev_action.clone(), pol.counter.clone()
        with pytest.raises(DiralError) as ei:
            env.step_policy(a, 0, pol, nxt, slots=4, **kw)
        assert ei.value.status == ERR_UNSUPPORTED, (name, str(ei.value))
        torch.cuda.synchronize()
        after = env.export_state()
        for k in before:
            assert torch.equal(before[k], after[k]), (name, k)
        assert torch.equal(pol.prev_action, prev) and torch.equal(pol.counter, cnt), name
        env.check()
