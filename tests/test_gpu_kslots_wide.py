"""K slots per launch at 64 < N <= 256 vehicles (step_wide_slots_kernel, k_wide_slots.hip): `diral_env_step_policy` with
DiralSlotPolicy::slots = K > 1 against K one-slot calls - at these sizes each of those is three launches (the step with the
channel observation, diral_driver_shape, diral_sps_step_chobs) - bit for bit."""
import numpy as np
import pytest
import torch

from diral_amd.config import (KERNEL_PACKED, KERNEL_POLICY, KERNEL_RICH, KERNEL_WIDE, STEP_MY_STEP_CH, ERR_UNSUPPORTED,
                              bench_config)
from tests.kslots_harness import closed_loop_twins, compare_closed_loop

pytestmark = pytest.mark.gpu


def _is_wide_slots_kernel(lk):
    return lk & (15 | KERNEL_POLICY | KERNEL_RICH) == KERNEL_WIDE | KERNEL_POLICY | KERNEL_RICH


def _wide_twins(cfg, B, dt, K, t0, *, x0=None, **kw):
    """tests/kslots_harness.closed_loop_twins as this file runs it: a one-slot call behind the launches, three launches
    behind every one-slot call."""
    topo = 21 if x0 is None else (x0, None, np.full(x0.shape, 1.7))
    kw.setdefault("keep", 0.8)
    return closed_loop_twins(cfg, B, dt, K, t0, topo=topo, pol_seed=3, tail_slot=True,
                             expect_one=lambda lk: lk & KERNEL_POLICY == 0, expect_fused=_is_wide_slots_kernel, **kw)


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
    monkeypatch.setenv("DIRAL_TABLE_FORM", form)
    runs = _wide_twins(cfg, B, dt, K, 5, want_obs=want_obs, want_chobs=True)
    packed = runs[1].env.last_kernel() & KERNEL_PACKED
    assert bool(packed) == (form == "packed")
    compare_closed_loop(runs, want_obs=want_obs, want_chobs=True)


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
    runs = _wide_twins(cfg, B, dt, K, t0, want_chobs=case == "rich_vel", keep=0.95 if case in ("stuck_penalty", "prop_fair") else 0.8,
                       vel_seed=4242, clock=case == "slot_clock", pen=case == "stuck_penalty")
    sa = compare_closed_loop(runs, want_chobs=case == "rich_vel")
    if vary:
        assert not torch.equal(sa["vel"], torch.full_like(sa["vel"], 1.7))
    if case == "rich_vel":
        o = runs[1].outs
        vcol = cfg.state_space - 1                                # add_velocity: the last column
        assert not torch.equal(o[0]["obs"][:, :, vcol], torch.full_like(o[0]["obs"][:, :, vcol], 1.7))
    if case == "stuck_penalty":
        assert int(runs[1].pen[2].max()) > 2


def test_wide_k_slots_when_every_agent_reselects():
    """keep_prob = 0 and every counter at 0: every agent of every env re-selects in slot 0 (and many later) - N = 256,
    A = 64, float64 - against the three-launch loop."""
    N, A = 256, 64
    cfg = bench_config(N, A, 10.0 * N + 400, reward_design=2)

    def prep(env, pol):
        pol.counter.zero_()
    runs = _wide_twins(cfg, 8, torch.float64, 6, 0, keep=0.0, want_chobs=True, prep=prep)
    compare_closed_loop(runs, want_chobs=True)


def test_wide_k_slots_on_a_highway_that_breaks_apart(monkeypatch):
    """A sparse 128-vehicle packed highway with mobility_vary, long enough that entries fall beyond the codes inside the
    K-slot launches (flagged passes, the far-entry guard): K-slot launches against the three-launch loop."""
    N, A, L, B = 128, 16, 4000.0, 6
    cfg = bench_config(N, A, L, mobility_vary=True)
    rng = np.random.default_rng(N + A)
    x0 = rng.integers(0, int(L), size=(B, N)).astype(np.float64)
    x0[0] = np.concatenate([rng.integers(0, 1200, size=N // 2), rng.integers(2400, 3600, size=N - N // 2)])
    monkeypatch.setenv("DIRAL_TABLE_FORM", "packed")
    runs = _wide_twins(cfg, B, torch.float64, 25, 100, keep=0.9, vel_seed=99, x0=x0, reps=8)
    sa = compare_closed_loop(runs)
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
