"""An open-loop rollout - K slots of a GIVEN action sequence - as ONE launch (`diral_env_rollout`: the slot loops of
step_fast64_slots_kernel / step_wide_slots_kernel with the actions read from `actions_seq`) against the loop it stands
for: K `diral_env_step` calls, each followed by `diral_driver_shape` and, at an episode end, `diral_env_update_velocity` -
states, rewards, shaped rewards, sums, collisions, done, tables, ring, positions, velocities, metrics, penalty state: bit
for bit."""
import numpy as np
import pytest
import torch

from diral_amd.config import (ERR_BAD_ARG, ERR_BAD_CONFIG, ERR_UNSUPPORTED, KERNEL_PACKED, KERNEL_POLICY, KERNEL_WIDE,
                              STEP_MY_STEP, STEP_MY_STEP_CH, bench_config, c2_config)
from diral_amd.driver import DriverLoop
from diral_amd.vec_env import DiralError, VecV2VEnv
from tests.kslots_harness import RICH, VEL_SEED, check_rollout, start, twins

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype,K,mode,rd,states", [
    (torch.float32, 1, "my_step", 2, "last"),
    (torch.float64, 1, "my_step", 2, "all"),
    (torch.float32, 5, "my_step", 2, "all"),
    (torch.float64, 6, "my_step", 2, "last"),
    (torch.float32, 25, "my_step", 2, None),
    (torch.float64, 30, "my_step", 2, "all"),
    (torch.float32, 30, "my_step", 1, "last"),
    (torch.float64, 1, "my_step_ch", 2, "last"),
    (torch.float32, 5, "my_step_ch", 2, "all"),
    (torch.float64, 6, "my_step_ch", 3, "all"),
    (torch.float32, 25, "my_step_ch", 4, "last"),
    (torch.float64, 30, "my_step_ch", 3, None),
    (torch.float32, 6, "my_step_ch", 4, "all"),
])
def test_rollout_in_one_launch_equals_the_loop_of_one_slot_calls(dtype, K, mode, rd, states):
    """C2 in both dtypes, K = 1 ... 30, my_step and my_step_ch (reward_design 2, 3, 4), states last / all / none, from t = 3,
    a second launch continuing the first."""
    check_rollout(c2_config(reward_design=rd), 24, dtype, K, mode=mode, states=states, t0=3)


@pytest.mark.parametrize("mode", ["my_step", "my_step_ch"])
@pytest.mark.parametrize("states", ["last", "all"])
def test_rollout_with_the_rich_state_columns_and_the_fingerprint(mode, states):
    check_rollout(c2_config(State=RICH, enable_fingerprint=True), 16, torch.float64, 6, mode=mode, states=states)
    check_rollout(c2_config(State=RICH, enable_fingerprint=True), 16, torch.float32, 5, mode=mode, states=states, avg=False)


@pytest.mark.parametrize("mode", ["my_step", "my_step_ch"])
@pytest.mark.parametrize("t0,K", [(20, 6), (20, 5), (24, 1), (0, 30)])
def test_rollout_updates_the_velocities_at_episode_ends_inside_the_launch(mode, t0, K):
    """mobility_vary, episode_interval 25: an episode end inside the launch (t = 24 of 20 ... 25), on its last slot, as the
    only slot, and one inside a launch of 30; the second launch of each case runs behind the update.  The velocity column of
    every slot's state vector shows the velocities that slot started with."""
    cfg = bench_config(40, 12, 900.0, State=RICH, mobility_vary=True)
    assert cfg.episode_interval == 25
    s, _, _ = check_rollout(cfg, 16, torch.float32, K, mode=mode, states="all", t0=t0)
    assert not torch.equal(s["vel"], torch.full_like(s["vel"], 1.7))


@pytest.mark.parametrize("mode", ["my_step", "my_step_ch"])
def test_rollout_on_a_sparse_highway_takes_the_keyed_quads(mode):
    cfg = bench_config(64, 8, 9000.0, communication_range=100.0)
    s, _, _ = check_rollout(cfg, 24, torch.float32, 25, mode=mode, states="all", warm=12)
    own = torch.diagonal(s["seq"], dim1=1, dim2=2).unsqueeze(1)
    assert bool(((own - s["seq"] >= 8) & (s["seq"] > 0)).any()), "no entry fell beyond the codes"


@pytest.mark.parametrize("N,A", [(8, 3), (33, 7)])
@pytest.mark.parametrize("mode", ["my_step", "my_step_ch"])
def test_rollout_with_few_vehicles(N, A, mode):
    check_rollout(bench_config(N, A, 30.0 * N + 200), 24, torch.float64, 6, mode=mode, states="all")
    check_rollout(bench_config(N, A, 30.0 * N + 200, State=RICH), 24, torch.float32, 25, mode=mode, states="last")


@pytest.mark.parametrize("mode,avg", [("my_step", True), ("my_step", False), ("my_step_ch", True)])
def test_rollout_stuck_action_penalty_fires_on_a_constant_sequence(mode, avg):
    _, pen, _ = check_rollout(c2_config(), 24, torch.float64, 6, mode=mode, states="last", avg=avg, pen=True, constant=True)
    assert int(pen[2].max()) > 2                                      # beyond the threshold: the penalty was paid


def test_rollout_without_shaping_flags_returns_the_reward_of_every_slot():
    """shape_flags = 0: shaped[k] is the reward as step k returns it, and a [K, N] sequence is every env's."""
    cfg = c2_config()
    e_loop, e_one = twins(cfg, 8, torch.float32, start(cfg, 8, 3))
    seq = torch.stack([e_loop.sample(40 + k)[0] for k in range(5)])           # [K, N]
    got = e_one.rollout(seq, 0)
    for k in range(5):
        _, rew, _ = e_loop.step(seq[k], k)
        assert torch.equal(got["shaped"][k], rew)
    assert torch.equal(got["reward"], rew)


@pytest.mark.parametrize("N,A,form,dtype,K,states", [
    (128, 64, "packed", torch.float32, 25, "last"),
    (128, 64, "plane", torch.float64, 6, None),
    (256, 64, "packed", torch.float64, 5, "last"),
    (256, 64, "plane", torch.float32, 30, "last"),
    (256, 64, "packed", torch.float32, 1, "last"),
    (96, 48, "plane", torch.float32, 6, "last"),
])
def test_wide_rollout_equals_the_loop(N, A, form, dtype, K, states, monkeypatch):
    """64 < N <= 256, my_step, both table forms: step_wide_slots_kernel with the actions of every slot from the sequence."""
    monkeypatch.setenv("DIRAL_TABLE_FORM", form)
    cfg = bench_config(N, A, 10.0 * N + 400, reward_design=2, State=dict(add_reward=True, add_velocity=True), mobility_vary=True)
    _, _, env = check_rollout(cfg, 12, dtype, K, states=states, t0=20, family=KERNEL_WIDE, pen=(K == 6))
    assert bool(env.last_kernel() & KERNEL_PACKED) == (form == "packed")


def test_wide_rollout_on_a_highway_that_breaks_apart(monkeypatch):
    """The sparse 128-vehicle packed highway of test_gpu_kslots_wide.py: entries fall beyond the codes inside the launches."""
    monkeypatch.setenv("DIRAL_TABLE_FORM", "packed")
    N, A, L, B = 128, 16, 4000.0, 6
    cfg = bench_config(N, A, L, mobility_vary=True)
    rng = np.random.default_rng(N + A)
    x0 = rng.integers(0, int(L), size=(B, N)).astype(np.float64)
    x0[0] = np.concatenate([rng.integers(0, 1200, size=N // 2), rng.integers(2400, 3600, size=N - N // 2)])
    s, _, _ = check_rollout(cfg, B, torch.float64, 25, states="last", warm=100, x0=x0, reps=8, family=KERNEL_WIDE)
    own = torch.diagonal(s["seq"], dim1=1, dim2=2).unsqueeze(1)
    assert bool(((own - s["seq"] >= 8) & (s["seq"] > 0)).any()), "no entry fell beyond the codes"


# ---- refusals: one case per row of the list in include/diral_env.h -------------------------------------------------
def _refusals():
    b = dict(reward_design=2)
    return [
        ("n_lt_8", bench_config(7, 3, 400.0, **b), {}),
        ("my_step_ch_wide", bench_config(128, 32, 1700.0, **b), dict(mode="my_step_ch")),
        ("states_all_wide", bench_config(128, 32, 1700.0, **b), dict(states="all")),
        ("large", bench_config(257, 32, 3000.0, **b), {}),
        ("a_gt_64", bench_config(64, 65, 2000.0, **b), {}),
        ("off_lane", bench_config(128, 32, 1700.0, **b), {}),
        ("off_lane_64", c2_config(), {}),
        ("arrival_stamps", c2_config(track_arrival=True), {}),
        ("prr", c2_config(track_prr=True), {}),
        ("trace_replay", c2_config(), {}),
        ("static", c2_config(mobility=False, enable_design_topology=True), {}),
        ("no_tables", c2_config(State=dict(add_positional_dist_piggy=False, num_bins=0)), {}),
        ("sorted_distances", c2_config(State=dict(add_positional_dist=True)), {}),
        ("type1_histogram", c2_config(State=dict(add_positional_dist_type=1)), {}),
        ("piggybacking", bench_config(32, 8, 1400.0, State=dict(piggybacking=True, add_channel_obs=True), **b), {}),
    ]


@pytest.mark.parametrize("name,cfg,kw", _refusals(), ids=[r[0] for r in _refusals()])
def test_rollout_refusals_leave_the_env_untouched_and_the_driver_loops(name, cfg, kw):
    """Configurations the slot loops do not take raise DIRAL_ERR_UNSUPPORTED with nothing launched - export_state(), the
    metrics and the env's slot counter are unchanged - and DriverLoop.rollout then returns the loop's result."""
    B, K = 4, 4
    N = cfg.num_users
    envs = []
    for _ in range(2):
        env = VecV2VEnv(cfg, batch=B, device="cuda:0")
        if name.startswith("off_lane"):
            rng = np.random.default_rng(1)
            env.reset_topology(rng.integers(0, 1700, size=(B, N)).astype(np.float64), rng.uniform(0, 5, size=(B, N)),
                               np.full((B, N), 1.7))
        else:
            env.reset_topology(seed=2)
        if name == "trace_replay":
            rng = np.random.default_rng(2)
            env.load_saved_positions(rng.uniform(0, cfg.highway_length, size=(10, N)))
        envs.append(env)
    e1, e2 = envs
    if name == "piggybacking":
        # (a receiver out of every transmitter's range is the reference's KeyError: everybody close together)
        for env in envs:
            env.reset_topology(np.arange(N, dtype=np.float64)[None].repeat(B, 0) * 3.0, 0.0, np.full((B, N), 1.7))
    seq = torch.stack([e1.sample(60 + k) for k in range(K)])
    before = {k: v.clone() for k, v in e2.export_state().items()}
    m0 = e2.metrics().clone()
    with pytest.raises(DiralError) as ei:
        e2.rollout(seq, 0, **kw)
    assert ei.value.status == ERR_UNSUPPORTED, (name, str(ei.value))
    torch.cuda.synchronize()
    after = e2.export_state()
    for k in before:
        assert torch.equal(before[k], after[k]), (name, k)
    assert torch.equal(m0, e2.metrics()) and e2.t == 0
    # DriverLoop.rollout: the loop of slot() calls, the same layout
    ch = kw.get("mode") == "my_step_ch"
    l1, l2 = (DriverLoop(e, enable_channel=ch, global_reward_avg=True) for e in (e1, e2))
    every = kw.get("states") == "all"
    got = l2.rollout(seq, 0, states="all" if every else "last", vel_seed=VEL_SEED)
    assert not (e2.last_kernel() & KERNEL_POLICY)
    for k in range(K):
        out = l1.slot(seq[k], k)
        assert torch.equal(got["shaped"][k], out["reward"]) and torch.equal(got["sum_r"][k], out["sum_r"])
        assert torch.equal(got["collision"][k], out["collision"])
        if every:
            assert torch.equal(got["states"][k], out["next_state"]), k
    assert every or torch.equal(got["states"], out["next_state"])
    assert torch.equal(got["reward"], out["raw_reward"])
    assert got["done"].tolist() == [0] * B
    s1, s2 = e1.export_state(), e2.export_state()
    for k in s1:
        assert torch.equal(s1[k], s2[k]), (name, k)
    e1.check(); e2.check()


def test_driver_loop_rollout_takes_the_launch_where_it_can():
    """DriverLoop.rollout on C2: the launch (KERNEL_POLICY), equal to the loop of slot() calls with the velocity updates at
    the episode ends - shaped rewards with the stuck-action penalty and the global average, every slot's state vector with
    the loop's fingerprint columns."""
    cfg = c2_config(State=RICH, enable_fingerprint=True, mobility_vary=True)
    e1, e2 = twins(cfg, 8, torch.float64, start(cfg, 8, 11))
    kw = dict(global_reward_avg=True, ia_penalty_enable=True, ia_penalty_threshold=1, ia_penalty_value=-7.0)
    l1, l2 = DriverLoop(e1, **kw), DriverLoop(e2, **kw)
    K, t0 = 8, 20
    seq = e1.sample(5).unsqueeze(0).expand(K, 8, cfg.num_users).contiguous()
    got = l2.rollout(seq, t0, states="all", vel_seed=VEL_SEED)
    assert e2.last_kernel() & KERNEL_POLICY
    for k in range(K):
        out = l1.slot(seq[k], t0 + k)
        assert torch.equal(got["shaped"][k], out["reward"]), k
        assert torch.equal(got["sum_r"][k], out["sum_r"]) and torch.equal(got["collision"][k], out["collision"])
        assert torch.equal(got["states"][k], out["next_state"]), k
        if out["episode_end"]:
            e1.update_velocity(seed=VEL_SEED + (t0 + k) // 25)
    assert torch.equal(got["reward"], out["raw_reward"])
    assert torch.equal(l1._pen_counter, l2._pen_counter) and int(l2._pen_counter.max()) > 1
    s1, s2 = e1.export_state(), e2.export_state()
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k


def test_rollout_argument_checks():
    import ctypes
    from diral_amd.config import DiralRollout
    env = VecV2VEnv(c2_config(reward_design=1), batch=2, device="cuda:0")
    env.reset_topology(seed=1)
    seq = torch.stack([env.sample(k) for k in range(3)])
    out = torch.empty((3, 2, 64), dtype=torch.float32, device="cuda:0")
    rew = torch.empty((2, 64), dtype=torch.float32, device="cuda:0")
    ro = DiralRollout()
    ro.struct_bytes = ctypes.sizeof(DiralRollout)

    def call(h=env._h, a=seq.data_ptr(), K=3, r=ro, rw=rew.data_ptr(), mode=STEP_MY_STEP):
        return env.lib.diral_env_rollout(h, mode, a, K, 0, None, 0, rw, None, 0, None if r is None else ctypes.byref(r), None)
    assert call(a=None) == ERR_BAD_ARG and call(r=None) == ERR_BAD_ARG and call(K=0) == ERR_BAD_ARG
    assert call(mode=STEP_MY_STEP_CH) == ERR_BAD_CONFIG                       # reward_design 1
    ro.struct_bytes -= 8
    assert call() == ERR_BAD_ARG
    ro.struct_bytes += 8
    ro.shape_flags = 2                                                        # the information-age term: not here
    assert call() == ERR_BAD_ARG
    ro.shape_flags = 4
    ro.shaped_out = out.data_ptr()
    assert call() == ERR_BAD_ARG                                              # the penalty without its buffers
    ro.shape_flags = 0
    assert call(rw=None) == ERR_BAD_ARG                                       # a shaped output without rew_out
    assert call() == 0
    torch.cuda.synchronize()
    assert float(env.metrics()[:, 0].sum()) == 6.0                            # only the last call ran: 3 slots, 2 envs
    env.check()
