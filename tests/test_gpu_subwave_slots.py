"""K slots per launch for toy-size envs (csrc/step_subwave_slots.hpp): `rollout` and `prefill` on a handle pinned with
`use_subwave_path(slots=True)` against the loop of one-slot calls (tests/kslots_harness.py `slot_loop`) on a twin pinned
WITHOUT `slots` - states, the last reward / done, shaped / sum_r / collision of every slot, the exported state (tables,
positions, velocities, arrival stamps), the metrics with the PRR columns and the penalty state, bit for bit; afterwards
both envs take three more one-slot steps and still agree (which is where the proportional-fair counters show).

Shapes (N, A, B): (4, 3, 65) G = 4, the second block holds one env; (3, 16, 17) N < G, A at its limit, a partial wave;
(5, 3, 33) G = 8 with N < G, the second block holds one env; (8, 16, 9) G = 8 full, the pairwise np.sum branch;
(7, 2, 17) the sequential sum at its longest.

One anchor per G against the CPU oracle with the shaping in NumPy's order (tests/host_closed_loop.py) shares no code
with the device."""
import numpy as np
import pytest
import torch

from diral_amd.config import (ERR_BAD_ARG, ERR_UNSUPPORTED, KERNEL_POLICY, KERNEL_SUBWAVE, OPT_SUBWAVE_SLOTS, STEP_DESIGN,
                              STEP_MY_STEP, STEP_MY_STEP_CH, bench_config)
from tests import host_closed_loop as H
from tests.gpu_util import exported, make_env
from tests.oracle_compare import metrics_equal
from tests.kslots_harness import (RICH, VEL_SEED, as_rollout, assert_equal, assert_same, assert_same_envs, go_on_alike,
                                  slot_loop, stuck_penalty_state)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(4, 3, 65), (3, 16, 17), (5, 3, 33), (8, 16, 9), (7, 2, 17)]
KS = (1, 2, 7, 30)
FUSED = KERNEL_SUBWAVE | KERNEL_POLICY


def toy(N=4, A=3, K=20, L=300.0, Rc=120.0, **kw):
    """configs/4ue_3r_toy's shape on a highway where some pairs are out of range."""
    state = dict(num_bins=K)
    state.update(kw.pop("State", {}))
    return bench_config(N, A, L, communication_range=Rc, State=state, **kw)


def lanes(rng, B, N):
    return rng.integers(0, 2, size=(B, N)).astype(np.float64) * 1.5


def pair(cfg, B, dtype, seed, y0=False, trace=None, offset=0):
    """(the loop's handle - pinned, without `slots` -, the launches' handle - pinned with `slots`), on one topology."""
    rng = np.random.default_rng(seed)
    x0 = rng.integers(0, int(cfg.highway_length), size=(B, cfg.num_users)).astype(np.float64)
    v0 = np.full((B, cfg.num_users), 1.7) if cfg.mobility_vary else rng.uniform(1.1, 2.7, size=(B, cfg.num_users))
    yy = lanes(rng, B, cfg.num_users) if y0 else None
    envs = []
    for slots in (False, True):
        env = make_env(cfg, B, STEP_MY_STEP, dtype)
        env.use_subwave_path(slots=slots)
        if offset:
            env.set_env_offset(offset)
        env.reset_topology(x0, yy, v0)
        if trace is not None:
            env.load_saved_positions(trace)
        envs.append(env)
    return envs


def sequence(env, K, base, sticky=False):
    """[K, B, N]: a fresh draw every slot, or (`sticky`) one draw held for four slots."""
    return torch.stack([env.sample(base + (k // 4 if sticky else k)) for k in range(K)])


def run(cfg, B, dtype, plan, mode="my_step", states="last", seed=31, pen=False, sticky=False, t0=0, avg=None, y0=False, trace=None,
        clock=None, entries=True):
    """The launches of `plan` (slots per launch), each continuing the one before, against the loop on the twin; then the
    exported state, the metrics, the penalty state, three further one-slot steps and env.check()."""
    e_loop, e_one = pair(cfg, B, dtype, seed, y0=y0, trace=trace)
    if clock is not None:
        for env in (e_loop, e_one):
            env.set_clock(clock)
    pens = [stuck_penalty_state(B, cfg.num_users) if pen else None for _ in range(2)]
    t = t0
    for i, K in enumerate(plan):
        seq = sequence(e_loop, K, 7000 + 100 * i, sticky)
        g = bool(i & 1) if avg is None else avg
        want = as_rollout(slot_loop(e_loop, seq, t, mode, avg=g, pen=pens[0], want_obs=states is not None), states)
        got = e_one.rollout(seq, t, mode=mode, states=states, global_reward_avg=g, stuck_penalty=pens[1], vel_seed=VEL_SEED)
        torch.cuda.synchronize()
        assert e_one.last_kernel() == FUSED and e_loop.last_kernel() == KERNEL_SUBWAVE
        assert_same(want, got, (i, K, t))
        assert e_one.t == t + K
        t += K
    s = assert_same_envs(e_loop, e_one, entries=entries)
    if pen:
        assert torch.equal(pens[0][2], pens[1][2]) and torch.equal(pens[0][3], pens[1][3])
    if clock is not None:
        for env in (e_loop, e_one):
            env.set_clock(None)
    go_on_alike(e_loop, e_one, mode, t + (int(clock.item()) if clock is not None else 0))
    return s, pens[1], e_one


# ---- the sweep ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,rd", [("my_step", 1), ("my_step", 2), ("my_step", 3), ("my_step", 4), ("my_step", 5),
                                     ("my_step_ch", 2), ("my_step_ch", 3), ("my_step_ch", 4)])
@pytest.mark.parametrize("N,A,B", SHAPES)
def test_rollout_equals_the_loop_of_one_slot_calls(N, A, B, mode, rd):
    """K = 1, 2, 7 and 30 as four launches behind each other (t > 0 from the second on, global_reward_avg off and on in
    turn), f32 and f64, states last / all / None, the rich State flags with the fingerprint."""
    cfg = toy(N, A, reward_design=rd, enable_fingerprint=True, track_prr=(rd % 2 == 0), State=RICH)
    for dtype in (torch.float32, torch.float64):
        for states in ("last", "all", None):
            run(cfg, B, dtype, KS, mode, states, seed=100 * N + rd)


@pytest.mark.parametrize("N,A,B", SHAPES)
def test_the_plain_toy_state_vector(N, A, B):
    """[one-hot(action) | type-2 histogram], the toy YAML's State flags."""
    for states in ("last", "all"):
        run(toy(N, A), B, torch.float32, (7, 2), "my_step", states, seed=40 + N)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("N,A,B", SHAPES)
def test_stuck_penalty_on_a_held_sequence(N, A, B, dtype):
    """Actions held for four slots at a time with A resources for N vehicles: collisions repeat and the counters pass the
    threshold (PEN_THR = 2)."""
    cfg = toy(N, min(A, 3), reward_design=2, State=dict(add_reward=True))
    _, pn, _ = run(cfg, B, dtype, (7, 30), "my_step", "last", seed=50 + N, pen=True, sticky=True, avg=True)
    assert int(pn[2].max()) > 2                                      # the penalty branch ran


@pytest.mark.parametrize("N,A,B", SHAPES)
def test_episode_ends_inside_the_launch_on_its_last_slot_and_as_its_only_slot(N, A, B):
    """mobility_vary with an episode of five slots: K = 5 ends one on its last slot, K = 7 (t = 5 ... 11) inside, K = 2
    none, K = 1 at t = 14 as its only slot; the velocity column is the velocity the slot ran with."""
    cfg = toy(N, A, mobility_vary=True, episode_interval=5, reward_design=1, State=RICH)
    for dtype, states in ((torch.float64, "all"), (torch.float32, "last")):
        s, _, _ = run(cfg, B, dtype, (5, 7, 2, 1), "my_step", states, seed=60 + N)
        assert float(s["vel"].min()) < 1.7 or float(s["vel"].max()) > 1.7      # velocities did change


@pytest.mark.parametrize("N,A,B", [(4, 3, 65), (8, 16, 9)])
def test_slot_clock_and_arrival_stamps(N, A, B):
    """A device slot clock of 3 on a `track_arrival` handle: `done`, the my_step_ch stamps and my_step's -1 follow
    t + ks + clock."""
    clock = torch.full((1,), 3, dtype=torch.int64, device=DEV)
    for mode in ("my_step_ch", "my_step"):
        cfg = toy(N, A, reward_design=2, track_arrival=True, episode_interval=4, State=dict(add_channel_obs=True))
        s, _, _ = run(cfg, B, torch.float64, (7, 2), mode, "last", seed=70 + N, clock=clock)
        assert "la" in s and int(s["la"].max()) == (3 + 8 if mode == "my_step_ch" else -1)


@pytest.mark.parametrize("N,A,B", SHAPES)
def test_track_arrival_handles(N, A, B):
    for mode in ("my_step", "my_step_ch"):
        cfg = toy(N, A, reward_design=3, track_arrival=True, State=dict(add_channel_obs=True, add_reward=True))
        s, _, _ = run(cfg, B, torch.float32, (1, 30), mode, "all", seed=80 + N)
        assert "la" in s


@pytest.mark.parametrize("N,A,B", [(4, 3, 65), (7, 2, 17), (8, 16, 9)])
def test_proportional_fairness_with_sticky_actions(N, A, B):
    """Held actions take the pf counters over the threshold inside a launch; the further steps behind it (held actions
    again) read the counters the launch wrote back."""
    cfg = toy(N, A, reward_design=1, proportional_fair=True, State=dict(add_reward=True))
    e_loop, e_one = pair(cfg, B, torch.float64, 90 + N)
    t = 0
    for K in (2, 30):
        seq = e_loop.sample(55).unsqueeze(0).expand(K, B, N).contiguous()
        want = as_rollout(slot_loop(e_loop, seq, t, "my_step", avg=False), "all")
        got = e_one.rollout(seq, t, states="all", vel_seed=VEL_SEED)
        assert_same(want, got, K)
        t += K
    if A < N:                                                        # (somebody always collides: test_env.py:89-90)
        assert bool((got["reward"] == -10.0).any())                  # pf_penalty was paid
    assert_same_envs(e_loop, e_one)
    for k in range(3):
        a = e_loop.sample(55)
        r1 = e_loop._step(STEP_MY_STEP, a, t + k)[1].clone()
        r2 = e_one._step(STEP_MY_STEP, a, t + k)[1].clone()
        assert torch.equal(r1, r2)
    e_loop.check(); e_one.check()


@pytest.mark.parametrize("per_env", [False, True])
@pytest.mark.parametrize("N,A,B", [(4, 3, 65), (5, 3, 33)])
def test_a_handle_with_a_trace_shorter_than_the_launch(N, A, B, per_env):
    """load_saved_positions with T = 5 rows, [T, N] and [B, T, N]: row (t + ks) mod T, wrapping inside a launch of 7."""
    rng = np.random.default_rng(110 + N)
    trace = rng.uniform(0, 300, size=(B, 5, N) if per_env else (5, N))
    cfg = toy(N, A, State=dict(add_position=True, add_channel_obs=True))
    run(cfg, B, torch.float64, (7, 2, 30), "my_step", "all", seed=111, trace=trace)


@pytest.mark.parametrize("N,A,B", SHAPES)
def test_off_lane_vehicles_a_static_topology_and_a_handle_without_tables(N, A, B):
    run(toy(N, A, reward_design=5, State=dict(add_position=True)), B, torch.float64, (7, 2), "my_step", "all", seed=120 + N, y0=True)
    run(toy(N, A, mobility=False, enable_design_topology=True, State=dict(add_position=True)), B, torch.float32, (7, 2),
        "my_step_ch", "last", seed=130 + N)
    run(toy(N, A, State=dict(add_positional_dist_piggy=False, add_channel_obs=True)), B, torch.float64, (7, 2), "my_step", "all",
        seed=140 + N, entries=False)


@pytest.mark.parametrize("N,A,B", [(4, 3, 65), (8, 16, 9)])
def test_f32_outputs_are_the_cast_of_the_f64_ones(N, A, B):
    """Rewards and states (not the shaped sums, which are summed in the output dtype)."""
    cfg = toy(N, A, reward_design=2, State=RICH)
    outs = []
    for dtype in (torch.float32, torch.float64):
        _, env = pair(cfg, B, dtype, 150)
        seq = sequence(env, 7, 7100)
        outs.append(env.rollout(seq, 0, states="all"))
    assert torch.equal(outs[0]["states"], outs[1]["states"].to(torch.float32))
    assert torch.equal(outs[0]["reward"], outs[1]["reward"].to(torch.float32))
    assert torch.equal(outs[0]["done"], outs[1]["done"])


# ---- the oracle anchor ----------------------------------------------------------------------------------------------------

class _Given:
    """Stands where HostSps stands in HostClosedLoop: nothing is decided, the caller hands every slot its actions."""
    log = ()

    def step(self, chobs=None, actions=None, seed=None):
        return np.asarray(actions).copy()


@pytest.mark.parametrize("N,A,B", [(4, 3, 65), (8, 16, 9)])
def test_rollout_against_the_host_loop(N, A, B):
    """One rollout per lane-group width against the CPU oracle step + the driver's shaping in NumPy's order + the velocity
    mirror: everything bit for bit (reward_design 2: no exp), the metric float sums at rtol 1e-12."""
    cfg = toy(N, A, reward_design=2, mobility_vary=True, episode_interval=5, State=RICH)
    x0, v0 = H.draw_topology(5, B, N, cfg.highway_length, True)
    host = H.HostClosedLoop(cfg, B, x0, v0, _Given(), 0, mode="my_step", dtype=np.float64, stuck_penalty=(2, -10.0), vel_seed=VEL_SEED)
    env = make_env(cfg, B, STEP_MY_STEP, torch.float64)
    env.use_subwave_path(slots=True)
    env.reset_topology(seed=5)
    pn = stuck_penalty_state(B, N)
    keep = np.ones(B, bool)
    t = 0
    for K in (6, 25):
        seq = np.stack([H.draw_sample(9000 + (t + k) // 3, B, N, A) for k in range(K)])
        outs = [host.slot(seq[k], t + k, 0) for k in range(K)]
        got = env.rollout(torch.as_tensor(seq, device=DEV), t, states="all", global_reward_avg=True, stuck_penalty=pn, vel_seed=VEL_SEED)
        torch.cuda.synchronize()
        assert env.last_kernel() == FUSED
        for k, o in enumerate(outs):
            H._eq("shaped %d" % k, got["shaped"][k], o["shaped"], keep)
            H._eq("sum_r %d" % k, got["sum_r"][k], o["sum_r"], keep)
            H._eq("collision %d" % k, got["collision"][k], o["coll"], keep)
            H._eq("state %d" % k, got["states"][k], o["state"], keep)
        H._eq("reward", got["reward"], outs[-1]["rew"], keep)
        H._eq("done", got["done"], outs[-1]["done"], keep)
        H._eq("penalty counter", pn[2], host.pen_counter, keep)
        H._eq("penalty prev_actions", pn[3], host.pen_prev, keep)
        t += K
    assert host.vel_updates > 0
    st, he = env.export_state(), host.export_state()
    for k in ("pos_x", "vel", "seq", "age", "x"):
        H._eq("export_state " + k, st[k], he[k], keep)
    m, hm = env.metrics().cpu().numpy(), host.metrics()
    metrics_equal(m, hm, "metrics")
    assert float(m[:, 0].min()) == t
    env.check()


# ---- the prefill ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_rew", [True, False])
@pytest.mark.parametrize("K", [1, 5, 30])
@pytest.mark.parametrize("mode", ["my_step_design", "my_step_ch"])
@pytest.mark.parametrize("N,A,B", [(4, 3, 65), (8, 16, 9)])
def test_prefill_equals_the_loop_of_sample_step_observe(N, A, B, mode, K, with_rew):
    """sample(seed + k) + my_step_design / my_step_ch at t = 0 + obtain_state with the stale reward column (or the slot's
    own), with env_offset > 0 so that the draws use global indices."""
    cfg = toy(N, A, reward_design=2, enable_fingerprint=True, State=RICH)
    step_mode = STEP_DESIGN if mode == "my_step_design" else STEP_MY_STEP_CH
    for dtype in (torch.float32, torch.float64):
        e_loop, e_one = pair(cfg, B, dtype, 160 + N, offset=1000)
        a0 = e_loop.sample(123)
        rews0 = None
        for env in (e_loop, e_one):
            _, rew, _ = env._step(STEP_MY_STEP, a0, 0)               # the bootstrap step: `rews` of main_test.py:92
            rews0 = rew.to(torch.float64).clone()
        seed = 77001
        want_s, want_a = [], []
        for k in range(K):
            a = e_loop.sample(seed + k)
            want_a.append(a.clone())
            _, rew, _ = e_loop._step(step_mode, a, 0, want_chobs=True, want_obs=False)
            want_s.append(e_loop.obtain_state(e_loop._chobs, a, rews0 if with_rew else rew).clone())
        states, acts, nxt = e_one.prefill(e_one.sample(seed), K, seed, rew_in=rews0 if with_rew else None, mode=mode)
        torch.cuda.synchronize()
        assert e_one.last_kernel() == FUSED
        assert_equal(torch.stack(want_a), acts, "actions_all")
        assert_equal(e_loop.sample(seed + K), nxt, "next actions")
        assert_equal(torch.stack(want_s), states, "states")
        assert_same_envs(e_loop, e_one)
        go_on_alike(e_loop, e_one, "my_step", 0)


# ---- CandidateSearch, graph capture -----------------------------------------------------------------------------------------

def test_candidate_search_on_a_toy_env_equals_the_search_that_loops():
    from diral_amd.search import CandidateSearch
    B, C, K = 5, 4, 6
    cfg = toy(4, 3, reward_design=2)
    e_loop, e_one = pair(cfg, B, torch.float64, 170)
    searches = []
    rng = np.random.default_rng(171)
    seqs = torch.as_tensor(rng.integers(0, 3, size=(K, B, C, 4)).astype(np.int32), device=DEV)
    res = []
    for env in (e_loop, e_one):
        cs = CandidateSearch(env, C)
        searches.append(cs)
        r = cs.evaluate(seqs, 0, global_reward_avg=True)
        cs.commit(r["returns"].argmax(1))
        res.append(r)
    torch.cuda.synchronize()
    assert searches[1].work.last_kernel() == FUSED and searches[0].work.last_kernel() == KERNEL_SUBWAVE
    for key in res[0]:
        assert_equal(res[0][key], res[1][key], key)
    assert e_loop.t == e_one.t == K
    assert_same_envs(e_loop, e_one)
    go_on_alike(e_loop, e_one, "my_step", K)


def test_driver_loop_picks_the_launch_up_through_the_env():
    """DriverLoop.prefill / DriverLoop.rollout: one launch on the handle with `slots`, the loop of slots on the twin."""
    from diral_amd.driver import DriverLoop
    N, A, B, K = 4, 3, 17, 6
    cfg = toy(N, A, reward_design=2, mobility_vary=True, episode_interval=4, State=RICH)
    e_loop, e_one = pair(cfg, B, torch.float64, 175)
    loops = [DriverLoop(e, global_reward_avg=True, episode_interval=4) for e in (e_loop, e_one)]
    a0 = e_loop.sample(1)
    res = []
    for lp, env in zip(loops, (e_loop, e_one)):
        lp.bootstrap(a0)
        states, acts = lp.prefill(K, 4400)
        fused_prefill = bool(env.last_kernel() & KERNEL_POLICY)
        seq = sequence(env, K, 7400)
        out = lp.rollout(seq, 0, states="all", vel_seed=VEL_SEED)
        res.append((states.clone(), acts.clone(), {k: v.clone() for k, v in out.items() if v is not None}, fused_prefill,
                    bool(env.last_kernel() & KERNEL_POLICY)))
    assert res[0][3:] == (False, False) and res[1][3:] == (True, True)
    assert_equal(res[0][0], res[1][0], "prefill states")
    assert_equal(res[0][1], res[1][1], "prefill actions")
    for key in ("states", "reward", "done", "shaped", "sum_r", "collision"):
        assert_equal(res[0][2][key], res[1][2][key], key)
    assert_same_envs(e_loop, e_one)


def test_one_captured_rollout_replayed_twice_with_a_slot_clock_equals_the_eager_run():
    """The launch is enqueue-only: a rollout of K = 4 (my_step_ch on a tracking handle: stamps and `done` read the slot
    number on the device) captured once and replayed twice with a clock that moves on by four = eight eager slots."""
    from diral_amd.rollout import SlotClock, no_finalizers_during_capture
    N, A, B, K = 4, 3, 33, 4
    cfg = toy(N, A, reward_design=3, track_arrival=True, episode_interval=3, State=dict(add_channel_obs=True))
    eager, graphed = pair(cfg, B, torch.float32, 180)
    eager.use_subwave_path(slots=True)
    seq = sequence(eager, K, 7200)
    for e in (eager, graphed):
        e.rollout(seq[:1], 0, mode="my_step_ch")                     # (slot 0 outside the capture: the output buffers exist)
    outs_e = []
    for rep in range(2):
        o = eager.rollout(seq, 1 + K * rep, mode="my_step_ch", global_reward_avg=True)
        outs_e.append({k: None if v is None else v.clone() for k, v in o.items()})
    clock = SlotClock(DEV, 1)
    graphed.set_clock(clock.t)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with no_finalizers_during_capture(), torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out_g = graphed.rollout(seq, 0, mode="my_step_ch", global_reward_avg=True)
            graphed.lib.diral_clock_add(clock.ptr(), K, graphed._stream())
    for rep in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert graphed.last_kernel() == FUSED
        assert_same(outs_e[rep], out_g, rep)
    assert clock.value() == 1 + 2 * K
    graphed.set_clock(None)
    a, b = exported(eager), exported(graphed)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert torch.equal(eager.metrics(), graphed.metrics())
    eager.check(); graphed.check()


# ---- refusals, the option -----------------------------------------------------------------------------------------------------

def test_what_the_slot_loop_does_not_take_is_refused_with_the_env_untouched():
    from diral_amd.sps import SpsPolicy
    from diral_amd.vec_env import DiralError
    N, A, B = 4, 3, 17
    cfg = toy(N, A, reward_design=2, track_arrival=True)
    _, env = pair(cfg, B, torch.float64, 190)
    pol = SpsPolicy(B, N, A, device=DEV, seed=11)
    seq = sequence(env, 4, 7300)
    env.rollout(seq, 0, mode="my_step_ch")
    assert env.last_kernel() == FUSED
    before = exported(env)
    nxt = torch.empty((B, N), dtype=torch.int32, device=DEV)
    calls = [lambda: env.step_policy(seq[0].contiguous(), 4, pol, nxt, slots=4),
             lambda: env.rollout(seq, 4, mode="my_step_ch", info_age=True),
             lambda: env.rollout(seq, 4, log_positions=True),
             lambda: env.prefill(seq[0], 4, seed=5),                  # (a tracking handle)
             lambda: env.prefill(seq[0], 4, seed=5, mode="my_step_ch")]
    for i, call in enumerate(calls):
        with pytest.raises(DiralError) as ei:
            call()
        assert ei.value.status == ERR_UNSUPPORTED, i
        torch.cuda.synchronize()
        after = exported(env)
        for k in before:
            assert np.array_equal(before[k], after[k]), (i, k)
    assert env.last_kernel() == FUSED                                # (nothing was launched)
    # a state vector with a secondary observation mode
    for state in (dict(add_positional_dist=True), dict(add_positional_dist_type=1, num_bins=12)):
        _, e2 = pair(toy(N, A, State=state), B, torch.float64, 191)
        with pytest.raises(DiralError) as ei:
            e2.rollout(sequence(e2, 2, 1), 0)
        assert ei.value.status == ERR_UNSUPPORTED
        e2.rollout(sequence(e2, 2, 1), 0, states=None)                # (without a state vector the loop runs)
        assert e2.last_kernel() == FUSED


def test_the_option_needs_the_pin_and_leaves_with_it():
    from diral_amd.vec_env import DiralError
    N, A, B = 4, 3, 9
    cfg = toy(N, A)
    env = make_env(cfg, B)
    env.reset_topology(seed=3)
    opt = lambda v: env.lib.diral_env_set_option(env._h, OPT_SUBWAVE_SLOTS, v)
    assert opt(1) == ERR_UNSUPPORTED and opt(0) == 0                 # an unpinned handle
    assert opt(2) == ERR_BAD_ARG and opt(-1) == ERR_BAD_ARG
    env.use_subwave_path(slots=True)
    assert opt(2) == ERR_BAD_ARG
    seq = sequence(env, 3, 1)
    env.rollout(seq, 0)
    assert env.last_kernel() == FUSED
    env.use_subwave_path(False)                                      # leaving the path clears the option ...
    env.use_subwave_path()                                           # ... so a plain pin refuses again
    with pytest.raises(DiralError) as ei:
        env.rollout(seq, 3)
    assert ei.value.status == ERR_UNSUPPORTED
    assert opt(1) == 0
    env.rollout(seq, 3)
    assert env.last_kernel() == FUSED
    env.use_subwave_path(slots=True)
    tw = env.twin()
    tw.reset_topology(seed=3)
    tw.rollout(seq, 0)
    assert tw.last_kernel() == FUSED
