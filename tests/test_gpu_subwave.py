"""GPU parity of the sub-wave step kernel (csrc/step_subwave.hpp): toy-size envs, 4 or 8 lanes per env, on handles
pinned with `use_subwave_path()`.  The bars are the parity tests' own - bit-exact against the oracle (exp() rewards
within the exp() bar), DIST_ULP against the reference's fixtures - and after every test the handles it made say
KERNEL_SUBWAVE behind a step:
  * every reference fixture the path takes, selected by its config;
  * random runs at the sizes where the grouping can go wrong: N on and around 4 and 8, B on and around a group, a wave
    and a block for both group widths, every step kind, reward design, State flag and mobility form;
  * path switches on one handle, env copies between pinned and AUTO handles, snapshot / restore;
  * imported tables with entries of every lag class, and the 24-bit horizon;
  * histogram bin edges with the viewers at 0, L / 2 and one step below L;
  * refusals, the err flags, float32 outputs, graph capture with a slot clock."""
import math

import numpy as np
import pytest
import torch

import tests.gpu_util as gu
from diral_amd.config import (ERR_ACTION_RANGE, ERR_BAD_ARG, ERR_UNSUPPORTED, KERNEL_FAST64, KERNEL_GENERAL, KERNEL_OBSERVE,
                              KERNEL_SUBWAVE, MAX_SLOTS, OPT_KERNEL_PATH, STEP_DESIGN, STEP_MY_STEP, STEP_MY_STEP_CH, bench_config)
from tests import hist_edge_cases as H
from tests.golden_util import Golden, golden_names, horizon_tables
from tests.gpu_util import _expect_overflow, exported, load, make_oracle, oracle_slot
from tests.oracle_compare import metrics_equal, slot_equal, tables_equal

pytestmark = pytest.mark.gpu


@pytest.fixture
def subwave_path(monkeypatch):
    """make_env of the parity tests hands out handles pinned to the sub-wave path; yields the handles it made.
    (random_rollout calls `force_general_kernel(False)` right behind make_env, which would put the handle back on AUTO:
    the method is shadowed on the instance.)"""
    plain = gu.make_env
    made = []

    def make(cfg, B, mode=STEP_MY_STEP, dtype=torch.float64):
        env = plain(cfg, B, mode, dtype)
        env.use_subwave_path()
        env.force_general_kernel = lambda on=True: None
        made.append(env)
        return env
    monkeypatch.setattr(gu, "make_env", make)
    yield made


def ran_subwave(made):
    assert made
    for env in made:
        assert (env.last_kernel() & 15) == KERNEL_SUBWAVE, env.last_kernel()


def pinned(cfg, B, dtype=torch.float64, mode=STEP_MY_STEP):
    env = gu.make_env(cfg, B, mode, dtype)
    env.use_subwave_path()
    return env


def toy(N=4, A=3, K=20, L=100.0, Rc=250.0, **kw):
    """configs/4ue_3r_toy's shape by default: 4 vehicles, 3 resources, L = 100, Rc = 250, 20 bins."""
    state = dict(num_bins=K)
    state.update(kw.pop("State", {}))
    return bench_config(N, A, L, communication_range=Rc, State=state, **kw)


# ---- 1. the reference's fixtures -----------------------------------------------------------------------------------------

def _fits(cfg):
    return (cfg.num_users <= 8 and cfg.num_channels <= 16 and cfg.State.num_bins <= 64 and not cfg.State.piggybacking)


SMALL_GOLDENS = [n for n in golden_names() if _fits(Golden(n).cfg)]


def test_the_fixture_filter_selects_the_small_fixtures():
    assert len(SMALL_GOLDENS) >= 20, SMALL_GOLDENS


@pytest.mark.parametrize("name", SMALL_GOLDENS)
def test_golden_replay_on_the_subwave_path(name, subwave_path):
    """B = 3 replicas: a wave whose last groups hold no env."""
    gu.golden_replay_on_gpu(name)
    ran_subwave(subwave_path)


@pytest.mark.parametrize("name", ["g1_step_rd2", "g1_ch_rd2", "g1_design"])
def test_testenv_shim_forwards_the_opt_in(name):
    """`TestEnv(subwave=True, **config["EnvironmentTest"])` driven with the reference's call sequence."""
    from diral_amd import TestEnv
    from tests.golden_util import ulp_diff
    g = Golden(name)
    env = TestEnv(subwave=True, **g.cfg_dict)
    env.reset_mobility_env()
    step = {STEP_MY_STEP: env.my_step, STEP_MY_STEP_CH: env.my_step_ch, STEP_DESIGN: env.my_step_design}
    for i, mode, acts, t, (ep, eps) in g.steps():
        obs, rews = step[mode](acts, t)
        assert (env._env.last_kernel() & 15) == KERNEL_SUBWAVE
        state = env.obtain_state(obs, acts, list(rews), ep, eps)
        assert np.array_equal(rews, g["rews"][i])
        assert ulp_diff(np.array(state), g["state"][i]) <= gu.DIST_ULP
        assert env.get_x_pos() == list(g["pos_x"][i])


# ---- 2. random runs against the oracle -----------------------------------------------------------------------------------

# (N, A, K, B, L, Rc): every N with every A and K somewhere; B on and around a group of lanes, a wave (16 envs of 4 lanes,
# 8 of 8) and a block (64 / 32), and more than one block; Rc above L (everybody hears everybody) and below (some hear nobody)
SIZES = [
    (2, 1, 1, 1, 100.0, 250.0), (3, 3, 10, 15, 100.0, 250.0), (4, 16, 64, 16, 100.0, 250.0), (5, 1, 10, 7, 100.0, 250.0),
    (7, 3, 64, 8, 100.0, 250.0), (8, 16, 1, 9, 100.0, 250.0),
    (2, 3, 64, 17, 300.0, 60.0), (3, 16, 1, 33, 300.0, 60.0), (4, 3, 20, 130, 300.0, 60.0), (5, 16, 10, 130, 300.0, 60.0),
    (7, 1, 1, 33, 300.0, 60.0), (8, 3, 10, 17, 300.0, 60.0),
    (4, 1, 10, 9, 400.0, 120.0), (4, 3, 20, 7, 100.0, 250.0), (3, 3, 20, 8, 400.0, 120.0), (8, 1, 64, 15, 400.0, 120.0),
    (8, 16, 64, 16, 100.0, 250.0), (5, 3, 20, 1, 400.0, 120.0), (2, 16, 10, 130, 100.0, 250.0), (7, 16, 20, 130, 400.0, 120.0),
]


@pytest.mark.parametrize("N,A,K,B,L,Rc", SIZES)
def test_sizes_around_the_lane_groups_vs_oracle(N, A, K, B, L, Rc, subwave_path):
    cfg = toy(N, A, K, L, Rc, State=dict(add_channel_obs=True, add_reward=True))
    gu.random_rollout(cfg, B=B, T=30, seed=5000 + 17 * N + A + K + B, sticky=0.5, track_prr=bool(B & 1),
                      expect_kernel=KERNEL_SUBWAVE)
    ran_subwave(subwave_path)


RICH = dict(add_channel_obs=True, add_reward=True, add_index=True, add_velocity=True, add_position=True)


@pytest.mark.parametrize("N,A,B", [(4, 3, 17), (8, 16, 9), (7, 3, 33)])
@pytest.mark.parametrize("mode,rd,toyw", [(STEP_MY_STEP, 1, False), (STEP_MY_STEP, 1, True), (STEP_MY_STEP, 2, False),
                                          (STEP_MY_STEP, 2, True), (STEP_MY_STEP, 3, False), (STEP_MY_STEP, 4, False),
                                          (STEP_MY_STEP, 5, False), (STEP_MY_STEP, 5, True), (STEP_MY_STEP_CH, 2, False),
                                          (STEP_MY_STEP_CH, 3, False), (STEP_MY_STEP_CH, 4, False), (STEP_DESIGN, 2, False)])
def test_step_kinds_and_reward_designs_vs_oracle(N, A, B, mode, rd, toyw, subwave_path):
    """All three step kinds, reward_design 1-5 with toy and non-toy weights, the rich State flags, the fingerprint."""
    cfg = toy(N, A, 20, 300.0, 120.0, reward_design=rd, congestion_test=toyw, enable_fingerprint=True, State=RICH)
    gu.random_rollout(cfg, B=B, T=30, seed=6000 + 100 * mode + 10 * rd + N + int(toyw), mode=mode, sticky=0.6,
                      track_prr=(mode == STEP_MY_STEP and rd % 2 == 0), expect_kernel=KERNEL_SUBWAVE)
    ran_subwave(subwave_path)


@pytest.mark.parametrize("N,A,B", [(4, 3, 16), (8, 16, 15), (5, 3, 9)])
def test_state_type_1_with_the_real_action_index(N, A, B, subwave_path):
    cfg = toy(N, A, 10, 300.0, 120.0, State=dict(type=1, action_index="real", add_channel_obs=True, add_reward=True))
    gu.random_rollout(cfg, B=B, T=30, seed=6500 + N, expect_kernel=KERNEL_SUBWAVE)
    ran_subwave(subwave_path)


@pytest.mark.parametrize("N,A,mode", [(4, 3, STEP_MY_STEP), (8, 3, STEP_MY_STEP), (4, 3, STEP_MY_STEP_CH), (7, 2, STEP_DESIGN)])
def test_proportional_fairness_with_sticky_actions(N, A, mode, subwave_path):
    """Sticky actions take the pf counters over the threshold (random_rollout asserts that they did)."""
    cfg = toy(N, A, 20, 100.0, 250.0, reward_design=2 if mode != STEP_MY_STEP else 1, proportional_fair=True,
              State=dict(add_reward=True))
    gu.random_rollout(cfg, B=17, T=45, seed=6600 + N + mode, mode=mode, sticky=0.9, expect_kernel=KERNEL_SUBWAVE)
    ran_subwave(subwave_path)


def _lanes(rng, B, N):
    return rng.integers(0, 2, size=(B, N)).astype(np.float64) * 1.5


@pytest.mark.parametrize("N,A,B", [(4, 3, 17), (8, 5, 9), (3, 16, 33)])
def test_velocity_updates_and_lanes_off_the_line(N, A, B, subwave_path):
    cfg = toy(N, A, 20, 300.0, 120.0, mobility_vary=True, reward_design=1, State=dict(add_velocity=True, add_position=True))
    gu.random_rollout(cfg, B=B, T=30, seed=6700 + N, vel_every=25, y0=_lanes, sticky=0.4, track_prr=True,
                      expect_kernel=KERNEL_SUBWAVE)
    ran_subwave(subwave_path)


@pytest.mark.parametrize("N,A,mode", [(4, 3, STEP_DESIGN), (6, 3, STEP_MY_STEP), (8, 4, STEP_MY_STEP_CH)])
def test_static_design_topology(N, A, mode, subwave_path):
    cfg = toy(N, A, 20, 300.0, 120.0, mobility=False, enable_design_topology=True, State=dict(add_position=True))
    gu.random_rollout(cfg, B=9, T=30, seed=6800 + N, mode=mode, sticky=0.5, expect_kernel=KERNEL_SUBWAVE)
    ran_subwave(subwave_path)


@pytest.mark.parametrize("state", [dict(add_positional_dist_piggy=False, add_channel_obs=True),
                                   dict(add_positional_dist_piggy=False, add_positional_dist=True),
                                   dict(add_positional_dist=True, add_reward=True),
                                   dict(add_positional_dist_type=1, num_bins=12, add_channel_obs=True)])
@pytest.mark.parametrize("N,A", [(4, 3), (8, 16)])
def test_handles_without_tables_and_the_secondary_observation_launches(N, A, state, subwave_path):
    """No piggybacked tables at all; the sorted distances and the type-1 histogram, launches of their own behind this step."""
    cfg = toy(N, A, 20, 300.0, 120.0, State=state)
    gu.random_rollout(cfg, B=17, T=30, seed=6900 + N + len(state), sticky=0.3, y0=_lanes if N == 8 else None,
                      expect_kernel=KERNEL_SUBWAVE)
    ran_subwave(subwave_path)


@pytest.mark.parametrize("per_env", [False, True])
@pytest.mark.parametrize("N,A", [(4, 3), (7, 5)])
def test_trace_replay_vs_oracle(N, A, per_env):
    """load_saved_positions with a [T, N] and a [B, T, N] trace, slot numbers past the trace's end and out of order."""
    from oracle.oracle import Oracle, SQ_IEEE
    cfg = toy(N, A, 20, 300.0, 120.0, State=dict(add_position=True, add_channel_obs=True))
    B, T = 9, 11
    rng = np.random.default_rng(7000 + N + int(per_env))
    x0 = rng.integers(0, 300, size=(B, N)).astype(np.float64)
    v0 = rng.uniform(1.1, 2.7, size=(B, N))
    traces = rng.uniform(0, 300, size=(B, T, N) if per_env else (T, N))
    env = pinned(cfg, B)
    env.reset_topology(x0, None, v0)
    env.load_saved_positions(traces)
    orcs = [Oracle(cfg, batch=1, sq_mode=SQ_IEEE) for _ in range(B)]
    for b, o in enumerate(orcs):
        o.reset(x0[b:b + 1], np.zeros((1, N)), v0[b:b + 1])
        o.set_trace(traces[b] if per_env else traces)
    for t in list(range(14)) + [40, 41, 5]:
        a = rng.integers(0, A, size=(B, N)).astype(np.int32)
        obs, rew, chobs, _ = gu.gpu_step(env, STEP_MY_STEP, a, t)
        assert (env.last_kernel() & 15) == KERNEL_SUBWAVE
        for b, o in enumerate(orcs):
            o_rew, o_chobs = o.step(STEP_MY_STEP, a[b:b + 1], t)
            assert np.array_equal(obs[b], o.obtain_state(a[b:b + 1], o_chobs, o_rew)[0]), (t, b)
            assert np.array_equal(rew[b], o_rew[0]) and np.array_equal(chobs[b], o_chobs[0]), (t, b)
    st = exported(env)
    for b, o in enumerate(orcs):
        oe = o.export()
        for k in ("pos_x", "seq", "x"):
            assert np.array_equal(st[k][b], oe[k][0]), (k, b)
    env.check()


# ---- 3. path switches, env copies ------------------------------------------------------------------------------------------

def _set_path(env, path):
    if path == "subwave":
        env.use_subwave_path()
    else:
        env.force_general_kernel(path == "general")                 # (False: back to AUTO)


@pytest.mark.parametrize("N,A", [(4, 3), (8, 16)])
def test_path_switches_on_one_handle(N, A):
    """AUTO -> SUBWAVE -> GENERAL -> SUBWAVE -> AUTO every four slots over 40 slots: the step that moves the tables without
    the xpos ring leaves them where every other path finds them.  Outputs every slot, exported tables at every switch."""
    cfg = toy(N, A, 20, 300.0, 120.0, track_arrival=True, State=dict(add_channel_obs=True, add_reward=True))
    B = 17
    rng = np.random.default_rng(7100 + N)
    tab = dict(pos_x=rng.integers(0, 300, size=(B, N)).astype(np.float64), vel=rng.uniform(1.1, 2.7, size=(B, N)))
    env = gu.make_env(cfg, B)
    env.reset_topology(tab["pos_x"], 0.0, tab["vel"])
    from oracle.oracle import Oracle, SQ_IEEE
    orc = Oracle(cfg, batch=B, sq_mode=SQ_IEEE, threads=4)
    orc.reset(tab["pos_x"], np.zeros((B, N)), tab["vel"])
    order = ["auto", "subwave", "general", "subwave", "auto"]
    family = dict(auto=KERNEL_FAST64, subwave=KERNEL_SUBWAVE, general=KERNEL_GENERAL)
    seen = set()
    for t in range(40):
        path = order[(t // 4) % len(order)]
        if t % 4 == 0:
            tables_equal(exported(env), orc.export(), ("before", path, t))
            _set_path(env, path)
        acts = rng.integers(0, A, size=(B, N)).astype(np.int32)
        mode = STEP_MY_STEP_CH if t % 3 == 2 else STEP_MY_STEP
        obs, rew, chobs, _ = gu.gpu_step(env, mode, acts, t)
        assert (env.last_kernel() & 15) == family[path], (t, path, env.last_kernel())
        seen.add(env.last_kernel() & 15)
        slot_equal(cfg, mode, (obs, rew, chobs), oracle_slot(orc, mode, acts, t), (path, t))
        if t % 4 == 1:
            fa = rng.integers(0, A, size=(B, N)).astype(np.int32)
            fc, fr = rng.uniform(0.0, 300.0, size=(B, N, A)), rng.uniform(-3.0, 1.0, size=(B, N))
            s1 = env.obtain_state(fc, fa, fr).cpu().numpy()
            assert (env.last_kernel() & 15) == (KERNEL_GENERAL if path == "general" else KERNEL_OBSERVE)
            assert np.array_equal(s1, orc.obtain_state(fa, fc, fr)), (path, t)
    assert seen == set(family.values())
    tables_equal(exported(env), orc.export(), "end")
    assert np.array_equal(env.info_age(39).cpu().numpy(), orc.info_age(39))
    env.check()


@pytest.mark.parametrize("N,A", [(4, 3), (8, 16)])
def test_env_copies_between_a_pinned_and_an_auto_handle_and_snapshot_restore(N, A):
    cfg = toy(N, A, 20, 300.0, 120.0, proportional_fair=True, reward_design=1, State=dict(add_channel_obs=True, add_reward=True))
    B = 17
    rng = np.random.default_rng(7200 + N)
    x0, v0 = rng.integers(0, 300, size=(B, N)).astype(np.float64), rng.uniform(1.1, 2.7, size=(B, N))
    tab = dict(pos_x=x0, vel=v0)
    sub, auto = pinned(cfg, B), gu.make_env(cfg, B)
    sub.reset_topology(x0, 0.0, v0)
    auto.reset_topology(seed=5)
    from oracle.oracle import Oracle, SQ_IEEE
    orc = Oracle(cfg, batch=B, sq_mode=SQ_IEEE, threads=4)
    orc.reset(tab["pos_x"], np.zeros((B, N)), tab["vel"])
    t = 0

    def both(n, envs, kinds):
        nonlocal t
        for _ in range(n):
            acts = rng.integers(0, A, size=(B, N)).astype(np.int32)
            got = []
            for env, kind in zip(envs, kinds):
                obs, rew, chobs, _ = gu.gpu_step(env, STEP_MY_STEP, acts, t)
                assert (env.last_kernel() & 15) == kind
                got.append((obs, rew, chobs))
            slot_equal(cfg, STEP_MY_STEP, got[0], oracle_slot(orc, STEP_MY_STEP, acts, t), t)
            for g in got[1:]:
                assert all(np.array_equal(x, y) for x, y in zip(got[0], g)), t
            t += 1
    both(6, [sub], [KERNEL_SUBWAVE])
    auto.copy_envs_from(sub)                                          # pinned -> AUTO (planes -> a handle that steps on the ring)
    both(5, [sub, auto], [KERNEL_SUBWAVE, KERNEL_FAST64])
    sub2 = pinned(cfg, B)
    sub2.reset_topology(seed=6)
    sub2.copy_envs_from(auto)                                         # AUTO (ring form) -> pinned
    both(5, [sub, auto, sub2], [KERNEL_SUBWAVE, KERNEL_FAST64, KERNEL_SUBWAVE])
    for env in (sub, auto, sub2):
        tables_equal(exported(env), orc.export(), "copies")
        metrics_equal(gu.host(env.metrics()), orc.metrics(), "copies")
    # snapshot / restore on the pinned handle: the same three slots twice
    snap = sub.snapshot()
    before = exported(sub)
    acts = rng.integers(0, A, size=(3, B, N)).astype(np.int32)
    first = [gu.gpu_step(sub, STEP_MY_STEP, acts[i], t + i) for i in range(3)]
    after = exported(sub)
    sub.restore(snap)
    again = exported(sub)
    for k in before:
        assert np.array_equal(before[k], again[k]), k
    second = [gu.gpu_step(sub, STEP_MY_STEP, acts[i], t + i) for i in range(3)]
    assert (sub.last_kernel() & 15) == KERNEL_SUBWAVE
    for f, s in zip(first, second):
        assert all(np.array_equal(x, y) for x, y in zip(f, s))
    twice = exported(sub)
    for k in after:
        assert np.array_equal(after[k], twice[k]), k
    for env in (sub, auto, sub2):
        env.check()


# ---- 4. old tables, the 24-bit horizon -------------------------------------------------------------------------------------

@pytest.mark.parametrize("A", [3, 16])
def test_entries_of_every_lag_class_a_million_stamps_old(A):
    """horizon_tables at N = 8: never heard, fresh, hand-over, mid, the last byte ranks, ancient (lag >= 2^20): the merge is
    on 32-bit (sequence number, source) keys whatever the lag.  Six slots against the oracle."""
    N, B, L = 8, 33, 300.0
    cfg = toy(N, A, 20, L, 120.0, track_arrival=True)
    rng = np.random.default_rng(7300 + A)
    T0 = 1_300_000
    tab = horizon_tables(rng, B, N, L, T0)
    lag = T0 - tab["seq"].astype(np.int64)
    heard = tab["seq"] > 0
    for lo, hi in ((1, 3), (6, 8), (9, 40), (253, 255), (1 << 20, 1 << 21)):
        assert (heard & (lag >= lo) & (lag <= hi)).any(), (lo, hi)
    assert (~heard).any()
    env = pinned(cfg, B)
    load(env, tab)
    orc = make_oracle(cfg, tab)
    for t in range(6):
        acts = rng.integers(0, A, size=(B, N)).astype(np.int32)
        obs, rew, chobs, _ = gu.gpu_step(env, STEP_MY_STEP, acts, t)
        assert (env.last_kernel() & 15) == KERNEL_SUBWAVE
        slot_equal(cfg, STEP_MY_STEP, (obs, rew, chobs), oracle_slot(orc, STEP_MY_STEP, acts, t), t)
        tables_equal(exported(env), orc.export(), t)
    env.check()


@pytest.mark.parametrize("N,mode", [(8, STEP_MY_STEP), (4, STEP_MY_STEP_CH)])
def test_the_slot_past_the_last_number_is_reported_once(N, mode):
    """From DIRAL_MAX_SLOTS - 3: three clean slots that are the oracle's, the fourth raises ERR_SEQ_OVERFLOW once - where
    the other paths report it (tests/test_gpu_seq_horizon.py)."""
    A, B, L = 3, 9, 300.0
    cfg = toy(N, A, 20, L, 120.0, track_arrival=True)
    rng = np.random.default_rng(7400 + N)
    tab = horizon_tables(rng, B, N, L, MAX_SLOTS - 3)
    env = pinned(cfg, B)
    load(env, tab)
    orc = make_oracle(cfg, tab)
    for t in range(3):
        acts = rng.integers(0, A, size=(B, N)).astype(np.int32)
        obs, rew, chobs, _ = gu.gpu_step(env, mode, acts, t)
        assert (env.last_kernel() & 15) == KERNEL_SUBWAVE
        slot_equal(cfg, mode, (obs, rew, chobs), oracle_slot(orc, mode, acts, t), t)
        env.check()
    st = exported(env)
    tables_equal(st, orc.export(), "horizon")
    assert st["seq"].max() == MAX_SLOTS
    gu.gpu_step(env, mode, rng.integers(0, A, size=(B, N)).astype(np.int32), 3)
    assert (env.last_kernel() & 15) == KERNEL_SUBWAVE
    _expect_overflow(env)


# ---- 5. histogram bin edges --------------------------------------------------------------------------------------------------

EDGE_N, EDGE_A, EDGE_L, EDGE_RB = 8, 4, 2000.0, 500.0
EDGE_TYPE = (0, 1, 2, 1, 0, 1, 2, 1)                       # the vehicle's post-move position: 0, L / 2, one step below L
YOUNG, OLD = (0, 5, 17, 18), (19, 25, 200)                 # ages at the import: 18 -> 19 is the last one counted, 19 -> 20 the first not


def edge_tables(K):
    """Imported tables whose entries sit on and one double either side of every edge of linspace(-Rb, Rb, K + 1) as seen
    from viewers whose move ends on 0, on L / 2 and one step below L (tests/hist_edge_cases.py `move`: the reference's own
    arithmetic).  Nobody hears anybody (communication range 0), so the entries reach the histogram stamped and aged only.
    Every viewer holds its own sequence number about a subject (lag 1 + viewer): equal numbers, equal xpos holds trivially;
    viewer (k + 1) % N never heard subject k (number 0, a ghost xpos aimed like the others).  Entries aimed at an edge are
    young enough to count, the slots left over carry uniform values and ages on both sides of info_age_limit."""
    N, L, rb = EDGE_N, EDGE_L, EDGE_RB
    vel = 1.5
    npx_t = [0.0, L / 2, None]
    px_t = [L - vel, L / 2 - vel, math.nextafter(L, 0.0) - vel]
    while float(H.move([px_t[2]], [vel], L)[0]) < L / 2:     # (a sum that rounds up to 2 L wraps to 0: one step further down)
        px_t[2] = math.nextafter(px_t[2], 0.0)
    npx_t = [float(H.move([p], [vel], L)[0]) for p in px_t]
    assert npx_t[0] == 0.0 and npx_t[1] == L / 2 and L - 1e-9 < npx_t[2] < L
    edges = np.linspace(-rb, rb, K + 1)
    targets = {ty: [] for ty in range(3)}
    for ty in range(3):
        for e in edges:
            x0 = npx_t[ty] + float(e)
            for x in (math.nextafter(x0, -math.inf), x0, math.nextafter(x0, math.inf)):
                if 0.0 <= x <= L:
                    targets[ty].append(x)
    per_env = {ty: 7 * EDGE_TYPE.count(ty) for ty in range(3)}
    B = max(-(-len(targets[ty]) // per_env[ty]) for ty in range(3)) + 1
    rng = np.random.default_rng(7500 + K)
    for ty in range(3):
        rng.shuffle(targets[ty])
    T0 = 50
    ptype = np.array(EDGE_TYPE)
    px = np.broadcast_to(np.array(px_t)[ptype], (B, N)).copy()
    seq = np.zeros((B, N, N), np.int32)
    age = np.zeros((B, N, N), np.int32)
    x = np.zeros((B, N, N))
    dealt = 0
    for b in range(B):
        for u in range(N):
            for k in range(N):
                if u == k:
                    seq[b, u, k], x[b, u, k] = T0, px[b, k]
                    continue
                never = u == (k + 1) % N
                seq[b, u, k] = 0 if never else T0 - 1 - u
                pool = targets[EDGE_TYPE[u]]
                if pool:
                    x[b, u, k], age[b, u, k] = pool.pop(), YOUNG[(b + u + k) % len(YOUNG)]
                    dealt += 1
                else:
                    x[b, u, k] = rng.uniform(0.0, L)
                    age[b, u, k] = (YOUNG + OLD)[int(rng.integers(0, len(YOUNG + OLD)))]
    assert not any(targets.values()) and dealt >= 3 * (K + 1)
    assert (age[seq != T0] >= 19).any() and (age == 18).any()
    acts = rng.integers(0, EDGE_A, size=(2, B, N)).astype(np.int32)
    return dict(B=B, px=px, vel=np.full((B, N), vel), seq=seq, age=age, x=x, acts=acts, npx=np.array(npx_t)[ptype])


@pytest.mark.parametrize("K", [10, 20, 40, 64])
def test_histogram_bin_edges_vs_oracle_and_numpy(K):
    from oracle.oracle import Oracle, SQ_IEEE
    N, A = EDGE_N, EDGE_A
    t = edge_tables(K)
    B = t["B"]
    cfg = bench_config(N, A, EDGE_L, bin_range=EDGE_RB, communication_range=0.0, State=dict(num_bins=K))
    zeros = np.zeros((B, N))
    # np.histogram on the imported values, one viewer at a time (the plain statement, tests/hist_edge_cases.py)
    ok = (t["age"] + 1 < H.AGE_LIMIT) & ~np.eye(N, dtype=bool)[None]
    dx = t["x"] - t["npx"][None, :, None]
    direct = np.stack([np.stack([H.numpy_hist(dx[b, u], np.zeros(N), ok[b, u], K, EDGE_RB) for u in range(N)]) for b in range(B)])
    for dt in (torch.float64, torch.float32):
        env = pinned(cfg, B, dtype=dt)
        env.reset_topology(t["px"], 0.0, t["vel"])
        env.import_state(t["px"], zeros, t["vel"], seq=t["seq"], age=t["age"], x=t["x"])
        env.check()
        if dt == torch.float64:
            o = Oracle(cfg, batch=B, sq_mode=SQ_IEEE, threads=4)
            o.reset(t["px"], zeros, t["vel"])
            o.import_state(seq=t["seq"], age=t["age"], x=t["x"], y=np.zeros((B, N, N)))
        for slot in range(2):
            a = t["acts"][slot]
            obs, rew, _ = env.step(a, slot)
            torch.cuda.synchronize()
            assert (env.last_kernel() & 15) == KERNEL_SUBWAVE
            got = obs.cpu().numpy().copy()
            if dt == torch.float64:
                o_rew, o_chobs = o.step(STEP_MY_STEP, a, slot)
                want = o.obtain_state(a, o_chobs, o_rew)
                if slot == 0:
                    first = want
                assert np.array_equal(got, want), (K, slot, np.argwhere(got != want)[:5])
                assert np.array_equal(rew.cpu().numpy(), o_rew)
                if slot == 0:
                    assert np.array_equal(o.export()["pos_x"], np.broadcast_to(t["npx"], (B, N)))
                    assert np.array_equal(got[:, :, -K:], direct), (K, np.argwhere(got[:, :, -K:] != direct)[:5])
                tables_equal(exported(env), o.export(), (K, slot))
            elif slot == 0:
                assert np.array_equal(got, first.astype(np.float32)), K
                assert np.array_equal(got[:, :, -K:], direct.astype(np.float32)), K
        env.check()


# ---- 6. refusals and flags -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", [toy(9, 3, 20), toy(4, 17, 20), toy(4, 3, 65),
                                 toy(4, 3, 20, 100.0, 250.0, State=dict(piggybacking=True, add_channel_obs=True)),
                                 bench_config(300, 8, 5000.0)],
                         ids=["N9", "A17", "K65", "piggybacking", "N300"])
def test_handles_the_path_does_not_take_keep_their_kernel(cfg):
    from diral_amd.vec_env import DiralError
    B = 3
    env = gu.make_env(cfg, B)
    env.reset_topology(seed=3)
    acts = np.broadcast_to(np.arange(cfg.num_users) % cfg.num_channels, (B, cfg.num_users)).astype(np.int32)
    env.step(acts, 0)
    before = env.last_kernel()
    assert (before & 15) != KERNEL_SUBWAVE
    with pytest.raises(DiralError) as ei:
        env.use_subwave_path()
    assert ei.value.status == ERR_UNSUPPORTED
    env.step(acts, 1)
    assert env.last_kernel() == before
    env.check()


def test_option_values_beyond_the_paths_are_bad_arguments():
    env = gu.make_env(toy(), 3)
    assert env.lib.diral_env_set_option(env._h, OPT_KERNEL_PATH, 4) == ERR_BAD_ARG
    assert env.lib.diral_env_set_option(env._h, OPT_KERNEL_PATH, -1) == ERR_BAD_ARG
    assert env.lib.diral_env_set_option(env._h, OPT_KERNEL_PATH, 3) == 0
    assert env.lib.diral_env_set_option(env._h, OPT_KERNEL_PATH, 4) == ERR_BAD_ARG   # ... and the pin stays
    env.reset_topology(seed=1)
    env.step(np.zeros((3, 4), np.int32), 0)
    assert (env.last_kernel() & 15) == KERNEL_SUBWAVE


@pytest.mark.parametrize("N,A", [(4, 3), (8, 16)])
def test_k_slot_calls_are_refused_with_the_env_untouched_and_one_policy_slot_equals_the_auto_twin(N, A):
    from diral_amd.sps import SpsPolicy
    from diral_amd.vec_env import DiralError
    cfg = toy(N, A, 20, 300.0, 120.0, reward_design=2)
    B = 17
    rng = np.random.default_rng(7600 + N)
    x0, v0 = rng.integers(0, 300, size=(B, N)).astype(np.float64), rng.uniform(1.1, 2.7, size=(B, N))
    sub, auto = pinned(cfg, B), gu.make_env(cfg, B)
    pols = []
    for env in (sub, auto):
        env.reset_topology(x0, 0.0, v0)
        pols.append(SpsPolicy(B, N, A, device="cuda:0", seed=11))
    for t in range(3):
        a = rng.integers(0, A, size=(B, N)).astype(np.int32)
        for env in (sub, auto):
            env.step(a, t)
    before = exported(sub)
    seq = torch.as_tensor(rng.integers(0, A, size=(4, B, N)).astype(np.int32), device="cuda:0")
    nxt = torch.empty((B, N), dtype=torch.int32, device="cuda:0")
    calls = [lambda: sub.rollout(seq, 3),
             lambda: sub.prefill(seq[0], 4, seed=5),
             lambda: sub.prefill(seq[0], 4, seed=5, mode="my_step_ch"),
             lambda: sub.step_policy(seq[0].contiguous(), 3, pols[0], nxt, slots=4)]
    for call in calls:
        with pytest.raises(DiralError) as ei:
            call()
        assert ei.value.status == ERR_UNSUPPORTED
        torch.cuda.synchronize()
        after = exported(sub)
        for k in before:
            assert np.array_equal(before[k], after[k]), k
    assert (sub.last_kernel() & 15) == KERNEL_SUBWAVE                  # (nothing was launched)
    # one policy slot: three launches around this step on the pinned handle, whatever the AUTO twin runs
    outs = []
    for env, pol in zip((sub, auto), pols):
        a = pol.prev_action.clone()
        got = []
        for t in range(3, 8):
            n = torch.empty_like(a)
            sh = torch.zeros((B, N), dtype=env.out_dtype, device="cuda:0")
            sr = torch.zeros((B,), dtype=env.out_dtype, device="cuda:0")
            co = torch.zeros((B,), dtype=env.out_dtype, device="cuda:0")
            obs, rew, done = env.step_policy(a, t, pol, n, shaped_out=sh, sum_r_out=sr, collision_out=co)
            got.append([x.clone() for x in (obs, rew, done, n, sh, sr, co)])
            a = n
        torch.cuda.synchronize()
        outs.append(got)
    assert (sub.last_kernel() & 15) == KERNEL_SUBWAVE
    for s, g in zip(*outs):
        for x, y in zip(s, g):
            assert torch.equal(x, y)
    assert torch.equal(pols[0].prev_action, pols[1].prev_action) and torch.equal(pols[0].counter, pols[1].counter)
    es, ea = exported(sub), exported(auto)
    for k in es:
        assert np.array_equal(es[k], ea[k]), k
    sub.check(); auto.check()


@pytest.mark.parametrize("N,A,B", [(4, 3, 17), (8, 16, 9)])
def test_an_action_out_of_range_is_reported_once(N, A, B):
    from diral_amd.vec_env import DiralError
    env = pinned(toy(N, A), B)
    env.reset_topology(seed=3)
    a = np.zeros((B, N), np.int32)
    a[B - 1, N - 1] = A
    env.step(a, 0)
    assert (env.last_kernel() & 15) == KERNEL_SUBWAVE
    with pytest.raises(DiralError) as ei:
        env.check()
    assert ei.value.status == ERR_ACTION_RANGE
    env.check()
    a[B - 1, N - 1] = -1
    env.step(a, 1)
    with pytest.raises(DiralError) as ei:
        env.check()
    assert ei.value.status == ERR_ACTION_RANGE
    env.step(np.zeros((B, N), np.int32), 2)
    env.check()


@pytest.mark.parametrize("N,A,mode,rd", [(4, 3, STEP_MY_STEP, 3), (8, 16, STEP_MY_STEP_CH, 4), (7, 5, STEP_DESIGN, 2)])
def test_f32_outputs_are_the_cast_of_the_f64_ones(N, A, mode, rd):
    cfg = toy(N, A, 20, 300.0, 120.0, reward_design=rd, enable_fingerprint=True, State=RICH)
    B = 33
    rng = np.random.default_rng(7700 + N)
    x0, v0 = rng.integers(0, 300, size=(B, N)).astype(np.float64), rng.uniform(1.1, 2.7, size=(B, N))
    e64, e32 = pinned(cfg, B, torch.float64), pinned(cfg, B, torch.float32)
    for e in (e64, e32):
        e.reset_topology(x0, 0.0, v0)
    for t in range(25):
        a = rng.integers(0, A, size=(B, N)).astype(np.int32)
        o64, r64, c64, d64 = gu.gpu_step(e64, mode, a, t, 2.0, 0.5)
        o32, r32, c32, d32 = gu.gpu_step(e32, mode, a, t, 2.0, 0.5)
        assert (e32.last_kernel() & 15) == (e64.last_kernel() & 15) == KERNEL_SUBWAVE
        assert o32.dtype == np.float32 and np.array_equal(o64.astype(np.float32), o32), t
        assert np.array_equal(r64.astype(np.float32), r32) and np.array_equal(c64.astype(np.float32), c32), t
        assert np.array_equal(d64, d32)
    a, b = exported(e64), exported(e32)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- 7. capture ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,A", [(4, 3), (8, 16)])
def test_four_captured_steps_replayed_twice_with_a_slot_clock_equal_the_eager_run(N, A):
    """The launch is enqueue-only: four my_step_ch calls (arrival stamps and `done` read the slot number on the device)
    captured into one single-branch graph and replayed twice with a clock that moves on by four = eight eager slots."""
    from diral_amd.rollout import SlotClock, no_finalizers_during_capture
    cfg = toy(N, A, 20, 300.0, 120.0, reward_design=3, track_arrival=True, episode_interval=3, State=dict(add_channel_obs=True))
    B = 33
    rng = np.random.default_rng(7800 + N)
    x0, v0 = rng.integers(0, 300, size=(B, N)).astype(np.float64), rng.uniform(1.1, 2.7, size=(B, N))
    acts = [torch.as_tensor(rng.integers(0, A, size=(B, N)).astype(np.int32), device="cuda:0") for _ in range(4)]
    eager, graphed = pinned(cfg, B, torch.float32), pinned(cfg, B, torch.float32)
    for e in (eager, graphed):
        e.reset_topology(x0, None, v0)
        e._step(STEP_MY_STEP_CH, acts[3], 0, want_chobs=True)       # (slot 0 outside the capture: the output buffers exist)
    outs_e = []
    for j in range(8):
        obs, rew, done = eager._step(STEP_MY_STEP_CH, acts[j % 4], 1 + j, want_chobs=True)
        if j % 4 == 3:
            outs_e.append([x.clone() for x in (obs, rew, done, eager._chobs)])
    clock = SlotClock("cuda:0", 1)
    graphed.set_clock(clock.t)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with no_finalizers_during_capture(), torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for i in range(4):
                obs_g, rew_g, done_g = graphed._step(STEP_MY_STEP_CH, acts[i], i, want_chobs=True)
            graphed.lib.diral_clock_add(clock.ptr(), 4, graphed._stream())
    for rep in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert (graphed.last_kernel() & 15) == KERNEL_SUBWAVE
        for x, y in zip(outs_e[rep], (obs_g, rew_g, done_g, graphed._chobs)):
            assert torch.equal(x, y), rep
    assert clock.value() == 9
    a, b = exported(eager), exported(graphed)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    graphed.set_clock(None)
    assert np.array_equal(eager.info_age(8).cpu().numpy(), graphed.info_age(8).cpu().numpy())
    assert torch.equal(eager.metrics(), graphed.metrics())
    eager.check(); graphed.check()
