"""The host reference of the closed loop (tests/host_closed_loop.py) pinned on the CPU before it judges the device
launches in tests/test_gpu_closed_loop_host.py: the generator against the published splitmix64 outputs, HostSps against
the seven fixtures recorded from the reference's SPS agent and against a brute-force statement on windows that tie, the
prefill against DriverLoop.prefill on the oracle."""
import itertools
import math
import os

import numpy as np
import pytest
import torch

from diral_amd.config import bench_config, c2_config
from diral_amd.driver import DriverLoop
from oracle.oracle import SQ_IEEE
from tests import host_closed_loop as H
from tests.oracle_backend import OracleBackend

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPS_FIXTURES = ["s1_sps_int_threshold", "s2_sps_frac_threshold", "s3_sps_small_window", "s4_sps_window64",
                "s5_sps_window100", "s6_sps_window200", "s7_sps_window300"]


def test_mix64_is_splitmix64():
    """The first two outputs of splitmix64 from state 0 (Vigna's reference implementation): the state advances by the
    golden gamma, so they are mix64(0) and mix64(gamma)."""
    assert int(H.mix64(0)[0]) == 0xE220A8397B1DCDAF
    assert int(H.mix64(0x9E3779B97F4A7C15)[0]) == 0x6E789E6AA1B965F4


def test_generator_draws_are_pure_and_in_range():
    """rng_u64 is vectorised over the index (array == element by element), wraps modulo 2**64 on a seed near the top,
    and the draw rules stay in their documented ranges."""
    idx = np.arange(1000, dtype=np.uint64)
    for seed in (0, 7, 2**64 - 3):
        all_ = H.rng_u64(seed, 9, idx)
        assert all(int(H.rng_u64(seed, 9, i)[0]) == int(all_[i]) for i in (0, 1, 63, 999))
    assert not np.array_equal(H.rng_u64(1, 3, idx), H.rng_u64(1, 4, idx))
    u = H.rng_unit(H.rng_u64(5, 8, idx))
    assert u.min() >= 0.0 and u.max() < 1.0 and H.rng_unit(np.uint64(2**64 - 1)) < 1.0
    x, v = H.draw_topology(3, 8, 64, 2000.0, False)
    assert x.min() >= 0 and x.max() <= 1999 and np.array_equal(x, np.floor(x)) and v.min() >= 1.1 and v.max() < 2.7
    assert np.array_equal(H.draw_topology(3, 8, 64, 2000.0, True)[1], np.full((8, 64), 1.7))
    a = H.draw_sample(11, 8, 64, 7)
    assert set(np.unique(a)) == set(range(7))
    assert set(np.unique(H.draw_velocity(11, 8, 64))) == {1, 2, 3}
    prev, cnt = H.draw_sps_init(2, 4096, 31)
    assert prev.min() == 0 and prev.max() == 31 and cnt.min() == 5 and cnt.max() == 15
    c, k, ch = H.draw_sps_step(2, 4096)
    assert c.min() == 5 and c.max() == 16 and k.min() >= 0 and k.max() < 1 and ch.min() >= 0 and ch.max() < 2**31
    # sharding: what a handle at env offset 3 draws is rows 3.. of the whole batch (global index); the SPS draws are
    # indexed per handle
    assert np.array_equal(H.draw_sample(11, 5, 64, 7, env_offset=3), H.draw_sample(11, 8, 64, 7)[3:])
    assert np.array_equal(H.draw_velocity(11, 5, 64, env_offset=3), H.draw_velocity(11, 8, 64)[3:])
    assert np.array_equal(H.draw_topology(3, 5, 64, 2000.0, False, env_offset=3)[0], x[3:])


@pytest.mark.parametrize("name", SPS_FIXTURES)
def test_host_sps_replays_the_reference_fixtures(name):
    """HostSps on the recorded windows and draws of the reference's own SemiPersistentScheduling objects
    (tests/golden/gen_golden.py run_sps_case): action, reselection counter and prev_action after every step."""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    A = int(g["A"])
    T, n = g["actions"].shape
    sps = H.HostSps(n, A, threshold=float(g["threshold"]), prev_action=g["init_prev"], counter=g["init_counter"])
    step = float(g["tie_step"])
    for t in range(T):
        win = g["codes"][t].astype(np.float64) * step
        got = sps.step(win, g["draw_counter"][t], g["draw_keep"][t], g["draw_choice"][t])
        assert np.array_equal(got, g["actions"][t]), (t, np.argwhere(got != g["actions"][t])[:4])
        assert np.array_equal(sps.counter, g["counters"][t]), t
        assert np.array_equal(sps.prev_action, g["prev_actions"][t]), t
    assert len(sps.log) == int(g["reselections"]) >= 40
    assert sum(r["raises"] for r in sps.log) > 0


def brute_choice(w, prev, threshold, inc_db, r):
    """choose_new_resource without a sort: the pick is the candidate that exactly `pick` candidates precede in the
    (value, subframe) order, counted pair by pair."""
    A = len(w)
    thr = threshold
    while True:
        cand = [s for s in range(A) if s != prev and w[s] < thr]
        if len(cand) >= A / 5:
            break
        thr += inc_db
    need = max(1, math.ceil(min(A / 5, len(cand))))
    pick = r % need
    hits = [s for s in cand if sum(1 for q in cand if w[q] < w[s] or (w[q] == w[s] and q < s)) == pick]
    assert len(hits) == 1
    return hits[0]


@pytest.mark.parametrize("A", [2, 5, 7])
def test_host_sps_on_exact_ties_equals_brute_force(A):
    """Every window over the three plateaus (-200 idle, -160 out of range, -60 own) plus one heard value, every previous
    action and every pick, at the thresholds that put the plateaus on either side."""
    levels = (-200.0, -160.0, -60.0, -131.5) if A < 7 else (-200.0, -160.0, -131.5)
    n = 0
    for w in itertools.product(levels, repeat=A):
        for prev in range(A):
            for thr in (-110.0, -165.0, -230.0):
                for r in range(3):
                    got, _, _ = H.choose_new_resource(list(w), prev, thr, 3.0, r)
                    assert got == brute_choice(w, prev, thr, 3.0, r), (w, prev, thr, r)
                    n += 1
    assert n == len(levels) ** A * A * 9


def test_host_sps_ties_on_wide_windows_against_brute_force():
    """A = 32, 33 and 64 (need = 7, 7, 13): random plateau windows, through HostSps.step with injected draws."""
    rng = np.random.default_rng(4)
    for A in (32, 33, 64):
        n = 200
        win = rng.choice([-200.0, -160.0, -60.0, -75.25], size=(n, A), p=[0.3, 0.3, 0.2, 0.2])
        prev = rng.integers(0, A, size=n)
        r = rng.integers(0, 1 << 20, size=n)
        for thr in (-110.0, -150.0, -165.0, -230.0):
            sps = H.HostSps(n, A, threshold=thr, prev_action=prev, counter=np.zeros(n))
            got = sps.step(win, np.full(n, 9), np.ones(n), r)
            want = [brute_choice(win[i].tolist(), int(prev[i]), thr, 3.0, int(r[i])) for i in range(n)]
            assert np.array_equal(got, want), (A, thr)
            assert len(sps.log) == n and np.array_equal(sps.counter, np.full(n, 9))


def test_window_formula_and_the_record_of_a_reselection():
    """window_from_chobs is the documented formula (own -60, out of range -160, idle -200, heard -40 - 30 log10(max(d, 1)));
    the record says shortcut / general, counts raises and measures the margin."""
    chobs = np.array([[0.0, 100000.0, 10.0, 0.5, 0.0, 6000.0, 0.0, 0.0, 0.0, 0.0]])
    w, heard = H.window_from_chobs(chobs, np.array([4]))
    assert w[0].tolist() == [-200.0, -160.0, -70.0, -40.0, -60.0, -40.0 - 30.0 * math.log10(6000.0), -200.0, -200.0, -200.0, -200.0]
    assert heard[0].tolist() == [False, False, True, True, False, True, False, False, False, False]
    kw = dict(prev_action=[4], counter=[0])
    sps = H.HostSps(1, 10, **kw)
    sps.step(chobs=chobs, actions=[4], draw_counter=[7], draw_keep=[0.99], draw_choice=[1])
    assert sps.log[0]["far"] and sps.log[0]["shortcut"] is False            # a transmitter beyond 5 km: the general path
    near = chobs.copy()
    near[0, 5] = 600.0
    sps = H.HostSps(1, 10, **kw)
    got = sps.step(chobs=near, actions=[4], draw_counter=[7], draw_keep=[0.99], draw_choice=[1])
    assert sps.log[0]["shortcut"] is True and sps.log[0]["raises"] == 0 and got[0] == 6      # need = 2: idle 0, 6
    assert sps.log[0]["margin"] == pytest.approx(40.0 + 30.0 * math.log10(600.0) - 110.0)      # 600 m against -110
    sps = H.HostSps(1, 10, threshold=-230.0, **kw)
    sps.step(chobs=near, actions=[4], draw_counter=[7], draw_keep=[0.99], draw_choice=[1])
    assert sps.log[0]["shortcut"] is False and sps.log[0]["raises"] == 11   # -230 + 33 = -197 is the first above -200
    # a heard value that sits on a threshold of the loop is ambiguous
    d = 10.0 ** ((-40.0 + 110.0) / 30.0)
    edge = np.array([[d] * 9 + [0.0]])
    sps = H.HostSps(1, 10, threshold=-110.0, prev_action=[9], counter=[0])
    sps.step(chobs=edge, actions=[9], draw_counter=[7], draw_keep=[0.99], draw_choice=[0])
    assert sps.log[0]["margin"] < 1e-9


@pytest.mark.parametrize("enable_channel", [False, True])
def test_host_prefill_equals_the_driver_loop_on_the_oracle(enable_channel):
    """HostClosedLoop.prefill against DriverLoop.prefill on the same oracle-backed env and the same actions: every state,
    the tables and the positions."""
    rich = dict(add_channel_obs=True, add_reward=True, add_index=True, add_velocity=True, add_position=True)
    cfg = bench_config(24, 6, 900.0, State=rich, reward_design=2)
    B, K, seed = 5, 7, 314
    rng = np.random.default_rng(1)
    x0 = rng.integers(0, 900, size=(B, 24)).astype(np.float64)
    v0 = rng.uniform(1.1, 2.7, size=(B, 24))
    ob = OracleBackend(cfg, batch=B, sq_mode=SQ_IEEE)
    ob.reset_topology(x0, np.zeros_like(x0), v0)
    loop = DriverLoop(ob, enable_channel=enable_channel)
    a0 = rng.integers(0, 6, size=(B, 24)).astype(np.int32)
    loop.bootstrap(a0)
    host = H.HostClosedLoop(cfg, B, x0, v0, sps=None, policy_seed=0)
    _, rew0 = host.ob.my_step(a0, 0)
    assert np.array_equal(rew0, loop._rews0.numpy())
    want_s, want_a = loop.prefill(K, seed)
    mode = "my_step_ch" if enable_channel else "my_step_design"
    got_s, got_a, nxt = host.prefill(want_a[0].numpy(), K, seed, rew_in=rew0, mode=mode, actions_all=want_a.numpy())
    assert np.array_equal(got_a, want_a.numpy()) and np.array_equal(got_s, want_s.numpy())
    assert np.array_equal(nxt, H.draw_sample(seed + K, B, 24, 6))
    e1, e2 = ob.export_state(), host.ob.export_state()
    for k in ("pos_x", "vel", "seq", "age", "x"):
        assert np.array_equal(e1[k], e2[k]), k
    assert np.array_equal(ob.o.metrics(), host.metrics())


def test_host_closed_loop_runs_and_keeps_its_own_record():
    """A short closed loop on the CPU: seeds advance as VecV2VEnv.step_policy derives them, K slots equal K one-slot
    runs, the record counts re-selections on both paths and the velocity updates of a mobility_vary config."""
    cfg = c2_config(reward_design=4, mobility_vary=True)
    B, N, A = 3, 64, 32
    x0, v0 = H.draw_topology(21, B, N, cfg.highway_length, True)

    def make():
        sps = H.HostSps.from_seed(B * N, A, 3, keep_prob=0.0)
        return H.HostClosedLoop(cfg, B, x0, v0, sps, policy_seed=3, dtype=np.float32, stuck_penalty=(2, -10.0), vel_seed=9)
    one, many = make(), make()
    a = one.sps.prev_action.reshape(B, N).copy()
    out_k = many.run(a, 20, K=16)
    for k in range(16):
        o = one.run(a, 20 + k)
        assert np.array_equal(o["shaped"][0], out_k["shaped"][k]) and o["shaped"].dtype == np.float32
        a = o["actions"]
    assert np.array_equal(a, out_k["actions"]) and one._t == many._t == 16
    assert np.array_equal(o["state"], out_k["state"]) and out_k["done"].tolist() == [0] * B
    rec = many.record()
    assert rec["reselections"] > N and rec["shortcut"] > 0 and rec["vel_changed"] > 0 and rec["left_out"] == 0
    assert torch.float32 == many.tdtype
