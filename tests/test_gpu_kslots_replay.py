"""Recorded mobility inside the K-slot launches (`diral_env_rollout_replay` / `diral_env_step_policy_replay`: the slot loop
of step_fast64_slots_kernel takes the position behind every slot from the caller's sequence and / or writes the position
log) against what it stands for: the loop of one-slot calls on a twin handle that had `load_saved_positions` with the same
sequence - bit for bit -, the CPU oracle, the host closed loop and the reference's recorded trace replay."""
import ctypes

import numpy as np
import pytest
import torch

from diral_amd.config import (ERR_BAD_ARG, ERR_UNSUPPORTED, KERNEL_CH, KERNEL_EXTRA, KERNEL_FAST64, KERNEL_POLICY,
                              STEP_MY_STEP, STEP_MY_STEP_CH, DiralRollout, DiralSlotInfoAge, DiralSlotPolicy, DiralSlotReplay,
                              bench_config, c2_config)
from diral_amd.driver import DriverLoop
from diral_amd.rollout import SlotClock, no_finalizers_during_capture
from diral_amd.search import CandidateSearch
from diral_amd.sps import SpsPolicy
from diral_amd.vec_env import DiralError, VecV2VEnv
from oracle.oracle import SQ_IEEE, Oracle
from tests import host_closed_loop as H
from tests.golden_util import Golden
from tests.oracle_compare import tables_equal
from tests.kslots_harness import (DEV, PEN_THR, VEL_SEED, assert_equal, assert_same_envs, chain_cfg, go_on_alike, slot_loop, start,
                                   stuck_penalty_state, twins)

pytestmark = pytest.mark.gpu

def _trace(rng, L, shape):
    """A recorded run [..., T, N]: a row either moves on from the one before (1 ... 3 m, wrapped) or is drawn afresh - a
    replayed file jumps where it wraps, and nothing ties a row to the velocities."""
    tr = rng.uniform(0, L, size=shape)
    for k in range(1, shape[-2]):
        smooth = rng.random(shape[:-2] + (1,)) < 0.6
        tr[..., k, :] = np.where(smooth, (tr[..., k - 1, :] + rng.uniform(1, 3, size=shape[:-2] + (shape[-1],))) % L, tr[..., k, :])
    return tr


def _launches(env, want, seq, t, plan, mode, states="all", avg=True, pen=None, positions=None, log=True, **kw):
    """The slots of `seq` as the launches of `plan` (a list of K) on `env`, every launch compared with its slots of the
    loop's result `want`."""
    k0 = 0
    for K in plan:
        got = env.rollout(seq[k0:k0 + K], t + k0, mode=mode, states=states, global_reward_avg=avg, stuck_penalty=pen,
                          vel_seed=VEL_SEED, positions=positions, log_positions=log, **kw)
        torch.cuda.synchronize()
        lk = env.last_kernel()
        assert (lk & 15) == KERNEL_FAST64 and (lk & KERNEL_POLICY) and not (lk & KERNEL_EXTRA), lk
        assert bool(lk & KERNEL_CH) == (mode == "my_step_ch")
        tag = "slots %d ... %d: " % (k0, k0 + K - 1)
        sl = slice(k0, k0 + K)
        for key in ("shaped", "sum_r", "collision") + (("xpos",) if log else ()) + tuple(k for k in ("ia", "ia_sum", "ia_penalty") if k in want):
            assert_equal(want[key][sl], got[key], tag + key)
        assert log or "xpos" not in got
        assert_equal(want["reward"][k0 + K - 1], got["reward"], tag + "reward")
        assert_equal(want["done"][k0 + K - 1], got["done"], tag + "done")
        if states is None or env.S == 0:
            assert got["states"] is None
        elif states == "all":
            assert_equal(want["states"][sl], got["states"], tag + "states")
        else:
            assert_equal(want["states"][k0 + K - 1], got["states"], tag + "states")
        assert env.t == t + k0 + K
        k0 += K
    assert k0 == seq.shape[0]


def _check(N, A, rd, mode, K, T, t0, dtype, per_env=False, states="all", vary=False, pen=False, rich=False, reps=2, B=4, seed=31):
    """`reps` launches of K slots, each continuing the one before, against the loop on a twin handle that carries the trace.
    T = 0: no sequence - the position log of the velocity model."""
    cfg = chain_cfg(N, A, rd, vary, rich)
    begin = start(cfg, B, seed)
    e_loop, e_one = twins(cfg, B, dtype, begin)
    rng = np.random.default_rng(seed + 7)
    tr = None
    if T:
        tr = torch.as_tensor(_trace(rng, cfg.highway_length, ((B,) if per_env else ()) + (T, N)), device=DEV)
        e_loop.load_saved_positions(tr)
    pens = [stuck_penalty_state(B, N) if pen else None for _ in range(2)]
    Kt = K * reps
    if pen:                                                           # agents that repeat their action: the penalty fires
        seq = e_loop.sample(7000).unsqueeze(0).expand(Kt, B, N).contiguous()
    else:
        seq = torch.stack([e_loop.sample(7000 + k) for k in range(Kt)])
    want = slot_loop(e_loop, seq, t0, mode, pen=pens[0], want_xpos=True)
    _launches(e_one, want, seq, t0, [K] * reps, mode, states=states, pen=pens[1], positions=tr)
    if T:                                                             # row (t + k) mod T, Python's sign
        rows = torch.as_tensor([(t0 + k) % T for k in range(Kt)], device=DEV)
        exp = tr[:, rows].transpose(0, 1) if per_env else tr[rows].unsqueeze(1).expand(Kt, B, N)
        assert torch.equal(want["xpos"], exp)
    assert e_loop.t == e_one.t == t0 + Kt
    s = assert_same_envs(e_loop, e_one)
    if pen:
        assert torch.equal(pens[0][2], pens[1][2]) and torch.equal(pens[0][3], pens[1][3])
        assert int(pens[1][2].max()) > PEN_THR
    if vary:
        assert not torch.equal(s["vel"], torch.full_like(s["vel"], 1.7))
    e_loop.load_saved_positions(None)
    go_on_alike(e_loop, e_one, mode, t0 + Kt)


@pytest.mark.parametrize("N,A,rd,mode,K,T,t0,dtype,per_env,states,vary,pen", [
    (8, 3, 2, "my_step", 1, 7, 5, torch.float64, False, "last", False, False),
    (8, 3, 3, "my_step_ch", 6, 1, 0, torch.float32, True, "all", False, False),
    (8, 3, 2, "my_step_ch", 30, 40, 20, torch.float32, False, None, True, True),
    (33, 9, 2, "my_step", 30, 7, 20, torch.float32, True, "all", True, False),
    (33, 9, 3, "my_step_ch", 1, 40, 1000003, torch.float64, True, "all", False, False),
    (33, 9, 2, "my_step", 12, 12, 1000003, torch.float64, False, "last", False, True),
    (33, 9, 2, "my_step_ch", 12, 7, 5, torch.float64, False, None, False, False),
    (64, 32, 2, "my_step", 30, 40, 20, torch.float64, False, "last", True, True),
    (64, 32, 3, "my_step_ch", 30, 30, 20, torch.float32, True, "last", True, False),
    (64, 32, 2, "my_step", 6, 7, 0, torch.float32, False, "all", False, False),
    (64, 5, 2, "my_step_ch", 6, 1, 5, torch.float64, False, "all", False, True),
    (64, 5, 2, "my_step", 1, 40, 0, torch.float32, True, None, False, False),
    (33, 9, 2, "my_step", 12, 0, 20, torch.float32, False, "all", True, False),
    (64, 32, 3, "my_step_ch", 30, 0, 20, torch.float64, False, "last", True, True),
])
def test_launch_with_recorded_positions_equals_the_loop_on_a_handle_with_the_trace(N, A, rd, mode, K, T, t0, dtype, per_env,
                                                                                   states, vary, pen):
    """N = 8 / 33 / 64, both dtypes, my_step and my_step_ch (reward_design 2, 3), states last / all / none, shared and per-env
    sequences, T = 1, 7 (wraps inside the launch), K and 40, t = 0, 5, 20 and 1 000 003, mobility_vary with K = 30 from 20 - an
    episode end inside the launch (24) and one on its last slot (49) -, the stuck-action penalty, K = 1; every launch
    followed by another.  T = 0: the position log alone, of the velocity model.  The log is compared slot by slot with
    get_x_pos() of the loop in every case."""
    _check(N, A, rd, mode, K, T, t0, dtype, per_env=per_env, states=states, vary=vary, pen=pen, reps=3 if K == 1 else 2)


def test_rich_state_columns_show_the_velocities_while_the_positions_are_replayed():
    """The velocity column keeps reporting the drawn velocities (mobility_vary: redrawn at the episode end inside the
    launch), the position column the recorded positions."""
    _check(33, 9, 2, "my_step", 30, 7, 20, torch.float64, states="all", vary=True, rich=True)
    _check(33, 9, 2, "my_step_ch", 6, 40, 22, torch.float32, per_env=True, states="last", vary=True, rich=True)


# ---- 2: the closed loop ------------------------------------------------------------------------------------------------
def _policy(B, N, A, seed=3):
    pol = SpsPolicy(B, N, A, rssi_threshold=-110.0, device=DEV, seed=seed)
    pol.keep_prob = 0.8
    pol.counter.remainder_(4)                                         # re-selections in every launch
    return pol


@pytest.mark.parametrize("mode,dtype,per_env,vary", [
    (STEP_MY_STEP, torch.float32, False, True),
    (STEP_MY_STEP, torch.float64, True, False),
    (STEP_MY_STEP_CH, torch.float64, False, True),
    (STEP_MY_STEP_CH, torch.float32, True, False),
])
def test_closed_loop_with_recorded_positions_equals_the_one_slot_calls(mode, dtype, per_env, vary):
    """`step_policy(slots=K, positions=)` = K three-launch `step_policy` calls on a twin that carries the trace: the per-slot
    outputs, the last slot's state / reward / done, the next actions, the SPS state, the position log, the envs."""
    N, A, B, K, T, t0 = 33, 9, 5, 12, 7, 20
    cfg = chain_cfg(N, A, 2, vary, rich=True)
    begin = start(cfg, B, 17)
    e_loop, e_one = twins(cfg, B, dtype, begin)
    tr = torch.as_tensor(_trace(np.random.default_rng(4), cfg.highway_length, ((B,) if per_env else ()) + (T, N)), device=DEV)
    e_loop.load_saved_positions(tr)
    p1, p2 = _policy(B, N, A), _policy(B, N, A)
    pn1, pn2 = stuck_penalty_state(B, N), stuck_penalty_state(B, N)
    o = dict(dtype=dtype, device=DEV)
    EI = cfg.episode_interval
    t = t0
    for rep in range(2):
        a = p1.prev_action.clone()
        sh1, sr1, co1 = torch.zeros((K, B, N), **o), torch.zeros((K, B), **o), torch.zeros((K, B), **o)
        xp1 = torch.zeros((K, B, N), dtype=torch.float64, device=DEV)
        cur, nxt = a.clone(), torch.empty_like(a)
        for k in range(K):
            obs1, rew1, done1 = e_loop.step_policy(cur, t + k, p1, nxt, shaped_out=sh1[k], sum_r_out=sr1[k], collision_out=co1[k],
                                                   mode=mode, stuck_penalty=pn1, want_chobs=True)
            assert not (e_loop.last_kernel() & KERNEL_POLICY)
            xp1[k] = e_loop.get_x_pos()
            if vary and (t + k) % EI == EI - 1:
                e_loop.update_velocity(seed=VEL_SEED + (t + k) // EI)
            cur, nxt = nxt, cur
        sh2, sr2, co2 = torch.zeros((K, B, N), **o), torch.zeros((K, B), **o), torch.zeros((K, B), **o)
        xp2 = torch.zeros((K, B, N), dtype=torch.float64, device=DEV)
        out2 = torch.empty_like(a)
        obs2, rew2, done2 = e_one.step_policy(a, t, p2, out2, shaped_out=sh2, sum_r_out=sr2, collision_out=co2, mode=mode,
                                              slots=K, vel_seed=VEL_SEED, stuck_penalty=pn2, want_chobs=True, positions=tr,
                                              xpos_out=xp2)
        torch.cuda.synchronize()
        lk = e_one.last_kernel()
        assert (lk & KERNEL_POLICY) and (lk & 15) == KERNEL_FAST64 and not (lk & KERNEL_EXTRA), lk
        for name, x, y in (("shaped", sh1, sh2), ("sum_r", sr1, sr2), ("collision", co1, co2), ("xpos", xp1, xp2),
                           ("state", obs1, obs2), ("reward", rew1, rew2), ("done", done1, done2), ("actions_out", cur, out2),
                           ("chobs", e_loop._chobs, e_one._chobs), ("prev_action", p1.prev_action, p2.prev_action),
                           ("counter", p1.counter, p2.counter), ("pen_counter", pn1[2], pn2[2]), ("pen_prev", pn1[3], pn2[3])):
            assert_equal(x, y, (rep, name))
        assert p1._t == p2._t
        t += K
    assert_same_envs(e_loop, e_one)
    e_loop.check(); e_one.check()


@pytest.mark.parametrize("mode", [STEP_MY_STEP, STEP_MY_STEP_CH])
def test_closed_loop_with_recorded_positions_against_the_host_loop(mode):
    """... and against tests/host_closed_loop.HostClosedLoop on an OracleBackend that had load_saved_positions (a shared
    trace): CPU oracle step, the shaping in NumPy's order, the SPS agent on the host."""
    from tests.host_closed_loop import MODE_NAME, _eq as eq
    N, A, B, T = 33, 9, 6, 7
    plan = [12, 9]
    cfg = chain_cfg(N, A, 2, vary=True, rich=True)
    x0, v0 = H.draw_topology(21, B, N, cfg.highway_length, True, 0)
    tr = _trace(np.random.default_rng(9), cfg.highway_length, (T, N))
    sps = H.HostSps.from_seed(B * N, A, 3, threshold=-110.0, keep_prob=0.8)
    sps.counter %= 4
    host = H.HostClosedLoop(cfg, B, x0, v0, sps, 3, mode=MODE_NAME[mode], dtype=np.float64, stuck_penalty=(2, -10.0), vel_seed=VEL_SEED)
    host.ob.load_saved_positions(tr)
    env = VecV2VEnv(cfg, batch=B, device=DEV, out_dtype=torch.float64)
    env.reset_topology(x0, None, v0)
    pol = _policy(B, N, A)
    pn = stuck_penalty_state(B, N)
    trd = torch.as_tensor(tr, device=DEV)
    a, nxt, t = pol.prev_action.clone(), torch.empty_like(pol.prev_action), 20
    ha = sps.prev_action.reshape(B, N).copy()
    host._t = 0
    for K in plan:
        o = host.run(ha, t, K)
        sh, sr, co = (torch.zeros(s, dtype=torch.float64, device=DEV) for s in ((K, B, N), (K, B), (K, B)))
        xp = torch.zeros((K, B, N), dtype=torch.float64, device=DEV)
        env.step_policy(a, t, pol, nxt, shaped_out=sh, sum_r_out=sr, collision_out=co, slots=K, vel_seed=VEL_SEED, mode=mode,
                        want_chobs=True, stuck_penalty=pn, positions=trd, xpos_out=xp)
        torch.cuda.synchronize()
        assert env.last_kernel() & KERNEL_POLICY
        keep = ~host.left_out
        tag = "K = %d, t = %d: " % (K, t)
        eq(tag + "shaped", sh, o["shaped"], keep, 1); eq(tag + "sum_r", sr, o["sum_r"], keep, 1); eq(tag + "coll", co, o["coll"], keep, 1)
        eq(tag + "reward", env._rew, o["rew"], keep); eq(tag + "done", env._done, o["done"], keep)
        eq(tag + "state", env._obs, o["state"], keep); eq(tag + "chobs", env._chobs, o["chobs"], keep)
        eq(tag + "actions_out", nxt, o["actions"], keep)
        eq(tag + "prev_action", pol.prev_action, sps.prev_action.reshape(B, N), keep)
        eq(tag + "counter", pol.counter, sps.counter.reshape(B, N), keep)
        eq(tag + "pen", pn[2], host.pen_counter, keep)
        rows = [(t + k) % T for k in range(K)]
        assert np.array_equal(xp.cpu().numpy(), np.broadcast_to(tr[rows][:, None, :], (K, B, N)))
        ha, t = o["actions"], t + K
        a, nxt = nxt, a
    rec = host.record()
    assert rec["left_out"] == 0 and rec["reselections"] > 3 * N and rec["vel_changed"] > 0, rec
    st, he = env.export_state(), host.export_state()
    for k in ("pos_x", "vel", "seq", "age", "x"):
        eq("export_state " + k, st[k], he[k], keep)
    env.check()


# ---- 3: the information-age block next to the replay block ---------------------------------------------------------------
@pytest.mark.parametrize("N,A,dtype,K,T,per_env,avg_term", [
    (33, 9, torch.float32, 30, 7, False, True),
    (64, 32, torch.float64, 12, 40, True, True),
    (8, 3, torch.float64, 6, 6, True, False),
])
def test_information_age_block_with_recorded_positions(N, A, dtype, K, T, per_env, avg_term):
    """A tracking handle: stamps, histograms, sums, the ia_averaging term and the caller's sum_ia_prev of a launch that
    replays positions = the loop of my_step_ch + info_age + diral_driver_shape on the twin with the trace."""
    B, t0 = 4, 20
    cfg = chain_cfg(N, A, 2, vary=True, track=True)
    begin = start(cfg, B, 5)
    e_loop, e_one = twins(cfg, B, dtype, begin)
    tr = torch.as_tensor(_trace(np.random.default_rng(6), cfg.highway_length, ((B,) if per_env else ()) + (T, N)), device=DEV)
    e_loop.load_saved_positions(tr)
    prevs = [torch.zeros((B,), dtype=torch.int64, device=DEV) if avg_term else None for _ in range(2)]
    pens = [stuck_penalty_state(B, N), stuck_penalty_state(B, N)]
    seq = torch.stack([e_loop.sample(7000 + k // 3) for k in range(2 * K)])      # (every action held for three slots)
    want = slot_loop(e_loop, seq, t0, "my_step_ch", pen=pens[0], ia_prev=prevs[0], want_ia=True, want_xpos=True)
    _launches(e_one, want, seq, t0, [K, K], "my_step_ch", states="all", pen=pens[1], positions=tr, info_age=True,
              sum_ia_prev=prevs[1])
    if avg_term:
        assert torch.equal(prevs[0], prevs[1]) and torch.equal(prevs[0], want["ia_sum"][-1])
        assert len(set(want["ia_penalty"].unique().tolist())) >= 2
    s = assert_same_envs(e_loop, e_one)
    la = s["la"].cpu().numpy()
    off = ~np.eye(N, dtype=bool)[None]
    assert ((la == -1) & off).any() and ((la >= t0 + K) & off).any()
    assert int((want["ia"].sum(1) > 0).sum(-1).max()) >= 3
    for k in range(2):
        assert torch.equal(e_loop.info_age(t0 + 2 * K + k), e_one.info_age(t0 + 2 * K + k))
    e_loop.load_saved_positions(None)
    go_on_alike(e_loop, e_one, "my_step_ch", t0 + 2 * K)


# ---- 4: the CPU oracle, one per env; the reference's own recording ---------------------------------------------------------
def test_per_env_sequences_against_one_oracle_per_env():
    """As test_per_env_trace_replay_vs_oracle: every env against an oracle of its own that replays the env's sequence - the
    slots 0 ... 13, 40, 41 and 5 as the launches [0, 14), [40, 42) and [5, 6)."""
    cfg = bench_config(20, 6, 800.0, communication_range=200.0)
    B, N, A, T = 4, 20, 6, 9
    rng = np.random.default_rng(33)
    x0 = rng.integers(0, 800, size=(B, N)).astype(np.float64)
    v0 = rng.uniform(1.1, 2.7, size=(B, N))
    traces = rng.uniform(0, 800, size=(B, T, N))
    env = VecV2VEnv(cfg, batch=B, device=DEV, out_dtype=torch.float64)
    env.reset_topology(x0, None, v0)
    trd = torch.as_tensor(traces, device=DEV)
    orcs = [Oracle(cfg, batch=1, sq_mode=SQ_IEEE) for _ in range(B)]
    for b, o in enumerate(orcs):
        o.reset(x0[b:b + 1], np.zeros((1, N)), v0[b:b + 1])
        o.set_trace(traces[b])
    for t0, K in ((0, 14), (40, 2), (5, 1)):
        a = rng.integers(0, A, size=(K, B, N)).astype(np.int32)
        got = env.rollout(torch.as_tensor(a, device=DEV), t0, states="all", positions=trd, log_positions=True)
        torch.cuda.synchronize()
        assert env.last_kernel() & KERNEL_POLICY
        st, sh, xp = got["states"].cpu().numpy(), got["shaped"].cpu().numpy(), got["xpos"].cpu().numpy()
        for k in range(K):
            for b, o in enumerate(orcs):
                o_rew, o_chobs = o.step(STEP_MY_STEP, a[k, b:b + 1], t0 + k)
                assert np.array_equal(st[k, b], o.obtain_state(a[k, b:b + 1], o_chobs, o_rew)[0]), (t0, k, b)
                assert np.array_equal(sh[k, b], o_rew[0])
                assert np.array_equal(xp[k, b], o.export()["pos_x"][0]) and np.array_equal(xp[k, b], traces[b, (t0 + k) % T])
    st = {k: v.cpu().numpy() for k, v in env.export_state().items()}
    for b, o in enumerate(orcs):
        tables_equal({k: v[b] for k, v in st.items()}, {k: v[0] for k, v in o.export().items()}, b)
    env.check()


def test_reference_recording_of_a_trace_replay_with_every_run_of_slots_as_one_launch():
    """tests/golden/g9_trace_replay.npz, recorded from the reference: from the slot behind which it loaded the positions,
    each maximal run of consecutive slot numbers of one mode is ONE launch that carries the trace - its slot list jumps
    7 -> 13 -> 20 -> 3, so K = 1 launches occur -; rewards, state vectors, positions and the table checkpoints are the
    reference's."""
    g = Golden("g9_trace_replay")
    cfg = g.cfg.replace(track_arrival=False)                        # (a tracking handle needs the information-age block)
    B = 3
    env = VecV2VEnv(cfg, batch=B, device=DEV, out_dtype=torch.float64)
    env.reset_topology(g["x0"], g["y0"], g["v0"])
    steps = list(g.steps())
    assert not g.vel_updates and g.trace is not None
    trd = torch.as_tensor(g.trace, device=DEV)
    ck = g.table_checkpoints()

    def tables(i):
        if i in ck:
            st = env.export_state()
            for b in range(B):
                assert np.array_equal(st["seq"][b].cpu().numpy(), g["tab_seq"][ck[i]]), i
                assert np.array_equal(st["x"][b].cpu().numpy(), g["tab_x"][ck[i]]), i
                assert np.array_equal(st["age"][b].cpu().numpy(), np.minimum(g["tab_age"][ck[i]], 255)), i
    i, runs = 0, []
    while i <= g.trace_after:                                        # the velocity model, one slot a call
        _, mode, acts, t, _ = steps[i]
        env._step(mode, env._actions(acts), t)
        assert np.array_equal(env.get_x_pos()[0].cpu().numpy(), np.asarray(g.out("pos_x", i)).reshape(-1))
        tables(i)
        i += 1
    while i < len(steps):
        j = i
        while j + 1 < len(steps) and steps[j + 1][1] == steps[j][1] and steps[j + 1][3] == steps[j][3] + 1:
            j += 1
        K = j - i + 1
        mode = steps[i][1]
        seq = torch.as_tensor(np.stack([steps[k][2] for k in range(i, j + 1)]).astype(np.int32), device=DEV)
        seq = seq.reshape(K, 1, g.N).expand(K, B, g.N).contiguous()
        got = env.rollout(seq, steps[i][3], mode="my_step_ch" if mode == STEP_MY_STEP_CH else "my_step", states="all",
                          positions=trd, log_positions=True)
        torch.cuda.synchronize()
        assert env.last_kernel() & KERNEL_POLICY
        runs.append(K)
        for k in range(K):
            ref_px = np.asarray(g.out("pos_x", i + k)).reshape(-1)
            for b in range(B):
                rew, obs = got["shaped"][k, b].cpu().numpy(), got["states"][k, b].cpu().numpy()
                assert np.array_equal(rew, np.asarray(g.out("rews", i + k)).reshape(-1)), (i + k, b)
                assert np.array_equal(obs, np.asarray(g.out("state", i + k)).reshape(obs.shape)), (i + k, b)
                assert np.array_equal(got["xpos"][k, b].cpu().numpy(), ref_px), (i + k, b)
        tables(j)
        i = j + 1
    assert runs == [5, 1, 1, 1, 4], runs
    env.check()


# ---- 5: positions the velocity model never produces ------------------------------------------------------------------------
@pytest.mark.parametrize("mode,dtype", [("my_step", torch.float32), ("my_step", torch.float64), ("my_step_ch", torch.float32),
                                        ("my_step_ch", torch.float64)])
def test_recorded_positions_outside_what_the_velocity_model_produces(mode, dtype):
    """Negative and beyond L; 3e6, beyond the range the float32 screening is bounded for; 1e-160, 5e-324 and -0.0, where the
    per-env shortcut of P1's distance is off; exact duplicates (distance 0, first-index ties); pairs exactly Rc apart - each
    in some slots and not in the others, in different slots for different envs, as one launch and split so that a special
    row is slot 0 of a launch: a decision taken once per launch instead of once per slot shows."""
    N, A, B, L, Rc = 16, 4, 4, 500.0, 120.0
    cfg = chain_cfg(N, A, 2, L=L, Rc=Rc, rich=True)
    rng = np.random.default_rng(77)
    T = 14
    base = np.sort(rng.uniform(0, L, size=(T, N)), axis=1)
    rows = {
        2: {0: -37.5, 1: -1000.0, 14: L + 10.0, 15: 2 * L, 7: L},
        4: {3: 3e6, 4: -3e6, 5: 3e6},
        6: {0: 1e-160, 1: 5e-324, 2: -0.0, 3: 0.0, 4: 2e-160, 5: -1e-160},
        8: {0: 100.0, 1: 100.0, 2: 100.0, 3: 100.0, 4: 250.0, 5: 250.0},
        9: {0: 50.0, 1: 50.0 + Rc, 2: 50.0 + 2 * Rc, 3: 50.0 - Rc},
        11: {u: 1e-160 * (u + 1) for u in range(N)},
        12: {0: 1e-300, 1: 3e6, 2: -0.0, 3: 120.0, 4: 0.0, 5: 120.0},
    }
    tr = np.broadcast_to(base, (B, T, N)).copy()
    for b in range(B):                                                # env b meets special row r in slot r + b
        for r, vals in rows.items():
            for u, x in vals.items():
                tr[b, (r + b) % T, u] = x
    trd = torch.as_tensor(tr, device=DEV)
    begin = (np.broadcast_to(base[0], (B, N)).copy(), np.full((B, N), 1.7))
    e_loop, e_one, e_split = twins(cfg, B, dtype, begin, n=3)
    e_loop.load_saved_positions(trd)
    seq = torch.stack([e_loop.sample(7000 + k) for k in range(2 * T)])
    want = slot_loop(e_loop, seq, 0, mode, want_xpos=True)
    assert torch.equal(want["xpos"][:T].transpose(0, 1), trd)       # (bit patterns too: -0.0 == 0.0 for torch.equal ...)
    assert bool((torch.signbit(want["xpos"]) & (want["xpos"] == 0)).any())
    _launches(e_one, want, seq, 0, [2 * T], mode, positions=trd)
    assert torch.equal(torch.signbit(e_one.get_x_pos()), torch.signbit(e_loop.get_x_pos()))
    _launches(e_split, want, seq, 0, [2, 2, 2, 2, 1, 2, 1, 2, 2, 12], mode, positions=trd)
    assert_same_envs(e_loop, e_one)
    assert_same_envs(e_loop, e_split)
    e_loop.load_saved_positions(None)
    go_on_alike(e_loop, e_one, mode, 2 * T)


# ---- 6: keyed quads --------------------------------------------------------------------------------------------------------
def test_a_highway_that_splits_and_merges_again_inside_the_trace():
    """N = 33, A = 8, L = 2000, Rc = 250: rows 0-9 and 22-29 one platoon in [0, 200], rows 10-21 seventeen vehicles there and
    sixteen in [1200, 1400] - entries about the other half fall beyond the codes while the halves are apart (the quads
    take their keyed form) and come back behind the merge.  One K = 30 launch, and [0, 18) + [18, 30): the second launch
    starts on flagged quads."""
    N, A, L, B = 33, 8, 2000.0, 4
    cfg = bench_config(N, A, L, communication_range=250.0)
    rng = np.random.default_rng(5)
    tr = np.empty((30, N))
    for r in range(30):
        if 10 <= r <= 21:
            tr[r] = np.concatenate([np.sort(rng.uniform(0, 200, 17)), np.sort(rng.uniform(1200, 1400, 16))])
        else:
            tr[r] = np.sort(rng.uniform(0, 200, N))
    trd = torch.as_tensor(tr, device=DEV)
    begin = (np.broadcast_to(tr[29], (B, N)).copy(), np.full((B, N), 1.7))
    for dtype in (torch.float32, torch.float64):
        e_loop, e_one, e_split = twins(cfg, B, dtype, begin, n=3)
        e_loop.load_saved_positions(trd)
        seq = torch.stack([e_loop.sample(7000 + k) for k in range(30)])
        far = {}

        def behind_17(env):
            s = env.export_state()
            own = torch.diagonal(s["seq"], dim1=1, dim2=2).unsqueeze(1)
            far[17] = int(((own - s["seq"] >= 8) & (s["seq"] > 0)).sum())
        want = slot_loop(e_loop, seq, 0, "my_step", stop=(17, behind_17), want_xpos=True)
        print("entries beyond the codes behind slot 17:", far[17])
        assert far[17] >= 1, "no entry with seq > 0 lags its subject by 8 or more"
        _launches(e_one, want, seq, 0, [30], "my_step", positions=trd)
        _launches(e_split, want, seq, 0, [18, 12], "my_step", positions=trd)
        s = assert_same_envs(e_loop, e_one)
        assert_same_envs(e_loop, e_split)
        own = torch.diagonal(s["seq"], dim1=1, dim2=2).unsqueeze(1)
        assert not bool(((own - s["seq"] >= 8) & (s["seq"] > 0)).any())        # behind the merge everything is within the codes
        e_loop.load_saved_positions(None)
        go_on_alike(e_loop, e_one, "my_step", 30)


# ---- 7: the position log replays its launch ----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,dtype", [("my_step", torch.float32), ("my_step_ch", torch.float64)])
def test_the_log_of_a_velocity_model_launch_replays_it(mode, dtype):
    """K = 25 from t = 0 with mobility_vary (the episode end on the last slot): the log, handed back as per-env positions
    with T = K on a fresh env from the same x0 / v0 and the same actions, leaves the same states, rewards, tables,
    velocities and positions."""
    N, A, B, K = 33, 9, 5, 25
    cfg = chain_cfg(N, A, 2, vary=True, rich=True)
    begin = start(cfg, B, 3)
    e_rec, e_rep = twins(cfg, B, dtype, begin)
    seq = torch.stack([e_rec.sample(7000 + k) for k in range(K)])
    rec = e_rec.rollout(seq, 0, mode=mode, states="all", global_reward_avg=True, vel_seed=VEL_SEED, log_positions=True)
    pos = rec["xpos"].transpose(0, 1).contiguous()                  # [B, T = K, N]
    rep = e_rep.rollout(seq, 0, mode=mode, states="all", global_reward_avg=True, vel_seed=VEL_SEED, positions=pos, log_positions=True)
    torch.cuda.synchronize()
    for key in ("states", "reward", "done", "shaped", "sum_r", "collision", "xpos"):
        assert_equal(rec[key], rep[key], key)
    assert int(rec["done"].min()) == 1
    s = assert_same_envs(e_rec, e_rep)
    assert torch.equal(s["pos_x"], rec["xpos"][-1]) and not torch.equal(s["vel"], torch.full_like(s["vel"], 1.7))
    e_rec.check(); e_rep.check()


# ---- 8: capture --------------------------------------------------------------------------------------------------------------
def test_captured_launch_follows_the_slot_clock():
    """One `rollout(positions=)` with t = 0 on a handle with a slot clock, captured and replayed twice: the row of the
    sequence follows the clock, as in the eager calls on a twin."""
    N, A, B, K, T = 33, 9, 4, 6, 7
    cfg = chain_cfg(N, A, 2, vary=True)
    begin = start(cfg, B, 8)
    e_cap, e_eag = twins(cfg, B, torch.float32, begin)
    tr = torch.as_tensor(_trace(np.random.default_rng(2), cfg.highway_length, (B, T, N)), device=DEV)
    seq = torch.stack([e_cap.sample(7000 + k) for k in range(K)])
    clk = SlotClock(DEV, 0)
    e_cap.set_clock(clk.t)
    kw = dict(mode="my_step", states="all", global_reward_avg=True, vel_seed=VEL_SEED, positions=tr, log_positions=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    wants = []
    with torch.cuda.stream(s):                                       # eager first: slots [0, K) at clock 0
        first = {k: v.clone() for k, v in e_cap.rollout(seq, 0, **kw).items()}
        e_cap.lib.diral_clock_add(clk.ptr(), K, e_cap._stream())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with no_finalizers_during_capture():
        with torch.cuda.graph(g, stream=s):
            out = e_cap.rollout(seq, 0, **kw)
            e_cap.lib.diral_clock_add(clk.ptr(), K, e_cap._stream())
    for rep in range(3):
        wants.append({k: v.clone() for k, v in e_eag.rollout(seq, rep * K, **kw).items()})
    for key in first:
        assert_equal(wants[0][key], first[key], ("eager", key))
    for rep in (1, 2):
        g.replay()
        torch.cuda.synchronize()
        for key in out:
            assert_equal(wants[rep][key], out[key], (rep, key))
    assert clk.value() == 3 * K
    rows = torch.as_tensor([(2 * K + k) % T for k in range(K)], device=DEV)
    assert torch.equal(out["xpos"], tr[:, rows].transpose(0, 1))
    s1, s2 = e_cap.export_state(), e_eag.export_state()
    for key in s1:
        assert torch.equal(s1[key], s2[key]), key
    e_cap.check(); e_eag.check()


# ---- 9: refusals and argument errors -----------------------------------------------------------------------------------------
def _refusals():
    b = dict(reward_design=2)
    return [
        ("handle_trace", c2_config(), {}),
        ("n_7", bench_config(7, 3, 400.0, **b), {}),
        ("n_128", bench_config(128, 32, 1700.0, **b), {}),
        ("off_lane", c2_config(), {}),
        ("prr", c2_config(track_prr=True), {}),
        ("static", c2_config(mobility=False, enable_design_topology=True), {}),
        ("piggybacking", bench_config(32, 8, 1400.0, State=dict(piggybacking=True, add_channel_obs=True), **b), {}),
        ("sorted_distances", c2_config(State=dict(add_positional_dist=True)), {}),
    ]


@pytest.mark.parametrize("name,cfg,kw", _refusals(), ids=[r[0] for r in _refusals()])
def test_refusals_leave_the_env_untouched_and_the_driver_loops_with_the_trace(name, cfg, kw):
    """A handle trace next to the block, N = 7, N = 128, vehicles off the lane, PRR tracking, a static topology,
    State.piggybacking, a secondary observation mode behind a state vector: DIRAL_ERR_UNSUPPORTED with export_state(), the
    metrics and the slot counter unchanged - with a sequence, with the log alone, and for the closed loop.
    `DriverLoop.rollout(positions=)` then returns the loop's result and leaves no trace on the handle."""
    B, K, T = 4, 4, 5
    N, A = cfg.num_users, cfg.num_channels
    rng = np.random.default_rng(1)
    x_off, y_off = rng.integers(0, 1700, size=(B, N)).astype(np.float64), rng.uniform(0, 5, size=(B, N))
    envs = []
    for _ in range(2):
        env = VecV2VEnv(cfg, batch=B, device=DEV)
        if name == "off_lane":
            env.reset_topology(x_off, y_off, np.full((B, N), 1.7))
        elif name == "piggybacking":
            env.reset_topology(np.arange(N, dtype=np.float64)[None].repeat(B, 0) * 3.0, 0.0, np.full((B, N), 1.7))
        else:
            env.reset_topology(seed=2)
        envs.append(env)
    e1, e2 = envs
    own = torch.as_tensor(np.random.default_rng(2).uniform(0, cfg.highway_length, size=(10, N)), device=DEV)
    if name == "piggybacking":                                      # (everybody stays within range of everybody)
        tr = torch.as_tensor(np.sort(np.random.default_rng(4).uniform(0, 90, size=(T, N)), axis=1), device=DEV)
    else:
        tr = torch.as_tensor(_trace(np.random.default_rng(4), cfg.highway_length, (T, N)), device=DEV)
    if name == "handle_trace":
        e2.load_saved_positions(own)
    seq = torch.stack([e1.sample(60 + k) for k in range(K)])
    before = {k: v.clone() for k, v in e2.export_state().items()}
    m0 = e2.metrics().clone()
    pol = SpsPolicy(B, N, A, device=DEV, seed=3)
    pol0 = (pol.prev_action.clone(), pol.counter.clone())
    calls = [lambda: e2.rollout(seq, 0, positions=tr, **kw), lambda: e2.rollout(seq, 0, log_positions=True, **kw),
             lambda: e2.rollout(seq, 0, positions=tr, log_positions=True, states="all", **kw)]
    if name != "sorted_distances":                                  # (the closed loop builds that state vector behind its launch)
        calls.append(lambda: e2.step_policy(seq[0], 0, pol, torch.empty_like(seq[0]), slots=K, positions=tr))
    for call in calls:
        with pytest.raises(DiralError) as ei:
            call()
        assert ei.value.status == ERR_UNSUPPORTED, (name, str(ei.value))
    torch.cuda.synchronize()
    after = e2.export_state()
    for k in before:
        assert torch.equal(before[k], after[k]), (name, k)
    assert torch.equal(m0, e2.metrics()) and e2.t == 0
    assert torch.equal(pol.prev_action, pol0[0]) and torch.equal(pol.counter, pol0[1]) and pol._t == 0
    l1, l2 = (DriverLoop(e, global_reward_avg=True) for e in (e1, e2))
    if name == "handle_trace":
        with pytest.raises(ValueError):
            l2.rollout(seq, 0, positions=tr)
        assert e2.has_trace
        return
    got = l2.rollout(seq, 0, states="last", vel_seed=VEL_SEED, positions=tr)
    assert not (e2.last_kernel() & KERNEL_POLICY) and not e2.has_trace
    e1.load_saved_positions(tr)
    for k in range(K):
        out = l1.slot(seq[k], k)
        assert torch.equal(got["shaped"][k], out["reward"]) and torch.equal(got["sum_r"][k], out["sum_r"])
    assert torch.equal(got["states"], out["next_state"]) and torch.equal(got["reward"], out["raw_reward"])
    e1.load_saved_positions(None)
    # no trace is left on the handle: both go on with the velocity model, alike
    for k in range(2):
        a = e1.sample(900 + k)
        o1, r1, _ = e1.step(a, K + k)
        o2, r2, _ = e2.step(a, K + k)
        assert torch.equal(o1, o2) and torch.equal(r1, r2)
    s1, s2 = e1.export_state(), e2.export_state()
    for k in s1:
        assert torch.equal(s1[k], s2[k]), (name, k)
    if name not in ("static",):
        assert not torch.equal(s2["pos_x"], tr[(K - 1) % T].expand(B, N))
    e1.check(); e2.check()


def test_one_slot_closed_loop_call_is_refused_and_the_driver_takes_the_launch_where_it_can():
    cfg = chain_cfg(33, 9, 2, vary=True)
    B, N, A, K, T = 4, 33, 9, 6, 7
    begin = start(cfg, B, 2)
    e1, e2 = twins(cfg, B, torch.float32, begin)
    tr = torch.as_tensor(_trace(np.random.default_rng(4), cfg.highway_length, (B, T, N)), device=DEV)
    pol = SpsPolicy(B, N, A, device=DEV, seed=3)
    a = pol.prev_action.clone()
    before = {k: v.clone() for k, v in e2.export_state().items()}
    xo = torch.empty((1, B, N), dtype=torch.float64, device=DEV)
    for kw in (dict(positions=tr), dict(xpos_out=xo), dict(positions=tr, want_chobs=True)):
        with pytest.raises(DiralError) as ei:
            e2.step_policy(a, 0, pol, torch.empty_like(a), slots=1, **kw)
        assert ei.value.status == ERR_UNSUPPORTED
    after = e2.export_state()
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert pol._t == 0
    # DriverLoop.rollout(positions=): the launch, equal to slot() on a handle with the trace
    l1, l2 = (DriverLoop(e, global_reward_avg=True) for e in (e1, e2))
    seq = torch.stack([e1.sample(60 + k) for k in range(K)])
    got = l2.rollout(seq, 22, states="all", vel_seed=VEL_SEED, positions=tr)
    assert (e2.last_kernel() & KERNEL_POLICY) and not e2.has_trace
    e1.load_saved_positions(tr)
    for k in range(K):
        out = l1.slot(seq[k], 22 + k)
        assert torch.equal(got["shaped"][k], out["reward"]) and torch.equal(got["states"][k], out["next_state"]), k
        if out["episode_end"]:
            e1.update_velocity(seed=VEL_SEED + (22 + k) // 25)
    assert torch.equal(e1.get_x_pos(), e2.get_x_pos()) and torch.equal(e1.export_state()["vel"], e2.export_state()["vel"])


def test_argument_errors_and_the_null_block():
    cfg = chain_cfg(33, 9, 2)
    B, N, K = 2, 33, 3
    begin = start(cfg, B, 1)
    env, twin = twins(cfg, B, torch.float32, begin)
    seq = torch.stack([env.sample(k) for k in range(K)])
    o = dict(dtype=torch.float32, device=DEV)
    out, rew = torch.empty((K, B, N), **o), torch.empty((B, N), **o)
    tr = torch.as_tensor(_trace(np.random.default_rng(4), cfg.highway_length, (5, N)), device=DEV)
    xo = torch.empty((K, B, N), dtype=torch.float64, device=DEV)
    ro = DiralRollout(); ro.struct_bytes = ctypes.sizeof(DiralRollout); ro.shaped_out = out.data_ptr()
    rp = DiralSlotReplay(); rp.struct_bytes = ctypes.sizeof(DiralSlotReplay)
    ia = DiralSlotInfoAge(); ia.struct_bytes = ctypes.sizeof(DiralSlotInfoAge)
    pol = SpsPolicy(B, N, cfg.num_channels, device=DEV, seed=3)
    nxt = torch.empty_like(pol.prev_action)
    q = DiralSlotPolicy(); q.struct_bytes = ctypes.sizeof(DiralSlotPolicy)
    q.sps_prev_action, q.sps_counter, q.actions_out, q.slots = pol.prev_action.data_ptr(), pol.counter.data_ptr(), nxt.data_ptr(), K
    q.rssi_threshold, q.inc_db, q.keep_prob = -110.0, 3.0, 0.8

    def roll(r=rp, i=None, h=env):
        return h.lib.diral_env_rollout_replay(h._h, STEP_MY_STEP, seq.data_ptr(), K, 0, None, 0, rew.data_ptr(), None, 0, ctypes.byref(ro),
                                              None if i is None else ctypes.byref(i), None if r is None else ctypes.byref(r), None)

    def step(r=rp):
        return env.lib.diral_env_step_policy_replay(env._h, STEP_MY_STEP, seq[0].data_ptr(), 0, None, rew.data_ptr(), None, None, 0,
                                                    ctypes.byref(q), None, ctypes.byref(r), None)
    m0 = env.metrics().clone()
    for setup in (lambda: setattr(rp, "struct_bytes", 24), lambda: setattr(rp, "flags", 1),
                  lambda: (setattr(rp, "x_positions", tr.data_ptr()), setattr(rp, "T", 0)),
                  lambda: (setattr(rp, "x_positions", tr.data_ptr()), setattr(rp, "T", -3)),
                  lambda: setattr(rp, "T", 5),                                  # rows without a sequence
                  lambda: (setattr(rp, "xpos_out", xo.data_ptr()), setattr(rp, "T", 2))):
        rp.struct_bytes, rp.flags, rp.x_positions, rp.T, rp.per_env, rp.xpos_out = ctypes.sizeof(DiralSlotReplay), 0, None, 0, 0, None
        setup()
        assert roll() == ERR_BAD_ARG and step() == ERR_BAD_ARG
    rp.struct_bytes, rp.flags, rp.x_positions, rp.T, rp.per_env, rp.xpos_out = ctypes.sizeof(DiralSlotReplay), 0, tr.data_ptr(), 5, 0, None
    ro.shape_flags = 2                                                # what the _ia entry point rejects, with a good block
    assert roll() == ERR_BAD_ARG
    ro.shape_flags = 0
    ia.struct_bytes -= 8
    assert roll(i=ia) == ERR_BAD_ARG
    ia.struct_bytes += 8
    torch.cuda.synchronize()
    assert torch.equal(m0, env.metrics())                            # nothing ran
    # replay NULL, and a block with both pointers NULL: the _ia entry point's call
    rp.x_positions, rp.T = None, 0
    want = twin.rollout(seq, 0, states=None)
    assert roll(r=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want["shaped"]) and torch.equal(rew, want["reward"])
    want = twin.rollout(seq, K, states=None)
    # (... and through the Python layer, slots K ... 2 K - 1)
    got = env.rollout(seq, K, states=None, positions=None, log_positions=False)
    assert torch.equal(got["shaped"], want["shaped"]) and "xpos" not in got
    assert not (env.last_kernel() & KERNEL_EXTRA)
    s1, s2 = env.export_state(), twin.export_state()
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k
    with pytest.raises(ValueError):
        env.rollout(seq, 0, positions=torch.zeros((5, N + 1), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        env.rollout(seq, 0, positions=torch.zeros((0, N), dtype=torch.float64, device=DEV))
    env.check()


# ---- 10: the candidates of a search -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_env", [False, True])
def test_candidate_search_with_recorded_positions_equals_the_candidates_one_by_one(per_env):
    C, B, K, N, A, T = 3, 4, 4, 33, 9, 6
    cfg = chain_cfg(N, A, 2)
    begin = start(cfg, B, 12)
    env, = twins(cfg, B, torch.float32, begin, n=1)
    for w in range(3):
        env.step(env.sample(w), w)
    tr = torch.as_tensor(_trace(np.random.default_rng(4), cfg.highway_length, ((B,) if per_env else ()) + (T, N)), device=DEV)
    rng = np.random.default_rng(0)
    seqs = torch.as_tensor(rng.integers(0, A, size=(K, B, C, N)).astype(np.int32), device=DEV)
    before = {k: v.clone() for k, v in env.export_state().items()}
    search = CandidateSearch(env, C)
    res = search.evaluate(seqs, 3, global_reward_avg=True, positions=tr)
    assert search.work.last_kernel() & KERNEL_POLICY
    for k, v in env.export_state().items():
        assert torch.equal(before[k], v), k
    for c in range(C):
        one = env.twin()
        one.copy_envs_from(env)
        got = one.rollout(seqs[:, :, c].contiguous(), 3, states=None, global_reward_avg=True, positions=tr)
        assert torch.equal(res["sum_r"][:, :, c], got["sum_r"]) and torch.equal(res["collision"][:, :, c], got["collision"]), c
    assert len(set(res["returns"].flatten().tolist())) > 1
    # the search's own loop (behind a refused launch) sets the expanded trace on the work handle and removes it
    work = search.work
    work.copy_envs_from(env, src_index=search._gather)
    pos = tr.repeat_interleave(C, dim=0) if per_env else tr
    work.load_saved_positions(pos)
    sum_r, coll, _ = search._loop(seqs.reshape(K, B * C, N).contiguous(), 3, STEP_MY_STEP, True, 0)
    work.load_saved_positions(None)
    assert torch.equal(sum_r.view(K, B, C), res["sum_r"]) and torch.equal(coll.view(K, B, C), res["collision"])
