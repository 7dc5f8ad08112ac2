"""Information age inside the K-slot my_step_ch launches (`diral_env_rollout_ia` / `diral_env_step_policy_ia`: the slot loop of
step_fast64_slots_kernel keeps the arrival stamps, builds Network.get_information_age behind every slot and applies the
`ia_averaging` term in its shaping) against what it stands for: the loop of one-slot `my_step_ch` steps, each followed by
`diral_env_info_age` and `diral_driver_shape` with the histogram - bit for bit -, the CPU oracle, and the reference's
recorded driver runs."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from diral_amd.config import (ERR_BAD_ARG, ERR_BAD_CONFIG, ERR_UNSUPPORTED, KERNEL_CH, KERNEL_EXTRA, KERNEL_FAST64,
                              KERNEL_POLICY, STEP_MY_STEP, STEP_MY_STEP_CH, DiralRollout, DiralSlotInfoAge, DiralSlotPolicy,
                              EnvConfig)
from diral_amd.driver import DriverLoop
from diral_amd.search import CandidateSearch
from diral_amd.sps import SpsPolicy
from diral_amd.vec_env import DiralError, VecV2VEnv
from oracle.oracle import SQ_IEEE, Oracle
from tests import host_closed_loop as H
from tests.golden_util import GOLDEN_DIR, ulp_diff
from tests.host_closed_loop import _exp_bounds
from tests.oracle_compare import exp_atol, same
from tests.kslots_harness import (DEV, PEN_VAL, VEL_SEED, as_rollout, assert_same, assert_same_envs, chain_cfg, go_on_alike,
                                   slot_loop, start, stuck_penalty_state, twins)

pytestmark = pytest.mark.gpu


def _check(N, A, rd, K, t0, dtype, vary=False, rich=False, pen=False, states="last", reps=2, B=4, seed=31, sticky=0.0,
           hold_from=None, conditions=True):
    """`reps` launches of K slots, each continuing the one before, against the loop on a twin handle.  `sticky`: the
    probability that an agent repeats its action; `hold_from`: from that slot of a launch on every agent repeats it."""
    cfg = chain_cfg(N, A, rd, vary, rich, track=True)
    e_loop, e_one = twins(cfg, B, dtype, start(cfg, B, seed))
    pens = [stuck_penalty_state(B, N) if pen else None for _ in range(2)]
    prevs = [torch.zeros((B,), dtype=torch.int64, device=DEV) for _ in range(2)]
    warm = 3 if t0 >= 3 else 0
    for w in range(warm):                                           # stamps older than the launches, from one-slot steps
        a = e_loop.sample(500 + w)
        for env in (e_loop, e_one):
            env._step(STEP_MY_STEP_CH, a, t0 - warm + w)
    rng = np.random.default_rng(seed + 1)
    acts = e_loop.sample(6999).cpu().numpy()
    t = t0
    wants = []
    for rep in range(reps):
        rows = []
        for k in range(K):
            fresh = e_loop.sample(7000 + 100 * rep + k).cpu().numpy()
            p = 1.0 if (hold_from is not None and k >= hold_from) else sticky
            acts = np.where(rng.random((B, N)) < p, acts, fresh).astype(np.int32)
            rows.append(acts)
        seq = torch.as_tensor(np.stack(rows), device=DEV)
        la_before = e_loop.export_state()["la"].cpu().numpy()      # the stamps the last launch starts from
        want = as_rollout(slot_loop(e_loop, seq, t, "my_step_ch", pen=pens[0], ia_prev=prevs[0], want_ia=True,
                                    want_obs=states is not None), states)
        got = e_one.rollout(seq, t, mode="my_step_ch", states=states, global_reward_avg=True, stuck_penalty=pens[1],
                            vel_seed=VEL_SEED, info_age=True, sum_ia_prev=prevs[1])
        torch.cuda.synchronize()
        lk = e_one.last_kernel()
        assert (lk & 15) == KERNEL_FAST64 and (lk & KERNEL_POLICY) and (lk & KERNEL_CH) and not (lk & KERNEL_EXTRA), lk
        assert_same(want, got, rep)
        assert torch.equal(prevs[0], prevs[1]) and torch.equal(prevs[0], want["ia_sum"][-1])
        assert e_one.t == t + K == e_loop.t
        wants.append(want)
        t_last, t = t, t + K
    s = assert_same_envs(e_loop, e_one)
    if pen:
        assert torch.equal(pens[0][2], pens[1][2]) and torch.equal(pens[0][3], pens[1][3])
    # what the inputs must exercise, from the LOOP's results: entries that never arrived (off the diagonal), stamps of the
    # last launch's own slots, stamps written before it started that its first histogram still counts (at N = 8 none
    # outlives 30 slots: they are looked for where the launch starts), and a histogram over several bins
    la = s["la"].cpu().numpy()
    off = ~np.eye(N, dtype=bool)[None]
    assert ((la == -1) & off).any()
    assert ((la >= t_last) & (la < t) & off).any()
    if conditions:
        assert ((la_before != -1) & (la_before < t_last) & off).any()
        assert int(wants[-1]["ia"][0, :, 1:].sum()) > 0
        assert int((wants[-1]["ia"].sum(1) > 0).sum(-1).max()) >= 3
    go_on_alike(e_loop, e_one, "my_step_ch", t, info_age=True)
    return wants, pens[0]


@pytest.mark.parametrize("N,A,rd,K,t0,dtype,vary,rich,pen,states", [
    (8, 3, 2, 1, 20, torch.float64, True, False, False, "last"),
    (8, 3, 3, 4, 0, torch.float32, False, False, True, "all"),
    (8, 3, 4, 30, 20, torch.float32, True, True, True, "all"),
    (33, 9, 2, 1, 0, torch.float32, False, False, False, None),
    (33, 9, 2, 30, 20, torch.float32, True, False, True, "last"),
    (33, 9, 3, 4, 0, torch.float64, False, True, False, None),
    (33, 9, 4, 30, 0, torch.float64, True, False, True, "all"),
    (64, 32, 2, 30, 20, torch.float32, True, False, True, "last"),
    (64, 32, 3, 1, 20, torch.float32, False, False, False, "last"),
    (64, 32, 4, 4, 0, torch.float64, True, True, True, "all"),
    (64, 5, 2, 4, 20, torch.float64, True, False, True, "last"),
    (64, 5, 3, 30, 0, torch.float32, True, True, False, "last"),
])
def test_launch_with_information_age_equals_the_loop_of_one_slot_calls(N, A, rd, K, t0, dtype, vary, rich, pen, states):
    """(N, A) = (8, 3) a partial last resource group, (33, 9) an idle wave and padded lanes, (64, 32) C2, (64, 5) many
    transmitters per resource; reward_design 2 ... 4, K = 1 / 4 / 30, both dtypes, t0 = 0 and 20 with mobility_vary - K = 30
    from 20 has an episode end inside the launch (24) and one on its last slot (49) -, the rich State flags, states last /
    all / none, the stuck penalty; every launch followed by another."""
    _check(N, A, rd, K, t0, dtype, vary=vary, rich=rich, pen=pen, states=states, reps=3 if K == 1 else 2)


def test_the_term_takes_every_value_and_meets_the_stuck_penalty():
    """From the loop's results: the term takes -1, 0 and +1, and the stuck penalty fires in a slot whose term is +1 - where
    `r + term < 1` and `r < 1` differ.  0 needs a histogram that stands still: fresh handles, nobody ever changes resource
    and - mobility_vary in front of the first episode end - every vehicle at one speed, so each slot stamps the pairs of the
    slot before again and nothing else ages; -1 / +1 and the penalty come from sticky agents."""
    still, _ = _check(33, 9, 2, 4, 0, torch.float32, vary=True, pen=True, states=None, hold_from=0, B=6, conditions=False)
    wants, _ = _check(33, 9, 2, 30, 20, torch.float64, vary=False, pen=True, states=None, sticky=0.7, B=6)
    pen = torch.cat([w["ia_penalty"] for w in wants])               # [2 K, B]
    shaped = torch.cat([w["shaped"] for w in wants])                # [2 K, B, N]
    seen = set(pen.unique().tolist()) | set(torch.cat([w["ia_penalty"] for w in still]).unique().tolist())
    assert seen == {-1, 0, 1}
    n_t = torch.as_tensor(33.0, dtype=shaped.dtype, device=DEV)     # (tensor / tensor: a true division, as the kernel's)
    paid = PEN_VAL + (torch.cat([w["sum_r"] for w in wants]) / n_t).unsqueeze(-1)
    fired = (shaped == paid).any(-1)                                # an agent was paid the penalty value (+ the average)
    assert bool((fired & (pen == 1)).any())


def test_imported_stamps_at_the_edges_of_the_histogram():
    """Stamps 98 ... 101 slots old, stamps from the future (Python's negative index wraps them, 101 ahead is dropped) and
    -1, imported on pairs that stay in range without the transmitter being the receiver's closest one - nothing overwrites
    or clears them: a 3-slot launch against the loop and against the oracle."""
    N, A, B, t0, K = 8, 3, 3, 200, 3
    cfg = chain_cfg(N, A, 2, track=True)
    x0 = np.tile(np.arange(N) * 10.0, (B, 1)) + 5.0 * np.arange(B)[:, None]
    v0 = np.full((B, N), 1.7)
    acts = np.array([0, 1, 2, 0, 1, 2, 1, 2], np.int32)              # resource 0: vehicles 0, 3; 1: 1, 4, 6; 2: 2, 5, 7
    pairs = [(0, 2), (0, 4), (0, 5), (0, 6), (0, 7), (3, 1), (1, 5), (1, 7), (4, 7), (6, 5)]   # (tx, rx): rx hears a closer tx
    stamps = [t0 - 98, t0 - 99, t0 - 100, t0 - 101, t0 + 1, t0 + 100, t0 + 101, -1, t0 - 99, t0 - 98]
    la = np.full((B, N, N), -1, np.int64)
    for (tx, rx), s in zip(pairs, stamps):
        la[:, tx, rx] = s
    envs = []
    for _ in range(2):
        env = VecV2VEnv(cfg, batch=B, device=DEV, out_dtype=torch.float64)
        env.reset_topology(x0, 0.0, v0)
        env.import_state(la=la.astype(np.int32))
        envs.append(env)
    e_loop, e_one = envs
    orc = Oracle(cfg, batch=B, sq_mode=SQ_IEEE)
    orc.reset(x0, np.zeros((B, N)), v0)
    orc.import_state(la=la)
    seq = torch.as_tensor(np.broadcast_to(acts, (K, B, N)).copy(), device=DEV)
    o_ia = []
    for k in range(K):
        orc.step(STEP_MY_STEP_CH, np.broadcast_to(acts, (B, N)).copy(), t0 + k)
        o_ia.append(orc.info_age(t0 + k))
    o_ia = np.stack(o_ia)
    want = as_rollout(slot_loop(e_loop, seq, t0, "my_step_ch", want_ia=True), "last")
    got = e_one.rollout(seq, t0, mode="my_step_ch", states="last", global_reward_avg=True, vel_seed=VEL_SEED, info_age=True)
    torch.cuda.synchronize()
    assert e_one.last_kernel() & KERNEL_POLICY
    assert_same(want, got, "edges")
    s = assert_same_envs(e_loop, e_one)
    assert np.array_equal(got["ia"].cpu().numpy(), o_ia)
    o_la = orc.export()["la"]
    assert np.array_equal(s["la"].cpu().numpy(), o_la)
    for (tx, rx), st in zip(pairs, stamps):                           # the imported stamps survived
        assert (o_la[:, tx, rx] == st).all(), (tx, rx)
    # slot 0: bin 99 holds the stamps of t0 - 99 and, wrapped, t0 + 1 (ia = -1); bin 0 the wrapped t0 + 100 (ia = -100);
    # t0 - 100, t0 - 101 and t0 + 101 are dropped
    assert (o_ia[0, :, 99] == 3).all() and (o_ia[0, :, 98] == 2).all()
    new0 = int((o_la == t0 + K - 1).sum()) // B                      # (the pairs every slot stamps afresh: the same every slot)
    assert new0 > 0 and (o_ia[0, :, 0] == new0 + 1).all()
    # slot 1: t0 - 99 has left - bin 99 is the two stamps of t0 - 98 -, t0 + 101 has come in at bin 0 beside the fresh
    # stamps and t0 + 1, t0 + 100 sits in bin 1
    assert (o_ia[1, :, 99] == 2).all() and (o_ia[1, :, 98] == 0).all()
    assert (o_ia[1, :, 0] == new0 + 2).all() and (o_ia[1, :, 1] == 1).all()


@pytest.mark.parametrize("N,A,rd,dtype", [(33, 9, 2, torch.float32), (64, 32, 3, torch.float64)])
def test_closed_loop_with_information_age_against_the_cpu_oracle(N, A, rd, dtype):
    """step_policy(slots=6, my_step_ch, info_age=True) with keep_prob = 1 against the host loop of tests/host_closed_loop.py
    (CPU oracle step, shaping, SPS): every slot's histogram and the final stamps exactly, rewards within that file's bars;
    and bit-equal to six one-slot step_policy calls, each followed by info_age."""
    B, K, t0, topo_seed, pol_seed = 4, 6, 3, 21, 3
    cfg = chain_cfg(N, A, rd, track=True)
    npdt = np.float32 if dtype == torch.float32 else np.float64
    x0, v0 = H.draw_topology(topo_seed, B, N, cfg.highway_length, cfg.mobility_vary, 0)
    sps = H.HostSps.from_seed(B * N, A, pol_seed, threshold=-110.0, keep_prob=1.0)
    host = H.HostClosedLoop(cfg, B, x0, v0, sps, pol_seed, mode="my_step_ch", dtype=npdt)
    a = sps.prev_action.reshape(B, N).copy()
    h_ia, h_out = [], []
    for k in range(K):
        o = host.run(a, t0 + k, 1)
        h_ia.append(host.ob.info_age(t0 + k))
        h_out.append(o)
        a = o["actions"]
    assert not host.left_out.any()
    envs, pols = [], []
    for _ in range(2):
        env = VecV2VEnv(cfg, batch=B, device=DEV, out_dtype=dtype)
        env.reset_topology(seed=topo_seed)
        pol = SpsPolicy(B, N, A, rssi_threshold=-110.0, device=DEV, seed=pol_seed)
        pol.keep_prob = 1.0
        envs.append(env); pols.append(pol)
    st = envs[0].export_state(tables=False)
    assert np.array_equal(st["pos_x"].cpu().numpy(), x0) and np.array_equal(st["vel"].cpu().numpy(), v0)
    o = dict(dtype=dtype, device=DEV)
    # one launch of K slots
    env, pol = envs[0], pols[0]
    sh, sr, co = torch.zeros((K, B, N), **o), torch.zeros((K, B), **o), torch.zeros((K, B), **o)
    nxt = torch.empty_like(pol.prev_action)
    obs, rew, done, iad = env.step_policy(pol.prev_action.clone(), t0, pol, nxt, shaped_out=sh, sum_r_out=sr, collision_out=co,
                                          slots=K, mode=STEP_MY_STEP_CH, info_age=True)
    torch.cuda.synchronize()
    lk = env.last_kernel()
    assert (lk & KERNEL_POLICY) and (lk & KERNEL_CH) and (lk & 15) == KERNEL_FAST64, lk
    assert np.array_equal(iad["ia"].cpu().numpy(), np.stack(h_ia))
    assert np.array_equal(env.export_state()["la"].cpu().numpy(), host.ob.export_state()["la"])
    exp = rd != 2
    sum_atol, shaped_atol = _exp_bounds(N) if exp else (0.0, 0.0)
    assert np.abs(sh.cpu().numpy() - np.stack([h["shaped"][0] for h in h_out])).max() <= shaped_atol
    assert np.abs(sr.cpu().numpy() - np.stack([h["sum_r"][0] for h in h_out])).max() <= sum_atol
    same(rew.cpu().numpy(), h_out[-1]["rew"], "reward", atol=exp_atol(exp))
    assert np.array_equal(nxt.cpu().numpy(), h_out[-1]["actions"])
    want_sum = np.stack([[sum((i + 1) * int(v) for i, v in enumerate(row) if v > 0) for row in ia] for ia in h_ia])
    assert np.array_equal(iad["ia_sum"].cpu().numpy(), want_sum)
    # K one-slot calls (three launches each on this handle), each followed by info_age
    env2, pol2 = envs[1], pols[1]
    a, nx2 = pol2.prev_action.clone(), torch.empty_like(pol2.prev_action)
    for k in range(K):
        s1, r1, c1 = torch.zeros((B, N), **o), torch.zeros((B,), **o), torch.zeros((B,), **o)
        _, rew2, _ = env2.step_policy(a, t0 + k, pol2, nx2, shaped_out=s1, sum_r_out=r1, collision_out=c1, slots=1,
                                      mode=STEP_MY_STEP_CH)
        assert not (env2.last_kernel() & KERNEL_POLICY)
        assert torch.equal(env2.info_age(t0 + k), iad["ia"][k]), k
        assert torch.equal(s1, sh[k]) and torch.equal(r1, sr[k]) and torch.equal(c1, co[k]), k
        a, nx2 = nx2, a
    assert torch.equal(rew2, rew) and torch.equal(a, nxt)
    assert "la" in assert_same_envs(env, env2)
    assert torch.equal(pol.prev_action, pol2.prev_action) and torch.equal(pol.counter, pol2.counter)
    env.check(); env2.check()


@pytest.mark.parametrize("name", ["d2_driver_ch_vary", "d3_driver_ch_c2"])
def test_driver_rollout_in_chunks_reproduces_the_reference_recording(name):
    """The reference's recorded driver runs (`enable_channel`; d2: N = 16 with ia_averaging, the stuck penalty and
    mobility_vary, d3: N = 64) through DriverLoop.rollout: every stretch up to the slot in front of an episode end as ONE
    launch, the episode's last slot through slot() + end_episode(the recorded draws)."""
    d = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    cfg = EnvConfig.from_dict(json.loads(str(d["cfg"])), track_arrival=True)
    opts = json.loads(str(d["opts"]))
    assert opts["enable_channel"]
    env = VecV2VEnv(cfg, batch=1, out_dtype=torch.float64)
    loop = DriverLoop(env, enable_channel=True, global_reward_avg=opts["global_reward_avg"], ia_averaging=opts["ia_averaging"],
                      ia_penalty_enable=opts["ia_penalty_enable"], ia_penalty_threshold=opts["ia_penalty_threshold"],
                      ia_penalty_value=opts["ia_penalty_value"], episode_interval=opts["episode_interval"])
    env.reset_topology(d["x0"], d["y0"], d["v0"])

    def same(a, b, what):                                           # tests/test_driver_loop.py's rule for the GPU run
        a = a.detach().cpu().numpy().astype(np.float64)
        assert ulp_diff(a, b) <= 1 or np.allclose(a, b, rtol=0, atol=4e-15), what

    loop.bootstrap(d["boot_action"])
    for i in range(opts["n_prefill"]):
        loop.prefill_step(d["pre_actions"][i])
    T, EI = opts["T"], opts["episode_interval"]
    t, launches = 0, 0
    while t < T:
        end = min(T, (t // EI) * EI + EI - 1)                       # the slot that ends this episode (or the recording)
        K = end - t
        if K > 0:
            out = loop.rollout(torch.as_tensor(d["actions"][t:end].astype(np.int32), device=DEV).unsqueeze(1), t, states="all")
            assert env.last_kernel() & KERNEL_POLICY, (t, env.last_kernel())
            launches += 1
            assert np.array_equal(out["ia"][:, 0].cpu().numpy(), d["ia"][t:end]), ("ia", t)
            assert np.array_equal(out["ia_sum"][:, 0].cpu().numpy(), d["ia_sum"][t:end]), ("ia_sum", t)
            if opts["ia_averaging"]:
                assert np.array_equal(out["ia_penalty"][:, 0].cpu().numpy(), d["ia_pen"][t:end]), ("ia_pen", t)
            same(out["states"][:, 0], d["states"][t:end], ("states", t))
            same(out["shaped"][:, 0], d["shaped_reward"][t:end], ("shaped", t))
            same(out["sum_r"][:, 0], d["sum_r"][t:end], ("sum_r", t))
            same(out["collision"][:, 0], d["collision"][t:end], ("collision", t))
            same(out["reward"][0], d["raw_reward"][end - 1], ("raw reward", t))
            t = end
        if t < T:
            o = loop.slot(d["actions"][t], t, want_ia=True)
            assert np.array_equal(o["ia"][0].cpu().numpy(), d["ia"][t]) and int(o["ia_sum"][0]) == int(d["ia_sum"][t])
            if opts["ia_averaging"]:
                assert int(o["ia_penalty"][0]) == int(d["ia_pen"][t])
            same(o["next_state"][0], d["states"][t], ("state", t))
            same(o["reward"][0], d["shaped_reward"][t], ("shaped", t))
            assert bool(o["episode_end"]) == bool(d["episode_end"][t])
            if o["episode_end"]:
                loop.end_episode(d["vel_draws"][t])
            t += 1
    assert launches >= 3
    fin = env.export_state()
    assert np.array_equal(fin["pos_x"][0].cpu().numpy(), d["final_pos"]) and np.array_equal(fin["vel"][0].cpu().numpy(), d["final_vel"])
    assert np.array_equal(fin["seq"][0].cpu().numpy(), d["final_seq"]) and np.array_equal(fin["x"][0].cpu().numpy(), d["final_x"])
    env.check()


def test_stamps_only_keeps_the_stamps_and_builds_no_histogram():
    N, A, B, K, t0 = 33, 9, 4, 7, 5
    cfg = chain_cfg(N, A, 3, vary=True, track=True)
    e_loop, e_one = twins(cfg, B, torch.float32, start(cfg, B, 77))
    seq = torch.stack([e_loop.sample(300 + k) for k in range(K)])
    want = as_rollout(slot_loop(e_loop, seq, t0, "my_step_ch"), "last")
    got = e_one.rollout(seq, t0, mode="my_step_ch", states="last", global_reward_avg=True, vel_seed=VEL_SEED, info_age="stamps")
    assert e_one.last_kernel() & KERNEL_POLICY
    assert_same(want, got, "stamps")                                       # (no ia / ia_sum / ia_penalty in either)
    assert "la" in assert_same_envs(e_loop, e_one)
    assert torch.equal(e_loop.info_age(t0 + K), e_one.info_age(t0 + K))
    assert int(e_one.info_age(t0 + K).sum()) > 0
    e_one.check()


def _raw_rollout(env, mode, seq, K, t, blk, shaped=True, flags=0):
    """diral_env_rollout_ia as a C caller would call it: the status."""
    o = dict(dtype=env.out_dtype, device=env.device)
    keep = [torch.empty((K, env.B, env.N), **o), torch.empty((env.B, env.N), **o), torch.empty((env.B,), dtype=torch.uint8, device=env.device)]
    ro = DiralRollout()
    ro.struct_bytes = ctypes.sizeof(ro)
    ro.shape_flags = flags
    ro.shaped_out = keep[0].data_ptr() if shaped else None
    st = env.lib.diral_env_rollout_ia(env._h, mode, seq.data_ptr(), K, t, None, 0, keep[1].data_ptr(), keep[2].data_ptr(), env._dt,
                                      ctypes.byref(ro), None if blk is None else ctypes.byref(blk), env._stream())
    torch.cuda.synchronize()
    return st


def _raw_step_policy(env, pol, mode, a, nxt, t, slots, blk, shaped=True):
    o = dict(dtype=env.out_dtype, device=env.device)
    lead = (slots,) if slots > 1 else ()
    keep = [torch.empty(lead + (env.B, env.N), **o), torch.empty((env.B, env.N), **o), torch.empty((env.B,), dtype=torch.uint8, device=env.device)]
    q = DiralSlotPolicy()
    q.struct_bytes = ctypes.sizeof(q)
    q.shaped_out = keep[0].data_ptr() if shaped else None
    q.sps_prev_action, q.sps_counter = pol.prev_action.data_ptr(), pol.counter.data_ptr()
    q.rssi_threshold, q.inc_db, q.keep_prob = pol.threshold, pol.inc_db, pol.keep_prob
    q.seed, q.actions_out, q.slots = 99, nxt.data_ptr(), slots
    st = env.lib.diral_env_step_policy_ia(env._h, mode, a.data_ptr(), t, None, keep[1].data_ptr(), keep[2].data_ptr(), None, env._dt,
                                          ctypes.byref(q), None if blk is None else ctypes.byref(blk), env._stream())
    torch.cuda.synchronize()
    return st


def _block(B, K, flags=0, prev=True, size=None):
    blk = DiralSlotInfoAge()
    blk.struct_bytes = ctypes.sizeof(blk) if size is None else size
    blk.flags = flags
    keep = [torch.zeros((K, B, 100), dtype=torch.int32, device=DEV), torch.zeros((K, B), dtype=torch.int64, device=DEV),
            torch.zeros((K, B), dtype=torch.int32, device=DEV), torch.zeros((B,), dtype=torch.int64, device=DEV)]
    blk.ia_out, blk.ia_sum_out, blk.ia_pen_out = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr()
    blk.sum_ia_prev = keep[3].data_ptr() if prev else None
    return blk, keep


@pytest.mark.parametrize("what,N,track,mode,want", [
    ("my_step with the block", 33, True, STEP_MY_STEP, ERR_UNSUPPORTED),
    ("N = 7", 7, True, STEP_MY_STEP_CH, ERR_UNSUPPORTED),
    ("N = 128", 128, True, STEP_MY_STEP_CH, ERR_UNSUPPORTED),
    ("no arrival stamps", 33, False, STEP_MY_STEP_CH, ERR_BAD_CONFIG),
    ("bit 0 without sum_ia_prev", 33, True, STEP_MY_STEP_CH, ERR_BAD_ARG),
    ("bit 0 without shaped_out", 33, True, STEP_MY_STEP_CH, ERR_BAD_ARG),
    ("flags = 2", 33, True, STEP_MY_STEP_CH, ERR_BAD_ARG),
    ("struct_bytes", 33, True, STEP_MY_STEP_CH, ERR_BAD_ARG),
    ("one-slot step_policy_ia", 33, True, STEP_MY_STEP_CH, ERR_UNSUPPORTED),
    ("no block", 33, True, STEP_MY_STEP_CH, ERR_UNSUPPORTED),
])
def test_refusals_and_argument_checks_leave_the_env_untouched(what, N, track, mode, want):
    """One case per row of the header's list, through both entry points: the status, and - nothing was launched - the
    exported state with the stamps, the metrics and the slot counter are what they were."""
    A, B, K, t0 = 6, 3, 4, 3
    cfg = chain_cfg(N, A, 2, track=track)
    env = VecV2VEnv(cfg, batch=B, device=DEV, out_dtype=torch.float32)
    env.reset_topology(seed=5)
    for k in range(t0):
        env.step(env.sample(40 + k), k) if not track else env._step(STEP_MY_STEP_CH, env.sample(40 + k), k)
    env.t = t0
    before, m_before = env.export_state(), env.metrics()
    seq = torch.stack([env.sample(60 + k) for k in range(K)])
    pol = SpsPolicy(B, N, A, device=DEV, seed=4)
    p_before = (pol.prev_action.clone(), pol.counter.clone())
    nxt = torch.empty_like(pol.prev_action)
    a0 = seq[0].contiguous()
    blk, keep = _block(B, K)
    shaped, slots = True, K
    if what == "bit 0 without sum_ia_prev":
        blk, keep = _block(B, K, flags=1, prev=False)
    elif what == "bit 0 without shaped_out":
        blk, keep = _block(B, K, flags=1)
        shaped = False
    elif what == "flags = 2":
        blk, keep = _block(B, K, flags=2)
    elif what == "struct_bytes":
        blk, keep = _block(B, K, size=ctypes.sizeof(DiralSlotInfoAge) - 8)
    elif what == "no block":
        blk = None
    if what == "one-slot step_policy_ia":
        assert _raw_step_policy(env, pol, mode, a0, nxt, t0, 1, blk) == want
    else:
        assert _raw_rollout(env, mode, seq, K, t0, blk, shaped=shaped) == want, what
        assert _raw_step_policy(env, pol, mode, a0, nxt, t0, slots, blk, shaped=shaped) == want, what
    if what == "no block":                                           # the Python surface's default calls, too
        for call in (lambda: env.rollout(seq, t0, mode="my_step_ch"),
                     lambda: env.step_policy(a0, t0, pol, nxt, slots=K, mode=STEP_MY_STEP_CH)):
            with pytest.raises(DiralError) as exc:
                call()
            assert exc.value.status == ERR_UNSUPPORTED
    after = env.export_state()
    assert ("la" in before) == track
    for key in before:
        assert torch.equal(before[key], after[key]), (what, key)
    assert torch.equal(m_before, env.metrics()) and env.t == t0
    assert torch.equal(p_before[0], pol.prev_action) and torch.equal(p_before[1], pol.counter)
    assert all(int(k.abs().sum()) == 0 for k in keep)                # nothing was written
    env.check()


def test_candidate_search_scores_candidates_by_information_age():
    """CandidateSearch.evaluate(info_age=True): ia_sum[:, b, c] is what a lone handle forked from env b and stepped with
    candidate c's actions reports; `env` is untouched until commit."""
    N, A, B, C, K, t0 = 33, 9, 3, 3, 5, 4
    cfg = chain_cfg(N, A, 2, track=True)
    env = VecV2VEnv(cfg, batch=B, device=DEV, out_dtype=torch.float32, step_mode="my_step_ch")
    env.reset_topology(seed=9)
    for k in range(t0):
        env._step(STEP_MY_STEP_CH, env.sample(10 + k), k)
    env.t = t0
    before, m_before = env.export_state(), env.metrics()
    search = CandidateSearch(env, C)
    rng = np.random.default_rng(2)
    seqs = torch.as_tensor(rng.integers(0, A, size=(K, B, C, N)).astype(np.int32), device=DEV)
    res = search.evaluate(seqs, t0, mode="my_step_ch", global_reward_avg=True, info_age=True)
    assert search.work.last_kernel() & KERNEL_POLICY
    assert tuple(res["ia_sum"].shape) == (K, B, C) and res["ia_sum"].dtype == torch.int64
    after = env.export_state()
    for key in before:
        assert torch.equal(before[key], after[key]), key
    assert torch.equal(m_before, env.metrics()) and env.t == t0
    lone = env.twin(1)
    one = torch.zeros(1, dtype=torch.int32, device=DEV)
    for b in range(B):
        for c in range(C):
            lone.copy_envs_from(env, src_index=torch.full((1,), b, dtype=torch.int32, device=DEV), dst_index=one)
            for k in range(K):
                _, rew, _ = lone._step(STEP_MY_STEP_CH, seqs[k, b, c].unsqueeze(0).contiguous(), t0 + k, want_obs=False)
                ia = lone.info_age(t0 + k)
                w = torch.arange(1, 101, dtype=torch.int64, device=DEV)
                assert int((ia[0].to(torch.int64) * w).sum()) == int(res["ia_sum"][k, b, c]), (b, c, k)
    # the loop fallback computes the same
    work = search.work
    work.copy_envs_from(env, src_index=search._gather)
    _, _, ia_sum = search._loop(seqs.reshape(K, B * C, N).contiguous(), t0, STEP_MY_STEP_CH, True, 0, True)
    assert torch.equal(ia_sum.view(K, B, C), res["ia_sum"])
    assert int(res["ia_sum"].min()) > 0 and len(res["ia_sum"][-1].unique()) > 1
    choice = res["ia_sum"][-1].argmin(1)
    search.evaluate(seqs, t0, mode="my_step_ch", global_reward_avg=True, info_age=True)
    search.commit(choice)
    assert env.t == t0 + K
    env.check()
