"""The closed-loop and prefill launches against a HOST statement of the same loop (tests/host_closed_loop.py: CPU oracle
step + the driver's shaping in NumPy's order + the SPS agent with Python's `sorted` + a mirror of the device generator),
from the same start.  The other closed-loop tests compare one device path with another - both sides call the same device
functions; here the second side shares no code with the device.

Bars (the suite's own, tests/test_gpu_parity.py): everything bit for bit against the oracle in its IEEE-square mode; the
metric float sums at rtol 1e-12, atol 1e-9; exp()-based rewards (reward_design 3, and 4 in my_step_ch) within the exp() bar,
and what is summed from them within the bound `_exp_bounds` derives from that bar and the float64 format (tests/oracle_compare.py).

What is indexed how: the topology, `sample` and velocity draws are indexed by the GLOBAL vehicle index
(DIRAL_OPT_ENV_OFFSET * N + b * N + lane: shards draw what the whole batch draws); the SPS draws (initial state, new
counter, keep, choice) by the index within the handle, i = b * N + lane.

Ambiguous decisions: device log10 and NumPy's may differ in the last place.  An env one of whose re-selections has a
host-computed margin below 1e-9 dB is left out from that slot on (the host alone decides); at most 1 % of a test's envs,
and the seeds here leave out none (`assert_coverage`)."""
import numpy as np
import pytest
import torch

from diral_amd.config import (KERNEL_CH, KERNEL_FAST64, KERNEL_PACKED, KERNEL_POLICY, KERNEL_WIDE, STEP_MY_STEP_CH,
                              bench_config, c2_config)
from tests import host_closed_loop as H
from tests.oracle_compare import exp_atol, metrics_equal
from tests.host_closed_loop import RICH, Case, _eq, _exp_bounds, host_run, uses_exp

pytestmark = pytest.mark.gpu


def assert_coverage(c, host):
    """Non-vacuity, from the host's own record."""
    rec = host.record()
    print("host record:", rec)
    assert rec["left_out"] <= c.B // 100, rec                    # at most 1 % of the envs (none with these seeds)
    assert rec["reselections"] > 3 * c.N, rec
    if "both_paths" in c.expect:
        assert rec["shortcut"] > 0 and rec["general"] > 0, rec
    if "raises" in c.expect:
        assert rec["raises"] > 0, rec
    if "far" in c.expect:
        assert rec["far"] > 0, rec
    if c.cfg.mobility_vary:
        assert rec["vel_changed"] > 0, rec
    return rec


def device_run(c, monkeypatch=None):
    """The plan on the device, every launch compared with the host's."""
    from diral_amd.rollout import SlotClock
    from diral_amd.sps import SpsPolicy
    from diral_amd.vec_env import VecV2VEnv
    host, (x0, v0), outs = host_run(c)
    assert_coverage(c, host)
    if c.form is not None:
        monkeypatch.setenv("DIRAL_TABLE_FORM", c.form)
    cfg, B, N, A, dt = c.cfg, c.B, c.N, c.A, c.dt
    dev = "cuda:0"
    env = VecV2VEnv(cfg, batch=B, device=dev, out_dtype=dt, env_offset=c.env_offset)
    if c.x0 is not None:
        env.reset_topology(x0, None, v0)
    else:
        env.reset_topology(seed=c.topo_seed)                     # the device's own draws: the mirror's, bit for bit
        st = env.export_state(tables=False)
        assert np.array_equal(st["pos_x"].cpu().numpy(), x0) and np.array_equal(st["vel"].cpu().numpy(), v0)
    pol = SpsPolicy(B, N, A, rssi_threshold=c.thr, device=dev, seed=c.pol_seed)
    hp, hc = H.draw_sps_init(c.pol_seed, B * N, A - 1)
    assert np.array_equal(pol.prev_action.cpu().numpy().reshape(-1), hp) and np.array_equal(pol.counter.cpu().numpy().reshape(-1), hc)
    pol.keep_prob = c.keep
    if c.counter_mod:
        pol.counter.remainder_(c.counter_mod)
    clk = SlotClock(dev, 0) if c.clock else None
    if clk is not None:
        env.set_clock(clk.t)
    pn = None
    if c.pen:
        pn = (2, -10.0, torch.zeros((B, N), dtype=torch.int32, device=dev), torch.full((B, N), -1, dtype=torch.int32, device=dev))
    exp = uses_exp(cfg, c.mode)
    sum_atol, shaped_atol = _exp_bounds(N) if exp else (None, None)
    a, nxt, t = pol.prev_action.clone(), torch.empty_like(pol.prev_action), 0
    EI = cfg.episode_interval
    for li, (K, o) in enumerate(zip(c.plan, outs)):
        lead = (K,) if K > 1 else ()
        sh = torch.zeros(lead + (B, N), dtype=dt, device=dev)
        sr = torch.zeros(lead + (B,), dtype=dt, device=dev)
        co = torch.zeros(lead + (B,), dtype=dt, device=dev)
        env.step_policy(a, 0 if clk is not None else t, pol, nxt, shaped_out=sh, sum_r_out=sr, collision_out=co, slots=K,
                        vel_seed=c.vel_seed, clock=clk, seed_offset=0, mode=c.mode, want_chobs=c.want_chobs,
                        want_obs=c.want_obs, stuck_penalty=pn)
        lk = env.last_kernel()
        if K > 1 or c.kernel == "fused":
            assert lk & KERNEL_POLICY, lk
            assert (lk & 15) == (KERNEL_WIDE if N > 64 else KERNEL_FAST64), lk
            assert bool(lk & KERNEL_CH) == (c.mode == STEP_MY_STEP_CH), lk
            if c.form is not None:
                assert bool(lk & KERNEL_PACKED) == (c.form == "packed"), lk
        elif c.kernel == "three":
            assert not (lk & KERNEL_POLICY), lk
        if K == 1 and cfg.mobility_vary and t % EI == EI - 1:
            env.update_velocity(seed=c.vel_seed + t // EI)       # (a K-slot launch does this inside)
        if clk is not None:
            env.lib.diral_clock_add(clk.ptr(), K, env._stream())
        torch.cuda.synchronize()
        keep = ~o["left_out"]
        tag = "launch %d (K = %d, t = %d): " % (li, K, t)
        _eq(tag + "shaped", sh.reshape((K, B, N)), o["shaped"], keep, 1, shaped_atol)
        _eq(tag + "sum_r", sr.reshape((K, B)), o["sum_r"], keep, 1, sum_atol)
        _eq(tag + "collisions", co.reshape((K, B)), o["coll"], keep, 1, sum_atol)
        _eq(tag + "reward", env._rew, o["rew"], keep, 0, exp_atol(exp))
        _eq(tag + "done", env._done, o["done"], keep)
        if c.want_obs:
            _eq(tag + "state", env._obs, o["state"], keep, 0, exp_atol(exp and cfg.State.add_reward))
        if c.want_chobs:
            _eq(tag + "channel observation", env._chobs, o["chobs"], keep)
        _eq(tag + "actions_out", nxt, o["actions"], keep)
        _eq(tag + "prev_action", pol.prev_action, o["sps"][0], keep)
        _eq(tag + "counter", pol.counter, o["sps"][1], keep)
        if pn is not None:
            _eq(tag + "penalty counter", pn[2], o["pen"][0], keep)
            _eq(tag + "penalty prev_actions", pn[3], o["pen"][1], keep)
        a, nxt = nxt, a
        t += K
    keep = ~host.left_out
    st, he = env.export_state(), host.export_state()
    for k in ("pos_x", "vel", "seq", "age", "x"):
        _eq("export_state " + k, st[k], he[k], keep)
    m, hm = env.metrics().cpu().numpy()[keep], host.metrics()[keep]
    metrics_equal(m, hm, "metrics", prr=c.mode == STEP_MY_STEP_CH)
    assert c.mode != STEP_MY_STEP_CH or float(m[:, 5].min()) > 0
    env.check()
    return env, host


# ---- the generator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_offset", [0, 37])
def test_device_generator_equals_the_host_mirror(env_offset):
    """reset_topology(seed), sample(seed), SpsPolicy(...)'s initial state and update_velocity(seed=...) against the
    mirror, bit for bit; once with DIRAL_OPT_ENV_OFFSET non-zero: topology, sample and velocity follow the global index,
    the SPS draws the handle's own."""
    from diral_amd.sps import SpsPolicy
    from diral_amd.vec_env import VecV2VEnv
    for cfg, B in ((c2_config(), 9), (bench_config(40, 7, 1234.5, mobility_vary=True), 5), (bench_config(200, 33, 2400.0), 3)):
        N, A = cfg.num_users, cfg.num_channels
        env = VecV2VEnv(cfg, batch=B, device="cuda:0", env_offset=env_offset)
        for seed in (0, 21, 2**63 + 12345):
            env.reset_topology(seed=seed)
            st = env.export_state(tables=False)
            x, v = H.draw_topology(seed, B, N, cfg.highway_length, cfg.mobility_vary, env_offset)
            assert np.array_equal(st["pos_x"].cpu().numpy(), x) and np.array_equal(st["vel"].cpu().numpy(), v), seed
            assert np.array_equal(env.sample(seed).cpu().numpy(), H.draw_sample(seed, B, N, A, env_offset)), seed
            pol = SpsPolicy(B, N, A, device="cuda:0", seed=seed)
            hp, hc = H.draw_sps_init(seed, B * N, A - 1)             # per handle: no offset
            assert np.array_equal(pol.prev_action.cpu().numpy().reshape(-1), hp), seed
            assert np.array_equal(pol.counter.cpu().numpy().reshape(-1), hc), seed
            if cfg.mobility_vary:
                ob = H.OracleBackend(cfg, batch=B)
                ob.reset_topology(x, np.zeros_like(x), v)
                for rep in range(4):                                # up and down to the 1.1 / 2.77 clamps
                    env.update_velocity(seed=seed + rep)
                    ob.update_velocity(H.draw_velocity(seed + rep, B, N, env_offset))
                    assert np.array_equal(env.export_state(tables=False)["vel"].cpu().numpy(), ob.export_state()["vel"]), (seed, rep)
                assert len(np.unique(ob.export_state()["vel"])) > 3
        if env_offset:
            assert not np.array_equal(H.draw_sample(21, B, N, A, env_offset), H.draw_sample(21, B, N, A, 0))
        env.check()


# ---- the launches ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,A,L", [(6, 4, 300.0), (96, 33, 1500.0)])
def test_three_launch_slot_against_the_host_loop(N, A, L):
    """`step_policy` where it runs as three launches (N < 8: NumPy sums sequentially; N > 64: step_wide + the two policy
    launches), slot by slot."""
    cfg = bench_config(N, A, L, reward_design=4)
    c = Case(cfg, 16 if N > 8 else 96, torch.float32, [1] * 40, kernel="three", counter_mod=4, expect=("both_paths",) if N > 8 else ())
    device_run(c)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
@pytest.mark.parametrize("N,A,thr", [(64, 32, -110.0), (40, 7, -150.0), (9, 5, -165.0)])
def test_fused_one_slot_launch_against_the_host_loop(N, A, thr, dt):
    """The fused slot (env step + shaping + SPS decision in ONE launch, the observation handed over in LDS)."""
    cfg = bench_config(N, A, 30.0 * N + 100, reward_design=4 if N != 40 else 1)
    c = Case(cfg, {64: 12, 40: 16, 9: 64}[N], dt, [1] * 36, thr=thr, kernel="fused", want_chobs=(N == 40), counter_mod=4,
             expect=("both_paths", "raises") if N < 64 else ())        # (A = 32 at -110: every decision takes the shortcut)
    device_run(c)


def _fractional_x0(B, N, L, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, int(L) - 1, size=(B, N)).astype(np.float64) + rng.random((B, N))


FAST = {
    # K = 5 and 25 behind warm-ups of different length (t0 offsets), then a one-slot launch behind the K-slot ones
    "k5_a32": dict(cfg=c2_config(reward_design=4), dt=torch.float32, plan=[1] * 3 + [5, 5, 5, 5, 1], counter_mod=3),
    "k25_a33_thr150": dict(cfg=bench_config(64, 33, 2020.0, reward_design=1), dt=torch.float64, plan=[1] * 7 + [25, 25, 1], thr=-150.0),
    # mobility_vary: the episodes that end at t = 24 and 49 end inside the launches
    "vary_inside_a5": dict(cfg=bench_config(64, 5, 2020.0, reward_design=4, mobility_vary=True), dt=torch.float32,
                           plan=[1] * 10 + [25, 25], vel_seed=777, thr=-165.0, expect=("raises",)),
    # (mobility_vary starts every vehicle at 1.7: on integer positions the distances of different pairs agree to a few
    # ulps and the order of their log10 values is ambiguous - these cases start from fractional positions)
    "vary_rich_a7": dict(cfg=bench_config(40, 7, 1300.0, reward_design=5, mobility_vary=True, State=RICH), dt=torch.float64,
                         plan=[1] * 19 + [6, 6, 25], vel_seed=4242, keep=0.0, x0=_fractional_x0(24, 40, 1300.0, 7),
                         expect=("both_paths",)),
    "stuck_penalty_a2": dict(cfg=bench_config(64, 2, 2020.0, reward_design=2), dt=torch.float32, plan=[1] * 21 + [6, 6, 6], pen=True,
                             keep=0.8, counter_mod=3),
    "no_obs_a64_thr230": dict(cfg=bench_config(64, 64, 2020.0, reward_design=4), dt=torch.float32, plan=[1] * 3 + [25, 5],
                              want_obs=False, want_chobs=False, thr=-230.0, keep=0.0, expect=("raises",)),
    # communication_range 6000 on a 9 km highway: heard transmitters beyond 5 km refuse the shortcut
    "far_9km": dict(cfg=bench_config(64, 32, 9000.0, reward_design=4, communication_range=6000.0), dt=torch.float64,
                    plan=[1] * 2 + [5, 25], keep=0.0, expect=("far", "both_paths")),
    # ... and on a 30 km highway with a 20 km range they read below -160 (beyond 10 km), i.e. sort BEFORE the out-of-range
    # subframes: only here does the order the general path gives differ from the shortcut's
    "far_30km": dict(cfg=bench_config(64, 32, 30000.0, reward_design=4, communication_range=20000.0), dt=torch.float32,
                     plan=[1] * 2 + [5, 25], keep=0.0, expect=("far",)),
    # exp() rewards: the exp() bar
    "rd3_exp": dict(cfg=c2_config(reward_design=3), dt=torch.float64, plan=[1] * 2 + [5, 25], counter_mod=3),
}


@pytest.mark.parametrize("case", sorted(FAST))
def test_k_slots_on_fast64_against_the_host_loop(case):
    """K `my_step` slots in one launch at N <= 64 (the env kept on the chip), and the one-slot launches around them."""
    kw = dict(FAST[case])
    c = Case(kw.pop("cfg"), 24, kw.pop("dt"), kw.pop("plan"), **kw)
    env, host = device_run(c)
    if c.pen:
        assert int(host.pen_counter.max()) > 2                     # the penalty branch ran


CH = {
    "rd2_f32": dict(cfg=c2_config(reward_design=2), dt=torch.float32, plan=[1] * 3 + [5, 25, 1], counter_mod=3, expect=("both_paths",)),
    "rd4_exp_vary": dict(cfg=c2_config(reward_design=4, mobility_vary=True), dt=torch.float64, plan=[1] * 10 + [25, 25], vel_seed=777),
    "dense_40_6": dict(cfg=bench_config(40, 6, 900.0, reward_design=2, communication_range=30.0), dt=torch.float32,
                       plan=[1] * 2 + [6, 6, 25], keep=0.0, thr=-165.0, expect=("raises",)),
    "sparse_64_8": dict(cfg=bench_config(64, 8, 9000.0, reward_design=2, communication_range=100.0, State=RICH), dt=torch.float64,
                        plan=[1] * 12 + [9, 9, 9], expect=()),
}


@pytest.mark.parametrize("case", sorted(CH))
def test_k_slots_of_my_step_ch_against_the_host_loop(case):
    """K `my_step_ch` slots in one launch (the PRR reward and the PRR metric columns every slot); the one-slot calls of
    that mode are three launches each."""
    kw = dict(CH[case])
    c = Case(kw.pop("cfg"), 24, kw.pop("dt"), kw.pop("plan"), mode=STEP_MY_STEP_CH, **kw)
    device_run(c)


@pytest.mark.parametrize("N,form,dt", [(128, "packed", torch.float32), (128, "plane", torch.float64), (256, "packed", torch.float64),
                                       (256, "plane", torch.float32)])
def test_k_slots_on_step_wide_against_the_host_loop(N, form, dt, monkeypatch):
    """K slots in one launch at 65 to 256 vehicles (step_wide_slots_kernel), A = 64, both table forms."""
    cfg = bench_config(N, 64, 10.0 * N + 400, reward_design=4)
    # (N = 128 at -110: shortcut decisions; N = 256 at -165: four vehicles per resource leave few idle ones - raises)
    c = Case(cfg, 8, dt, [1] * 2 + [6, 6, 6, 1], form=form, keep=0.0 if N == 256 else 0.8, counter_mod=2 if N == 128 else 4,
             thr=-110.0 if N == 128 else -165.0, expect=("raises",) if N == 256 else ())
    device_run(c, monkeypatch)


def test_k_slots_on_a_wide_highway_that_breaks_apart(monkeypatch):
    """A sparse 128-vehicle packed highway with mobility_vary, long enough that entries fall beyond the codes inside the
    K-slot launches."""
    N, A, L, B = 128, 16, 4000.0, 6
    cfg = bench_config(N, A, L, mobility_vary=True, reward_design=4)
    rng = np.random.default_rng(N + A)
    x0 = rng.integers(0, int(L), size=(B, N)).astype(np.float64)
    x0[0] = np.concatenate([rng.integers(0, 1200, size=N // 2), rng.integers(2400, 3600, size=N - N // 2)])
    x0 += rng.random((B, N))                                      # (fractional positions: see FAST["vary_rich_a7"])
    c = Case(cfg, B, torch.float64, [1] * 20 + [25] * 4, x0=x0, form="packed", keep=0.5, vel_seed=99, want_chobs=False)
    env, host = device_run(c, monkeypatch)
    seq = host.export_state()["seq"]
    own = np.diagonal(seq, axis1=1, axis2=2)[:, None, :]
    assert bool(((own - seq >= 8) & (seq > 0)).any()), "no entry fell beyond the codes"


@pytest.mark.parametrize("N,A", [(64, 7), (128, 64)])
def test_clocked_slots_against_the_host_loop(N, A):
    """The clocked form, eager: the slot number and the policy's seed read from a device SlotClock (seed * 1000003 + offset
    + clock); one-slot and K-slot launches."""
    cfg = bench_config(N, A, 30.0 * N + 100 if N <= 64 else 10.0 * N + 400, reward_design=4)
    c = Case(cfg, 12 if N <= 64 else 6, torch.float32, [1] * 4 + [6, 25, 1], clock=True, counter_mod=3, keep=0.5,
             thr=-150.0 if A == 7 else -110.0, expect=("both_paths",) if A == 7 else ())
    device_run(c)


@pytest.mark.parametrize("mode,rd,dt", [("my_step_design", 2, torch.float64), ("my_step_ch", 2, torch.float32)])
def test_prefill_launch_against_the_host_loop(mode, rd, dt):
    """`diral_env_prefill_mode` (K slots of sample -> my_step_design / my_step_ch -> obtain_state in one launch, rich
    State) against HostClosedLoop.prefill: [K][B][N][S], actions_all, the next actions, tables, positions, metrics."""
    from diral_amd.vec_env import VecV2VEnv
    cfg = bench_config(40, 12, 900.0, State=RICH, reward_design=rd)
    B, N, A, K, seed = 24, 40, 12, 26, 77001
    npdt = np.float32 if dt == torch.float32 else np.float64
    env = VecV2VEnv(cfg, batch=B, device="cuda:0", out_dtype=dt)
    env.reset_topology(seed=5)
    x0, v0 = H.draw_topology(5, B, N, cfg.highway_length, False)
    host = H.HostClosedLoop(cfg, B, x0, v0, None, 0, dtype=npdt)
    a0 = H.draw_sample(123, B, N, A)
    assert np.array_equal(env.sample(123).cpu().numpy(), a0)
    _, rew = env.my_step(torch.as_tensor(a0, device="cuda:0"), 0)               # the bootstrap step: the stale reward column
    _, hrew = host.ob.my_step(a0, 0)
    assert np.array_equal(rew.cpu().numpy(), hrew.astype(npdt))
    rew_in = hrew.astype(npdt).astype(np.float64)                                # (what DriverLoop hands on: the handle's dtype)
    states, acts, nxt = env.prefill(env.sample(seed), K, seed, rew_in=rew_in, mode=mode)
    torch.cuda.synchronize()
    lk = env.last_kernel()
    assert (lk & 15) == KERNEL_FAST64 and (lk & KERNEL_POLICY) and bool(lk & KERNEL_CH) == (mode == "my_step_ch"), lk
    hs, ha, hn = host.prefill(H.draw_sample(seed, B, N, A), K, seed, rew_in=rew_in, mode=mode)
    assert np.array_equal(acts.cpu().numpy(), ha) and np.array_equal(nxt.cpu().numpy(), hn)
    assert len({ha[k].tobytes() for k in range(K)}) == K                         # every slot drew anew
    got = states.cpu().numpy()
    assert got.shape == hs.shape and np.array_equal(got, hs), np.argwhere(got != hs)[:4]
    st, he = env.export_state(), host.export_state()
    for k in ("pos_x", "vel", "seq", "age", "x"):
        assert np.array_equal(st[k].cpu().numpy(), he[k]), k
    m, hm = env.metrics().cpu().numpy(), host.metrics()
    metrics_equal(m, hm, "metrics", prr=mode == "my_step_ch")
    env.check()
