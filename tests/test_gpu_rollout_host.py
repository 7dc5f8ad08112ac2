"""The open-loop rollout launch (`diral_env_rollout`) against the HOST statement of the same loop: the CPU oracle step +
the driver's shaping in NumPy's order + the velocity mirror of tests/host_closed_loop.py, driven through the `Case` /
`host_run` helpers of tests/test_gpu_closed_loop_host.py with a GIVEN action sequence in the place of the SPS agent.
tests/test_gpu_rollout.py compares the launch with the device's own one-slot loop; here the second side shares no code
with the device.

Bars: those of tests/test_gpu_closed_loop_host.py - everything bit for bit, but exp()-based rewards (reward_design 3, and
4 in my_step_ch) within the exp() bar of tests/oracle_compare.py and what is summed from them within `_exp_bounds`; the metric float sums at rtol 1e-12,
atol 1e-9."""
import numpy as np
import pytest
import torch

from diral_amd.config import (KERNEL_CH, KERNEL_FAST64, KERNEL_PACKED, KERNEL_POLICY, KERNEL_WIDE, STEP_MY_STEP,
                              STEP_MY_STEP_CH, bench_config, c2_config)
from tests import host_closed_loop as H
from tests.oracle_compare import exp_atol, metrics_equal
from tests.host_closed_loop import MODE_NAME, RICH, Case, _eq, _exp_bounds, host_run, uses_exp

pytestmark = pytest.mark.gpu


class GivenActions:
    """Stands where HostSps stands in HostClosedLoop: slot k's "decision" is row k + 1 of a given sequence."""

    def __init__(self, seq):
        self.seq = np.ascontiguousarray(seq, dtype=np.int32)          # [T, B, N]
        self.k = 0
        self.log = []
        self.prev_action = self.seq[0].reshape(-1).copy()
        self.counter = np.zeros_like(self.prev_action)

    def step(self, chobs=None, actions=None, seed=None):
        assert np.array_equal(np.asarray(actions).reshape(-1), self.seq[self.k].reshape(-1))
        self.k += 1
        self.prev_action = self.seq[min(self.k, len(self.seq) - 1)].reshape(-1).copy()
        return self.prev_action.copy()


def _sequence(c, T, constant):
    if constant:
        return np.stack([H.draw_sample(9000 + (k // constant), c.B, c.N, c.A) for k in range(T)])
    return np.stack([H.draw_sample(7000 + k, c.B, c.N, c.A) for k in range(T)])


def run_case(c, states, monkeypatch, constant=0):
    """`c.plan`: the slots of each launch.  The host runs the same slots one by one (its result does not depend on how
    the slots are grouped) and keeps every slot's state vector."""
    from diral_amd.vec_env import VecV2VEnv
    T = sum(c.plan)
    seq = _sequence(c, T, constant)
    stub = GivenActions(seq)
    monkeypatch.setattr(H.HostSps, "from_seed", staticmethod(lambda *a, **k: stub))
    hc = Case(c.cfg, c.B, c.dt, [1] * T, mode=c.mode, pen=c.pen, vel_seed=c.vel_seed, x0=c.x0, topo_seed=c.topo_seed)
    host, (x0, v0), outs = host_run(hc)
    assert stub.k == T and not host.left_out.any()
    if c.cfg.mobility_vary:
        assert host.vel_updates > 0
    if c.form is not None:
        monkeypatch.setenv("DIRAL_TABLE_FORM", c.form)
    cfg, B, N, dt = c.cfg, c.B, c.N, c.dt
    env = VecV2VEnv(cfg, batch=B, device="cuda:0", out_dtype=dt)
    if c.x0 is not None:
        env.reset_topology(x0, None, v0)
    else:
        env.reset_topology(seed=c.topo_seed)                     # the device's own draws: the mirror's, bit for bit
        st = env.export_state(tables=False)
        assert np.array_equal(st["pos_x"].cpu().numpy(), x0) and np.array_equal(st["vel"].cpu().numpy(), v0)
    pn = None
    if c.pen:
        pn = (2, -10.0, torch.zeros((B, N), dtype=torch.int32, device="cuda:0"), torch.full((B, N), -1, dtype=torch.int32, device="cuda:0"))
    exp = uses_exp(cfg, c.mode)
    sum_atol, shaped_atol = _exp_bounds(N) if exp else (None, None)
    state_atol = exp_atol(exp and cfg.State.add_reward)
    keep = np.ones(B, bool)
    dseq = torch.as_tensor(seq, device="cuda:0")
    t = 0
    for li, K in enumerate(c.plan):
        got = env.rollout(dseq[t:t + K], t, mode=MODE_NAME[c.mode], states=states, global_reward_avg=True, stuck_penalty=pn,
                          vel_seed=c.vel_seed)
        torch.cuda.synchronize()
        lk = env.last_kernel()
        assert lk & KERNEL_POLICY and (lk & 15) == (KERNEL_WIDE if N > 64 else KERNEL_FAST64), lk
        assert bool(lk & KERNEL_CH) == (c.mode == STEP_MY_STEP_CH), lk
        if c.form is not None:
            assert bool(lk & KERNEL_PACKED) == (c.form == "packed"), lk
        tag = "launch %d (K = %d, t = %d): " % (li, K, t)
        for k in range(K):
            o = outs[t + k]
            _eq(tag + "shaped %d" % k, got["shaped"][k], o["shaped"][0], keep, 0, shaped_atol)
            _eq(tag + "sum_r %d" % k, got["sum_r"][k], o["sum_r"][0], keep, 0, sum_atol)
            _eq(tag + "collisions %d" % k, got["collision"][k], o["coll"][0], keep, 0, sum_atol)
            if states == "all":
                _eq(tag + "state %d" % k, got["states"][k], o["state"], keep, 0, state_atol)
        last = outs[t + K - 1]
        _eq(tag + "reward", got["reward"], last["rew"], keep, 0, exp_atol(exp))
        _eq(tag + "done", got["done"], last["done"], keep)
        if states == "last":
            _eq(tag + "state", got["states"], last["state"], keep, 0, state_atol)
        if pn is not None:
            _eq(tag + "penalty counter", pn[2], last["pen"][0], keep)
            _eq(tag + "penalty prev_actions", pn[3], last["pen"][1], keep)
        t += K
    st, he = env.export_state(), host.export_state()
    for k in ("pos_x", "vel", "seq", "age", "x"):
        _eq("export_state " + k, st[k], he[k], keep)
    m, hm = env.metrics().cpu().numpy(), host.metrics()
    metrics_equal(m, hm, "metrics", prr=c.mode == STEP_MY_STEP_CH)
    assert float(m[:, 0].min()) == T and (c.mode != STEP_MY_STEP_CH or float(m[:, 5].min()) > 0)
    env.check()
    return env, host


FAST = {
    "c2_f32_all": dict(cfg=c2_config(), dt=torch.float32, plan=[5, 25, 1], states="all"),
    "c2_rd3_exp_f64": dict(cfg=c2_config(reward_design=3), dt=torch.float64, plan=[6, 30], states="last"),
    "c2_rd1_none": dict(cfg=c2_config(reward_design=1), dt=torch.float32, plan=[25, 6], states=None),
    # mobility_vary: the episodes end at t = 24 (the last slot of the second launch) and 49 (inside the fourth)
    "vary_rich": dict(cfg=bench_config(40, 12, 900.0, State=RICH, mobility_vary=True), dt=torch.float64, plan=[20, 5, 6, 25],
                      states="all", vel_seed=4242),
    "stuck_penalty": dict(cfg=bench_config(64, 2, 2020.0), dt=torch.float32, plan=[6, 6, 6], states="last", pen=True, constant=9),
    "sparse": dict(cfg=bench_config(64, 8, 9000.0, communication_range=100.0, State=RICH), dt=torch.float64, plan=[12, 9, 9],
                   states="all"),
    "n8": dict(cfg=bench_config(8, 3, 440.0, State=RICH), dt=torch.float64, plan=[6, 25], states="all"),
    "n33": dict(cfg=bench_config(33, 7, 1190.0), dt=torch.float32, plan=[1, 5, 30], states="last"),
    "ch_rd2_f32": dict(cfg=c2_config(reward_design=2), dt=torch.float32, plan=[5, 25, 1], states="all", mode=STEP_MY_STEP_CH),
    "ch_rd3_exp": dict(cfg=c2_config(reward_design=3, State=RICH), dt=torch.float64, plan=[6, 6], states="all", mode=STEP_MY_STEP_CH),
    "ch_rd4_exp_vary": dict(cfg=c2_config(reward_design=4, mobility_vary=True), dt=torch.float64, plan=[30, 25], states="last",
                            mode=STEP_MY_STEP_CH, vel_seed=777),
    "ch_sparse_pen": dict(cfg=bench_config(64, 8, 9000.0, reward_design=2, communication_range=100.0, State=RICH), dt=torch.float64,
                          plan=[12, 9, 9], states="all", mode=STEP_MY_STEP_CH, pen=True, constant=5),
}


@pytest.mark.parametrize("case", sorted(FAST))
def test_rollout_on_fast64_against_the_host_loop(case, monkeypatch):
    """K slots of a given sequence at 8 <= N <= 64 (the env kept on the chip), my_step and my_step_ch."""
    kw = dict(FAST[case])
    states, constant = kw.pop("states"), kw.pop("constant", 0)
    c = Case(kw.pop("cfg"), 24, kw.pop("dt"), kw.pop("plan"), topo_seed=5, **kw)
    env, host = run_case(c, states, monkeypatch, constant)
    if c.pen:
        assert int(host.pen_counter.max()) > 2                     # the penalty branch ran


@pytest.mark.parametrize("N,form,dt", [(128, "packed", torch.float32), (128, "plane", torch.float64), (256, "packed", torch.float64),
                                       (256, "plane", torch.float32)])
def test_rollout_on_step_wide_against_the_host_loop(N, form, dt, monkeypatch):
    """... and at 65 to 256 vehicles (step_wide_slots_kernel), A = 64, both table forms, mobility_vary."""
    cfg = bench_config(N, 64, 10.0 * N + 400, reward_design=4, mobility_vary=True, State=dict(add_reward=True, add_velocity=True))
    c = Case(cfg, 8, dt, [6, 25, 1], form=form, vel_seed=99, topo_seed=5)
    run_case(c, "last", monkeypatch)
