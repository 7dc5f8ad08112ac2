"""K slots per launch of the `my_step_ch` closed loop at N <= 64 (step_fast64_slots_kernel<..., CH, ..., POL>):
`diral_env_step_policy(DIRAL_STEP_MY_STEP_CH)` with DiralSlotPolicy::slots = K > 1 against K one-slot calls - in this
mode each of those is three launches (the step with the channel observation, diral_driver_shape, diral_sps_step_chobs) -
bit for bit, against the CPU oracle, and the refusals."""
import numpy as np
import pytest
import torch

from diral_amd.config import (ERR_BAD_CONFIG, ERR_UNSUPPORTED, KERNEL_CH, KERNEL_FAST64, KERNEL_POLICY, STEP_MY_STEP_CH,
                              bench_config, c2_config)
from tests.kslots_harness import RICH, assert_same_envs, closed_loop_twins, compare_closed_loop
from tests.oracle_compare import metrics_equal, tables_equal

pytestmark = pytest.mark.gpu


def _is_ch_slots_kernel(lk):
    return (lk & 15) == KERNEL_FAST64 and bool(lk & KERNEL_POLICY) and bool(lk & KERNEL_CH)


def in_range_counts(x, a, rc):
    """test_env.py:395-397 on the one-lane highway: for every transmitter of a resource more than one vehicle transmits
    on, the number of vehicles on OTHER resources closer than `rc`; -1 for a transmitter that is alone.  x, a: [B, N]."""
    x, a = np.asarray(x, dtype=np.float64), np.asarray(a)
    same = a[:, :, None] == a[:, None, :]                                  # [B, tx, rx]
    coll = same.sum(2) > 1
    near = np.abs(x[:, :, None] - x[:, None, :]) < rc
    n_in = (near & ~same).sum(2)
    return np.where(coll, n_in, -1)


def _one_slot_is_three_launches(lk):
    return lk & KERNEL_POLICY == 0 and bool(lk & KERNEL_CH)


def _ch_twins(cfg, B, dt, K, t0, *, want_obs=True, keep=0.8, vel_seed=0, pen=False):
    """tests/kslots_harness.closed_loop_twins in this file's mode, with the start behind the warm-up kept."""
    return closed_loop_twins(cfg, B, dt, K, t0, topo=21, pol_seed=3, keep=keep, mode=STEP_MY_STEP_CH, want_obs=want_obs,
                             want_chobs=True, vel_seed=vel_seed, pen=pen, want_start=True,
                             expect_one=_one_slot_is_three_launches, expect_fused=_is_ch_slots_kernel)


def _compare_and_go_on(runs, want_obs=True):
    """The shared comparison; then what this file adds: the PRR columns were paid, and the envs go on alike - three plain
    slots, the state and the metrics once more, the sticky flags."""
    compare_closed_loop(runs, want_obs=want_obs, want_chobs=True, check=False)
    e1, e2 = runs[0].env, runs[1].env
    assert float(e1.metrics()[:, 5].min()) > 0.0                 # DIRAL_M_PRR_CNT: the PRR columns were paid
    for t in range(3):
        a = e1.sample(900 + t)
        q1, r1, _ = e1.step(a, t)
        q2, r2, _ = e2.step(a, t)
        assert torch.equal(q1, q2) and torch.equal(r1, r2), t
    sa = assert_same_envs(e1, e2, entries=False)
    e1.check()
    e2.check()
    return sa


CASES = {
    "c2_rd2_f32": dict(cfg=c2_config(reward_design=2), dt=torch.float32, K=5, t0=3),
    # episode_interval 25: the episode that ends at t = 24 ends inside both launches' range (t = 10 ... 59)
    "rd3_f64_vary": dict(cfg=c2_config(reward_design=3, mobility_vary=True), dt=torch.float64, K=25, t0=10, vel_seed=777),
    "rd4_rich": dict(cfg=c2_config(reward_design=4, State=RICH), dt=torch.float32, K=6, t0=4),
    # dense: 40 vehicles on 6 resources collide nearly always; a 30 m range leaves some transmitters nobody to reach (R = 1)
    "dense_40_6": dict(cfg=bench_config(40, 6, 900.0, reward_design=2, communication_range=30.0), dt=torch.float32, K=6, t0=2),
    "sparse_64_8": dict(cfg=bench_config(64, 8, 9000.0, reward_design=2, communication_range=100.0), dt=torch.float32, K=9,
                        t0=12),                                  # keyed quads
    "n8": dict(cfg=bench_config(8, 4, 400.0, reward_design=2), dt=torch.float64, K=6, t0=2),
    "n33": dict(cfg=bench_config(33, 7, 1200.0, reward_design=3), dt=torch.float32, K=6, t0=2),      # padded lanes
    "stuck_penalty": dict(cfg=c2_config(reward_design=2), dt=torch.float32, K=6, t0=21, keep=0.95, pen=True),
    "no_obs": dict(cfg=c2_config(reward_design=2), dt=torch.float32, K=25, t0=3, want_obs=False),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_ch_k_slots_equal_k_one_slot_calls(case):
    """K `my_step_ch` slots in one launch equal K one-slot calls (three launches each): per-slot shaped rewards / sums /
    collisions, the last slot's state, reward, done and channel observation, the next actions, the policy state, the
    exported tables, positions, velocities and the metrics - the PRR sum and count included -, then three more plain
    slots on both handles.  exp()-based rewards (reward_design 3) bit for bit too: both sides are the same device function."""
    kw = dict(CASES[case])
    cfg, dt, K, t0 = kw.pop("cfg"), kw.pop("dt"), kw.pop("K"), kw.pop("t0")
    want_obs = kw.get("want_obs", True)
    runs = _ch_twins(cfg, 24, dt, K, t0, **kw)
    if case == "dense_40_6":
        n_in = in_range_counts(runs[1].start[0], runs[1].start[1], cfg.communication_range)
        assert (n_in == 0).any() and (n_in > 0).any()             # both sides of `R = received / in_range` ran
        assert (n_in >= 0).mean() > 0.5                           # most transmitters collide
    sa = _compare_and_go_on(runs, want_obs=want_obs)
    if cfg.mobility_vary:
        assert not torch.equal(sa["vel"], torch.full_like(sa["vel"], 1.7))      # an episode ended inside the launches
    if case == "stuck_penalty":
        assert int(runs[1].pen[2].max()) > 2
    if case == "sparse_64_8":
        seq = sa["seq"]
        own = torch.diagonal(seq, dim1=1, dim2=2).unsqueeze(1)
        assert bool(((own - seq >= 8) & (seq > 0)).any()), "no entry fell beyond the codes"


# the shape of the oracle anchor: 16 vehicles on 4 resources over 3 km with a 100 m range - nearly every transmitter
# collides, and about half of them have no vehicle of another resource in range
ANCHOR = dict(N=16, A=4, L=3000.0, rc=100.0, B=16, K=12, seed=5)


def anchor_inputs():
    c = ANCHOR
    cfg = bench_config(c["N"], c["A"], c["L"], reward_design=2, communication_range=c["rc"])
    rng = np.random.default_rng(c["seed"])
    x0 = rng.integers(0, int(c["L"]), size=(c["B"], c["N"])).astype(np.float64)
    v0 = rng.uniform(1.1, 2.7, size=(c["B"], c["N"]))
    a = rng.integers(0, c["A"], size=(c["B"], c["N"])).astype(np.int32)
    return cfg, x0, v0, a


def anchor_oracle(cfg, x0, v0, a, K):
    """K `my_step_ch` slots of the CPU oracle on constant actions; returns (backend, last reward, last observation,
    in_range counts of every slot)."""
    from tests.oracle_backend import OracleBackend
    ob = OracleBackend(cfg, batch=x0.shape[0])
    ob.reset_topology(x0, np.zeros_like(x0), v0)
    n_in = []
    for t in range(K):
        n_in.append(in_range_counts(ob.get_x_pos(), a, cfg.communication_range))
        chobs, rew = ob.my_step_ch(a, t)
    return ob, rew, chobs, np.stack(n_in)


def test_ch_k_slots_against_the_cpu_oracle():
    """One launch of K = 12 `my_step_ch` slots with keep_prob = 1 (no agent ever re-selects: the actions stay slot 0's; the
    loop with agents that do re-select is checked against a host SPS in tests/test_gpu_closed_loop_host.py) against tests/oracle_backend.OracleBackend stepped K times on the same actions: positions and tables
    bit for bit, the last slot's reward and channel observation bit for bit, the PRR count exact and the PRR sum within
    the suite's tolerance for that column (test_gpu_parity: rtol 1e-12, atol 1e-9 - the summation order differs)."""
    from diral_amd.sps import SpsPolicy
    from diral_amd.vec_env import VecV2VEnv
    cfg, x0, v0, a_np = anchor_inputs()
    B, N, A, K = ANCHOR["B"], ANCHOR["N"], ANCHOR["A"], ANCHOR["K"]
    ob, o_rew, o_chobs, n_in = anchor_oracle(cfg, x0, v0, a_np, K)
    # neither branch of `R = received / in_range if in_range > 0 else 1` is vacuous
    assert (n_in == 0).any(axis=(0, 2)).any() and (n_in > 0).any(axis=(0, 2)).any()
    env = VecV2VEnv(cfg, batch=B, device="cuda:0", out_dtype=torch.float64)
    env.reset_topology(x0, 0.0, v0)
    pol = SpsPolicy(B, N, A, device="cuda:0", seed=1)
    pol.keep_prob = 1.0
    a = torch.as_tensor(a_np, device="cuda:0")
    pol.prev_action.copy_(a)
    nxt = torch.empty_like(a)
    env.step_policy(a, 0, pol, nxt, slots=K, mode=STEP_MY_STEP_CH, want_chobs=True)
    torch.cuda.synchronize()
    assert _is_ch_slots_kernel(env.last_kernel()), env.last_kernel()
    assert torch.equal(nxt, a)                                   # nobody re-selected
    assert np.array_equal(env._rew.cpu().numpy(), o_rew)
    assert np.array_equal(env._chobs.cpu().numpy(), o_chobs)
    st = {k: v.cpu().numpy() for k, v in env.export_state().items()}
    oe = ob.export_state()
    tables_equal(st, oe, "end")
    metrics_equal(env.metrics().cpu().numpy(), ob.o.metrics(), "end", prr=True)
    env.check()


def test_ch_k_slots_refusals_leave_the_env_untouched():
    """my_step_ch with slots = 4 and arrival stamps, or vehicles off the lane: DIRAL_ERR_UNSUPPORTED; with reward_design 1:
    DIRAL_ERR_BAD_CONFIG.  Nothing is launched: export_state() and the policy state are unchanged."""
    from diral_amd.sps import SpsPolicy
    from diral_amd.vec_env import DiralError, VecV2VEnv
    B = 4
    cases = [("arrival_stamps", c2_config(reward_design=2, track_arrival=True), ERR_UNSUPPORTED),
             ("reward_design_1", c2_config(reward_design=1), ERR_BAD_CONFIG),
             ("off_lane", c2_config(reward_design=2), ERR_UNSUPPORTED)]
    for name, cfg, status in cases:
        env = VecV2VEnv(cfg, batch=B, device="cuda:0")
        N, A = cfg.num_users, cfg.num_channels
        if name == "off_lane":
            rng = np.random.default_rng(1)
            env.reset_topology(rng.integers(0, 2000, size=(B, N)).astype(np.float64), rng.uniform(0, 5, size=(B, N)),
                               np.full((B, N), 1.7))
        else:
            env.reset_topology(seed=2)
        pol = SpsPolicy(B, N, A, device="cuda:0", seed=1)
        a = pol.prev_action.clone()
        nxt = torch.empty_like(a)
        before = {k: v.clone() for k, v in env.export_state().items()}
        prev, cnt, steps = pol.prev_action.clone(), pol.counter.clone(), pol._t
        with pytest.raises(DiralError) as ei:
            env.step_policy(a, 0, pol, nxt, slots=4, mode=STEP_MY_STEP_CH)
        assert ei.value.status == status, (name, str(ei.value))
        torch.cuda.synchronize()
        after = env.export_state()
        for k in before:
            assert torch.equal(before[k], after[k]), (name, k)
        assert torch.equal(pol.prev_action, prev) and torch.equal(pol.counter, cnt) and pol._t == steps, name
        env.check()
