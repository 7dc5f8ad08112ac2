"""State.piggybacking on the HIP path (piggyback_kernel.hpp) against the oracle and the reference fixtures.

The reference's branch (test_env.py:71-79, 241-254, 260-264) is defined while every receiver hears a transmitter
on every used resource, i.e. communication_range >= highway_length; beyond that its `self.prev_obs[tx_id]` raises
KeyError (tx_id None), which the build reports as the sticky DIRAL_ERR_PIGGY_NO_TX.  The fixtures recorded from
the reference itself (g1_piggyback*, g8_piggyback*) are replayed by test_gpu_parity.test_golden_replay_on_gpu;
here: larger random rollouts on every kernel family against the oracle - whose restatement replays np.insert on
real arrays, where the kernel walks the resources backwards per output position -, both output types, the
stand-alone obtain_state, the reference-shaped shim, and the calls the mode does not define.
"""
import numpy as np
import pytest
import torch

from diral_amd.config import (ERR_BAD_CONFIG, ERR_PIGGY_NO_TX, ERR_UNSUPPORTED, KERNEL_FAST64, KERNEL_GENERAL, KERNEL_WIDE,
                              STEP_DESIGN, STEP_MY_STEP, STEP_MY_STEP_CH, bench_config)
from tests.golden_util import Golden
from tests.gpu_util import gpu_step, make_env, random_rollout
from tests.oracle_compare import slot_equal

pytestmark = pytest.mark.gpu

PB = dict(piggybacking=True, add_channel_obs=True)


def pb_config(N, A, L, **kw):
    state = dict(PB, **kw.pop("State", {}))
    return bench_config(N, A, L, communication_range=L + 1.0, State=state, **kw)


@pytest.mark.parametrize("N,A,L,kw,kernel,general", [
    (64, 8, 400.0, dict(), KERNEL_FAST64, False),
    (64, 8, 400.0, dict(), KERNEL_GENERAL, True),
    (20, 5, 300.0, dict(reward_design=1, mobility_vary=True, State=dict(add_reward=True, add_index=True, add_velocity=True)),
     KERNEL_FAST64, False),
    (12, 16, 200.0, dict(State=dict(add_positional_dist=True, add_position=True), enable_fingerprint=True), KERNEL_FAST64, False),
    (33, 3, 500.0, dict(State=dict(add_positional_dist_type=1, num_bins=12)), KERNEL_FAST64, False),
    (130, 6, 600.0, dict(), KERNEL_WIDE, False),
    (200, 4, 900.0, dict(State=dict(add_positional_dist_piggy=False)), KERNEL_WIDE, False),
    (70, 70, 300.0, dict(), KERNEL_GENERAL, False),                # A > 64: the general kernel
])
def test_piggybacking_rollouts_vs_oracle(N, A, L, kw, kernel, general):
    cfg = pb_config(N, A, L, **kw)
    assert cfg.chobs_width == A * A and cfg.state_space >= A + A * A
    random_rollout(cfg, B=5, T=14, seed=900 + N + A, sticky=0.3, vel_every=6 if cfg.mobility_vary else None,
                   expect_kernel=kernel, force_general=general)


@pytest.mark.parametrize("N,A", [(64, 8), (130, 5)])
def test_piggybacking_f32_outputs_are_the_cast_of_f64(N, A):
    cfg = pb_config(N, A, 400.0)
    rng = np.random.default_rng(7)
    B = 4
    x0 = rng.integers(0, 400, size=(B, N)).astype(np.float64)
    v0 = rng.uniform(1.1, 2.7, size=(B, N))
    e64, e32 = make_env(cfg, B), make_env(cfg, B, dtype=torch.float32)
    for e in (e64, e32):
        e.reset_topology(x0, np.zeros((B, N)), v0)
    for t in range(8):
        a = rng.integers(0, A, size=(B, N)).astype(np.int32)
        o64, r64, c64, _ = gpu_step(e64, STEP_MY_STEP, a, t)
        o32, r32, c32, _ = gpu_step(e32, STEP_MY_STEP, a, t)
        assert c32.shape == (B, N, A * A) and c32.dtype == np.float32
        assert np.array_equal(c32, c64.astype(np.float32)) and np.array_equal(o32, o64.astype(np.float32))
        assert np.array_equal(r32, r64.astype(np.float32))
    assert np.array_equal(e32.prev_obs().cpu().numpy(), e64.prev_obs().cpu().numpy())     # prev_obs stays float64
    e64.check(); e32.check()


def test_piggybacking_prev_obs_round_trip_and_reset():
    """export / import of TestEnv.prev_obs: a second handle that imports state + prev_obs continues bit for bit;
    a reset zeroes it (test_env.py:76-79)."""
    N, A, B = 24, 6, 3
    cfg = pb_config(N, A, 300.0)
    rng = np.random.default_rng(11)
    x0 = rng.integers(0, 300, size=(B, N)).astype(np.float64)
    v0 = rng.uniform(1.1, 2.7, size=(B, N))
    a_env, b_env = make_env(cfg, B), make_env(cfg, B)
    a_env.reset_topology(x0, np.zeros((B, N)), v0)
    acts = [rng.integers(0, A, size=(B, N)).astype(np.int32) for _ in range(10)]
    for t in range(5):
        gpu_step(a_env, STEP_MY_STEP, acts[t], t)
    st = a_env.export_state()
    b_env.import_state(pos_x=st["pos_x"], pos_y=st["pos_y"], vel=st["vel"], seq=st["seq"], age=st["age"], x=st["x"])
    b_env.set_prev_obs(a_env.prev_obs())
    for t in range(5, 10):
        oa, ra, ca, _ = gpu_step(a_env, STEP_MY_STEP, acts[t], t)
        ob, rb, cb, _ = gpu_step(b_env, STEP_MY_STEP, acts[t], t)
        assert np.array_equal(ca, cb) and np.array_equal(oa, ob) and np.array_equal(ra, rb)
    assert a_env.prev_obs().abs().sum().item() > 0
    a_env.reset_topology(x0, np.zeros((B, N)), v0)
    assert a_env.prev_obs().abs().sum().item() == 0


def test_piggybacking_calls_the_mode_does_not_define():
    from diral_amd.sps import SpsPolicy
    from diral_amd.vec_env import DiralError
    N, A, B = 16, 4, 2
    env = make_env(pb_config(N, A, 200.0), B)
    env.reset_topology(seed=3)
    a = env.sample(seed=1)
    # my_step_ch / my_step_design return the plain A-wide observation (test_env.py:316, 443): no state vector of
    # get_state_space() columns exists for them
    for mode in (STEP_MY_STEP_CH, STEP_DESIGN):
        with pytest.raises(DiralError) as ei:
            env._step(mode, a, 0, want_chobs=True)
        assert ei.value.status == ERR_BAD_CONFIG
    pol = SpsPolicy(B, N, A, device=env.device, seed=5)
    with pytest.raises(DiralError) as ei:
        env.step_policy(a, 0, pol, torch.empty_like(a), want_chobs=True)
    assert ei.value.status == ERR_UNSUPPORTED
    # a handle without the flag has no prev_obs
    plain = make_env(bench_config(N, A, 200.0), B)
    with pytest.raises(DiralError) as ei:
        plain.prev_obs()
    assert ei.value.status == ERR_BAD_CONFIG


def test_piggybacking_receiver_out_of_range_raises_like_the_reference():
    """communication_range < highway_length: the first slot in which some receiver hears nobody on a used resource is
    the slot the oracle (and the reference: g8_piggyback_keyerror) raises KeyError in; the device flag is raised in
    exactly that slot, in exactly the envs concerned."""
    from oracle.oracle import Oracle, SQ_IEEE
    from diral_amd.vec_env import DiralError
    N, A = 10, 3
    cfg = bench_config(N, A, 1000.0, communication_range=400.0, State=PB)
    rng = np.random.default_rng(21)
    raised = 0
    for trial in range(6):
        x0 = rng.integers(0, 300, size=(1, N)).astype(np.float64) + 650.0     # a cluster about to wrap around
        v0 = rng.uniform(1.1, 2.7, size=(1, N))
        env = make_env(cfg, 1)
        env.reset_topology(x0, np.zeros((1, N)), v0)
        orc = Oracle(cfg, batch=1, sq_mode=SQ_IEEE)
        orc.reset(x0, np.zeros((1, N)), v0)
        for t in range(60):
            a = rng.integers(0, A, size=(1, N)).astype(np.int32)
            obs, rew, chobs, _ = gpu_step(env, STEP_MY_STEP, a, t)
            try:
                o_rew, o_chobs = orc.step(STEP_MY_STEP, a, t)
            except KeyError:
                with pytest.raises(DiralError) as ei:
                    env.check()
                assert ei.value.status == ERR_PIGGY_NO_TX
                raised += 1
                break
            env.check()
            slot_equal(cfg, STEP_MY_STEP, (None, rew, chobs), (None, o_rew, o_chobs), (trial, t))
    assert raised >= 3


@pytest.mark.parametrize("name", ["g1_piggyback", "g8_piggyback_n6_a4"])
def test_piggybacking_shim_reads_like_the_reference(name):
    """diral_amd.TestEnv (B = 1, the reference's Python shapes) on the GPU against the recorded reference outputs."""
    from diral_amd.compat import TestEnv
    g = Golden(name)
    env = TestEnv(device="cuda:0", **g.cfg_dict)
    env._env.reset_topology(g["x0"], g["y0"], g["v0"])
    A = g.cfg.num_channels
    assert env.get_state_space() == int(g["state_space"])
    for i, mode, acts, t, (ep, eps) in g.steps():
        obs, rews = env.my_step(acts, t)
        assert all(obs[u].shape == (A * A,) for u in range(g.N))
        st = env.obtain_state(obs, acts, rews, ep, eps)
        got = np.array([obs[u] for u in range(g.N)])
        assert np.array_equal(got, g["chobs"][i]) or np.max(np.abs(got - g["chobs"][i])) < 1e-12
        assert np.allclose(np.array(st), g["state"][i], rtol=0, atol=1e-12)
        assert np.array_equal(rews, g["rews"][i])
