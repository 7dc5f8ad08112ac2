"""P1 of the 64-vehicle step kernel (csrc/step_fast64_body.inc) at the resource counts where dealing resources to the
four waves can go wrong, against the CPU oracle (IEEE squares), bit for bit: state, reward, channel observation every
slot for 30 slots, then tables, positions, velocities and metrics through the handle's export.

Resource counts: 1, 3, 4, 5, 13, 16, 17, 32, 33, 63, 64 - a partial last group of four resources (1, 3, 5, 13, 17, 33,
63), fewer groups than waves (1 ... 13: some waves own nothing), exactly one group per wave (16), more than two groups
per wave (33, 63, 64) and the 64-mask form of `s_mask` (33 ... 64).  Vehicle counts 8, 33 and 64 (padded lanes).  Six
envs; env 0 is built by hand: vehicles 0 - 2 transmit on resource 0 every slot from one end of the highway, some
receivers within range of them and the others out of range of all three, and the last resource is never used (with
one resource there is no second one to leave unused).

Which (N, A) pairs run on step_fast64: `plan_step` (csrc/diral_env.hip) takes every handle with one vehicle per lane
(N <= 64) and A <= 64 whose configuration is one of the specialised ones - every pair of this file; none is refused,
none skipped, and every case asserts `last_kernel()`.  The K-slot forms need N >= 8, which holds too.

The oracle runs once per (N, A, mode); the float32 / float64 and with / without channel-observation variants of a
mode share that reference (float32 outputs are the float32 cast of the float64 values)."""
import functools

import numpy as np
import pytest
import torch

from diral_amd.config import KERNEL_FAST64, KERNEL_POLICY, STEP_DESIGN, STEP_MY_STEP, STEP_MY_STEP_CH, bench_config
from tests.gpu_util import exported, host, make_env, ran_on
from tests.kslots_harness import check_rollout, closed_loop_twins, compare_closed_loop
from tests.oracle_compare import metrics_equal, same, slot_equal, tables_equal

pytestmark = pytest.mark.gpu

A_VALUES = (1, 3, 4, 5, 13, 16, 17, 32, 33, 63, 64)
N_VALUES = (8, 33, 64)
B, T = 6, 30
L, RC = 2000.0, 180.0
RICH_STATE = dict(add_channel_obs=True, add_reward=True, add_index=True, add_velocity=True, add_position=True)
# kind -> (step mode, config overrides).  reward_design 1 in the RICH case: the collision reward of a resource is then
# computed per resource in P1 (`need_rw`, s_rv[i]) instead of for all resources at once in P2
KINDS = {
    "my_step": (STEP_MY_STEP, dict()),
    "my_step_ch": (STEP_MY_STEP_CH, dict()),
    "design": (STEP_DESIGN, dict(track_arrival=True)),                       # an EXTRA instantiation, arrival stamps
    "rich": (STEP_MY_STEP, dict(reward_design=1, State=RICH_STATE)),
}


def _cfg(N, A, kind):
    return bench_config(N, A, L, communication_range=RC, **KINDS[kind][1])


def _n_for(A):
    """One vehicle count per resource count for the cases that do not cross both."""
    return N_VALUES[A_VALUES.index(A) % 3]


def _topology(rng, N):
    x0 = rng.integers(0, int(L), size=(B, N)).astype(np.float64)
    # env 0: three transmitters at one end; half of the others within RC of all three, the rest beyond RC of all three
    # (no vehicle wraps around or crosses that boundary in T slots of at most 2.7 m)
    near = 3 + (N - 3) // 2
    x0[0, :3] = (100.0, 103.0, 106.0)
    x0[0, 3:near] = np.linspace(120.0, 170.0, near - 3)
    x0[0, near:] = np.linspace(700.0, 1700.0, N - near)
    v0 = rng.uniform(1.1, 2.7, size=(B, N))
    return x0, v0


def _actions(rng, N, A):
    a = rng.integers(0, A, size=(B, N)).astype(np.int32)
    a[0] = rng.integers(0, max(A - 1, 1), size=N)                            # resource A - 1: nobody
    a[0, :3] = 0                                                             # resource 0: at least three transmitters
    return a


@functools.lru_cache(maxsize=None)
def reference(N, A, kind):
    """The oracle's T slots of one (N, A, kind): inputs, per-slot outputs, final export and metrics.  Never modified."""
    from oracle.oracle import Oracle, SQ_IEEE
    mode, cfg = KINDS[kind][0], _cfg(N, A, kind)
    rng = np.random.default_rng(1000 * N + 10 * A + len(kind))
    x0, v0 = _topology(rng, N)
    orc = Oracle(cfg, batch=B, sq_mode=SQ_IEEE, threads=4)
    orc.reset(x0, np.zeros((B, N)), v0)
    slots = []
    for t in range(T):
        acts = _actions(rng, N, A)
        rew, chobs = orc.step(mode, acts, t)
        slots.append((acts, rew.copy(), chobs.copy(), orc.obtain_state(acts, chobs, rew).copy()))
    # what the hand-built env is there for
    if A > 1:
        assert not any((s[0][0] == A - 1).any() for s in slots)
    if mode == STEP_MY_STEP and A >= 4:                                      # (the other two modes observe 0 / 1, not distances)
        co = np.stack([s[2][0, 3:, 0] for s in slots])                       # env 0, the receivers' view of resource 0
        assert (co == 100000.0).any() and ((co > 0.0) & (co < RC)).any()     # out of range of all three / in range
    return dict(x0=x0, v0=v0, slots=slots, export=orc.export(), metrics=orc.metrics(), info_age=orc.info_age(T - 1))


def _run(N, A, kind, dtype, chobs):
    mode, cfg = KINDS[kind][0], _cfg(N, A, kind)
    ref = reference(N, A, kind)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    env = make_env(cfg, B, mode=mode, dtype=dtype)
    env.reset_topology(ref["x0"], np.zeros((B, N)), ref["v0"])
    for t, (acts, o_rew, o_chobs, o_state) in enumerate(ref["slots"]):
        obs, rew, _ = env._step(mode, env._actions(acts), t, 0.0, 1.0, want_chobs=chobs)
        ran_on(env, KERNEL_FAST64)
        got = (host(obs), host(rew), host(env._chobs) if chobs else None)
        slot_equal(cfg, mode, got, (o_state, o_rew, o_chobs), (N, A, kind, t), npdt)
    tables_equal(exported(env), ref["export"], (N, A, kind))
    if cfg.track_arrival:
        same(host(env.info_age(T - 1)), ref["info_age"], (N, A, kind, "information age"))
    metrics_equal(host(env.metrics()), ref["metrics"], (N, A, kind), prr=mode == STEP_MY_STEP_CH)
    env.check()


@pytest.mark.parametrize("chobs", [True, False], ids=["chobs", "nochobs"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("N", N_VALUES)
@pytest.mark.parametrize("A", A_VALUES)
def test_my_step_vs_oracle(A, N, dtype, chobs):
    _run(N, A, "my_step", dtype, chobs)


@pytest.mark.parametrize("N", N_VALUES)
@pytest.mark.parametrize("A", A_VALUES)
def test_my_step_ch_vs_oracle(A, N):
    """The reception ratios: `s_inr` / `s_rtx` per transmitter, written and read back inside one resource's turn."""
    _run(N, A, "my_step_ch", torch.float64, True)


@pytest.mark.parametrize("A", A_VALUES)
def test_my_step_design_with_arrival_stamps_vs_oracle(A):
    _run(_n_for(A), A, "design", torch.float64, True)


@pytest.mark.parametrize("A", A_VALUES)
def test_rich_state_with_per_resource_rewards_vs_oracle(A):
    _run(_n_for(A), A, "rich", torch.float32 if A % 2 else torch.float64, True)


@pytest.mark.parametrize("A", A_VALUES)
def test_step_policy_of_five_slots_equals_five_one_slot_calls(A):
    """The K-slot compilation of the same text (step_fast64_slots_kernel), the SPS agents reading the staged rows."""
    N, K = _n_for(A), 5
    x0, v0 = _topology(np.random.default_rng(77 + A), N)
    runs = closed_loop_twins(_cfg(N, A, "my_step"), B, torch.float32, K, 3, topo=(x0, 0.0, v0), pol_seed=5, keep=0.7,
                             expect_fused=lambda lk: (lk & 15) == KERNEL_FAST64 and bool(lk & KERNEL_POLICY))
    compare_closed_loop(runs)


@pytest.mark.parametrize("A", A_VALUES)
def test_rollout_of_five_slots_equals_five_one_slot_calls(A):
    """`rollout(K = 5)` with every slot's state against the loop of step + shaping calls on a twin env."""
    N = _n_for(A)
    x0, _ = _topology(np.random.default_rng(99 + A), N)
    _, _, env = check_rollout(_cfg(N, A, "my_step"), B, torch.float32 if A % 2 else torch.float64, 5, states="all", warm=3, x0=x0)
    # (`check_rollout` asserts the family and the policy bit behind each of its launches; once more here, on a launch of this
    # file's own, so that a fallback to one-slot launches cannot pass unseen)
    seq = torch.stack([env.sample(300 + k) for k in range(5)])
    got = env.rollout(seq, env.t, states="all")
    lk = env.last_kernel()
    assert (lk & 15) == KERNEL_FAST64 and (lk & KERNEL_POLICY), lk
    assert got["states"].shape[0] == 5
    env.check()
