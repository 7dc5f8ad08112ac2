"""The write-out loops of the 64-vehicle step kernel (csrc/step_fast64_body.inc) - the state rows [one-hot(A) |
histogram(K)] of P4 and the channel observation, both starting from a row and piece computed with the host's
multiply-shift reciprocals (csrc/step_params.hpp, WriteoutParams; the K-slot kernel keeps P4's own division) - against
the CPU oracle (IEEE squares), bit for bit: state, reward and channel observation of every slot for 12 slots.

Shapes, chosen where the mapping of threads to rows and 16-byte pieces can go wrong:
* N = 8, 33, 64: padded lanes, row counts the writing threads do not divide (192 threads with `late_p2`, else 256);
* (A, State.num_bins) = (4, 4), (8, 20), (32, 20), (64, 24), (12, 8), (32, 4), (28, 36), (4, 64): the vector path with one
  piece per row and section, an odd number, more pieces in a row than a wave has lanes; (5, 20), (32, 10), (33, 7): the
  element-wise fallbacks (float64 outputs take (32, 10) on the vector path: pieces of two).  A / 4 and A / 2 run through
  1, 2, 3, 4, 6, 7, 8, 14, 16, 32, the pieces per state row (A + K) / 4 and / 2 through 2, 4, 5, 7, 9, 10, 13, 14, 16, 17, 18,
  21, 22, 26, 32, 34, 44: reciprocals of powers of two and of others;
* float32 and float64 outputs, with and without the channel observation;
* plain `my_step` (`late_p2`: waves 1-3 write the rows) and a one-slot `step_policy` call (POL: all four waves do);
* `rollout(states="all")` and `prefill` of three slots at (64, 32, 20): every slot's rows through the same text in the
  K-slot kernel.
Six envs.  In env 4 vehicle 0 stays out of everybody's range: it hears nobody, n = 0, an all-zero histogram row.  In env 5
every vehicle picks the last resource every slot: the 1 sits in the last piece of the one-hot section.

The oracle runs once per (N, A, num_bins); every variant shares that reference (float32 outputs are the float32 cast
of the float64 values).

Not marked `gpu`: the integer identities behind the float32 screening of the bin (`column32`) and the range of the
multiply-shift reciprocal, swept in NumPy."""
import functools

import numpy as np
import pytest
import torch

from diral_amd.config import KERNEL_FAST64, KERNEL_POLICY, STEP_DESIGN, STEP_MY_STEP, bench_config
from tests.gpu_util import host, make_env
from tests.oracle_compare import slot_equal

gpu = pytest.mark.gpu

N_VALUES = (8, 33, 64)
VECTOR_SHAPES = ((4, 4), (8, 20), (32, 20), (64, 24), (12, 8), (32, 4), (28, 36), (4, 64))
FALLBACK_SHAPES = ((5, 20), (32, 10), (33, 7))
SHAPES = VECTOR_SHAPES + FALLBACK_SHAPES
B, T = 6, 12
L, RC = 2000.0, 180.0
ALONE, LAST = 4, 5                                                           # the two hand-built envs


def _cfg(N, A, K):
    return bench_config(N, A, L, communication_range=RC, State=dict(num_bins=K))


def _topology(rng, N):
    x0 = rng.integers(0, int(L), size=(B, N)).astype(np.float64)
    # env ALONE: vehicle 0 more than RC + T * 2.7 m from the others (nobody wraps around in T slots)
    x0[ALONE, 0] = 1500.0
    x0[ALONE, 1:] = np.linspace(100.0, min(1200.0, 100.0 + 40.0 * (N - 2)), N - 1)          # (within RC of their neighbours)
    v0 = rng.uniform(1.1, 2.7, size=(B, N))
    return x0, v0


def _actions(rng, N, A):
    a = rng.integers(0, A, size=(B, N)).astype(np.int32)
    a[LAST] = A - 1
    return a


@functools.lru_cache(maxsize=None)
def reference(N, A, K):
    """The oracle's T slots of `my_step` at one shape: inputs and per-slot outputs.  Never modified."""
    from oracle.oracle import Oracle, SQ_IEEE
    rng = np.random.default_rng(100000 * N + 100 * A + K)
    x0, v0 = _topology(rng, N)
    orc = Oracle(_cfg(N, A, K), batch=B, sq_mode=SQ_IEEE, threads=4)
    orc.reset(x0, np.zeros((B, N)), v0)
    slots = []
    for t in range(T):
        acts = _actions(rng, N, A)
        rew, chobs = orc.step(STEP_MY_STEP, acts, t)
        slots.append((acts, rew.copy(), chobs.copy(), orc.obtain_state(acts, chobs, rew).copy()))
    # what the two hand-built envs are there for
    states = np.stack([s[3] for s in slots])                                 # [T, B, N, A + K]
    assert states.shape[-1] == A + K
    assert not states[:, ALONE, 0, A:].any() and states[:, ALONE, 1:, A:].any()
    assert (states[:, LAST, :, A - 1] == 1.0).all() and not states[:, LAST, :, :A - 1].any()
    return dict(x0=x0, v0=v0, slots=slots)


def _same(got, want, where):
    got = got.cpu().numpy()
    assert np.array_equal(got, want), (where, np.argwhere(got != want)[:5])


def _run(N, A, K, dtype, chobs, pol):
    cfg, ref = _cfg(N, A, K), reference(N, A, K)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    env = make_env(cfg, B, dtype=dtype)
    env.reset_topology(ref["x0"], np.zeros((B, N)), ref["v0"])
    if pol:
        from diral_amd.sps import SpsPolicy
        policy = SpsPolicy(B, N, A, device="cuda:0", seed=5)
        nxt = torch.empty((B, N), dtype=torch.int32, device="cuda:0")
    for t, (acts, o_rew, o_chobs, o_state) in enumerate(ref["slots"]):
        a = env._actions(acts)
        if pol:
            obs, rew, _ = env.step_policy(a, t, policy, nxt, want_chobs=chobs)
        else:
            obs, rew, _ = env._step(STEP_MY_STEP, a, t, 0.0, 1.0, want_chobs=chobs)
        torch.cuda.synchronize()
        lk = env.last_kernel()
        assert (lk & 15) == KERNEL_FAST64 and bool(lk & KERNEL_POLICY) == pol, lk
        got = (host(obs), host(rew), host(env._chobs) if chobs else None)
        slot_equal(cfg, STEP_MY_STEP, got, (o_state, o_rew, o_chobs), (N, A, K, t), npdt)
    env.check()


@gpu
@pytest.mark.parametrize("chobs", [True, False], ids=["chobs", "nochobs"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("N", N_VALUES)
@pytest.mark.parametrize("A,K", SHAPES)
def test_my_step_state_rows_and_channel_observation_vs_oracle(A, K, N, dtype, chobs):
    _run(N, A, K, dtype, chobs, pol=False)


@gpu
@pytest.mark.parametrize("N", N_VALUES)
@pytest.mark.parametrize("A,K", SHAPES)
def test_one_slot_step_policy_state_rows_and_channel_observation_vs_oracle(A, K, N):
    """POL: P2 runs in front of the last barrier and all four waves write rows.  Output dtype and the channel
    observation alternate over the shapes (both dtypes and both forms at every N)."""
    i = SHAPES.index((A, K)) + N_VALUES.index(N)
    _run(N, A, K, torch.float64 if i % 2 else torch.float32, (i // 2) % 2 == 0, pol=True)


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_rollout_of_three_slots_writes_every_slots_rows(dtype):
    N, A, K = 64, 32, 20
    ref = reference(N, A, K)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    env = make_env(_cfg(N, A, K), B, dtype=dtype)
    env.reset_topology(ref["x0"], np.zeros((B, N)), ref["v0"])
    t = 0
    for rep in range(2):                                                     # the second launch continues the first
        seq = torch.stack([env._actions(ref["slots"][t + k][0]).clone() for k in range(3)])
        got = env.rollout(seq, t, states="all")
        torch.cuda.synchronize()
        lk = env.last_kernel()
        assert (lk & 15) == KERNEL_FAST64 and (lk & KERNEL_POLICY), lk
        assert got["states"].shape == (3, B, N, A + K)
        for k in range(3):
            _same(got["states"][k], ref["slots"][t + k][3].astype(npdt), (rep, k))
        _same(got["reward"], ref["slots"][t + 2][1].astype(npdt), rep)
        t += 3
    env.check()


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_prefill_of_three_slots_writes_every_slots_rows(dtype):
    """`prefill`: every slot is my_step_design(a_k, 0) + obtain_state with the launch's own draws."""
    from oracle.oracle import Oracle, SQ_IEEE
    N, A, K = 64, 32, 20
    cfg, ref = _cfg(N, A, K), reference(N, A, K)
    npdt = np.float64 if dtype == torch.float64 else np.float32
    env = make_env(cfg, B, dtype=dtype)
    env.reset_topology(ref["x0"], np.zeros((B, N)), ref["v0"])
    states, acts, _ = env.prefill(env.sample(4100), 3, 4100)
    torch.cuda.synchronize()
    lk = env.last_kernel()
    assert (lk & 15) == KERNEL_FAST64 and (lk & KERNEL_POLICY), lk
    assert states.shape == (3, B, N, A + K)
    orc = Oracle(cfg, batch=B, sq_mode=SQ_IEEE, threads=4)
    orc.reset(ref["x0"], np.zeros((B, N)), ref["v0"])
    for k in range(3):
        a = acts[k].cpu().numpy()
        rew, chobs = orc.step(STEP_DESIGN, a, 0)
        _same(states[k], orc.obtain_state(a, chobs, rew).astype(npdt), k)
    env.check()


def test_screening_identities_and_the_reciprocal_formula_in_numpy():
    """`column32` keeps ONE sum s = t + m of the fixed-point bin t (16 fraction bits) and the margin m = f32_m16:
    * the band test "the fraction of t is within m of an integer", ((t - m) mod 2^16) >= 2^16 - 2 m, is (s mod 2^16) < 2 m;
    * outside the band the bin is s >> 16 == t >> 16 (adding m carries nothing into it),
    for every t in [-2^17, 2^22) and m = 1 ... 64 - what the host's own bound gives (`f32_margin16` switches the screening
    off beyond 64) - and for 1024, 16384 and 32768: the DIRAL_F32_MARGIN hook widens the band up to 16384, and the identities
    hold while 2 m <= 2^16.
    The FORMULA of `writeout_reciprocal` (csrc/step_params.hpp), restated here - the C++ helper itself runs in the GPU cases
    above, with A / CV = 1 ... 32 and (A + K) / CV = 2 ... 44: i / q == (i * mul) >> shift with mul = ceil(2^shift / q),
    shift = 16 + ceil(log2 q), both factors below 2^24 and the product below 2^32, for every i < 2^15 and every q up to 4096."""
    t = np.arange(-2**17, 2**22, dtype=np.int32)
    for m in list(range(1, 65)) + [1024, 16384, 32768]:
        s = t + np.int32(m)
        band = ((t - np.int32(m)) & 0xffff) >= 65536 - 2 * m
        assert np.array_equal(band, (s & 0xffff) < 2 * m), m
        assert not (((s >> 16) != (t >> 16)) & ~band).any(), m
    i = np.arange(2**15, dtype=np.int64)
    for q in list(range(1, 400)) + [511, 512, 513, 1023, 1024, 1025, 4095, 4096]:
        shift = 16 + int(np.ceil(np.log2(q)))
        assert q == 1 or (1 << (shift - 16)) >= q > (1 << (shift - 17))
        mul = -((-1 << shift) // q)
        assert mul < 2**24 and int(i[-1]) * mul < 2**32, q
        assert np.array_equal((i * mul) >> shift, i // q), q
