"""`diral_memory_add` / `diral_memory_sample` without a device: the host statements the GPU test compares against
(tests/memory_cases.py) equal what the reference's Memory and the four regrouping functions of DRQN returned (fixtures
m1 ... m3, recorded by tests/golden/gen_memory_golden.py), restatements with one rule wrong are each told apart by some
fixture, the window permutation is one, and the C-ABI of the two entry points is what include/diral_env.h declares."""
import ctypes

import numpy as np
import pytest

from diral_amd import _lib
from diral_amd.config import (DT_BF16, DT_F16, DT_F32, DT_F64, ERR_BAD_ARG, ERR_UNSUPPORTED, DiralMemory, DiralMemoryAdd,
                              DiralMemorySample)
from tests import memory_cases as H

KEYS = ("m1", "m2", "m3")


def _host_batches(fx, key, wrong=None, ring=False):
    """Every recorded batch of a fixture from a statement: [(M, idx, (states, actions, rewards, next_states))]."""
    if ring:
        mem = H.RingMemory(fx["C"], 1, fx["N"], fx["S"], wrong=wrong)
    else:
        mem = H.DequeMemory(fx["C"], 1)
    H.replay_fixture(fx, mem)
    np.random.seed(H.FIXTURE_SEEDS[key])
    out = []
    for M in fx["batches"]:
        idx = H.reference_idx(len(mem), fx["step"], M, wrong)
        if ring:
            got = mem.sample(idx, [0] * M, fx["step"])
        else:
            got = H.train_batch(mem.windows(idx, [0] * M, fx["step"]), fx["N"], wrong=wrong)
        out.append((M, idx, got))
    return out


def _equals_fixture(fx, batches):
    for M, idx, got in batches:
        if not np.array_equal(idx, fx["b%d_idx" % M]):
            return False
        for g, e in zip(got, H.fixture_expected(fx, M)):
            if g.shape != e.shape or not np.array_equal(g, e):
                return False
    return True


# ---- the statements against the reference's recorded batches ----
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("ring", [False, True])
def test_statement_equals_the_reference_on_every_fixture(key, ring):
    fx = H.load_fixture(key)
    assert _equals_fixture(fx, _host_batches(fx, key, ring=ring))


def test_fixtures_cover_what_they_are_for():
    m1, m2, m3 = (H.load_fixture(k) for k in KEYS)
    assert (m1["N"], m1["S"], m1["C"], m1["adds"], m1["step"]) == (4, 23, 16, 23, 6) and m1["adds"] > m1["C"]      # wrapped
    assert (m2["N"], m2["S"], m2["step"]) == (9, 5, 1) and m2["b6_states"].shape == (54, 5)                         # the DQN form
    L = min(m3["adds"], m3["C"]) - m3["step"]
    assert (m3["N"], m3["C"]) == (4, 8) and m3["batches"] == list(range(1, L + 1))
    assert sorted(m3["b%d_idx" % L]) == list(range(L))              # the whole population, each start once
    for fx in (m1, m2, m3):                                         # float32 rings replay the fixtures exactly
        for k in ("state0", "next_states", "rewards"):
            assert np.array_equal(fx[k].astype(np.float32).astype(np.float64), fx[k])


@pytest.mark.parametrize("wrong, ring", [("sample_major", False), ("last_start", False), ("same_row", False),
                                         ("wrap_at_C", True), ("reward_next", True)])
def test_wrong_restatements_are_each_told_apart(wrong, ring):
    told = [key for key in KEYS if not _equals_fixture(H.load_fixture(key), _host_batches(H.load_fixture(key), key, wrong, ring))]
    assert told, wrong
    # ... and the unchanged statement of the same kind passes where the wrong one fails
    for key in told:
        fx = H.load_fixture(key)
        assert _equals_fixture(fx, _host_batches(fx, key, ring=ring))


def test_ring_statement_equals_the_deque_for_several_envs():
    rng = np.random.default_rng(3)
    B, N, S, C, step = 3, 5, 4, 7, 3
    dq, rg = H.DequeMemory(C, B), H.RingMemory(C, B, N, S)
    s0 = rng.standard_normal((B, N, S))
    dq.begin(s0)
    rg.begin(s0)
    for K in (1, 3, 7, 2, 6):                                       # across the wrap of the C + 1 rows
        a, r, s = rng.integers(0, 9, (K, B, N)).astype(np.int32), rng.standard_normal((K, B, N)), rng.standard_normal((K, B, N, S))
        rg.add_many(a, r, s)
        for k in range(K):
            dq.add(a[k], r[k], s[k])
        L = len(dq) - step
        if L < 1:
            continue
        idx, env = rng.integers(0, L, 11), rng.integers(0, B, 11)
        for last_only in (False, True):
            want = H.host_sample(dq, idx, env, step, N, last_only)
            for g, e in zip(rg.sample(idx, env, step, last_only), want[:4]):
                assert np.array_equal(g, e)
    # windows outside the population are zeros and counted
    s, a, r, n, bad = H.host_sample(dq, [0, L, -1, 1], [0, 0, 1, B], step, N)
    assert bad == 3 and not s[1::4].any() and not n[2::4].any() and not a[3::4].any() and s[0::4].any()


# ---- the window permutation ----
def test_permutation_is_one_for_every_small_population():
    for R in range(1, 301):
        seed = H.memory_seed(R, 1)
        got = [H.permute(m, R, seed) for m in range(R)]
        assert sorted(got) == list(range(R)), R
        assert np.array_equal(H.permute_all(R, seed), got), R       # the array form used below is the same statement


def test_permutation_is_one_around_the_powers_of_two():
    rng = np.random.default_rng(9)
    sizes = sorted({R for k in range(1, 21) for R in (2 ** k - 1, 2 ** k, 2 ** k + 1) if R >= 1})
    for R in sizes:
        for seed in (int(s) for s in rng.integers(0, 2 ** 63, size=3 if R <= 2 ** 14 else 2)):
            assert np.array_equal(np.sort(H.permute_all(R, seed)), np.arange(R)), (R, seed)      # {P(m)} == range(R), exactly
    assert [H.half_bits(R) for R in (1, 2, 3, 4, 5, 16, 17, 64, 65, 2 ** 20)] == [1, 1, 1, 1, 2, 2, 3, 3, 4, 10]
    # the draw depends on the seed, and a window is (v div B, v mod B)
    assert [H.permute(m, 97, 1) for m in range(97)] != [H.permute(m, 97, 2) for m in range(97)]
    idx, env = H.drawn_windows(12, 3, 4, 77)
    assert sorted(idx * 3 + env) == list(range(12))


# ---- C-ABI ----
def _buf():
    return ctypes.cast((ctypes.c_char * 64)(), ctypes.c_void_p).value           # never dereferenced by a refused call


def _memory(**kw):
    m = DiralMemory()
    m.struct_bytes = ctypes.sizeof(DiralMemory)
    m.capacity, m.batch, m.num_users, m.state_space, m.dtype = 16, 2, 4, 5, DT_F32
    m.states, m.actions, m.rewards, m.count = _buf(), _buf(), _buf(), 10
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def _add(**kw):
    a = DiralMemoryAdd()
    a.struct_bytes = ctypes.sizeof(DiralMemoryAdd)
    a.slots, a.next_states, a.actions, a.rewards, a.src_dtype, a.rewards_dtype = 3, _buf(), _buf(), _buf(), DT_F32, DT_F64
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _sample(**kw):
    s = DiralMemorySample()
    s.struct_bytes = ctypes.sizeof(DiralMemorySample)
    s.windows, s.step, s.out_dtype, s.states_out = 4, 6, DT_F32, _buf()
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_entry_points_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    add, sample = lib.diral_memory_add, lib.diral_memory_sample
    for fn in (add, sample):
        assert fn(None, None, None) == ERR_BAD_ARG
    assert add(ctypes.byref(_memory()), None, None) == ERR_BAD_ARG and sample(ctypes.byref(_memory()), None, None) == ERR_BAD_ARG
    bad_memory = [dict(struct_bytes=60), dict(struct_bytes=0), dict(states=None), dict(actions=None), dict(rewards=None),
                  dict(capacity=0), dict(batch=0), dict(num_users=-1), dict(state_space=0), dict(dtype=DT_F16), dict(dtype=-1),
                  dict(count=-1)]
    for kw in bad_memory:
        assert add(ctypes.byref(_memory(**kw)), ctypes.byref(_add()), None) == ERR_BAD_ARG, kw
        assert sample(ctypes.byref(_memory(**kw)), ctypes.byref(_sample()), None) == ERR_BAD_ARG, kw
    for kw in (dict(struct_bytes=52), dict(slots=0), dict(slots=17), dict(next_states=None), dict(actions=None), dict(rewards=None),
               dict(src_dtype=DT_BF16), dict(rewards_dtype=DT_F16), dict(src_dtype=-1)):
        assert add(ctypes.byref(_memory()), ctypes.byref(_add(**kw)), None) == ERR_BAD_ARG, kw
    for kw in (dict(struct_bytes=108), dict(step=0), dict(step=-2), dict(windows=0), dict(idx=_buf()), dict(env=_buf()),
               dict(step=10), dict(step=11),                        # len <= step (count = 10)
               dict(windows=9)):                                    # drawn: R = batch * (len - step) = 8
        assert sample(ctypes.byref(_memory()), ctypes.byref(_sample(**kw)), None) == ERR_BAD_ARG, kw
    assert sample(ctypes.byref(_memory(count=40)), ctypes.byref(_sample(step=16)), None) == ERR_BAD_ARG      # len = capacity
    for ring, out in ((DT_F32, DT_F64), (DT_F64, DT_F16), (DT_F64, DT_BF16)):
        assert sample(ctypes.byref(_memory(dtype=ring)), ctypes.byref(_sample(out_dtype=out)), None) == ERR_UNSUPPORTED
    assert sample(ctypes.byref(_memory()), ctypes.byref(_sample(out_dtype=7)), None) == ERR_UNSUPPORTED
