"""`diral_env_rollout_memory` / `diral_env_prefill_memory` (the K-slot launches write the replay memory's ring rows
themselves) are part of the library and of include/diral_env.h, within ABI 8.  No GPU needed: the argument checks come
first.  (The checks that need a handle - its B, N and state size against the block's - run in
tests/test_gpu_rollout_memory.py, each on an otherwise valid call.)"""
import ctypes

import pytest

from diral_amd import _lib
from diral_amd.config import (DT_F32, DT_F64, ERR_BAD_ARG, STEP_DESIGN, STEP_MY_STEP, STEP_MY_STEP_CH, DiralMemory,
                              DiralRollout)
from tests import abi_header


def a_block(**kw):
    buf = (ctypes.c_int32 * 64)()
    m = DiralMemory()
    m.struct_bytes = ctypes.sizeof(DiralMemory)
    m.capacity, m.batch, m.num_users, m.state_space, m.dtype = 7, 1, 4, 3, DT_F32
    m.states = m.actions = m.rewards = ctypes.cast(buf, ctypes.c_void_p)
    for k, v in kw.items():
        setattr(m, k, v)
    m._keep = buf
    return m


def test_the_two_entry_points_are_exported_and_declared_as_their_base_plus_the_block():
    protos = abi_header.prototypes()
    # diral_env_rollout_replay / diral_env_prefill_mode with `const DiralMemory* memory` in front of the stream
    for name, base in (("diral_env_rollout_memory", "diral_env_rollout_replay"), ("diral_env_prefill_memory", "diral_env_prefill_mode")):
        got, want = protos[name], protos[base]
        assert (got.ret, got.params) == (want.ret, want.params[:-1] + [abi_header.PTR, abi_header.PTR]), (name, got, want)
        assert got.text.endswith("const DiralMemory* memory, void* stream);")


@pytest.mark.parametrize("mode", [STEP_MY_STEP, STEP_MY_STEP_CH])
def test_rollout_memory_checks_its_arguments_before_any_device(mode):
    lib = _lib.load()
    fn, base = lib.diral_env_rollout_memory, lib.diral_env_rollout_replay
    buf = ctypes.cast((ctypes.c_int32 * 64)(), ctypes.c_void_p)
    ro = DiralRollout()
    ro.struct_bytes = ctypes.sizeof(DiralRollout)
    # memory = NULL is the base call: a NULL handle is what both reject
    assert base(None, mode, buf, 3, 0, None, 0, None, None, DT_F32, ctypes.byref(ro), None, None, None) == ERR_BAD_ARG
    assert fn(None, mode, buf, 3, 0, None, 0, None, None, DT_F32, ctypes.byref(ro), None, None, None, None) == ERR_BAD_ARG
    # ... and so with every block, good or bad: no case reaches a device (this box has none)
    blocks = [a_block(), a_block(struct_bytes=8), a_block(states=None), a_block(actions=None), a_block(rewards=None),
              a_block(capacity=0), a_block(capacity=2), a_block(count=-1), a_block(dtype=DT_F64), a_block(batch=0)]
    for m in blocks:
        assert fn(None, mode, buf, 3, 0, None, 0, None, None, DT_F32, ctypes.byref(ro), None, None, ctypes.byref(m), None) == ERR_BAD_ARG
    # a scratch output next to the block
    m = a_block()
    assert fn(None, mode, buf, 3, 0, buf, 1, None, None, DT_F32, ctypes.byref(ro), None, None, ctypes.byref(m), None) == ERR_BAD_ARG


def test_prefill_memory_checks_its_arguments_before_any_device():
    lib = _lib.load()
    fn, base = lib.diral_env_prefill_memory, lib.diral_env_prefill_mode
    buf = ctypes.cast((ctypes.c_int32 * 64)(), ctypes.c_void_p)
    for mode in (STEP_DESIGN, STEP_MY_STEP_CH):
        assert base(None, mode, buf, 3, 1, None, DT_F32, None, buf, buf, 0.0, 1.0, None) == ERR_BAD_ARG
        assert fn(None, mode, buf, 3, 1, None, DT_F32, None, buf, buf, 0.0, 1.0, None, None) == ERR_BAD_ARG
        for m in (a_block(), a_block(struct_bytes=8), a_block(rewards=None), a_block(capacity=2), a_block(count=-1)):
            assert fn(None, mode, buf, 3, 1, None, DT_F32, None, buf, buf, 0.0, 1.0, ctypes.byref(m), None) == ERR_BAD_ARG
        m = a_block()
        # without rew_in; with a scratch output
        assert fn(None, mode, buf, 3, 1, None, DT_F32, None, buf, None, 0.0, 1.0, ctypes.byref(m), None) == ERR_BAD_ARG
        assert fn(None, mode, buf, 3, 1, buf, DT_F32, buf, buf, buf, 0.0, 1.0, ctypes.byref(m), None) == ERR_BAD_ARG
