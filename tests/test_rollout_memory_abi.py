"""`diral_env_rollout_memory` / `diral_env_prefill_memory` (the K-slot launches write the replay memory's ring rows
themselves) are part of the library and of include/diral_env.h, within ABI 8.  No GPU needed: the argument checks come
first.  (The checks that need a handle - its B, N and state size against the block's - run in
tests/test_gpu_rollout_memory.py, each on an otherwise valid call.)"""
import ctypes
import os
import re

import pytest

from diral_amd import _lib
from diral_amd.config import (ABI_VERSION, DT_F32, DT_F64, ERR_BAD_ARG, STEP_DESIGN, STEP_MY_STEP, STEP_MY_STEP_CH, DiralMemory,
                              DiralRollout)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, I64, U64, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double


def header():
    return open(os.path.join(ROOT, "include", "diral_env.h")).read()


def prototype(name):
    """The parameter types of `name` as the header declares them, pointers folded to one word."""
    m = re.search(r"^int %s\((.*?)\);" % name, header(), re.M | re.S)
    assert m, name
    kinds = []
    for par in m.group(1).split(","):
        par = " ".join(par.split())
        kinds.append("ptr" if "*" in par else par.rsplit(" ", 1)[0])
    return kinds


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
    lib = _lib.load()
    for name in ("diral_env_rollout_memory", "diral_env_prefill_memory"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    # diral_env_rollout_replay / diral_env_prefill_mode with `const DiralMemory* memory` in front of the stream
    for name, base in (("diral_env_rollout_memory", "diral_env_rollout_replay"), ("diral_env_prefill_memory", "diral_env_prefill_mode")):
        got, want = prototype(name), prototype(base)
        assert got == want[:-1] + ["ptr", "ptr"], (name, got, want)
        assert re.search(r"^int %s\([^;]*const DiralMemory\* memory,\s*void\* stream\);" % name, header(), re.M | re.S)
    ctype = {"ptr": P, "int": I, "int32_t": ctypes.c_int32, "int64_t": I64, "uint64_t": U64, "double": D}
    for name in ("diral_env_rollout_memory", "diral_env_prefill_memory"):
        fn = getattr(lib, name)
        assert fn.restype is I
        assert [ctypes.sizeof(t) for t in fn.argtypes] == [ctypes.sizeof(ctype[k]) for k in prototype(name)], name
    assert lib.diral_env_abi_version() == ABI_VERSION == 8


def test_the_descriptor_is_the_replay_memory_s():
    src = header()
    body = re.search(r"typedef struct DiralMemory \{(.*?)\} DiralMemory;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in
             [decl.split(",")[0].split()[-1]] + decl.split(",")[1:]]
    assert names == [f[0] for f in DiralMemory._fields_]
    # uint32 + 5 int32 | 3 pointers | int64 | pointer
    assert ctypes.sizeof(DiralMemory) == 24 + 24 + 8 + 8


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
