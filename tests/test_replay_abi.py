"""`diral_env_rollout_replay` / `diral_env_step_policy_replay` (the recorded-mobility block of the K-slot launches) are part of
the library and of include/diral_env.h, additive within ABI 8.  No GPU needed: the argument checks come first."""
import ctypes

from diral_amd import _lib
from diral_amd.config import (ERR_BAD_ARG, STEP_MY_STEP, STEP_MY_STEP_CH, DiralRollout, DiralSlotInfoAge,
                              DiralSlotPolicy, DiralSlotReplay)
from tests import abi_header


def test_replay_entry_points_are_exported_declared_and_reject_a_null_handle():
    lib = _lib.load()
    text = {name: p.text for name, p in abi_header.prototypes().items()}
    assert text["diral_env_rollout_replay"].startswith(
        "int diral_env_rollout_replay(DiralEnv* env, int mode, const int32_t* actions_seq, int32_t slots, int64_t t,")
    assert text["diral_env_step_policy_replay"].startswith(
        "int diral_env_step_policy_replay(DiralEnv* env, int mode, const int32_t* actions, int64_t t,")
    for name in ("diral_env_rollout_replay", "diral_env_step_policy_replay"):
        assert text[name].endswith("const DiralSlotInfoAge* ia, const DiralSlotReplay* replay, void* stream);")
    buf = ctypes.cast((ctypes.c_int32 * 64)(), ctypes.c_void_p)
    ro = DiralRollout()
    ro.struct_bytes = ctypes.sizeof(DiralRollout)
    q = DiralSlotPolicy()
    q.struct_bytes = ctypes.sizeof(DiralSlotPolicy)
    q.slots = 4
    ia = DiralSlotInfoAge()
    ia.struct_bytes = ctypes.sizeof(DiralSlotInfoAge)
    rp = DiralSlotReplay()
    rp.struct_bytes = ctypes.sizeof(DiralSlotReplay)
    for mode in (STEP_MY_STEP, STEP_MY_STEP_CH):
        for a in (None, ctypes.byref(ia)):            # a NULL handle, with and without either block
            for r in (None, ctypes.byref(rp)):
                assert lib.diral_env_rollout_replay(None, mode, buf, 3, 0, None, 0, None, None, 0, ctypes.byref(ro), a, r, None) == ERR_BAD_ARG
                assert lib.diral_env_step_policy_replay(None, mode, buf, 0, None, None, None, None, 0, ctypes.byref(q), a, r, None) == ERR_BAD_ARG
