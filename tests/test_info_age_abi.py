"""`diral_env_rollout_ia` / `diral_env_step_policy_ia` (the information-age block of the K-slot my_step_ch launches) are part
of the library and of include/diral_env.h, additive within ABI 8.  No GPU needed: the argument checks come first."""
import ctypes

from diral_amd import _lib
from diral_amd.config import (ERR_BAD_ARG, STEP_MY_STEP, STEP_MY_STEP_CH, DiralRollout, DiralSlotInfoAge,
                              DiralSlotPolicy)
from tests import abi_header


def test_info_age_entry_points_are_exported_declared_and_reject_a_null_handle():
    lib = _lib.load()
    text = {name: p.text for name, p in abi_header.prototypes().items()}
    assert text["diral_env_rollout_ia"].startswith(
        "int diral_env_rollout_ia(DiralEnv* env, int mode, const int32_t* actions_seq, int32_t slots, int64_t t,")
    assert text["diral_env_step_policy_ia"].startswith(
        "int diral_env_step_policy_ia(DiralEnv* env, int mode, const int32_t* actions, int64_t t,")
    for name in ("diral_env_rollout_ia", "diral_env_step_policy_ia"):
        assert text[name].endswith("const DiralSlotInfoAge* ia, void* stream);")
    buf = ctypes.cast((ctypes.c_int32 * 64)(), ctypes.c_void_p)
    ro = DiralRollout()
    ro.struct_bytes = ctypes.sizeof(DiralRollout)
    q = DiralSlotPolicy()
    q.struct_bytes = ctypes.sizeof(DiralSlotPolicy)
    q.slots = 4
    blk = DiralSlotInfoAge()
    blk.struct_bytes = ctypes.sizeof(DiralSlotInfoAge)
    for mode in (STEP_MY_STEP, STEP_MY_STEP_CH):
        for ia in (None, ctypes.byref(blk)):          # a NULL handle, whatever else is passed
            assert lib.diral_env_rollout_ia(None, mode, buf, 3, 0, None, 0, None, None, 0, ctypes.byref(ro), ia, None) == ERR_BAD_ARG
            assert lib.diral_env_step_policy_ia(None, mode, buf, 0, None, None, None, None, 0, ctypes.byref(q), ia, None) == ERR_BAD_ARG
