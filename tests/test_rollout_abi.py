"""`diral_env_rollout` (K slots of a given action sequence in one launch) is part of the library and of
include/diral_env.h, within ABI 8.  No GPU needed: the argument checks come first."""
import ctypes

from diral_amd import _lib
from diral_amd.config import ERR_BAD_ARG, STEP_MY_STEP, STEP_MY_STEP_CH, DiralRollout
from tests import abi_header


def test_rollout_is_exported_declared_and_checks_its_arguments():
    lib = _lib.load()
    assert abi_header.prototypes()["diral_env_rollout"].text.startswith(
        "int diral_env_rollout(DiralEnv* env, int mode, const int32_t* actions_seq, int32_t slots, int64_t t,")
    fn = lib.diral_env_rollout
    buf = ctypes.cast((ctypes.c_int32 * 64)(), ctypes.c_void_p)
    ro = DiralRollout()
    ro.struct_bytes = ctypes.sizeof(DiralRollout)
    for mode in (STEP_MY_STEP, STEP_MY_STEP_CH):
        # a NULL handle, whatever else is passed
        assert fn(None, mode, buf, 3, 0, None, 0, None, None, 0, ctypes.byref(ro), None) == ERR_BAD_ARG


def test_rollout_struct_mirrors_the_header_and_leaves_the_slot_policy_alone():
    # nothing of SPS in it (its fields, sizes and offsets against the header: tests/test_abi_mirror.py)
    assert not [f for f, _ in DiralRollout._fields_ if f.startswith(("sps_", "draw_", "seed", "actions_out", "slots"))]
