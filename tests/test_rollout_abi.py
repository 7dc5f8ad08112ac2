"""`diral_env_rollout` (K slots of a given action sequence in one launch) is part of the library and of
include/diral_env.h, within ABI 8.  No GPU needed: the argument checks come first."""
import ctypes
import os
import re

from diral_amd import _lib
from diral_amd.config import ABI_VERSION, ERR_BAD_ARG, STEP_MY_STEP, STEP_MY_STEP_CH, DiralRollout, DiralSlotPolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rollout_is_exported_declared_and_checks_its_arguments():
    lib = _lib.load()
    src = open(os.path.join(ROOT, "include", "diral_env.h")).read()
    assert re.search(r"^int diral_env_rollout\(DiralEnv\* env, int mode, const int32_t\* actions_seq, int32_t slots, int64_t t,", src, re.M)
    assert "diral_env_rollout" in _lib.SYMBOLS
    fn = lib.diral_env_rollout
    buf = ctypes.cast((ctypes.c_int32 * 64)(), ctypes.c_void_p)
    ro = DiralRollout()
    ro.struct_bytes = ctypes.sizeof(DiralRollout)
    for mode in (STEP_MY_STEP, STEP_MY_STEP_CH):
        # a NULL handle, whatever else is passed
        assert fn(None, mode, buf, 3, 0, None, 0, None, None, 0, ctypes.byref(ro), None) == ERR_BAD_ARG
    assert lib.diral_env_abi_version() == ABI_VERSION == 8


def test_rollout_struct_mirrors_the_header_and_leaves_the_slot_policy_alone():
    src = open(os.path.join(ROOT, "include", "diral_env.h")).read()
    body = re.search(r"typedef struct DiralRollout \{(.*?)\} DiralRollout;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip(" *") for n in decl.split(",")[:1]][0].split()[-1:] + [n.strip(" *") for n in decl.split(",")[1:]]
    assert [n.lstrip("*") for n in names] == [f[0] for f in DiralRollout._fields_]
    # uint32 + 3 int32 | double | 5 pointers | uint64
    assert ctypes.sizeof(DiralRollout) == 16 + 8 + 5 * 8 + 8
    assert DiralRollout.vel_seed.offset == 64
    # nothing of SPS in it, and the closed loop's struct is what it was
    assert not [f for f, _ in DiralRollout._fields_ if f.startswith(("sps_", "draw_", "seed", "actions_out", "slots"))]
    # 4 x int32 | double | 7 pointers | 3 doubles | 3 pointers | uint64 | 2 pointers | 2 x int32 | uint64
    assert ctypes.sizeof(DiralSlotPolicy) == 16 + 8 + 56 + 24 + 24 + 8 + 16 + 8 + 8
