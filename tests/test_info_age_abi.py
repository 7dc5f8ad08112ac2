"""`diral_env_rollout_ia` / `diral_env_step_policy_ia` (the information-age block of the K-slot my_step_ch launches) are part
of the library and of include/diral_env.h, additive within ABI 8.  No GPU needed: the argument checks come first."""
import ctypes
import os
import re
import subprocess
import tempfile

from diral_amd import _lib
from diral_amd.config import (ABI_VERSION, ERR_BAD_ARG, STEP_MY_STEP, STEP_MY_STEP_CH, DiralRollout, DiralSlotInfoAge,
                              DiralSlotPolicy)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "diral_env.h")


def test_info_age_entry_points_are_exported_declared_and_reject_a_null_handle():
    lib = _lib.load()
    src = open(HEADER).read()
    assert re.search(r"^int diral_env_rollout_ia\(DiralEnv\* env, int mode, const int32_t\* actions_seq, int32_t slots, int64_t t,", src, re.M)
    assert re.search(r"^int diral_env_step_policy_ia\(DiralEnv\* env, int mode, const int32_t\* actions, int64_t t,", src, re.M)
    for name in ("diral_env_rollout_ia", "diral_env_step_policy_ia"):
        assert name in _lib.SYMBOLS
        assert re.search(r"const DiralSlotInfoAge\* ia, void\* stream\);", src[src.index("int %s(" % name):][:500])
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


def test_info_age_struct_mirrors_the_header_and_the_abi_stays():
    src = open(HEADER).read()
    body = re.search(r"typedef struct DiralSlotInfoAge \{(.*?)\} DiralSlotInfoAge;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [decl.split()[-1].lstrip("*") for decl in (d.strip() for d in body.split(";")) if decl]
    assert names == [f[0] for f in DiralSlotInfoAge._fields_]
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        with open(c, "w") as fh:
            fh.write('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) { printf("%%zu %%zu %%zu %%zu %%zu %%d\\n", '
                     'sizeof(DiralSlotInfoAge), offsetof(DiralSlotInfoAge, ia_out), offsetof(DiralSlotInfoAge, sum_ia_prev), '
                     'sizeof(DiralRollout), sizeof(DiralSlotPolicy), DIRAL_ABI_VERSION); return 0; }\n' % HEADER)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", c, "-o", exe])
        size, o1, o2, s_ro, s_pol, abi = (int(x) for x in subprocess.check_output([exe]).split())
    # uint32 + int32 | 4 pointers
    assert size == ctypes.sizeof(DiralSlotInfoAge) == 8 + 4 * 8
    assert (o1, o2) == (DiralSlotInfoAge.ia_out.offset, DiralSlotInfoAge.sum_ia_prev.offset) == (8, 32)
    # neither existing struct grew, the ABI number is what it was
    assert s_ro == ctypes.sizeof(DiralRollout) == 72
    assert s_pol == ctypes.sizeof(DiralSlotPolicy) == 168
    assert abi == ABI_VERSION == _lib.load().diral_env_abi_version() == 8
