"""`diral_env_rollout_replay` / `diral_env_step_policy_replay` (the recorded-mobility block of the K-slot launches) are part of
the library and of include/diral_env.h, additive within ABI 8.  No GPU needed: the argument checks come first."""
import ctypes
import os
import re
import subprocess
import tempfile

from diral_amd import _lib
from diral_amd.config import (ABI_VERSION, ERR_BAD_ARG, STEP_MY_STEP, STEP_MY_STEP_CH, DiralRollout, DiralSlotInfoAge,
                              DiralSlotPolicy, DiralSlotReplay)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "diral_env.h")


def test_replay_entry_points_are_exported_declared_and_reject_a_null_handle():
    lib = _lib.load()
    src = open(HEADER).read()
    assert re.search(r"^int diral_env_rollout_replay\(DiralEnv\* env, int mode, const int32_t\* actions_seq, int32_t slots, int64_t t,", src, re.M)
    assert re.search(r"^int diral_env_step_policy_replay\(DiralEnv\* env, int mode, const int32_t\* actions, int64_t t,", src, re.M)
    for name in ("diral_env_rollout_replay", "diral_env_step_policy_replay"):
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None
        assert re.search(r"const DiralSlotInfoAge\* ia, const DiralSlotReplay\* replay, void\* stream\);",
                         src[src.index("int %s(" % name):][:600])
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


def test_replay_struct_mirrors_the_header_and_the_abi_stays():
    src = open(HEADER).read()
    body = re.search(r"typedef struct DiralSlotReplay \{(.*?)\} DiralSlotReplay;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in (d.strip() for d in body.split(";")):
        if decl:
            first, *more = decl.split(",")
            names += [first.split()[-1].lstrip("*")] + [m.strip().lstrip("*") for m in more]
    assert names == [f[0] for f in DiralSlotReplay._fields_]
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        with open(c, "w") as fh:
            fh.write('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) { printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%d\\n", '
                     'sizeof(DiralSlotReplay), offsetof(DiralSlotReplay, x_positions), offsetof(DiralSlotReplay, T), '
                     'offsetof(DiralSlotReplay, per_env), offsetof(DiralSlotReplay, xpos_out), '
                     'sizeof(DiralRollout), sizeof(DiralSlotPolicy), sizeof(DiralSlotInfoAge), DIRAL_ABI_VERSION); return 0; }\n' % HEADER)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", c, "-o", exe])
        size, o1, o2, o3, o4, s_ro, s_pol, s_ia, abi = (int(x) for x in subprocess.check_output([exe]).split())
    # uint32 + int32 | pointer | int32 + int32 | pointer
    assert size == ctypes.sizeof(DiralSlotReplay) == 32
    assert (o1, o2, o3, o4) == (DiralSlotReplay.x_positions.offset, DiralSlotReplay.T.offset, DiralSlotReplay.per_env.offset,
                                DiralSlotReplay.xpos_out.offset) == (8, 16, 20, 24)
    # no existing struct grew, the ABI number is what it was
    assert s_ro == ctypes.sizeof(DiralRollout) == 72
    assert s_pol == ctypes.sizeof(DiralSlotPolicy) == 168
    assert s_ia == ctypes.sizeof(DiralSlotInfoAge) == 40
    assert abi == ABI_VERSION == _lib.load().diral_env_abi_version() == 8
