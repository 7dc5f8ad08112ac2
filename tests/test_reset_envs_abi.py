"""`diral_env_reset_envs` (a chosen subset of a handle's envs back to a fresh topology, one launch) is part of the library
and of include/diral_env.h, within ABI 8.  No GPU needed: the argument checks come first and without a device.  (The one
refusal that reads the handle's batch size - a NULL index with count > B - needs a real handle:
tests/test_gpu_reset_envs.py.)"""
import ctypes
import inspect
import os
import re

from diral_amd import _lib
from diral_amd.config import ABI_VERSION, ERR_BAD_ARG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reset_envs_is_exported_declared_and_checks_its_arguments_first():
    lib = _lib.load()
    src = open(os.path.join(ROOT, "include", "diral_env.h")).read()
    flat = re.sub(r"\s+", " ", src)
    assert ("int diral_env_reset_envs(DiralEnv* env, const int32_t* index, int32_t count, const uint8_t* mask, "
            "const double* x0, const double* y0, const double* v0, uint64_t seed, void* stream);") in flat
    assert "diral_env_reset_envs" in _lib.SYMBOLS
    fn = lib.diral_env_reset_envs
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 9
    assert fn.argtypes[2] is ctypes.c_int and fn.argtypes[7] is ctypes.c_uint64
    # never dereferenced: every one of these refusals is decided by which pointers are NULL and by `count` alone
    idx = ctypes.cast((ctypes.c_int32 * 8)(), ctypes.c_void_p)
    msk = ctypes.cast((ctypes.c_uint8 * 8)(), ctypes.c_void_p)
    fake = ctypes.cast((ctypes.c_char * 64)(), ctypes.c_void_p)
    for count in (1, 4):
        # a NULL handle, in every form of the call
        assert fn(None, idx, count, None, None, None, None, 0, None) == ERR_BAD_ARG
        assert fn(None, None, count, msk, None, None, None, 0, None) == ERR_BAD_ARG
        assert fn(None, None, count, None, None, None, None, 0, None) == ERR_BAD_ARG
        # index and mask both given
        assert fn(fake, idx, count, msk, None, None, None, 0, None) == ERR_BAD_ARG
    for count in (0, -1, -2 ** 31):
        # count < 1 without a mask: with an index list, and as "envs 0 ... count - 1"
        assert fn(fake, idx, count, None, None, None, None, 0, None) == ERR_BAD_ARG
        assert fn(fake, None, count, None, None, None, None, 0, None) == ERR_BAD_ARG
    assert lib.diral_env_abi_version() == ABI_VERSION == 8


def test_no_status_code_was_added_and_the_python_entry_point_has_the_documented_signature():
    src = open(os.path.join(ROOT, "include", "diral_env.h")).read()
    codes = sorted(int(v) for v in re.findall(r"DIRAL_ERR_\w+ = (-\d+)", src))
    assert codes == list(range(-11, 0))
    from diral_amd.vec_env import VecV2VEnv
    sig = inspect.signature(VecV2VEnv.reset_envs)
    assert list(sig.parameters) == ["self", "index", "mask", "count", "x0", "y0", "v0", "seed"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [None] * 6 + [0]
