"""`diral_env_reset_envs` (a chosen subset of a handle's envs back to a fresh topology, one launch) is part of the library
and of include/diral_env.h, within ABI 8.  No GPU needed: the argument checks come first and without a device.  (The one
refusal that reads the handle's batch size - a NULL index with count > B - needs a real handle:
tests/test_gpu_reset_envs.py.)"""
import ctypes
import inspect

from diral_amd import _lib
from diral_amd.config import ERR_BAD_ARG
from tests import abi_header


def test_reset_envs_is_exported_declared_and_checks_its_arguments_first():
    lib = _lib.load()
    assert abi_header.prototypes()["diral_env_reset_envs"].text == (
        "int diral_env_reset_envs(DiralEnv* env, const int32_t* index, int32_t count, const uint8_t* mask, "
        "const double* x0, const double* y0, const double* v0, uint64_t seed, void* stream);")
    fn = lib.diral_env_reset_envs
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


def test_the_python_entry_point_has_the_documented_signature():
    from diral_amd.vec_env import VecV2VEnv
    sig = inspect.signature(VecV2VEnv.reset_envs)
    assert list(sig.parameters) == ["self", "index", "mask", "count", "x0", "y0", "v0", "seed"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [None] * 6 + [0]
