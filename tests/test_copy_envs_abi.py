"""`diral_env_copy_envs` (whole envs from one handle to another in their stored form, one launch) is part of the library
and of include/diral_env.h, within ABI 8.  No GPU needed: the argument checks come first."""
import ctypes

from diral_amd import _lib
from diral_amd.config import ERR_BAD_ARG, ERR_ENV_INDEX
from tests import abi_header


def test_copy_envs_is_exported_declared_and_checks_its_handles():
    lib = _lib.load()
    assert abi_header.prototypes()["diral_env_copy_envs"].text.startswith(
        "int diral_env_copy_envs(DiralEnv* dst, const int32_t* dst_index, DiralEnv* src, const int32_t* src_index,")
    fn = lib.diral_env_copy_envs
    idx = ctypes.cast((ctypes.c_int32 * 8)(), ctypes.c_void_p)
    fake = ctypes.cast((ctypes.c_char * 64)(), ctypes.c_void_p)      # never dereferenced: the other handle is NULL
    for count in (1, 4):
        assert fn(None, idx, fake, idx, count, None) == ERR_BAD_ARG
        assert fn(fake, idx, None, idx, count, None) == ERR_BAD_ARG
        assert fn(None, None, None, None, count, None) == ERR_BAD_ARG


def test_env_index_status_has_a_number_and_a_message_of_its_own():
    lib = _lib.load()
    assert ERR_ENV_INDEX == -11
    msg = lib.diral_env_strerror(-11).decode()
    assert msg and msg != lib.diral_env_strerror(-999).decode()
    others = [lib.diral_env_strerror(s).decode() for s in range(-10, 1)]
    assert msg not in others and len(set(others)) == len(others)
