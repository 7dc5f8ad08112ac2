"""`diral_env_prefill_mode` (the random prefill with the step of the driver's branch: my_step_design or my_step_ch) is
part of the library and of include/diral_env.h, within ABI 8.  No GPU needed: the argument checks come first."""
import ctypes

from diral_amd import _lib
from diral_amd.config import ERR_BAD_ARG, STEP_DESIGN, STEP_MY_STEP_CH
from tests import abi_header


def test_prefill_mode_is_exported_declared_and_checks_its_arguments():
    lib = _lib.load()
    assert abi_header.prototypes()["diral_env_prefill_mode"].text.startswith("int diral_env_prefill_mode(DiralEnv* env, int mode,")
    fn = lib.diral_env_prefill_mode
    buf = (ctypes.c_int32 * 64)()
    for mode in (STEP_DESIGN, STEP_MY_STEP_CH):
        # a NULL handle, whatever else is passed
        assert fn(None, mode, ctypes.cast(buf, ctypes.c_void_p), 3, 1, None, 0, None, ctypes.cast(buf, ctypes.c_void_p), None,
                  0.0, 1.0, None) == ERR_BAD_ARG
    assert lib.diral_env_prefill(None, ctypes.cast(buf, ctypes.c_void_p), 3, 1, None, 0, None, ctypes.cast(buf, ctypes.c_void_p),
                                 None, 0.0, 1.0, None) == ERR_BAD_ARG
