"""ctypes loader for libdiral_env.so (the C-ABI of include/diral_env.h).

There is NO CPU fallback: if the HIP library is missing or fails to load, every
product entry point raises.  (The CPU restatement under oracle/ is test
infrastructure and is never imported from here.)
"""
from __future__ import annotations

import contextlib
import ctypes
import os

from .config import DiralCfg

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DIRAL_LIB") or os.path.join(HERE, "libdiral_env.so")   # DIRAL_LIB: tuning variants

P, I, I64, U64, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
CFG = ctypes.POINTER(DiralCfg)

# every function include/diral_env.h declares, in the header's order: name -> (restype, argtypes).  The one hand-written mirror
# of the prototypes; tests/test_abi_mirror.py compares every row with the header, kind by kind.
SIGNATURES = {
    "diral_cfg_defaults": (None, [CFG]),
    "diral_env_state_space": (I, [CFG]),
    "diral_env_validate": (I, [CFG]),
    "diral_env_subwave_ok": (I, [CFG]),
    "diral_env_strerror": (ctypes.c_char_p, [I]),
    "diral_env_abi_version": (I, []),
    "diral_env_create": (I, [CFG, I, I, ctypes.POINTER(P)]),
    "diral_env_destroy": (I, [P]),
    "diral_env_hbm_bytes": (I64, [P]),
    "diral_env_set_option": (I, [P, I, I64]),
    "diral_env_last_kernel": (I, [P]),
    "diral_env_reset": (I, [P, P, P, P, U64, P]),
    "diral_env_step": (I, [P, I, P, I64, P, P, P, P, I, D, D, P]),
    "diral_env_observe": (I, [P, P, P, P, P, I, D, D, P]),
    "diral_env_update_velocity": (I, [P, P, U64, P]),
    "diral_env_sample": (I, [P, P, U64, P]),
    "diral_env_info_age": (I, [P, I64, P, P]),
    "diral_env_set_trace": (I, [P, P, I, I, P]),
    "diral_env_export_state": (I, [P] + [P] * 8 + [P]),
    "diral_env_import_state": (I, [P] + [P] * 7 + [P]),
    "diral_env_export_prev_obs": (I, [P, P, P]),
    "diral_env_import_prev_obs": (I, [P, P, P]),
    "diral_env_export_entries": (I, [P, P, P]),
    "diral_env_import_entries": (I, [P, P, P]),
    "diral_env_copy_envs": (I, [P, P, P, P, I, P]),
    "diral_env_reset_envs": (I, [P, P, I, P, P, P, P, U64, P]),
    "diral_env_metrics": (I, [P, P, I, P]),
    "diral_env_check": (I, [P, P]),
    "diral_driver_shape": (I, [I, I, I, P, I, P, P, P, P, P, I, I, D, P, P, P, P, P, P]),
    "diral_sps_step": (I, [I, I, P, P, P, D, D, D, P, P, P, U64, P, P]),
    "diral_sps_window_from_chobs": (I, [I, I, P, I, P, P, P]),
    "diral_sps_step_chobs": (I, [I, I, P, I, P, P, P, D, D, D, P, P, P, U64, P, P]),
    "diral_env_step_policy": (I, [P, I, P, I64, P, P, P, P, I, P, P]),
    "diral_env_prefill": (I, [P, P, I, U64, P, I, P, P, P, D, D, P]),
    "diral_env_prefill_mode": (I, [P, I, P, I, U64, P, I, P, P, P, D, D, P]),
    "diral_env_rollout": (I, [P, I, P, I, I64, P, I, P, P, I, P, P]),
    "diral_env_rollout_ia": (I, [P, I, P, I, I64, P, I, P, P, I, P, P, P]),
    "diral_env_step_policy_ia": (I, [P, I, P, I64, P, P, P, P, I, P, P, P]),
    "diral_env_rollout_replay": (I, [P, I, P, I, I64, P, I, P, P, I, P, P, P, P]),
    "diral_env_step_policy_replay": (I, [P, I, P, I64, P, P, P, P, I, P, P, P, P]),
    "diral_env_set_clock": (I, [P, P]),
    "diral_env_set_capture_rotation": (I, [P, I, P]),
    "diral_env_align_phase": (I, [P, I, P]),
    "diral_clock_add": (I, [P, I64, P]),
    "diral_sps_step_chobs_clocked": (I, [I, I, P, I, P, P, P, D, D, D, U64, P, P, P]),
    "diral_policy_select": (I, [P, P]),
    "diral_memory_add": (I, [P, P, P]),
    "diral_memory_sample": (I, [P, P, P]),
    "diral_memory_history": (I, [P, I, I, P, P, P]),
    "diral_td_head": (I, [I, I, P, P, P, I, P, P, I, D, I, P, P, P, P, P, P, P]),
    "diral_qnet_forward": (I, [I, I, P, P, I, I64, P, I64, I, D, P, P]),
    "diral_env_rollout_memory": (I, [P, I, P, I, I64, P, I, P, P, I, P, P, P, P, P]),
    "diral_env_prefill_memory": (I, [P, I, P, I, U64, P, I, P, P, P, D, D, P, P]),
    "diral_sps_init": (I, [I, I, P, P, U64, P]),
    "diral_env_last_hip_error": (ctypes.c_char_p, [P]),
}
SYMBOLS = list(SIGNATURES)

_lib = None                     # what load() returns: bind(LIB_PATH) once made, or the library of a use() block


class DiralLibraryError(RuntimeError):
    pass


def bind(path, lacking=()) -> ctypes.CDLL:
    """A libdiral_env.so at `path` with every prototype of SIGNATURES set, but for the names in `lacking` (a library built from
    an earlier commit predates them).  Touches no module state: a second library next to load()'s is a supported thing."""
    # PyTorch-ROCm bundles its own libamdhip64; it must be in the process BEFORE
    # libdiral_env.so is dlopen'ed so both bind to the SAME HIP runtime (same
    # SONAME -> the loader reuses it).  Loading ours first would pull in
    # /opt/rocm's copy and torch's device pointers would belong to another runtime.
    import torch  # noqa: F401
    if not os.path.exists(path):
        raise DiralLibraryError(
            "%s is missing - build it with `python -m diral_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback." % path)
    try:
        lib = ctypes.CDLL(path)
    except OSError as exc:  # e.g. libamdhip64 not present
        raise DiralLibraryError("cannot load %s: %s" % (path, exc)) from exc
    for name, (restype, argtypes) in SIGNATURES.items():
        if name in lacking:
            continue
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            raise DiralLibraryError("libdiral_env.so lacks symbol %s" % name) from exc
        fn.restype, fn.argtypes = restype, argtypes
    from .config import ABI_VERSION
    got = int(lib.diral_env_abi_version())
    if got != ABI_VERSION:
        raise DiralLibraryError("%s speaks ABI %d, this package binds ABI %d (include/diral_env.h): rebuild it with "
                                "`python -m diral_amd.build`" % (path, got, ABI_VERSION))
    return lib


def load() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = bind(LIB_PATH)
    return _lib


@contextlib.contextmanager
def use(lib):
    """Inside the block load() returns `lib`: what is built there (VecV2VEnv, SpsPolicy, QPolicy, ReplayMemory) binds to it and
    keeps it (`self.lib`).  On exit, exception included, the previous library is back.  Single-threaded by contract."""
    global _lib
    keep, _lib = _lib, lib
    try:
        yield lib
    finally:
        _lib = keep


def strerror(status: int) -> str:
    return load().diral_env_strerror(status).decode()
