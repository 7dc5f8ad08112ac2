"""The sub-wave step kernel's host surface (csrc/step_subwave.hpp): `DIRAL_PATH_SUBWAVE`, `DIRAL_KERNEL_SUBWAVE`, the two
limits and the pure host helper `diral_env_subwave_ok` are part of include/diral_env.h and of the library, additive within
ABI 8, and diral_amd/config.py mirrors them.  No GPU needed."""
import ctypes

import pytest

from diral_amd import _lib, config
from diral_amd.config import ERR_BAD_ARG, ERR_BAD_CONFIG, ERR_UNSUPPORTED, OK, bench_config
from tests import abi_header


def test_header_declares_the_constants_and_the_helper_and_config_mirrors_them():
    # the header's values are config.py's: tests/test_abi_mirror.py
    assert (config.PATH_SUBWAVE, config.KERNEL_SUBWAVE, config.SUBWAVE_MAX_USERS, config.SUBWAVE_MAX_CHANNELS) == (3, 5, 8, 16)
    assert abi_header.prototypes()["diral_env_subwave_ok"].text == "int diral_env_subwave_ok(const DiralCfg* cfg);"
    # the family code stays inside the low four bits existing callers mask with, and is no other family's
    assert config.KERNEL_SUBWAVE < 16
    assert config.KERNEL_SUBWAVE not in (config.KERNEL_GENERAL, config.KERNEL_FAST64, config.KERNEL_WIDE,
                                         config.KERNEL_OBSERVE, config.KERNEL_LARGE)
    assert config.PATH_SUBWAVE not in (config.PATH_AUTO, config.PATH_GENERAL, config.PATH_LARGE)


def _cfg(N, A, K, **kw):
    return bench_config(N, A, 100.0, State=dict(num_bins=K, **kw.pop("State", {})), **kw)


@pytest.mark.parametrize("N,A,K,state,want", [
    (4, 3, 20, {}, OK),                                              # the reference's toy configuration
    (1, 1, 1, {}, OK),
    (8, 16, 64, {}, OK),                                             # on every limit at once
    (9, 16, 64, {}, ERR_UNSUPPORTED),                                # one past each
    (8, 17, 64, {}, ERR_UNSUPPORTED),
    (8, 16, 65, {}, ERR_UNSUPPORTED),
    (64, 32, 20, {}, ERR_UNSUPPORTED),
    (300, 8, 20, {}, ERR_UNSUPPORTED),
    (4, 3, 20, dict(piggybacking=True, add_channel_obs=True), ERR_UNSUPPORTED),
    (4, 3, 20, dict(add_channel_obs=True), OK),
    (4, 3, 20, dict(add_channel_obs=True, add_reward=True, add_index=True, add_velocity=True, add_position=True), OK),
])
def test_subwave_ok_over_the_limits(N, A, K, state, want):
    lib = _lib.load()
    c = _cfg(N, A, K, State=state).to_c()
    assert lib.diral_env_subwave_ok(ctypes.byref(c)) == want
    # a config the helper accepts is one the build runs
    if want == OK:
        assert lib.diral_env_validate(ctypes.byref(c)) == OK


def test_subwave_ok_passes_on_what_validate_says_about_a_bad_config():
    lib = _lib.load()
    assert lib.diral_env_subwave_ok(None) == ERR_BAD_ARG
    short = _cfg(4, 3, 20).to_c()
    short.struct_bytes = 4
    assert lib.diral_env_subwave_ok(ctypes.byref(short)) == ERR_BAD_ARG
    bad = _cfg(4, 3, 20).to_c()
    bad.reward_design = 9
    assert lib.diral_env_subwave_ok(ctypes.byref(bad)) == ERR_BAD_CONFIG
    none = _cfg(4, 3, 20).to_c()
    none.num_users = 0
    assert lib.diral_env_subwave_ok(ctypes.byref(none)) == ERR_BAD_CONFIG


def test_set_option_rejects_a_null_handle_before_it_looks_at_the_value():
    lib = _lib.load()
    for v in (0, 1, 2, 3, 4):
        assert lib.diral_env_set_option(None, config.OPT_KERNEL_PATH, v) == ERR_BAD_ARG
