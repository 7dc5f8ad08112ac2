"""The host surface of the sub-wave slot loop (csrc/step_subwave_slots.hpp): the option `DIRAL_OPT_SUBWAVE_SLOTS` is part of
include/diral_env.h, additive within ABI 8 - no new entry point, no new symbol - and diral_amd/config.py mirrors it.  No GPU
needed."""
from diral_amd import _lib, config
from diral_amd.config import ERR_BAD_ARG
from tests import abi_header


def test_header_and_config_agree_on_the_option():
    assert config.OPT_SUBWAVE_SLOTS == 3                         # the header's value is config.py's: tests/test_abi_mirror.py
    assert config.OPT_SUBWAVE_SLOTS not in (config.OPT_ENV_OFFSET, config.OPT_KERNEL_PATH)
    # the launch says KERNEL_SUBWAVE | KERNEL_POLICY: the family stays in the low four bits, the bit is the policy bit
    assert (config.KERNEL_SUBWAVE | config.KERNEL_POLICY) & 15 == config.KERNEL_SUBWAVE


def test_set_option_rejects_a_null_handle():
    assert _lib.load().diral_env_set_option(None, config.OPT_SUBWAVE_SLOTS, 1) == ERR_BAD_ARG


def test_the_option_adds_no_symbol():
    """The slot loop is reached through `diral_env_set_option` and the existing rollout / prefill entry points: the only
    sub-wave symbol stays `diral_env_subwave_ok`, and the header declares no function that names the slot loop."""
    assert [s for s in _lib.SYMBOLS if "subwave" in s] == ["diral_env_subwave_ok"]
    assert not [n for n in abi_header.prototypes() if "subwave_slots" in n]
