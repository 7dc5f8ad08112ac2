"""The refusals of the thirteen handle-free entry points (csrc/diral_agent.hip), as one table.  No GPU needed: every call here
is refused by an argument check, and the argument checks come before the first HIP call.

Each entry point has a call that WOULD launch (`GOOD`, never sent) and a handful of cases, each the good call with a few
arguments replaced and the exact status it must return.  A case with more than one replacement that is a violation by
itself pins which refusal wins: the order of the checks inside an entry point is part of its contract.  The pointers are
arbitrary non-null integers - a refused call dereferences none of them; `widths` of diral_qnet_forward is the one host array.
(diral_clock_add has one check, so no pair of violations exists for it.)"""
import copy
import ctypes

import pytest

from diral_amd import _lib
from diral_amd.config import (DT_BF16, DT_F16, DT_F32, DT_F64, ERR_BAD_ARG, ERR_UNSUPPORTED, SELECT_EPS_GREEDY, SELECT_SOFTMAX,
                              DiralMemory, DiralMemoryAdd, DiralMemorySample, DiralSelect)

PTR = 0x1000                    # "a device pointer": never dereferenced
BAD, UNS = ERR_BAD_ARG, ERR_UNSUPPORTED
INF, NAN = float("inf"), float("nan")

MEMORY = dict(_type=DiralMemory, capacity=16, batch=4, num_users=4, state_space=6, dtype=DT_F32, states=PTR, actions=PTR,
              rewards=PTR, count=10, count_dev=None)
SPS_HEAD = dict(agents=8, num_channels=4)
SPS_TAIL = dict(prev_action=PTR, counter=PTR, rssi_threshold=-110.0, inc_db=3.0, keep_prob=0.8)
DRAWS = dict(draw_counter=None, draw_keep=None, draw_choice=None)

# entry point -> its arguments in the order of include/diral_env.h, with values that pass every check
GOOD = {
    "diral_sps_init": dict(agents=8, selection_window=4, prev_action=PTR, counter=PTR, seed=1, stream=None),
    "diral_sps_step": dict(**SPS_HEAD, selection_window=PTR, **SPS_TAIL, **DRAWS, seed=1, actions_out=PTR, stream=None),
    "diral_sps_window_from_chobs": dict(**SPS_HEAD, chobs=PTR, chobs_dtype=DT_F32, actions=PTR, window_out=PTR, stream=None),
    "diral_sps_step_chobs": dict(**SPS_HEAD, chobs=PTR, chobs_dtype=DT_F64, actions=PTR, **SPS_TAIL, **DRAWS, seed=1,
                                 actions_out=PTR, stream=None),
    "diral_sps_step_chobs_clocked": dict(**SPS_HEAD, chobs=PTR, chobs_dtype=DT_F32, actions=PTR, **SPS_TAIL, seed=1, clock=PTR,
                                         actions_out=PTR, stream=None),
    "diral_clock_add": dict(clock=PTR, inc=1, stream=None),
    "diral_driver_shape": dict(envs=4, num_users=8, num_channels=4, reward_in=PTR, dtype=DT_F32, actions=PTR, ia=None,
                               sum_ia_prev=None, pen_counter=PTR, prev_actions=PTR, flags=5, ia_penalty_threshold=3,
                               ia_penalty_value=-1.0, reward_out=PTR, sum_r_out=None, collision_out=None, ia_sum_out=None,
                               ia_penalty_out=None, stream=None),
    "diral_policy_select": dict(s=dict(_type=DiralSelect, kind=SELECT_EPS_GREEDY, agents=8, num_users=4, num_channels=4, q=PTR,
                                       q_dtype=DT_F32, eps=0.1, tmp=1.0, actions_out=PTR), stream=None),
    "diral_memory_add": dict(m=MEMORY, a=dict(_type=DiralMemoryAdd, slots=2, next_states=PTR, state0=None, src_dtype=DT_F32,
                                              rewards_dtype=DT_F32, actions=PTR, rewards=PTR), stream=None),
    "diral_memory_sample": dict(m=MEMORY, s=dict(_type=DiralMemorySample, windows=8, step=3, out_dtype=DT_F32, states_out=PTR,
                                                 next_states_out=PTR, actions_out=PTR, rewards_out=PTR), stream=None),
    "diral_memory_history": dict(m=MEMORY, step=3, out_dtype=DT_F32, out=PTR, bad=None, stream=None),
    "diral_td_head": dict(rows=8, num_actions=4, q=PTR, q_next_target=PTR, q_next_eval=None, q_dtype=DT_F32, actions=PTR,
                          rewards=PTR, rewards_dtype=DT_F32, gamma=0.9, hysteretic=0, targets_out=PTR, td_out=PTR,
                          next_action_out=None, grad_q_out=None, loss_out=PTR, bad_rows=None, stream=None),
    # the blob of 8 -> 16 -> 4: 8 * 16 + 3 * 16 + 16 * 4 + 4 floats
    "diral_qnet_forward": dict(rows=8, num_hidden=1, widths=[8, 16, 4], x=PTR, x_dtype=DT_F32, x_row_stride=8, params=PTR,
                               params_len=244, norm=1, ln_eps=1e-5, q_out=PTR, stream=None),
}

BIG = 1 << 30
# (entry point, what is replaced - "m.capacity": a field of the struct argument `m` -, the status)
CASES = [
    ("diral_sps_init", {"agents": 0}, BAD),
    ("diral_sps_init", {"agents": -3}, BAD),
    ("diral_sps_init", {"selection_window": -1}, BAD),
    ("diral_sps_init", {"prev_action": None}, BAD),
    ("diral_sps_init", {"counter": None}, BAD),
    ("diral_sps_init", {"agents": 0, "counter": None}, BAD),

    ("diral_sps_step", {"agents": 0}, BAD),
    ("diral_sps_step", {"num_channels": 0}, BAD),
    ("diral_sps_step", {"num_channels": -1}, BAD),
    ("diral_sps_step", {"selection_window": None}, BAD),
    ("diral_sps_step", {"prev_action": None}, BAD),
    ("diral_sps_step", {"counter": None}, BAD),
    ("diral_sps_step", {"actions_out": None}, BAD),
    ("diral_sps_step", {"num_channels": 0, "actions_out": None}, BAD),

    ("diral_sps_window_from_chobs", {"agents": 0}, BAD),
    ("diral_sps_window_from_chobs", {"num_channels": 0}, BAD),
    ("diral_sps_window_from_chobs", {"chobs": None}, BAD),
    ("diral_sps_window_from_chobs", {"actions": None}, BAD),
    ("diral_sps_window_from_chobs", {"window_out": None}, BAD),
    ("diral_sps_window_from_chobs", {"chobs_dtype": DT_F16}, BAD),
    ("diral_sps_window_from_chobs", {"chobs_dtype": -1}, BAD),
    ("diral_sps_window_from_chobs", {"chobs_dtype": 4, "window_out": None}, BAD),

    ("diral_sps_step_chobs", {"agents": 0}, BAD),
    ("diral_sps_step_chobs", {"num_channels": 0}, BAD),
    ("diral_sps_step_chobs", {"chobs": None}, BAD),
    ("diral_sps_step_chobs", {"actions": None}, BAD),
    ("diral_sps_step_chobs", {"prev_action": None}, BAD),
    ("diral_sps_step_chobs", {"counter": None}, BAD),
    ("diral_sps_step_chobs", {"actions_out": None}, BAD),
    ("diral_sps_step_chobs", {"chobs_dtype": DT_BF16}, BAD),
    ("diral_sps_step_chobs", {"chobs_dtype": 4}, BAD),
    ("diral_sps_step_chobs", {"num_channels": 257}, UNS),
    ("diral_sps_step_chobs", {"num_channels": 257, "chobs_dtype": DT_F16}, BAD),
    ("diral_sps_step_chobs", {"num_channels": 257, "counter": None}, BAD),

    ("diral_sps_step_chobs_clocked", {"clock": None}, BAD),
    ("diral_sps_step_chobs_clocked", {"agents": 0}, BAD),
    ("diral_sps_step_chobs_clocked", {"chobs": None}, BAD),
    ("diral_sps_step_chobs_clocked", {"actions_out": None}, BAD),
    ("diral_sps_step_chobs_clocked", {"chobs_dtype": DT_F16}, BAD),
    ("diral_sps_step_chobs_clocked", {"num_channels": 257}, UNS),
    ("diral_sps_step_chobs_clocked", {"num_channels": 257, "clock": None}, BAD),
    ("diral_sps_step_chobs_clocked", {"num_channels": 257, "chobs_dtype": -1}, BAD),

    ("diral_clock_add", {"clock": None}, BAD),
    ("diral_clock_add", {"clock": None, "inc": -1}, BAD),

    ("diral_driver_shape", {"envs": 0}, BAD),
    ("diral_driver_shape", {"num_users": 0}, BAD),
    ("diral_driver_shape", {"reward_in": None}, BAD),
    ("diral_driver_shape", {"reward_out": None}, BAD),
    ("diral_driver_shape", {"dtype": DT_F16}, BAD),
    ("diral_driver_shape", {"dtype": -1}, BAD),
    ("diral_driver_shape", {"actions": None}, BAD),
    ("diral_driver_shape", {"pen_counter": None}, BAD),
    ("diral_driver_shape", {"prev_actions": None}, BAD),
    ("diral_driver_shape", {"flags": 2}, BAD),
    ("diral_driver_shape", {"flags": 2, "ia": PTR}, BAD),
    ("diral_driver_shape", {"flags": 6, "actions": None}, BAD),
    ("diral_driver_shape", {"envs": -1, "dtype": 7}, BAD),

    ("diral_policy_select", {"s": None}, BAD),
    ("diral_policy_select", {"s.struct_bytes": ctypes.sizeof(DiralSelect) - 8}, BAD),
    ("diral_policy_select", {"s.struct_bytes": 0}, BAD),
    ("diral_policy_select", {"s.q": None}, BAD),
    ("diral_policy_select", {"s.actions_out": None}, BAD),
    ("diral_policy_select", {"s.agents": 0}, BAD),
    ("diral_policy_select", {"s.num_channels": 0}, BAD),
    ("diral_policy_select", {"s.num_users": 0}, BAD),
    ("diral_policy_select", {"s.num_users": 3}, BAD),
    ("diral_policy_select", {"s.kind": -1}, BAD),
    ("diral_policy_select", {"s.kind": 4}, BAD),
    ("diral_policy_select", {"s.q_dtype": -1}, BAD),
    ("diral_policy_select", {"s.q_dtype": 4}, BAD),
    ("diral_policy_select", {"s.kind": SELECT_SOFTMAX, "s.tmp": 0.0}, BAD),
    ("diral_policy_select", {"s.kind": SELECT_SOFTMAX, "s.tmp": INF}, BAD),
    ("diral_policy_select", {"s.kind": SELECT_SOFTMAX, "s.tmp": NAN}, BAD),
    ("diral_policy_select", {"s.param_per_env": 1}, BAD),
    ("diral_policy_select", {"s.num_channels": 4097}, UNS),
    ("diral_policy_select", {"s.num_channels": 4097, "s.kind": 9}, BAD),
    ("diral_policy_select", {"s.num_channels": 4097, "s.q_dtype": 4}, BAD),
    ("diral_policy_select", {"s.num_channels": 4097, "s.param_per_env": 1}, BAD),

    ("diral_memory_add", {"m": None}, BAD),
    ("diral_memory_add", {"m.struct_bytes": ctypes.sizeof(DiralMemory) + 8}, BAD),
    ("diral_memory_add", {"m.states": None}, BAD),
    ("diral_memory_add", {"m.actions": None}, BAD),
    ("diral_memory_add", {"m.rewards": None}, BAD),
    ("diral_memory_add", {"m.capacity": 0}, BAD),
    ("diral_memory_add", {"m.batch": 0}, BAD),
    ("diral_memory_add", {"m.num_users": 0}, BAD),
    ("diral_memory_add", {"m.state_space": 0}, BAD),
    ("diral_memory_add", {"m.dtype": DT_F16}, BAD),
    ("diral_memory_add", {"m.count": -1}, BAD),
    ("diral_memory_add", {"a": None}, BAD),
    ("diral_memory_add", {"a.struct_bytes": 4}, BAD),
    ("diral_memory_add", {"a.slots": 0}, BAD),
    ("diral_memory_add", {"a.slots": 17}, BAD),
    ("diral_memory_add", {"a.next_states": None}, BAD),
    ("diral_memory_add", {"a.actions": None}, BAD),
    ("diral_memory_add", {"a.rewards": None}, BAD),
    ("diral_memory_add", {"a.src_dtype": DT_F16}, BAD),
    ("diral_memory_add", {"a.rewards_dtype": DT_BF16}, BAD),
    ("diral_memory_add", {"a.rewards_dtype": -1}, BAD),
    ("diral_memory_add", {"a.slots": 0, "a.src_dtype": 4}, BAD),

    ("diral_memory_sample", {"m": None}, BAD),
    ("diral_memory_sample", {"m.struct_bytes": 0}, BAD),
    ("diral_memory_sample", {"m.dtype": DT_BF16}, BAD),
    ("diral_memory_sample", {"s": None}, BAD),
    ("diral_memory_sample", {"s.struct_bytes": ctypes.sizeof(DiralMemorySample) - 8}, BAD),
    ("diral_memory_sample", {"s.step": 0}, BAD),
    ("diral_memory_sample", {"s.windows": 0}, BAD),
    ("diral_memory_sample", {"s.idx": PTR}, BAD),
    ("diral_memory_sample", {"s.env": PTR}, BAD),
    ("diral_memory_sample", {"s.step": 10}, BAD),                          # a host count of 10: no window of 10 + 1 states
    ("diral_memory_sample", {"m.count": 100, "s.step": 16}, BAD),          # ... nor of capacity + 1
    ("diral_memory_sample", {"s.windows": 29}, BAD),                       # more than (10 - 3) * 4 distinct windows
    ("diral_memory_sample", {"s.out_dtype": DT_F64}, UNS),                 # a float32 ring widens to nothing
    ("diral_memory_sample", {"s.out_dtype": 4}, UNS),
    ("diral_memory_sample", {"s.out_dtype": -1}, UNS),
    ("diral_memory_sample", {"m.dtype": DT_F64, "s.out_dtype": DT_F16}, UNS),
    ("diral_memory_sample", {"m.dtype": DT_F64, "s.out_dtype": DT_BF16}, UNS),
    ("diral_memory_sample", {"m.num_users": 65536, "m.state_space": 32768}, UNS),
    ("diral_memory_sample", {"m.count_dev": PTR, "s.windows": BIG, "s.step": 1}, UNS),
    ("diral_memory_sample", {"s.out_dtype": DT_F64, "s.step": 0}, BAD),
    ("diral_memory_sample", {"s.out_dtype": DT_F64, "s.windows": 29}, BAD),
    ("diral_memory_sample", {"m.num_users": 65536, "m.state_space": 32768, "s.step": 10}, BAD),
    ("diral_memory_sample", {"m.num_users": 65536, "m.state_space": 32768, "s.out_dtype": 4}, UNS),

    ("diral_memory_history", {"m": None}, BAD),
    ("diral_memory_history", {"m.struct_bytes": 8}, BAD),
    ("diral_memory_history", {"m.capacity": 0}, BAD),
    ("diral_memory_history", {"m.dtype": 4}, BAD),
    ("diral_memory_history", {"step": 0}, BAD),
    ("diral_memory_history", {"out": None}, BAD),
    ("diral_memory_history", {"step": 12}, BAD),                           # a host count of 10: at most 10 + 1 states
    ("diral_memory_history", {"m.count": 100, "step": 18}, BAD),
    ("diral_memory_history", {"out_dtype": DT_F64}, UNS),
    ("diral_memory_history", {"out_dtype": 4}, UNS),
    ("diral_memory_history", {"m.dtype": DT_F64, "out_dtype": DT_F16}, UNS),
    ("diral_memory_history", {"m.num_users": 65536, "m.state_space": 32768}, UNS),
    ("diral_memory_history", {"m.count_dev": PTR, "m.batch": 1 << 20, "step": 1 << 11}, UNS),
    ("diral_memory_history", {"out_dtype": DT_F64, "out": None}, BAD),
    ("diral_memory_history", {"out_dtype": DT_F64, "step": 12}, BAD),
    ("diral_memory_history", {"m.num_users": 65536, "m.state_space": 32768, "out_dtype": -1}, UNS),

    ("diral_td_head", {"rows": 0}, BAD),
    ("diral_td_head", {"num_actions": 0}, BAD),
    ("diral_td_head", {"q_next_target": None}, BAD),
    ("diral_td_head", {"actions": None}, BAD),
    ("diral_td_head", {"rewards": None}, BAD),
    ("diral_td_head", {"q_dtype": -1}, BAD),
    ("diral_td_head", {"q_dtype": 4}, BAD),
    ("diral_td_head", {"rewards_dtype": DT_F16}, BAD),
    ("diral_td_head", {"gamma": INF}, BAD),
    ("diral_td_head", {"gamma": NAN}, BAD),
    ("diral_td_head", {"q": None}, BAD),                                   # td_out and loss_out need q
    ("diral_td_head", {"q": None, "td_out": None, "loss_out": None, "grad_q_out": PTR}, BAD),
    ("diral_td_head", {"td_out": None}, BAD),                              # loss_out without td_out
    ("diral_td_head", {"num_actions": 4097}, UNS),
    ("diral_td_head", {"rows": (1 << 24) + 1}, UNS),
    ("diral_td_head", {"q_dtype": DT_F64}, UNS),
    ("diral_td_head", {"q_dtype": DT_F64, "td_out": None}, BAD),
    ("diral_td_head", {"q_dtype": DT_F64, "rewards_dtype": 4}, BAD),
    ("diral_td_head", {"num_actions": 4097, "gamma": NAN}, BAD),
    ("diral_td_head", {"num_actions": 4097, "rows": 0}, BAD),

    ("diral_qnet_forward", {"widths": None}, BAD),
    ("diral_qnet_forward", {"x": None}, BAD),
    ("diral_qnet_forward", {"params": None}, BAD),
    ("diral_qnet_forward", {"q_out": None}, BAD),
    ("diral_qnet_forward", {"rows": 0}, BAD),
    ("diral_qnet_forward", {"num_hidden": -1}, BAD),
    ("diral_qnet_forward", {"x_dtype": -1}, BAD),
    ("diral_qnet_forward", {"x_dtype": 4}, BAD),
    ("diral_qnet_forward", {"ln_eps": NAN}, BAD),
    ("diral_qnet_forward", {"ln_eps": -1e-5}, BAD),
    ("diral_qnet_forward", {"num_hidden": 4, "widths": [8, 16, 16, 16, 16, 4]}, UNS),
    ("diral_qnet_forward", {"x_dtype": DT_F64}, UNS),
    ("diral_qnet_forward", {"widths": [8, 0, 4]}, BAD),
    ("diral_qnet_forward", {"widths": [8, 16, -1]}, BAD),
    ("diral_qnet_forward", {"widths": [8, 257, 4]}, UNS),
    ("diral_qnet_forward", {"widths": [8, 16, 257]}, UNS),
    ("diral_qnet_forward", {"widths": [1025, 16, 4], "x_row_stride": 1025}, UNS),
    ("diral_qnet_forward", {"x_row_stride": 7}, BAD),
    ("diral_qnet_forward", {"params_len": 243}, BAD),
    ("diral_qnet_forward", {"params_len": 245}, BAD),
    ("diral_qnet_forward", {"params_len": 8 * 16 + 16 + 16 * 4 + 4}, BAD),      # the blob without gamma and beta
    ("diral_qnet_forward", {"num_hidden": 0, "widths": [8, 4]}, BAD),           # ... and of another chain: 36 floats
    ("diral_qnet_forward", {"num_hidden": 4, "widths": None}, BAD),
    ("diral_qnet_forward", {"num_hidden": 4, "ln_eps": -1.0}, BAD),
    ("diral_qnet_forward", {"num_hidden": 4, "x_dtype": DT_F64}, UNS),
    ("diral_qnet_forward", {"x_dtype": DT_F64, "widths": [8, 0, 4]}, UNS),
    ("diral_qnet_forward", {"widths": [8, 257, 0]}, BAD),                       # every width is checked for < 1 first
    ("diral_qnet_forward", {"widths": [8, 257, 4], "params_len": 1}, UNS),
    ("diral_qnet_forward", {"widths": [8, 257, 4], "x_row_stride": 1}, UNS),
]


def _struct(fields):
    if fields is None:
        return None
    fields = dict(fields)
    cls = fields.pop("_type")
    fields.setdefault("struct_bytes", ctypes.sizeof(cls))
    return ctypes.byref(cls(**fields))


def _call(lib, name, replaced):
    args = copy.deepcopy(GOOD[name])
    for key, value in replaced.items():
        arg, _, field = key.partition(".")
        assert arg in args and (not field or field in dict(args[arg]["_type"]._fields_)), key
        if field:
            args[arg][field] = value
        else:
            args[arg] = value
    values = []
    for v in args.values():
        if isinstance(v, dict):
            v = _struct(v)
        elif isinstance(v, list):
            v = ctypes.cast((ctypes.c_int32 * len(v))(*v), ctypes.c_void_p)
        values.append(v)
    assert len(values) == len(_lib.SIGNATURES[name][1])
    return getattr(lib, name)(*values)


def _case_id(case):
    name, replaced, _ = case
    return "%s-%s" % (name[len("diral_"):], "+".join("%s=%s" % kv for kv in replaced.items()))


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_refused_before_any_hip_call(case):
    name, replaced, status = case
    assert replaced, "the good call is never sent"
    assert _call(_lib.load(), name, replaced) == status


def test_table_covers_every_handle_free_entry_point():
    handle_free = {n for n in _lib.SYMBOLS if not n.startswith(("diral_env_", "diral_cfg_"))}
    assert handle_free == set(GOOD) and len(GOOD) == 13
    for name in GOOD:
        mine = [c for c in CASES if c[0] == name]
        assert len(mine) >= 2 and any(len(c[1]) >= 2 for c in mine), name
    assert len({_case_id(c) for c in CASES}) == len(CASES)
