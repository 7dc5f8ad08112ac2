"""Which K-slot calls are taken and which are refused, with what status: handle kind x call x block on every kernel
family, at the smallest shapes each family takes.  The expected statuses are DATA (tests/slot_refusals_table.json): they
were recorded by running this enumeration (`record`) on commit 0c41657, the parent of the change that moved the verdict
of a slot call into `plan_step` (csrc/diral_env.hip) - the table pins that the one function answers as the scattered
checks did.  Status precedence is pinned where the enumeration makes two reasons meet: the information-age block in both
step modes on handles with and without arrival stamps, injected draws with slots > 1 (a bad argument) with and without the
block and on handles the closed loop refuses, every call on every handle kind and family.  A refused call must leave the env, the policy state and the memory's rings as
they were; an accepted call asserts its status only (what it computes is the other K-slot tests' business).

`step_policy` goes through the C-ABI directly: the Python layer repeats a refused one-slot call with a channel-observation
buffer, which would hide the status."""
import ctypes
import json
import os

import pytest
import torch

from diral_amd._tensors import _ptr
from diral_amd.config import DiralSlotPolicy
from diral_amd.memory import ReplayMemory
from diral_amd.sps import SpsPolicy
from diral_amd.vec_env import DiralError, VecV2VEnv
from tests.kslots_harness import DEV, MODES, assert_same_envs, chain_cfg, start

pytestmark = pytest.mark.gpu
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "slot_refusals_table.json")
B, K, T = 2, 3, 4

# family -> (N, A, how the handle is pinned)
FAMILIES = {
    "fast64": (9, 5, None),
    "below_slot_loops": (5, 3, None),
    "wide": (65, 3, None),
    "subwave": (4, 3, lambda e: e.use_subwave_path()),
    "subwave_slots": (4, 3, lambda e: e.use_subwave_path(slots=True)),
    "general": (9, 5, lambda e: e.force_general_kernel()),
    "large": (9, 5, lambda e: e.force_large_path()),
}
# handle kind -> what it changes in the config; `trace` and `y0_off_lane` change the handle instead (make_pair)
KINDS = {
    "plain": {},
    "track_arrival": dict(track_arrival=True),
    "track_prr": dict(track_prr=True),
    "trace": {},
    "static_topology": dict(mobility=False, enable_design_topology=True),
    "no_piggybacked_tables": dict(State=dict(add_positional_dist_piggy=False)),
    "y0_off_lane": {},
    "piggybacking": dict(State=dict(piggybacking=True, add_channel_obs=True)),
    "secondary_observation": dict(State=dict(add_positional_dist_type=1)),
}


def columns():
    """The calls of one handle, in the order of a table row: (id, call, its arguments)."""
    out = []
    for slots in (1, K):
        for chobs in (False, True):
            for mode, block in (("my_step", None), ("my_step_ch", None), ("my_step_ch", "ia"), ("my_step", "ia"), ("my_step", "positions"),
                                ("my_step", "log")):
                out.append(("step_policy slots=%d %s %s %s" % (slots, "chobs" if chobs else "nochobs", mode, block), "policy",
                            dict(slots=slots, chobs=chobs, mode=mode, block=block)))
    # injected draws with slots > 1, a bad argument: where it stands among the other refusals
    for mode, block in (("my_step", None), ("my_step_ch", "ia"), ("my_step", "ia")):
        out.append(("step_policy slots=%d chobs %s %s draws" % (K, mode, block), "policy",
                    dict(slots=K, chobs=True, mode=mode, block=block, draws=True)))
    for states in (None, "last", "all"):
        for mode, block in (("my_step", None), ("my_step_ch", None), ("my_step_ch", "ia"), ("my_step", "ia"), ("my_step", "positions"),
                            ("my_step", "log"), ("my_step", "memory")):
            out.append(("rollout states=%s %s %s" % (states, mode, block), "rollout", dict(states=states, mode=mode, block=block)))
    for mode in ("my_step_design", "my_step_ch"):
        for block in (None, "memory"):
            out.append(("prefill %s %s" % (mode, block), "prefill", dict(mode=mode, block=block)))
    return out


def make_pair(family, kind):
    """(env, twin) of one family and kind, or the status that refused the pin."""
    N, A, pin = FAMILIES[family]
    cfg = chain_cfg(N, A, 2)
    if KINDS[kind]:
        cfg = cfg.replace(**KINDS[kind])
    x0, v0 = start(cfg, B, 31)
    y0 = torch.tensor([0.0, 1.0] * N)[:N].expand(B, N) if kind == "y0_off_lane" else 0.0
    envs = []
    for _ in range(2):
        env = VecV2VEnv(cfg, batch=B, device=DEV, out_dtype=torch.float32)
        env.reset_topology(x0, y0, v0)
        if pin is not None:
            try:
                pin(env)
            except DiralError as exc:
                return exc.status
        if kind == "trace":
            env.load_saved_positions(torch.arange(T * N, dtype=torch.float64).reshape(T, N))
        envs.append(env)
    return envs


class Caller:
    """The three calls on one handle, each returning the status; the buffers a call needs are made here, at the sizes the
    entry points document."""

    def __init__(self, env):
        self.env = env
        N, A = env.N, env.A
        i32, out = dict(dtype=torch.int32, device=DEV), dict(dtype=env.out_dtype, device=DEV)
        self.pol = SpsPolicy(B, N, A, device=DEV, seed=5)
        self.pol0 = (self.pol.prev_action.clone(), self.pol.counter.clone())
        self.actions = env.sample(1)
        self.seq = torch.stack([env.sample(10 + k) for k in range(K)])
        self.actions_out = torch.zeros((B, N), **i32)
        self.chobs = torch.zeros((B, N, env.CW), **out)
        self.shaped, self.sum_r, self.coll = torch.zeros((K, B, N), **out), torch.zeros((K, B), **out), torch.zeros((K, B), **out)
        self.positions = torch.arange(T * N, dtype=torch.float64, device=DEV).reshape(T, N)
        self.xpos = torch.zeros((K, B, N), dtype=torch.float64, device=DEV)
        self.rew_in = torch.zeros((B, N), dtype=torch.float64, device=DEV)
        self.draws = (torch.ones((B, N), **i32), torch.zeros((B, N), dtype=torch.float64, device=DEV), torch.zeros((B, N), **i32))
        self.mem = None

    def memory(self):
        self.mem = ReplayMemory(K + 1, B, self.env.N, self.env.S, dtype=self.env.out_dtype, seed=3, device=DEV)
        self.mem.states.fill_(-7.0); self.mem.actions.fill_(-7); self.mem.rewards.fill_(-7.0)
        self.mem.begin(torch.zeros((B, self.env.N, self.env.S), dtype=self.env.out_dtype, device=DEV))
        return self.mem

    def policy(self, slots, chobs, mode, block, draws=False):
        env = self.env
        q = DiralSlotPolicy()
        q.struct_bytes = ctypes.sizeof(q)
        q.shape_flags = 1
        q.shaped_out, q.sum_r_out, q.collision_out = _ptr(self.shaped), _ptr(self.sum_r), _ptr(self.coll)
        q.sps_prev_action, q.sps_counter = _ptr(self.pol.prev_action), _ptr(self.pol.counter)
        q.rssi_threshold, q.inc_db, q.keep_prob = self.pol.threshold, self.pol.inc_db, self.pol.keep_prob
        q.seed, q.actions_out, q.slots = 7, _ptr(self.actions_out), slots
        if draws:
            q.draw_counter, q.draw_keep, q.draw_choice = (_ptr(d) for d in self.draws)
        args = (env._h, MODES[mode], _ptr(self.actions), 0, _ptr(env._obs) if env.S > 0 else None, _ptr(env._rew), _ptr(env._done),
                _ptr(self.chobs) if chobs else None, env._dt, ctypes.byref(q))
        if block == "ia":
            blk, keep = env._info_age_block("step_policy", "hist", None, slots)
            return env.lib.diral_env_step_policy_ia(*args, ctypes.byref(blk), env._stream())
        if block in ("positions", "log"):
            blk, keep = env._replay_block("step_policy", self.positions if block == "positions" else None,
                                          self.xpos[:slots] if block == "log" else None, slots)
            return env.lib.diral_env_step_policy_replay(*args, None, ctypes.byref(blk), env._stream())
        return env.lib.diral_env_step_policy(*args, env._stream())

    def rollout(self, states, mode, block):
        kw = dict(info_age=True) if block == "ia" else dict(positions=self.positions) if block == "positions" else \
            dict(log_positions=True) if block == "log" else dict(memory=self.memory()) if block == "memory" else {}
        try:
            self.env.rollout(self.seq, 0, mode=mode, states=states, **kw)
        except DiralError as exc:
            return exc.status
        return 0

    def prefill(self, mode, block):
        try:
            self.env.prefill(self.actions, K, 40, rew_in=self.rew_in, mode=mode, memory=self.memory() if block == "memory" else None)
        except DiralError as exc:
            return exc.status
        return 0

    def assert_nothing_moved(self, twin, what):
        torch.cuda.synchronize()
        assert_same_envs(self.env, twin)
        assert torch.equal(self.pol.prev_action, self.pol0[0]) and torch.equal(self.pol.counter, self.pol0[1]), what
        m = self.mem
        if m is not None:
            assert m.count == 0 and m._state0 is not None, what
            assert bool((m.states == -7).all()) and bool((m.actions == -7).all()) and bool((m.rewards == -7).all()), what


def run_row(family, kind, want=None):
    """Every call of `columns` on one handle: the list of statuses (or {"pin": status}).  With `want`, the recorded row,
    each status is asserted as it is seen."""
    pair = make_pair(family, kind)
    if isinstance(pair, int):
        assert want is None or want == {"pin": pair}, (family, kind, "pin", pair, want)
        return {"pin": pair}
    env, twin = pair
    c = Caller(env)
    row = []
    for n, (name, call, kw) in enumerate(columns()):
        c.mem = None
        st = int(getattr(c, call)(**kw))
        row.append(st)
        if want is not None:
            assert st == want[n], (family, kind, name, st, want[n])
        if st != 0:
            c.assert_nothing_moved(twin, (family, kind, name))
        else:                                                    # taken: back to where the twin is
            env.copy_envs_from(twin)
            env.t = 0
            c.pol.prev_action.copy_(c.pol0[0]); c.pol.counter.copy_(c.pol0[1])
    torch.cuda.synchronize()
    assert_same_envs(env, twin)
    return row


def record(path):
    """Write the table: run on the commit whose behaviour is to be pinned."""
    rows = {"%s/%s" % (f, k): run_row(f, k) for f in FAMILIES for k in KINDS}
    note = ("recorded by tests/test_gpu_slot_refusals.py::record on commit 0c41657 (MI355X), before the slot-call verdict moved "
            "into plan_step; statuses are include/diral_env.h's (0 ok, -1 bad argument, -2 bad config, -3 unsupported)")
    with open(path, "w") as fh:                                  # (one line per column name and per row)
        fh.write('{"provenance": %s,\n "columns": [\n  %s],\n "rows": {\n  %s}}\n' % (
            json.dumps(note), ",\n  ".join(json.dumps(name) for name, _, _ in columns()),
            ",\n  ".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in rows.items())))


def table():
    with open(TABLE) as fh:
        return json.load(fh)


def test_the_table_lists_this_enumeration():
    doc = table()
    assert doc["columns"] == [name for name, _, _ in columns()]
    assert sorted(doc["rows"]) == sorted("%s/%s" % (f, k) for f in FAMILIES for k in KINDS)
    assert all(isinstance(r, dict) or len(r) == len(doc["columns"]) for r in doc["rows"].values())


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_status_of_every_slot_call(family, kind):
    run_row(family, kind, table()["rows"]["%s/%s" % (family, kind)])
