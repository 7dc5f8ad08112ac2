"""TEST-ONLY: random CALL PROGRAMS for every kernel family, and the host model that says what each call must return.

The other tests run a fixed call pattern (reset -> step ... step -> export); what decides the NEXT launch - `plane_valid` /
`ring_valid`, `flat_y`, `kernel_path`, the rotating slow-env sets, the replay trace, the Python layer's `t`, `_vel_calls`,
`_spec` and its output ring (csrc/diral_env.hip, diral_amd/vec_env.py) - is host state that only a call ORDER reaches.
`draw_program(family, seed)` draws 40 to 60 operations from `np.random.default_rng`, never from device state;
`HostModel` executes the same list on the CPU: the oracle in its IEEE-square mode for plain calls,
tests/host_closed_loop.py for `step_policy` / `prefill`, the loop of step + shape for `rollout`.  Expected values never
come from the GPU; the actions behind a `step_policy` are the host policy's.  No GPU import here.

Transition classes: every op belongs to one of CLASSES.  The ordered pairs of classes a family accepts are dealt out
over the six residues of `seed % 6` (two shuffled decks of all pairs, three hands each), and a program walks its hand:
six seeds with different residues meet every pair at least twice (tests/test_call_programs.py checks the committed ones).

Calls the handle must refuse (a K-slot launch while some vehicle is off the y = 0 lane) are drawn on purpose, rarely:
the expected result is DiralError(DIRAL_ERR_UNSUPPORTED) and the next comparison proves the env untouched.
"""
import hashlib
import math

import numpy as np

from diral_amd.config import (KERNEL_FAST64, KERNEL_GENERAL, KERNEL_LARGE, KERNEL_WIDE, STEP_DESIGN, STEP_MY_STEP,
                              STEP_MY_STEP_CH, bench_config)
from tests import host_closed_loop as H
# the suite's own bars (importable without a GPU)
from tests.host_closed_loop import _exp_bounds, uses_exp  # noqa: F401  (re-exported)
from tests.oracle_compare import stored_age

RICH_STATE = dict(add_channel_obs=True, add_reward=True, add_index=True, add_velocity=True, add_position=True)
MODE_NAME = {STEP_MY_STEP: "my_step", STEP_MY_STEP_CH: "my_step_ch", STEP_DESIGN: "my_step_design"}

# family: config, batch, output dtype, the handle's step kind, DIRAL_TABLE_FORM, which K-slot launches it takes
FAMILIES = {
    "f64_full": dict(cfg=lambda: bench_config(64, 32, 2000.0), B=6, f64=False, mode=STEP_MY_STEP, form=None,
                     kslot=("rollout", "step_policy", "prefill")),
    "f64_sparse": dict(cfg=lambda: bench_config(40, 7, 6000.0, communication_range=140.0, mobility_vary=True), B=6, f64=True,
                       mode=STEP_MY_STEP, form=None, kslot=("rollout", "step_policy", "prefill"), sparse=True),
    "f64_rich": dict(cfg=lambda: bench_config(33, 9, 1200.0, State=RICH_STATE, track_arrival=True), B=5, f64=True,
                     mode=STEP_MY_STEP, form=None, kslot=(), trace=True),
    "f64_ch": dict(cfg=lambda: bench_config(64, 16, 2000.0, reward_design=3), B=6, f64=True, mode=STEP_MY_STEP_CH, form=None,
                   kslot=("rollout", "step_policy", "prefill")),
    "w2_plane": dict(cfg=lambda: bench_config(100, 20, 2500.0), B=4, f64=True, mode=STEP_MY_STEP, form="plane",
                     kslot=("rollout", "step_policy")),
    "w2_packed": dict(cfg=lambda: bench_config(128, 16, 4000.0, mobility_vary=True), B=4, f64=False, mode=STEP_MY_STEP,
                      form="packed", kslot=("rollout", "step_policy")),
    "w4_packed": dict(cfg=lambda: bench_config(256, 64, 4000.0), B=4, f64=True, mode=STEP_MY_STEP, form="packed",
                      kslot=("rollout", "step_policy")),
    "w4_sparse": dict(cfg=lambda: bench_config(200, 24, 30000.0, communication_range=140.0), B=4, f64=False, mode=STEP_MY_STEP,
                      form="plane", kslot=("rollout", "step_policy"), sparse=True),
}
FAMILY_ID = {name: i for i, name in enumerate(FAMILIES)}
# the committed programs: six seeds per family with six different residues mod 6 (see the module docstring); seeds for
# which the HOST says that no env is left out, every transition is met twice and the non-vacuity conditions hold
SEEDS = {name: (0, 1, 2, 3, 4, 5) for name in FAMILIES}
SEEDS["f64_sparse"] = (0, 1, 2, 3, 10, 5)       # (seed 4: a re-selection margin of 2.6e-12 dB leaves three envs out)
SEEDS["f64_ch"] = (0, 1, 2, 9, 4, 5)            # (seed 3 runs out of ops with one pair of its hand unwalked)

CLASSES = ("step", "step_general", "step_large", "observe", "kslot", "import", "flat_flip", "offroad", "velocity", "reset",
           "export")
OP_CLASS = {"step": "step", "step_general": "step_general", "step_large": "step_large", "observe": "observe",
            "rollout": "kslot", "step_policy": "kslot", "prefill": "kslot",
            "export_import": "import", "export_entries_import": "import", "import_partial": "import",
            "load_saved_positions": "import", "restore_flat": "import",
            "flat_flip": "flat_flip", "import_offroad": "offroad", "update_velocity": "velocity", "reset": "reset",
            "export": "export", "metrics": "export", "info_age": "export", "check": "export"}
STEP_LIKE = ("step", "step_general", "step_large", "rollout", "step_policy", "prefill")
MIN_OPS, MAX_OPS = 40, 60
POLICY = dict(seed=3, threshold=-110.0, keep_prob=0.5, counter_mod=4)


def family_classes(family):
    return tuple(c for c in CLASSES if c != "kslot" or FAMILIES[family]["kslot"])


def takes(family, op, flat):
    """Whether the handle takes a K-slot launch (csrc/diral_env.hip plan_step): every one of them needs all vehicles on
    the y = 0 lane; a one-slot `step_policy` falls back to three launches instead of refusing; 64 < N <= 256 keeps the
    tables in HBM between slots and writes one state vector only."""
    if op["op"] == "step_policy":
        return op["K"] == 1 or flat
    if op["op"] == "rollout":
        return flat and (FAMILIES[family]["cfg"]().num_users <= 64 or op["states"] != "all")
    return flat                                                     # prefill (drawn at N <= 64 only)


def predicted_kernel(family, op, flat):
    """`last_kernel() & 15` behind a step-like op: a wide handle with a vehicle off the lane runs the general kernel."""
    if op["op"] == "step_general":
        return KERNEL_GENERAL
    if op["op"] == "step_large":
        return KERNEL_LARGE
    if FAMILIES[family]["cfg"]().num_users <= 64:
        return KERNEL_FAST64
    return KERNEL_WIDE if flat else KERNEL_GENERAL


# ---- the generator ----------------------------------------------------------------------------------------------
def _hand(family, seed):
    """The ordered pairs of classes this program must walk: hand `seed % 3` of deck `(seed % 6) // 3`."""
    classes = family_classes(family)
    deck, hand = divmod(int(seed) % 6, 3)
    pairs = [(a, b) for a in classes for b in classes]
    np.random.default_rng([FAMILY_ID[family], 1000 + deck]).shuffle(pairs)
    return set(map(tuple, pairs[hand::3]))


def _positions(rng, B, N, L):
    """Fractional positions in [0, L): on integer positions the distances of different pairs agree to a few ulps and
    the order of their log10 values is ambiguous to the SPS agent (tests/test_gpu_closed_loop_host.py)."""
    return rng.integers(0, int(L) - 1, size=(B, N)).astype(np.float64) + rng.random((B, N))


def _speeds(rng, B, N, vary):
    if vary:
        return rng.choice(np.array([1.1, 1.15, 1.7, 2.25, 2.77]), size=(B, N))
    return rng.uniform(1.1, 2.7, size=(B, N))


def _offroad(rng, B, N, L, vary):
    """Positions in [-3L, 5L] with the edges (exactly L, 2L, -0.0, a tiny negative value, a sum one ulp below zero) and
    speeds in [-2L, 2L]: s = x + v + L is below zero on lane 0 and above 2L on lane 1 whatever the speeds become."""
    x, v = _positions(rng, B, N, L), _speeds(rng, B, N, vary)
    for b in range(B):
        lanes = rng.permutation(N)[:14]
        x[b, lanes[0]], x[b, lanes[1]] = -2.5 * L - rng.random(), 4.25 * L + rng.random()
        x[b, lanes[2]], x[b, lanes[3]], x[b, lanes[4]], x[b, lanes[5]] = L, 2.0 * L, -0.0, -1e-300
        v[b, lanes[6]] = 1.5
        x[b, lanes[6]] = np.nextafter(-(L + 1.5), -np.inf)          # s = -ulp: Python's % gives L - ulp, or L itself
        v[b, lanes[7]], x[b, lanes[7]] = -L, -0.0                    # s = +0.0
        v[b, lanes[8]], x[b, lanes[8]] = -L, -1e-300
        x[b, lanes[9:12]] = rng.uniform(-3.0 * L, 5.0 * L, size=3)
        v[b, lanes[11:14]] = rng.uniform(-2.0 * L, 2.0 * L, size=3)
    return x, v


def _actions(rng, B, N, A, lead=()):
    return rng.integers(0, A, size=lead + (B, N)).astype(np.int32)


class _Model:
    """What the generator tracks to know what the family accepts at this point."""

    def __init__(self):
        self.flat, self.t, self.stepped_off_lane, self.offroad_pending = True, 0, False, False
        self.trace_on, self.policy_next = False, False


def _make_op(cls, m, rng, family):
    f = FAMILIES[family]
    cfg = f["cfg"]()
    B, N, A, L = f["B"], cfg.num_users, cfg.num_channels, cfg.highway_length
    acts = (lambda lead=(): _actions(rng, B, N, A, lead))
    if cls == "step":
        return dict(op="step", acts=acts(), chobs=bool(rng.random() < 0.4))
    if cls in ("step_general", "step_large"):
        return dict(op=cls, acts=acts((int(rng.integers(1, 4)),)))
    if cls == "observe":
        chobs = rng.uniform(0.0, 300.0, size=(B, N, A))
        chobs[rng.random((B, N, A)) < 0.3] = 0.0
        chobs[rng.random((B, N, A)) < 0.2] = 100000.0
        return dict(op="observe", acts=acts(), chobs=chobs, rew=rng.uniform(-2.0, 1.0, size=(B, N)),
                    episode=float(rng.integers(0, 9)), eps=float(rng.random()))
    if cls == "kslot":
        kinds = list(f["kslot"])
        if not m.flat and rng.random() >= 0.3:
            kind, K = "step_policy", 1                               # off the lane: mostly what is not refused
        else:
            kind = kinds[int(rng.integers(len(kinds)))]
            K = int(rng.integers(1, 13 if kind == "rollout" else 9))
            if not m.flat and kind == "step_policy":
                K = max(K, 2)
        vel_seed = int(rng.integers(0, 1 << 20))
        if kind == "rollout":
            states = ("last", "all", None)[int(rng.integers(3))]
            if N > 64 and states == "all":
                states = "last"
            return dict(op="rollout", K=K, acts=acts((K,)), states=states, vel_seed=vel_seed)
        if kind == "prefill":
            return dict(op="prefill", K=K, seed=int(rng.integers(0, 1 << 30)))
        return dict(op="step_policy", K=K, acts=acts(), vel_seed=vel_seed)
    if cls == "import":
        if not m.flat and m.stepped_off_lane:
            return dict(op="restore_flat")
        kinds = ["export_import", "export_entries_import", "import_partial:tables"]
        if not m.offroad_pending:
            kinds.append("import_partial:pos")
        if f.get("trace"):
            kinds += ["load_saved_positions"] * 2
        kind = kinds[int(rng.integers(len(kinds)))]
        if kind == "load_saved_positions":
            if m.trace_on and rng.random() < 0.5:
                return dict(op=kind, trace=None)
            T = int(rng.integers(5, 10))
            tr = np.stack([_positions(rng, 1, N, L)[0] for _ in range(T)])
            wild = rng.random((T, N)) < 0.08                         # a replayed trace may leave the highway
            tr[wild] = rng.uniform(-3.0 * L, 5.0 * L, size=int(wild.sum()))
            return dict(op=kind, trace=tr)
        if kind == "import_partial:pos":
            return dict(op="import_partial", what="pos", pos_x=_positions(rng, B, N, L),
                        vel=_speeds(rng, B, N, cfg.mobility_vary) if rng.random() < 0.5 else None)
        if kind == "import_partial:tables":
            return dict(op="import_partial", what="tables")
        return dict(op=kind)
    if cls == "flat_flip":
        y = rng.choice(np.array([0.0, 0.0, 0.0, 1.0, 2.0]), size=(B, N))
        y[int(rng.integers(B)), int(rng.integers(N))] = 1.0
        return dict(op="flat_flip", pos_y=y)
    if cls == "offroad":
        x, v = _offroad(rng, B, N, L, cfg.mobility_vary)
        return dict(op="import_offroad", pos_x=x, vel=v)
    if cls == "velocity":
        if rng.random() < 0.5:
            return dict(op="update_velocity", draws=None)            # the default seed: counts the calls since the reset
        return dict(op="update_velocity", draws=rng.integers(1, 4, size=(B, N)).astype(np.uint8))
    if cls == "reset":
        if m.offroad_pending:
            x, v = _offroad(rng, B, N, L, cfg.mobility_vary)         # reset_topology(x0=...) may leave the highway too
        else:
            x, v = _positions(rng, B, N, L), _speeds(rng, B, N, cfg.mobility_vary)
        return dict(op="reset", x0=x, v0=v)
    assert cls == "export", cls
    r = rng.random()
    if r < 0.5:
        return dict(op="export")
    if r < 0.75:
        return dict(op="metrics", clear=bool(rng.random() < 0.5))
    if r < 0.9 and cfg.track_arrival:
        return dict(op="info_age")
    return dict(op="check")


def _advance(m, op, family):
    """The model behind `op`; marks a refusal and the kernel the dispatch must pick."""
    name = op["op"]
    if name in ("rollout", "step_policy", "prefill"):
        op["refused"] = not takes(family, op, m.flat)
    if name in STEP_LIKE and not op.get("refused"):
        op["kernel"] = predicted_kernel(family, op, m.flat)
        op["flat"] = m.flat
        if name != "prefill" and name != "rollout" and m.policy_next:
            op["policy_acts"] = True                                 # the first actions are the host policy's
        m.policy_next = name in ("step_policy", "prefill")
        m.offroad_pending = False
        if not m.flat:
            m.stepped_off_lane = True
        if name in ("step_general", "step_large"):
            m.t += len(op["acts"])
        elif name != "prefill":
            m.t += op.get("K", 1)
    elif name == "flat_flip":
        m.flat, m.stepped_off_lane = False, False
    elif name == "restore_flat":
        m.flat = True
    elif name == "reset":
        m.flat, m.t = True, 0
    elif name == "import_offroad":
        m.offroad_pending = True
    elif name == "load_saved_positions":
        m.trace_on = op["trace"] is not None


def draw_program(family, seed):
    """-> dict(family, seed, cfg, B, x0, v0, ops): deterministic in (family, seed)."""
    f = FAMILIES[family]
    cfg = f["cfg"]()
    rng = np.random.default_rng([FAMILY_ID[family], int(seed)])
    classes = family_classes(family)
    left = _hand(family, seed)
    B, N, L = f["B"], cfg.num_users, cfg.highway_length
    x0, v0 = _positions(rng, B, N, L), _speeds(rng, B, N, cfg.mobility_vary)
    m, ops = _Model(), []

    def emit(cls):
        op = _make_op(cls, m, rng, family)
        _advance(m, op, family)
        ops.append(op)

    def weight(c):
        w = 1.0
        if not m.flat:
            w *= 4.0 if (c == "import" and m.stepped_off_lane) else 1.0
            w *= 0.25 if c == "kslot" else 1.0
            w *= 2.0 if (c.startswith("step") and not m.stepped_off_lane) else 1.0
        return w

    emit("step")
    cur = "step"
    budget = MAX_OPS - 4                                             # room for the closing ops
    while len(ops) < budget and (left or len(ops) < MIN_OPS):
        cand = [c for c in classes if (cur, c) in left]
        if not cand:                                                 # in transit: towards the class with most pairs left
            out = {c: sum(1 for p in left if p[0] == c) for c in classes}
            best = max(out.values())
            cand = [c for c in classes if out[c] == best] if best else list(classes)
        w = np.array([weight(c) for c in cand])
        nxt = cand[int(rng.choice(len(cand), p=w / w.sum()))]
        left.discard((cur, nxt))
        emit(nxt)
        cur = nxt
    if not m.flat:                                                   # every program ends on the lane, with a step behind it
        if not m.stepped_off_lane:
            emit("step")
        emit("import")
    emit("step")
    return dict(family=family, seed=int(seed), cfg=cfg, B=B, x0=x0, v0=v0, ops=ops, uncovered=sorted(left))


def transitions(prog):
    cls = [OP_CLASS[o["op"]] for o in prog["ops"]]
    return list(zip(cls[:-1], cls[1:]))


def describe(op):
    bits = [op["op"]]
    for k in ("K", "states", "what", "chobs", "clear", "refused"):
        if k in op and not isinstance(op[k], np.ndarray):
            bits.append("%s=%s" % (k, op[k]))
    if op["op"] in ("step_general", "step_large"):
        bits.append("n=%d" % len(op["acts"]))
    return " ".join(bits)


# ---- the host model ---------------------------------------------------------------------------------------------
class HostModel:
    """Executes a program on the CPU; `run()` yields (op, expected) in order."""

    def __init__(self, prog):
        f = FAMILIES[prog["family"]]
        self.prog, self.f, self.cfg = prog, f, prog["cfg"]
        self.B, self.N, self.A = prog["B"], self.cfg.num_users, self.cfg.num_channels
        self.mode = f["mode"]
        self.npdt = np.float64 if f["f64"] else np.float32
        sps = H.HostSps.from_seed(self.B * self.N, self.A, POLICY["seed"], threshold=POLICY["threshold"],
                                  keep_prob=POLICY["keep_prob"])
        sps.counter %= POLICY["counter_mod"]
        self.loop = H.HostClosedLoop(self.cfg, self.B, prog["x0"], prog["v0"], sps, POLICY["seed"], mode=MODE_NAME[self.mode],
                                     dtype=self.npdt)
        self.orc = self.loop.ob.o
        self.t, self.vel_calls = 0, 0
        self.mbase = np.zeros_like(self.orc.metrics())
        self.checkpoint = self.tables()
        self.next_acts = None
        # the record the CPU test reads
        self.rec = dict(steps_off_lane=0, steps_after_restore=0, flips=0, offroad=[], lag_kslot=0, lag_export=0, refused=0)
        self._restored, self._offroad_open = False, False

    # -- pieces ----------------------------------------------------------------------------------------------------
    def tables(self):
        e = self.orc.export()
        return dict(seq=e["seq"].copy(), age=stored_age(e["age"]), x=e["x"].copy())

    def flat(self):
        return not self.orc.export()["pos_y"].any()

    def sync_table_y(self):
        """The handle stores no ypos plane: an entry's ypos IS its subject's pos_y once the subject was heard (DESIGN.md
        section 2, SURVEY.md Q7 - a vehicle never changes its lane), so an import of pos_y or of tables (import_state has
        no `y` argument) redefines it.  The oracle keeps the plane; it is brought to that definition behind such imports."""
        e = self.orc.export()
        self.orc.import_state(y=np.where(e["seq"] > 0, e["pos_y"][:, None, :], 0.0))

    def max_lag(self):
        seq = self.orc.export()["seq"]
        own = np.diagonal(seq, axis1=1, axis2=2)[:, None, :]
        lag = (own - seq)[seq > 0]
        return int(lag.max()) if lag.size else 0

    def cast(self, a):
        return None if a is None else np.asarray(a).astype(self.npdt)

    def _before_step(self):
        e = self.orc.export()
        if self._offroad_open:
            s = e["pos_x"] + e["vel"] + self.cfg.highway_length
            self.rec["offroad"].append((int((s < 0).sum()), int((s > 2 * self.cfg.highway_length).sum())))
            self._offroad_open = False
        if e["pos_y"].any():
            self.rec["steps_off_lane"] += 1
        elif self._restored:
            self.rec["steps_after_restore"] += 1

    def slot(self, acts, mode=None):
        self._before_step()
        a = np.ascontiguousarray(acts, dtype=np.int32)
        rew, chobs = self.orc.step(self.mode if mode is None else mode, a, self.t)
        state = self.orc.obtain_state(a, chobs, rew)
        EI = self.cfg.episode_interval
        out = dict(acts=a, rew=self.cast(rew), chobs=self.cast(chobs), state=self.cast(state), rew64=rew,
                   done=np.full(self.B, self.t % EI == EI - 1, np.uint8))
        self.t += 1
        return out

    def first_acts(self, op):
        a = self.next_acts if op.get("policy_acts") else None
        self.next_acts = None
        return a

    # -- the ops ---------------------------------------------------------------------------------------------------
    def run(self):
        for op in self.prog["ops"]:
            yield op, getattr(self, "op_" + op["op"])(op)

    def op_step(self, op):
        a = self.first_acts(op)
        return self.slot(op["acts"] if a is None else a)

    def op_step_general(self, op):
        a0 = self.first_acts(op)
        return dict(slots=[self.slot(a0 if (k == 0 and a0 is not None) else a) for k, a in enumerate(op["acts"])])

    op_step_large = op_step_general

    def op_observe(self, op):
        return dict(state=self.cast(self.orc.obtain_state(op["acts"], op["chobs"], op["rew"], op["episode"], op["eps"])))

    def _kslot_gate(self, op):
        if self.f.get("sparse"):
            self.rec["lag_kslot"] = max(self.rec["lag_kslot"], self.max_lag())
        refused = not takes(self.prog["family"], op, self.flat())
        assert refused == op["refused"], "the generator's model and the host model disagree"
        self.rec["refused"] += refused
        return refused

    def op_rollout(self, op):
        if self._kslot_gate(op):
            return dict(refused=True)
        self.next_acts = None
        EI, outs = self.cfg.episode_interval, []
        for k in range(op["K"]):
            o = self.slot(op["acts"][k])
            o["shaped"], o["sum_r"], o["coll"] = self.loop.shape(o["rew64"], o["acts"])
            if self.cfg.mobility_vary and o["done"][0]:
                self.orc.update_velocity(H.draw_velocity(op["vel_seed"] + (self.t - 1) // EI, self.B, self.N))
            outs.append(o)
        last = outs[-1]
        states = None if op["states"] is None else (np.stack([o["state"] for o in outs]) if op["states"] == "all" else last["state"])
        return dict(shaped=np.stack([o["shaped"] for o in outs]), sum_r=np.stack([o["sum_r"] for o in outs]),
                    coll=np.stack([o["coll"] for o in outs]), states=states, rew=last["rew"], done=last["done"])

    def op_step_policy(self, op):
        if self._kslot_gate(op):
            return dict(refused=True)
        a = self.first_acts(op)
        a = op["acts"] if a is None else a
        for _ in range(op["K"]):
            self._before_step()
        self.loop.vel_seed = op["vel_seed"]
        o = self.loop.run(a, self.t, op["K"])
        o["acts"], o["t"] = np.ascontiguousarray(a, dtype=np.int32), self.t
        o["sps"] = (self.loop.sps.prev_action.reshape(self.B, self.N).copy(), self.loop.sps.counter.reshape(self.B, self.N).copy())
        self.t += op["K"]
        self.next_acts = o["actions"]
        return o

    def op_prefill(self, op):
        if self._kslot_gate(op):
            return dict(refused=True)
        for _ in range(op["K"]):
            self._before_step()
        mode = "my_step_ch" if self.mode == STEP_MY_STEP_CH else "my_step_design"
        states, acts, nxt = self.loop.prefill(H.draw_sample(op["seed"], self.B, self.N, self.A), op["K"], op["seed"], mode=mode)
        self.next_acts = nxt
        return dict(states=states, acts_all=acts, next=nxt, mode=mode)

    def op_update_velocity(self, op):
        draws = op["draws"]
        self.vel_calls += 1                                          # the default seed counts the CALLS since the reset: given draws too
        if draws is None:
            draws = H.draw_velocity(self.vel_calls * 2654435761 + 12345, self.B, self.N)
        self.orc.update_velocity(draws)
        return {}

    def op_load_saved_positions(self, op):
        self.orc.set_trace(op["trace"])
        return {}

    def op_export_import(self, op):
        return dict(export=self.export())                            # (the device imports what it exported)

    def op_export_entries_import(self, op):
        e = self.orc.export()                                        # MA_NeighborTableEntry keeps pos_x as float32
        self.orc.import_state(x=e["x"].astype(np.float32).astype(np.float64), age=stored_age(e["age"]))
        self.sync_table_y()
        return {}

    def op_import_partial(self, op):
        if op["what"] == "pos":
            self.orc.import_state(pos_x=op["pos_x"], vel=op["vel"])
            return {}
        c = self.checkpoint
        self.orc.import_state(seq=c["seq"], age=c["age"], x=c["x"])
        self.sync_table_y()
        return dict(tables=c)

    def op_flat_flip(self, op):
        self.orc.import_state(pos_y=op["pos_y"])
        self.sync_table_y()
        self.rec["flips"] += 1
        self._restored = False
        return {}

    def op_restore_flat(self, op):
        self.orc.import_state(pos_y=np.zeros((self.B, self.N)))
        self.sync_table_y()
        self._restored = True
        return {}

    def op_import_offroad(self, op):
        self.orc.import_state(pos_x=op["pos_x"], vel=op["vel"])
        self._offroad_open = True
        return {}

    def op_reset(self, op):
        if self.rec["flips"] and not self.flat():
            self._restored = True                                    # reset_topology(y0=None) puts every vehicle back on the lane
        self.orc.reset(op["x0"], np.zeros((self.B, self.N)), op["v0"])
        self.t, self.vel_calls = 0, 0
        self.mbase[:] = 0.0
        return {}

    def export(self):
        e = self.orc.export()
        out = dict(pos_x=e["pos_x"], pos_y=e["pos_y"], vel=e["vel"], seq=e["seq"], age=stored_age(e["age"]), x=e["x"])
        if self.cfg.track_arrival:
            out["la"] = e["la"]
        return out

    def op_export(self, op):
        if self.f.get("sparse"):
            self.rec["lag_export"] = max(self.rec["lag_export"], self.max_lag())
        self.checkpoint = self.tables()
        return dict(export=self.export())

    def op_metrics(self, op):
        now = self.orc.metrics()
        m = now - self.mbase
        if op["clear"]:
            self.mbase = now.copy()
        return dict(metrics=m)

    def op_info_age(self, op):
        return dict(t=self.t, info_age=self.orc.info_age(self.t))

    def op_check(self, op):
        return {}

    def closing(self):
        """What closes every program: one full export, the metrics, the information age, `check`."""
        out = dict(export=self.export(), metrics=self.orc.metrics() - self.mbase, t=self.t)
        if self.cfg.track_arrival:
            out["info_age"] = self.orc.info_age(self.t)
        return out


def _feed(h, v):
    if isinstance(v, dict):
        for k in sorted(v):
            h.update(k.encode())
            _feed(h, v[k])
    elif isinstance(v, (list, tuple)):
        for x in v:
            _feed(h, x)
    elif isinstance(v, np.ndarray):
        h.update(str(v.dtype).encode() + str(v.shape).encode() + np.ascontiguousarray(v).tobytes())
    else:
        h.update(repr(v).encode())


def run_host(family, seed):
    """-> (program, [expected per op], closing, record, digest of program and expectations)."""
    prog = draw_program(family, seed)
    host = HostModel(prog)
    expected = [e for _, e in host.run()]
    closing = host.closing()
    h = hashlib.sha256()
    _feed(h, [prog["x0"], prog["v0"], prog["ops"], expected, closing])
    rec = dict(host.rec, left_out=int(host.loop.left_out.sum()), ops=len(prog["ops"]), uncovered=prog["uncovered"],
               host_record=host.loop.record())
    return prog, expected, closing, rec, h.hexdigest()


def python_wrap(x, v, L):
    """network.py:203 on Python floats."""
    return (float(x) + float(v) + float(L)) % float(L)


def same_float_bits(a, b):
    return a == b and math.copysign(1.0, a) == math.copysign(1.0, b)
