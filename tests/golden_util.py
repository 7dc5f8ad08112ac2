"""Shared helpers: load tests/golden/*.npz and replay them through a backend.

A fixture holds inputs (config JSON, x0/y0/v0, per-step mode/actions/t, velocity
draws) and the reference's outputs for the same (rews, chobs, state, positions,
table planes).  tests/golden/gen_golden.py recorded them from the reference.
"""
import glob
import hashlib
import json
import os

import numpy as np

from diral_amd.config import EnvConfig, STEP_DESIGN, STEP_MY_STEP, STEP_MY_STEP_CH
from oracle.oracle import Oracle, SQ_POW

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXP_ATOL = 2e-15   # device exp() vs glibc exp(): <= 1-2 ulp of exp(x) <= e; the rewards built
                   # from it (1-exp(1-R), test_env.py:414) cancel, so the bound is absolute
MODES = {"step": STEP_MY_STEP, "ch": STEP_MY_STEP_CH, "design": STEP_DESIGN}


def golden_names(prefix="g"):
    """step-level fixtures are g*.npz; driver-loop fixtures (main_test.py call sequence) are d*.npz"""
    return sorted(os.path.splitext(os.path.basename(p))[0]
                  for p in glob.glob(os.path.join(GOLDEN_DIR, prefix + "*.npz")))


OUT_KEYS = ("rews", "chobs", "state", "pos_x", "vel", "ia")     # the per-slot outputs run_case records


def out_sha(a):
    """The per-slot hash of a thinned fixture's outputs (gen_golden.py `record_every`): sha256 of the array's bytes,
    float arrays with -0.0 folded onto 0.0 (the comparison of the full arrays takes the two as equal too)."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = a.astype(np.float64) + 0.0
    else:
        a = a.astype(np.int64)
    return hashlib.sha256(a.tobytes()).hexdigest()


class Golden:
    def __init__(self, name, path=None):
        self.name = name
        self.d = np.load(path or os.path.join(GOLDEN_DIR, name + ".npz"))
        self._cache = {}
        self.cfg_dict = json.loads(str(self.d["cfg"]))
        self.cfg = EnvConfig.from_dict(self.cfg_dict, track_arrival=True)
        self.N = self.cfg.num_users
        self.A = self.cfg.num_channels
        self.T = len(self.d["modes"])
        self.vel_updates = {int(s): self.d["vel_update_draws"][i]
                            for i, s in enumerate(self.d["vel_update_steps"])}
        # trace replay fixtures: the recorded [T, N] trace and the step after which
        # the reference called load_saved_positions()
        self.trace = self.d["trace"] if "trace" in self.d and self.d["trace"].shape[0] else None
        self.trace_after = int(self.d["trace_after"]) if "trace_after" in self.d else -1

        # thinned fixtures (run_case(record_every=...)): the full per-slot outputs exist at the slots `rec_step`
        # lists, their hashes (`out_sha`, one column per OUT_KEYS) at every slot
        self.kept = {int(s): j for j, s in enumerate(self.d["rec_step"])} if "rec_step" in self.d.files else None

    def __getitem__(self, k):
        if k not in self._cache:                  # (an .npz member is inflated anew on every access)
            self._cache[k] = self.d[k]
        return self._cache[k]

    def out(self, key, i):
        """The recorded output `key` of slot i; None where a thinned fixture holds only its hash."""
        if self.kept is None:
            return self[key][i]
        j = self.kept.get(i)
        return None if j is None else self[key][j]

    def out_sha(self, key, i):
        return str(self["out_sha"][i][OUT_KEYS.index(key)])

    def steps(self):
        for i in range(self.T):
            yield (i, MODES[str(self.d["modes"][i])], self.d["actions"][i],
                   int(self.d["tsteps"][i]), tuple(self.d["episode_eps"][i]))

    def table_checkpoints(self):
        if "tab_step" not in self.d or len(self.d["tab_step"]) == 0:
            return {}
        return {int(s): j for j, s in enumerate(self.d["tab_step"])}


def ulp_diff(a, b):
    """max distance in units-in-the-last-place between two float64 arrays."""
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    ai = a.view(np.int64).copy()
    bi = b.view(np.int64).copy()
    ai[ai < 0] = np.int64(-2**63) - ai[ai < 0]
    bi[bi < 0] = np.int64(-2**63) - bi[bi < 0]
    if a.size == 0:
        return 0
    return int(np.max(np.abs(ai - bi)))


HORIZON_LAGS = ("never", "fresh", "handover", "mid", "byte", "ancient")


def horizon_tables(rng, B, N, L, own_seq, lags=HORIZON_LAGS):
    """Neighbour tables of a run that has been going for `own_seq` slots, for import_state: every vehicle's own entry
    carries `own_seq` (a number, or a [B, N] array: one number per vehicle), age 0 and the vehicle's position; an entry
    about subject k lags k's own number by a draw from the classes named in `lags`, chosen so that every representation
    of an entry meets its neighbour:
      never     never heard (number 0);
      fresh     lag 1 ... 3;
      handover  lag exactly 6, 7, 8 - where the thermometer codes / the xpos ring of N <= 256 hand over to the keys;
      mid       lag 9 ... 40;
      byte      lag exactly 253, 254, 255 - the last ranks a byte holds;
      ancient   lag >= 2^20 (beyond the 20-bit rank of the large path), where the subject's own number allows it.
    The entries beyond the byte ranks ("far": lag >= 254, the `byte` draws of 254 / 255 and the `ancient` ones alike) are
    arranged per column (env, subject), a quarter of the columns each:
      0  as drawn - the only columns where lags of exactly 254 / 255 sit next to ancient numbers;
      1  none (they become `mid`): a column without far entries;
      2  all far entries of the column share ONE number (the one-far-number shortcut of the 2-values-per-lane wide kernel);
      3  exactly two different far numbers (its 32-bit fallback).
    The shared numbers of 2 and 3 are ancient (lag >= 2^20) when `ancient` is among `lags`, else lags 254 / 255 and up to
    299 more: with `ancient`, about a sixth of all entries are ancient and a quarter of the columns hold none.
    xpos is a function of (subject, number) - equal numbers about one subject carry equal xpos, what every run produces and
    what import_state asks for -, ages are min(lag, 255).  An entry whose number would not be positive is never heard.
    Returns dict(pos_x, vel [B, N] float64; seq, age [B, N, N] int32; x [B, N, N] float64), indexed [env][viewer][subject]."""
    own = np.broadcast_to(np.asarray(own_seq, dtype=np.int64), (B, N))
    pos_x = rng.integers(0, int(L), size=(B, N)).astype(np.float64)
    vel = rng.uniform(1.1, 2.7, size=(B, N))
    shape = (B, N, N)
    draws = {
        "never": np.zeros(shape, np.int64),
        "fresh": rng.integers(1, 4, size=shape),
        "handover": rng.integers(6, 9, size=shape),
        "mid": rng.integers(9, 41, size=shape),
        "byte": rng.integers(253, 256, size=shape),
        "ancient": rng.integers(1 << 20, 1_200_000, size=shape),
    }
    names = list(lags)
    kind = rng.integers(0, len(names), size=shape)
    lag = np.zeros(shape, np.int64)
    for i, name in enumerate(names):
        lag = np.where(kind == i, draws[name], lag)
    heard = kind != (names.index("never") if "never" in names else -1)
    col = rng.integers(0, 4, size=(B, 1, N))                          # the column's arrangement of far entries
    far = heard & (lag >= 254)
    if "ancient" in names:
        far_a = rng.integers(1 << 20, 1_200_000, size=(B, 1, N))
    else:
        far_a = rng.integers(254, 256, size=(B, 1, N))
    far_b = far_a + rng.integers(1, 300, size=(B, 1, N))
    lag = np.where(far & (col == 1), draws["mid"], lag)
    lag = np.where(far & (col == 2), far_a, lag)
    lag = np.where(far & (col == 3), np.where(rng.integers(0, 2, size=shape) == 0, far_a, far_b), lag)
    seq = np.where(heard, own[:, None, :] - lag, 0)
    heard = seq > 0
    seq = np.where(heard, seq, 0)
    lag = np.where(heard, lag, 0)
    kk = np.arange(N)[None, None, :]
    x = np.where(heard, (kk * 7919 + seq * 31) % int(L), 0).astype(np.float64)
    age = np.minimum(lag, 255)
    d = np.arange(N)
    seq[:, d, d] = own
    age[:, d, d] = 0
    x[:, d, d] = pos_x
    return dict(pos_x=pos_x, vel=vel, seq=seq.astype(np.int32), age=age.astype(np.int32), x=x)


# ---- the oracle against a fixture (tests/test_oracle_golden.py, tests/golden/gen_golden.py) ------------------------------
def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def replay(g, sq_mode, batch=1):
    o = Oracle(g.cfg, batch=batch, sq_mode=sq_mode)
    o.reset(g["x0"], g["y0"], g["v0"])
    out = dict(rews=[], chobs=[], state=[], pos_x=[], vel=[], ia=[], exp=[])
    for i, mode, acts, t, (ep, eps) in g.steps():
        rews, chobs = o.step(mode, acts, t)
        st = o.obtain_state(acts, chobs, rews, ep, eps)
        out["rews"].append(rews)
        out["chobs"].append(chobs)
        out["state"].append(st)
        out["ia"].append(o.info_age(t))
        if i in g.vel_updates:
            o.update_velocity(g.vel_updates[i])
        if g.trace is not None and i == g.trace_after:
            o.set_trace(g.trace)
        e = o.export()
        out["pos_x"].append(e["pos_x"])
        out["vel"].append(e["vel"])
        out["exp"].append(e)
    return o, out


def compare_with_reference(g):
    """The oracle in its reference-faithful mode against one recorded fixture: every output of every slot bit for
    bit (a thinned fixture: by its per-slot hashes where it dropped the arrays), the table planes by hash at every
    slot and in full at the checkpoints.  AssertionError((key, slot)) on the first difference; also what
    tests/golden/gen_golden.py `fuzz` runs on every drawn case."""
    o, out = replay(g, SQ_POW)
    assert o.S == int(g["state_space"]), ("state_space", -1)
    ck = g.table_checkpoints()
    for i in range(g.T):
        for key in ("rews", "chobs", "state", "pos_x", "vel"):
            got = out[key][i][0]
            ref = g.out(key, i)
            if ref is None:
                assert out_sha(got) == g.out_sha(key, i), (key, i)
                continue
            assert got.shape == ref.shape, (key, i)
            assert np.array_equal(got.view(np.int64), ref.view(np.int64)) or \
                np.array_equal(got, ref), (key, i, "max ulp %d" % ulp_diff(got, ref))
        if g.kept is not None:                  # the hashes cover the kept slots as well
            for key in ("rews", "chobs", "state", "pos_x", "vel"):
                assert out_sha(out[key][i][0]) == g.out_sha(key, i), (key, i)
            assert out_sha(out["ia"][i][0]) == g.out_sha("ia", i), ("ia", i)
        if g.out("ia", i) is not None:
            assert np.array_equal(out["ia"][i][0], g.out("ia", i)), ("ia", i)
        e = out["exp"][i]
        shas = [sha(e["seq"][0].astype(np.int64)), sha(e["age"][0].astype(np.int64)),
                sha(e["x"][0]), sha(e["y"][0]), sha(e["la"][0])]
        assert shas == list(g["table_sha"][i]), ("table_sha", i)
        if i in ck:
            j = ck[i]
            for k in ("seq", "age", "x", "y", "la"):
                assert np.array_equal(e[k][0], g["tab_" + k][j]), ("tab_" + k, i)
    return o
