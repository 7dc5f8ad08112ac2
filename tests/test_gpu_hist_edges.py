"""GPU parity of the type-2 positional histogram at its bin edges with the viewers OFF the origin, on every path that
computes a bin (the sweep with every viewer at x == 0 is tests/test_gpu_edges.py):

* step_fast64, fast quads: the float64 body `column` (ti = trunc((v + Rb) inv_w 2^20)) and the float32 screening in
  front of it (`column32` / `band32`, the own position folded into a float32 addend), every row with the screening on
  run a second time with DIRAL_F32_MARGIN=0, where the float64 body decides every entry; the column loop `tally` (FLAT
  and, on the two-lane rows, the 2-D statement) through hand-overs, never-heard entries and the keyed quads;
* step_wide, plane and packed form: the one-fma form fma(xpos, inv_w 2^20, cfix_j), cfix_j rounded once per viewer, up
  to a highway of 2^30, common and slow quads;
* the general kernel (hist_bin against the edges), the three launches of step_large.hpp, observe_kernel and the large
  path's observe (a stand-alone obtain_state with foreign arguments behind the step);
* the K-slot instantiations of step_fast64 and step_wide: a two-slot rollout of the same import, every slot's state at
  N <= 64, the last one's beyond, against the oracle stepped twice.

The inputs and both references - the oracle and the plain NumPy statement - come from tests/hist_edge_cases.py;
tests/test_hist_edge_cases.py shows without a GPU that the two agree and that the inputs hold what they are there for.
Everything is compared bit for bit: states, rewards, and the exported tables at the end."""
import numpy as np
import pytest
import torch

from diral_amd.config import (KERNEL_FAST64, KERNEL_GENERAL, KERNEL_LARGE, KERNEL_OBSERVE, KERNEL_PACKED, KERNEL_POLICY,
                              KERNEL_RING, KERNEL_WIDE)
from tests import hist_edge_cases as H
from tests.gpu_util import make_env
from tests.gpu_util import ran_on, same

pytestmark = pytest.mark.gpu

STEP_FAMILY = {"fast64": KERNEL_FAST64, "fast64_y": KERNEL_FAST64, "wide": KERNEL_WIDE, "general": KERNEL_GENERAL,
               "large": KERNEL_LARGE}


def variants(r):
    """(DIRAL_TABLE_FORM, DIRAL_F32_MARGIN) a row runs under: both table forms of step_wide; the float32 screening as the
    host sets it and, where that leaves it on, switched off."""
    if r.path == "wide":
        return [("plane", None), ("packed", None)]
    return [(None, None), (None, "0")] if H.screening_on(r) else [(None, None)]


def imported(r, t, dt):
    cfg = H.config(r)
    env = make_env(cfg, H.B, dtype=dt)
    env.reset_topology(t["px"], t["py"], t["vel"])
    env.import_state(t["px"], t["py"], t["vel"], seq=t["seq"], age=t["age"], x=t["x"])
    if r.path == "general" and r.lanes == 1:                                 # (two lanes beyond 64 vehicles: the planner's own choice)
        env.force_general_kernel()
    if r.path == "large" and r.N <= 256 and r.K <= 64:
        env.force_large_path()
    env.check()                                                              # the import is one the contract allows
    return env


def tables_equal(env, want, tag):
    got = env.export_state()
    for key in H.EXPORT_KEYS:
        same(got[key].cpu().numpy(), want[key], tag + ("export", key))


@pytest.mark.parametrize("r", H.ROWS, ids=H.row_id)
def test_histogram_edges_with_viewers_off_the_origin_on_the_hip_path(r, monkeypatch):
    """Per table form / screening variant and output type two handles on the row's import.  Stepped: one my_step - the
    state against the oracle and its last K columns against np.histogram directly, the kernel family that ran, the
    exported tables -, then a stand-alone obtain_state with foreign arguments (observe_kernel; on forced handles the
    general kernel's / the large path's observe), then - where the handle has no slot loop: the general kernel, the large
    path, step_fast64 off y = 0 - the second my_step.  Rolled out: both slots in one launch on the slot loops of
    step_fast64 (every slot's state) and step_wide (the last one's); the second slot meets the values aimed at its
    position, one lag and one year of age further on."""
    t, o = H.tables(r), H.oracle(r)
    K, N = r.K, r.N
    fa, fc, fr = H.foreign_args(r)
    direct = {1: H.expected(r, t), 2: H.expected(r, t, slot=2)}
    has_slots = r.path in ("fast64", "wide")
    observe_family = {"general": KERNEL_GENERAL if r.lanes == 1 else KERNEL_OBSERVE, "large": KERNEL_LARGE}.get(r.path, KERNEL_OBSERVE)
    for form, margin in variants(r):
        if form:
            monkeypatch.setenv("DIRAL_TABLE_FORM", form)                     # both read when the handle is made
        if margin is not None:
            monkeypatch.setenv("DIRAL_F32_MARGIN", margin)
        for dt in (torch.float64, torch.float32):
            def cast(a):
                return a if dt == torch.float64 else a.astype(np.float32)
            tag = (H.row_id(r), form, margin, str(dt))
            # ---- stepped
            env = imported(r, t, dt)
            obs, rew, _ = env.step(t["acts"][0], 0)
            torch.cuda.synchronize()
            ran_on(env, STEP_FAMILY[r.path])
            if r.path in ("fast64", "fast64_y", "wide"):
                assert env.last_kernel() & KERNEL_RING
                assert bool(env.last_kernel() & KERNEL_PACKED) == (N <= 64 or form == "packed"), env.last_kernel()
            got, got_rew = obs.cpu().numpy().copy(), rew.cpu().numpy().copy()
            same(got[:, :, -K:], cast(direct[1]), tag + ("step vs numpy",))
            same(got, cast(o["state1"]), tag + ("step vs oracle",))
            same(got_rew, cast(o["rew1"]), tag + ("reward",))
            tables_equal(env, o["export1"], tag + ("step",))
            s1 = env.obtain_state(fc, fa, fr, H.FOREIGN_EPISODE, H.FOREIGN_EPS).cpu().numpy().copy()
            ran_on(env, observe_family)
            same(s1[:, :, -K:], cast(direct[1]), tag + ("observe vs numpy",))
            same(s1, cast(o["foreign"]), tag + ("observe vs oracle",))
            env.check()
            if has_slots:
                # ---- rolled out
                env = imported(r, t, dt)
                out = env.rollout(t["acts"], 0, states="all" if N <= 64 else "last")
                torch.cuda.synchronize()
                ran_on(env, STEP_FAMILY[r.path])
                assert env.last_kernel() & KERNEL_POLICY, env.last_kernel()
                st = out["states"].cpu().numpy().copy()
                if N <= 64:
                    same(st[0][:, :, -K:], cast(direct[1]), tag + ("rollout slot 1 vs numpy",))
                    same(st[0], cast(o["state1"]), tag + ("rollout slot 1 vs oracle",))
                    st = st[1]
                got_rew = out["reward"].cpu().numpy().copy()
            else:
                obs, rew, _ = env.step(t["acts"][1], 1)
                torch.cuda.synchronize()
                ran_on(env, STEP_FAMILY[r.path])
                st, got_rew = obs.cpu().numpy().copy(), rew.cpu().numpy().copy()
            same(st[:, :, -K:], cast(direct[2]), tag + ("slot 2 vs numpy",))
            same(st, cast(o["state2"]), tag + ("slot 2 vs oracle",))
            same(got_rew, cast(o["rew2"]), tag + ("slot 2 reward",))
            tables_equal(env, o["export2"], tag + ("slot 2",))
            env.check()
        monkeypatch.delenv("DIRAL_TABLE_FORM", raising=False)
        monkeypatch.delenv("DIRAL_F32_MARGIN", raising=False)
