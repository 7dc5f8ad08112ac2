"""GPU parity of the two secondary observation modes where a float comparison decides an output (the type-2 histogram's
sweep is tests/test_gpu_edges.py):

* a15, the type-1 weighted histogram (State.add_positional_dist_type == 1, network.py:432-471): scaled distances exactly
  on / one ulp around every edge of np.linspace(-1, 1, K + 1), several values on one edge, empty edges in between, +-0,
  viewers with nothing valid, norms of 0, never-heard entries off y = 0 - on the four implementations of
  csrc/posdist_kernel.hpp and the three forms of the table they read;
* a16, the sorted true distances (State.add_positional_dist, network.py:409-430): exact ties across the x ranking, both
  extremes equally far, everybody on one point (NaN rows) - on posdist_sorted_flat_kernel and the literal kernel.

The inputs and both references - the oracle and the plain NumPy statement - come from tests/posdist_cases.py;
tests/test_posdist_cases.py shows without a GPU that the two agree and that the inputs hold what they are there for.
Everything is compared bit for bit."""
import numpy as np
import pytest
import torch

from diral_amd.config import (KERNEL_FAST64, KERNEL_GENERAL, KERNEL_LARGE, KERNEL_OBSERVE, KERNEL_PACKED, KERNEL_RING,
                              KERNEL_WIDE)
from tests import posdist_cases as P
from tests.gpu_util import make_env, ran_on, same

pytestmark = pytest.mark.gpu


def step_family(N, K, off_lane):
    """The kernel family a my_step of this shape is meant for: the three launches of step_large.hpp beyond 256 vehicles or
    64 bins, step_fast64 to 64 vehicles, step_wide to 256 - on the y = 0 lane; off it the general kernel."""
    if N > 256 or K > 64:
        return KERNEL_LARGE
    if N <= 64:
        return KERNEL_FAST64
    return KERNEL_GENERAL if off_lane else KERNEL_WIDE


@pytest.mark.parametrize("case", P.A15_CASES, ids=P.a15_id)
def test_type1_histogram_edge_sweep_on_the_hip_path(case, monkeypatch):
    """Every vehicle sits at x = L - v, so its post-move position is exactly 0 and a table distance is the entry's xpos
    itself; communication_range 0: the imported tables reach the observation only stamped and aged.  Lag slot 0 of every
    subject is +-1024 at age 0: the norm of a viewer is exactly 1024 and the scaled values are the candidates themselves.
    Per output type two handles.  Stepped: import, one my_step - the state against the oracle and its last K columns
    against np.histogram directly -, then a stand-alone obtain_state with foreign arguments: the kernels read the ring,
    the packed words and the entries handed over to the plane at lag 7.  Observed only: vehicles at x = 0, the same
    tables, no step: the (seq, age) plane right after an import, ages as imported.
    The step of the two shapes off y = 0 beyond 64 vehicles runs on the general kernel (130) and on the three launches
    (300): step_wide takes the one-lane highway only; their observation launch is the kernel named in posdist_cases."""
    K, N, ylane, ghosts, degenerate, form = case
    if form:
        monkeypatch.setenv("DIRAL_TABLE_FORM", form)                         # read when the handle is made
    t, o, cfg = P.a15_tables(*case[:5]), P.a15_oracle(*case[:5]), P.a15_config(K, N)
    B = t["B"]
    fa, fc, fr = P.foreign_args(cfg, B, 1500 + K + N)
    family = step_family(N, K, ylane != 0)
    observe_family = KERNEL_LARGE if family == KERNEL_LARGE else KERNEL_OBSERVE
    direct = {True: P.a15_expected(t, stamped=True), False: P.a15_expected(t, stamped=False)}
    zeros = np.zeros((B, N))
    for dt in (torch.float64, torch.float32):
        def cast(a):
            return a if dt == torch.float64 else a.astype(np.float32)
        tag = (P.a15_id(case), str(dt))
        # ---- stepped
        env = make_env(cfg, B, dtype=dt)
        env.reset_topology(t["pos_x"], t["pos_y"], t["vel"])
        env.import_state(t["pos_x"], t["pos_y"], t["vel"], seq=t["seq"], age=t["age"], x=t["x"])
        env.check()                                                          # the import is one the contract allows
        obs, rew, _ = env.step(t["acts"], 0)
        torch.cuda.synchronize()
        ran_on(env, family)
        if family in (KERNEL_FAST64, KERNEL_WIDE):
            assert env.last_kernel() & KERNEL_RING
            assert bool(env.last_kernel() & KERNEL_PACKED) == (N <= 64 or form == "packed"), env.last_kernel()
        got, got_rew = obs.cpu().numpy().copy(), rew.cpu().numpy().copy()
        assert np.array_equal(env.export_state(tables=False)["pos_x"].cpu().numpy(), zeros)   # post-move x == 0
        assert got.dtype == cast(o["state"]).dtype
        same(got[:, :, -K:], cast(direct[True]), tag + ("step vs numpy",))
        same(got, cast(o["state"]), tag + ("step vs oracle",))
        same(got_rew, cast(o["rew"]), tag + ("reward",))
        env.check()
        s1 = env.obtain_state(fc, fa, fr, P.FOREIGN_EPISODE, P.FOREIGN_EPS).cpu().numpy().copy()
        ran_on(env, observe_family)
        same(s1[:, :, -K:], cast(direct[True]), tag + ("observe after step vs numpy",))
        same(s1, cast(o["foreign"]), tag + ("observe after step vs oracle",))
        env.check()
        # ---- observed only
        still = make_env(cfg, B, dtype=dt)
        still.reset_topology(zeros, t["pos_y"], t["vel"])
        still.import_state(zeros, t["pos_y"], t["vel"], seq=t["seq"], age=t["age"], x=t["x"])
        s2 = still.obtain_state(fc, fa, fr, P.FOREIGN_EPISODE, P.FOREIGN_EPS).cpu().numpy().copy()
        ran_on(still, observe_family)
        same(s2[:, :, -K:], cast(direct[False]), tag + ("observe after import vs numpy",))
        same(s2, cast(o["observed"]), tag + ("observe after import vs oracle",))
        still.check()


@pytest.mark.parametrize("N,lanes", P.A16_CASES)
def test_sorted_distances_ties_and_zero_norm_on_the_hip_path(N, lanes):
    """Integer-valued positions at one speed: clusters of equal x, everybody on one point (norm 0: the reference's row is
    NaN, and must be NaN in exactly the same places), two points, vehicles that wrap to 0 beside a tail of ties, viewers
    equally far from both extremes.  One lane: posdist_sorted_flat_kernel; lanes {0, 1.5}: the literal kernel (and the
    step itself on the general kernel at 64 < N <= 256).  One my_step, then a stand-alone obtain_state."""
    p, o, cfg = P.a16_positions(N, lanes), P.a16_oracle(N, lanes), P.a16_config(N)
    B = p["B"]
    fa, fc, fr = P.foreign_args(cfg, B, 1600 + N)
    family = step_family(N, cfg.State.num_bins, lanes)
    cols = slice(P.A, P.A + N - 1)
    direct = P.a16_expected(p)
    for dt in (torch.float64, torch.float32):
        def cast(a):
            return a if dt == torch.float64 else a.astype(np.float32)
        tag = (N, lanes, str(dt))
        env = make_env(cfg, B, dtype=dt)
        env.reset_topology(p["x0"], p["y0"], p["v0"])
        obs, rew, _ = env.step(p["acts"], 0)
        torch.cuda.synchronize()
        ran_on(env, family)
        got, got_rew = obs.cpu().numpy().copy(), rew.cpu().numpy().copy()
        assert got.dtype == cast(o["state"]).dtype
        same(got[:, :, cols], cast(direct), tag + ("step vs numpy",), equal_nan=True)
        same(got, cast(o["state"]), tag + ("step vs oracle",), equal_nan=True)
        same(got_rew, cast(o["rew"]), tag + ("reward",))
        env.check()
        s1 = env.obtain_state(fc, fa, fr, P.FOREIGN_EPISODE, P.FOREIGN_EPS).cpu().numpy().copy()
        ran_on(env, KERNEL_LARGE if family == KERNEL_LARGE else KERNEL_OBSERVE)
        same(s1[:, :, cols], cast(direct), tag + ("observe vs numpy",), equal_nan=True)
        same(s1, cast(o["foreign"]), tag + ("observe vs oracle",), equal_nan=True)
        env.check()
