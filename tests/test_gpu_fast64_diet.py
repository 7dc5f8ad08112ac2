"""The 64-vehicle step kernel (csrc/step_fast64_body.inc) around what DESIGN.md 3.2 item 23 changed in it - the LDS layout
with the fixed-size arrays in front, the histogram zeroed with 16-byte stores, the float32 screen `column32` with the margin
in the fma's addend - and around P1's per-resource tail, which that item measured in a leaner form and left as it was:
against the GENERAL kernel (`force_general_kernel`) on twin handles, bit for bit, asserting which family ran on either handle.

* P1's tail.  N = 8, 33, 64; A = 1, 5, 32, 33, 64; float32 and float64 outputs; my_step, my_step_ch, my_step_design, and
  my_step with State.type 1 (the observation is the constant 1).  Env 0 is placed by hand (`hand_env`), the others are
  random.  Three slots: the channel observation, state, reward of every slot and all tables behind the last one (the gather
  source of a receiver shows only through the merge).
* `column32`.  The bin-edge import of tests/hist_edge_cases.py (three envs; viewers behind the move at 0, near L / 3 and one
  step below L; entries on every interior edge, at -Rb and +Rb, one float64 step to either side) as it is and with every
  aimed entry moved one FLOAT32 step up / down, under DIRAL_F32_MARGIN unset, 0, 1024 and 16384 (read when the handle is made).
* Layout and zeroing.  State.num_bins = 1, 2, 19, 20, 63, 64 with A = 1, 32, 33, 64, plain and rich State flags, both output
  types, two slots each (a histogram cell left dirty, or two arrays that overlap, show in the second); one rollout of three
  slots in one launch (the slot loop) against three single slots of the general kernel.
The twin of a case is computed once per case; nothing sleeps or starts a process."""
import math

import numpy as np
import pytest
import torch

from diral_amd.config import KERNEL_FAST64, KERNEL_GENERAL, KERNEL_POLICY, STEP_DESIGN, STEP_MY_STEP, STEP_MY_STEP_CH, bench_config
from tests import hist_edge_cases as H
from tests.gpu_util import dev, everything, make_env, ran_on, same, slot

pytestmark = pytest.mark.gpu

L, RC = 2000.0, 180.0
B = 4
MODES = {"my_step": STEP_MY_STEP, "my_step_ch": STEP_MY_STEP_CH, "my_step_design": STEP_DESIGN}


def hand_env(N, A):
    """Positions, speeds and actions of env 0 (roles r mean resource r % A; N >= 8):
      v0 100 r0 | v1 100 + Rc r1 | v2 one float64 step below v1 r1 | v3 700 r0 | v4 800 r0 | v5 750 r2 | v6 1700 r0 | v7 1710 r0
      v8 1720 r0 (N > 8) | the others spread over [1000, 1400] on the resources 4 ... A - 1 (r0 where A <= 4).
    With A >= 4: resource 0 has five transmitters (six with N > 8), resource 1 two, resource 2 one, resource 3 none.  Of
    resource 0: v1 is exactly Rc from v0 and far from the rest - no transmitter in range, observation 100000, its gather
    source itself; v2 is one step inside; v5 has v3 and v4 at exactly 50 - the lower id wins; v6 ... v8 are in nobody's range
    on the resources 1 and 2; every transmitter reads 0 on its own resource."""
    x = np.empty(N)
    a = np.empty(N, np.int64)
    x[:8] = [100.0, 100.0 + RC, math.nextafter(100.0 + RC, 0.0), 700.0, 800.0, 750.0, 1700.0, 1710.0]
    a[:8] = [0, 1, 1, 0, 0, 2, 0, 0]
    if N > 8:
        x[8], a[8] = 1720.0, 0
        rest = N - 9
        x[9:] = np.linspace(1000.0, 1400.0, rest) if rest > 1 else 1200.0
        a[9:] = (4 + np.arange(rest) % (A - 4)) if A > 4 else 0
    return x, (a % A).astype(np.int32)


def p1_inputs(N, A):
    rng = np.random.default_rng([N, A, 23])
    x0 = rng.integers(0, int(L), size=(B, N)).astype(np.float64)
    v0 = rng.uniform(1.1, 2.7, size=(B, N))
    acts = rng.integers(0, A, size=(3, B, N)).astype(np.int32)
    acts[:, B - 1] = acts[0, B - 1]                          # the last env keeps its actions: its stragglers age
    x0[0], acts[0, 0] = hand_env(N, A)
    return x0, v0, acts


def twins(cfg, mode, dt, x0, v0):
    out = []
    for general in (False, True):
        env = make_env(cfg, x0.shape[0], mode=mode, dtype=dt)
        env.force_general_kernel(general)
        env.reset_topology(x0, np.zeros(x0.shape), v0)
        out.append(env)
    return out


def compare_slots(fast, gen, acts, tag, expect_errors=False):
    for t, a in enumerate(acts):
        got, want = slot(fast, a, t), slot(gen, a, t)
        ran_on(fast, KERNEL_FAST64)
        ran_on(gen, KERNEL_GENERAL)
        for key in ("chobs", "state", "reward", "done"):
            same(got[key], want[key], tag + (t, key), equal_nan=True)
        yield t, got
    ef, eg = everything(fast, len(acts) - 1), everything(gen, len(acts) - 1)
    for key in eg:
        if key == "metrics":                                 # (float sums in another order)
            assert np.allclose(ef[key], eg[key], rtol=1e-12, atol=1e-9), tag + (key,)
        else:
            same(ef[key], eg[key], tag + ("behind", key), equal_nan=True)
    if not expect_errors:
        fast.check()
        gen.check()


@pytest.mark.parametrize("A", [1, 5, 32, 33, 64])
@pytest.mark.parametrize("N", [8, 33, 64])
def test_p1_tail_against_the_general_kernel(N, A):
    x0, v0, acts = p1_inputs(N, A)
    # (arrival stamps: the EXTRA instantiations, whose search keeps in-range transmitters only; without: `search_min`)
    variants = [("my_step", STEP_MY_STEP, 2, False), ("my_step_arrival", STEP_MY_STEP, 2, True), ("my_step_ch", STEP_MY_STEP_CH, 2, True),
                ("my_step_design", STEP_DESIGN, 2, False), ("my_step_type1", STEP_MY_STEP, 1, False)]
    for name, mode, stype, arrival in variants:
        cfg = bench_config(N, A, L, communication_range=RC, State=dict(type=stype), track_arrival=arrival)
        for dt in (torch.float32, torch.float64):
            fast, gen = twins(cfg, mode, dt, x0, v0)
            # (State.type 1 next to the piggybacked histogram: the reference fails where no transmitter is in range - both
            # kernels raise the same flag, which is not what this case is about)
            for t, got in compare_slots(fast, gen, acts, (N, A, name, str(dt)), expect_errors=stype == 1):
                if t or A < 4:
                    continue
                ch = got["chobs"][0]                          # the hand-placed env holds what it was placed for
                if mode == STEP_MY_STEP and stype == 2:
                    assert ch[1, 0] == 100000.0 and ch[2, 0] == np.asarray(x0[0, 2] - x0[0, 0]).astype(ch.dtype)
                    assert ch[5, 0] == 50.0 and ch[0, 0] == 0.0 and ch[6, 1] == 100000.0 and ch[7, 2] == 100000.0
                    assert not ch[:, 3].any()
                else:
                    assert ch[1, 0] == 1.0 and ch[0, 0] == 0.0 and not ch[:, 3].any()


def _f32_step(x, filler, up, Lmax):
    """Every aimed entry one float32 step up or down (a function of the value: equal stamps stay equal)."""
    f = x.astype(np.float32)
    fd = f.astype(np.float64)
    beyond = (fd > x) if up else (fd < x)                    # the conversion already went that way
    y = np.where(beyond, f, np.nextafter(f, np.float32(np.inf if up else -np.inf))).astype(np.float64)
    ok = ~filler & (y >= 0.0) & (y <= Lmax) & ~np.eye(x.shape[-1], dtype=bool)[None]
    return np.where(ok, y, x)


COLUMN32_ROWS = [r for r in H.ROWS if r.path == "fast64" and r.L == 2000.0 and r.N == 64 and (r.K, r.rb) in ((20, 500.0), (7, 250.0), (64, 500.0))]


@pytest.mark.parametrize("margin", [None, "0", "1024", "16384"])
@pytest.mark.parametrize("r", COLUMN32_ROWS, ids=H.row_id)
def test_column32_on_bin_edges_against_the_general_kernel(r, margin, monkeypatch):
    if margin is None:
        monkeypatch.delenv("DIRAL_F32_MARGIN", raising=False)
    else:
        monkeypatch.setenv("DIRAL_F32_MARGIN", margin)
    t, cfg = H.tables(r), H.config(r)
    for step in (0, 1, -1):
        x = t["x"] if step == 0 else _f32_step(t["x"], t["filler"], step > 0, r.L)
        for dt in (torch.float32, torch.float64):
            envs = []
            for general in (False, True):
                env = make_env(cfg, H.B, dtype=dt)
                env.reset_topology(t["px"], t["py"], t["vel"])
                env.import_state(t["px"], t["py"], t["vel"], seq=t["seq"], age=t["age"], x=x)
                env.force_general_kernel(general)
                envs.append(env)
            for _ in compare_slots(envs[0], envs[1], t["acts"], (H.row_id(r), margin, step, str(dt))):
                pass


RICH_STATE = dict(add_reward=True, add_index=True, add_velocity=True, add_position=True, add_channel_obs=True)


@pytest.mark.parametrize("A", [1, 32, 33, 64])
@pytest.mark.parametrize("K", [1, 2, 19, 20, 63, 64])
def test_lds_layout_and_histogram_zeroing_against_the_general_kernel(K, A):
    N = 64
    x0, v0, acts = p1_inputs(N, A)
    for rich in (False, True):
        cfg = bench_config(N, A, L, communication_range=RC, State=dict(num_bins=K, **(RICH_STATE if rich else {})))
        for dt in (torch.float32, torch.float64):
            fast, gen = twins(cfg, STEP_MY_STEP, dt, x0, v0)
            for _ in compare_slots(fast, gen, acts[:2], (K, A, rich, str(dt))):
                pass


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_three_slots_in_one_launch_against_the_general_kernel(dt):
    N, A, K = 64, 32, 20
    x0, v0, acts = p1_inputs(N, A)
    cfg = bench_config(N, A, L, communication_range=RC, State=dict(num_bins=K))
    fast, gen = twins(cfg, STEP_MY_STEP, dt, x0, v0)
    t0 = 0
    for rep in range(2):                                     # (the second launch zeroes what the first left)
        seq = torch.stack([dev(a) for a in acts])
        out = fast.rollout(seq, t0, states="all")
        torch.cuda.synchronize()
        lk = fast.last_kernel()
        assert (lk & 15) == KERNEL_FAST64 and (lk & KERNEL_POLICY), lk
        for k, a in enumerate(acts):
            want = slot(gen, a, t0 + k)
            ran_on(gen, KERNEL_GENERAL)
            same(out["states"][k].cpu().numpy(), want["state"], (rep, k, "state"))
        same(out["reward"].cpu().numpy(), want["reward"], (rep, "reward"))
        t0 += len(acts)
    ef, eg = everything(fast, t0 - 1), everything(gen, t0 - 1)
    for key in eg:
        if key != "metrics":
            same(ef[key], eg[key], ("behind", key), equal_nan=True)
    fast.check()
    gen.check()
