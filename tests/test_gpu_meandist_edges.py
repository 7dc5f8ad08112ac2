"""The mean pair distance of colliding transmitters at its threshold, and `my_step_design`'s 2 Rc count, on every copy of
the loop (inputs and the plain host statement: tests/meandist_cases.py; tests/test_meandist_cases.py shows without a GPU
that every env sits where it claims and that eleven wrong restatements are each told apart):

* `fast_collision_reward` - step_fast64 plain and RICH at 64 and 33 vehicles, on the lane and off it, and its K-slot
  loop through a two-slot `rollout` and through `step_policy(slots=2)` with agents that keep their action;
* `wide_collision_reward` - step_wide at 128 and 256 vehicles in both table forms, plain and RICH, and
  `step_wide_slots_kernel` through a two-slot rollout;
  The prefill launch, which states the 2 Rc count a second time, is held to the per-env reward sums of its metrics;
* `reward_weight` + `weight_from_mean` - the general kernel, forced at 64 and reached by vehicles off the lane at 128;
* `large_reward_weight` - the large path, forced at 64 and natural at 300.

Every float64 reward equals the host statement bit for bit (reward designs 1, 2, 5 of `my_step`, and `my_step_design`),
every float32 reward is the float32 cast of the same path's float64 one, `last_kernel()` and `check()` in every case.
A K-slot launch is held to the statement in its first slot and to the oracle's second step in its second: positions with
a fraction move under the wrap's rounding even at velocity 0, so the second slot need not repeat the first.  Off-lane
envs run where the path takes them (not the slot loops, not step_wide)."""
import numpy as np
import pytest
import torch

from diral_amd.config import (KERNEL_CH, KERNEL_FAST64, KERNEL_GENERAL, KERNEL_LARGE, KERNEL_PACKED, KERNEL_POLICY, KERNEL_RICH,
                              KERNEL_WIDE, STEP_DESIGN)
from tests import meandist_cases as C
from tests.gpu_util import make_env

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLAG = dict(rich=KERNEL_RICH, ch=KERNEL_CH, packed=KERNEL_PACKED, policy=KERNEL_POLICY)
FAMILY = {"fast64": KERNEL_FAST64, "rollout": KERNEL_FAST64, "slots": KERNEL_FAST64, "wide": KERNEL_WIDE,
          "general": KERNEL_GENERAL, "offlane": KERNEL_GENERAL, "large": KERNEL_LARGE}
# (path, vehicles, table form).  `offlane`: the general kernel, taken because vehicles stand off the lane
PATHS = [("fast64", 64, None), ("fast64", 33, None), ("rollout", 64, None), ("rollout", 33, None), ("slots", 64, None),
         ("slots", 33, None), ("wide", 128, "plane"), ("wide", 128, "packed"), ("wide", 256, "plane"), ("wide", 256, "packed"),
         ("general", 64, None), ("offlane", 128, None), ("large", 64, None), ("large", 300, None)]
TAKES_OFFLANE = ("fast64", "general", "offlane", "large")


def path_id(p):
    return "%s-N%d%s" % (p[0], p[1], "-" + p[2] if p[2] else "")


def _np(t):
    return t.detach().cpu().numpy().copy()


def ran(env, family, **flags):
    lk = env.last_kernel()
    assert (lk & 15) == family, (lk, family)
    for name, want in flags.items():
        assert bool(lk & FLAG[name]) == want, (name, want, lk)


def handle(path, N, key, design, mode, dt):
    g = C.groups(N)[key]
    env = make_env(C.config(N, key, design), len(g["envs"]), mode=mode, dtype=dt)
    env.reset_topology(g["x"], g["y"] if key[2] else None, 0.0)
    if path == "general":
        env.force_general_kernel()
    if path == "large" and N <= 256:
        env.force_large_path()
    return env, torch.as_tensor(g["acts"], device=DEV)


def runs_of(path, N, form, key, design, mode, dt):
    """[(tag, first slot's rewards [B][N], second slot's or None)] of a path in one output type, the kernel asserted."""
    from diral_amd.sps import SpsPolicy
    fam = FAMILY[path]
    out = []

    def stepped(rich):
        env, a = handle(path, N, key, design, mode, dt)
        if rich:
            env._step(mode, a, 0, want_chobs=True)
        else:
            env.step(a, 0)
        torch.cuda.synchronize()
        if path in ("fast64", "wide"):
            ran(env, fam, rich=rich, ch=False, policy=False)
            if path == "wide":
                ran(env, fam, packed=form == "packed")
        else:
            ran(env, fam)
        env.check()
        out.append(("rich" if rich else "plain", _np(env._rew), None))
    if path in ("fast64", "wide", "general", "offlane", "large"):
        stepped(False)
        if path in ("fast64", "wide"):
            stepped(True)
    if mode == STEP_DESIGN or key[2]:                              # the slot loops: my_step, everybody on the lane
        return out
    if path in ("rollout", "wide"):
        env, a = handle(path, N, key, design, mode, dt)
        res = env.rollout(torch.stack([a, a]), 0, mode="my_step", states="all" if N <= 64 else "last")
        torch.cuda.synchronize()
        ran(env, fam, policy=True, ch=False)
        first, second = _np(res["shaped"][0]), _np(res["shaped"][1])
        assert second.tobytes() == _np(res["reward"]).tobytes()
        env.check()
        out.append(("rollout", first, second))
    if path == "slots":
        env, a = handle(path, N, key, design, mode, dt)
        B = a.shape[0]
        pol = SpsPolicy(B, N, C.A, device=DEV, seed=1)
        pol.keep_prob = 1.0                                       # nobody re-selects: both slots run the given actions
        pol.prev_action.copy_(a)
        nxt = torch.empty_like(a)
        sh = torch.zeros((2, B, N), dtype=dt, device=DEV)
        env.step_policy(a, 0, pol, nxt, shaped_out=sh, global_reward_avg=False, slots=2, mode=mode)
        torch.cuda.synchronize()
        ran(env, fam, policy=True, ch=False)
        assert torch.equal(nxt, a)
        assert _np(sh[1]).tobytes() == _np(env._rew).tobytes()
        env.check()
        out.append(("slots", _np(sh[0]), _np(sh[1])))
    return out


def where(N, key, got, want):
    """The envs that differ, by family / case / role - what a failure should name."""
    envs = C.groups(N)[key]["envs"]
    bad = sorted(set(np.argwhere(got != want)[:, 0].tolist()))
    return len(bad), [(envs[i]["family"], envs[i]["case"], envs[i]["role"]) for i in bad[:6]]


# (the slot loops run my_step: no my_step_design case for them)
CASES = [(p, d, m) for p in PATHS for d, m in C.MODES if not (m == STEP_DESIGN and p[0] in ("rollout", "slots"))]


def case_id(c):
    return "%s-%s" % (path_id(c[0]), "my_step_design" if c[2] == STEP_DESIGN else "design%d" % c[1])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_rewards_at_the_mean_distance_threshold_equal_the_host_statement(case, monkeypatch):
    p, design, mode = case
    path, N, form = p
    if form:
        monkeypatch.setenv("DIRAL_TABLE_FORM", form)             # read when the handle is made
    done, bad = 0, []                                              # every group runs: a failure names all it touches
    for key in C.groups(N):
        if key[2] != (path == "offlane") and not (key[2] and path in TAKES_OFFLANE):
            continue
        want = C.host(N, key, design, mode)
        r64 = runs_of(path, N, form, key, design, mode, torch.float64)
        r32 = runs_of(path, N, form, key, design, mode, torch.float32)
        assert [r[0] for r in r64] == [r[0] for r in r32] and len(r64) > 0
        for (tag, first, second), (_, first32, second32) in zip(r64, r32):
            tag = (path_id(p), key, tag)
            assert first.dtype == np.float64 and first32.dtype == np.float32, tag
            if not C.same_bits(first, want):
                bad.append((tag, where(N, key, first, want)))
            if not np.array_equal(first32.view(np.int32), first.astype(np.float32).view(np.int32)):
                bad.append((tag, "float32 is not the cast"))
            if second is not None:
                nxt = C.oracle_steps(N, key, design, mode)[1]
                if not C.same_bits(second, nxt):
                    bad.append((tag, "second slot", where(N, key, second, nxt)))
                if not np.array_equal(second32.view(np.int32), second.astype(np.float32).view(np.int32)):
                    bad.append((tag, "second slot", "float32 is not the cast"))
            done += 1
    assert done > 0
    assert not bad, bad


@pytest.mark.parametrize("N", (64, 33))
def test_prefill_slot_counts_the_transmitters_inside_twice_the_range(N):
    """The second statement of the count in step_fast64 (the K-slot prefill computes `my_step_design`'s reward in P2).  The
    launch hands no rewards back: their per-env sum in the metrics - integers, exact in any order - is compared."""
    from diral_amd.config import M_SUM_REWARD, M_TX_COLLIDED, M_TX_SOLE
    done = 0
    for key, g in C.groups(N).items():
        if key[2]:
            continue
        want = C.host(N, key, 1, STEP_DESIGN)
        for dt in (torch.float64, torch.float32):
            env, a = handle("prefill", N, key, 1, STEP_DESIGN, dt)
            env.prefill(a, 1, 7, rew_in=np.zeros(want.shape))
            torch.cuda.synchronize()
            ran(env, KERNEL_FAST64, policy=True, ch=False)
            env.check()
            m = _np(env.metrics())
            assert np.array_equal(m[:, M_SUM_REWARD], want.sum(axis=1)), (N, key, where(N, key, m[:, [M_SUM_REWARD]], want.sum(axis=1, keepdims=True)))
            sole = np.array([sum(len(ids) == 1 for ids in C.transmitters(e).values()) for e in g["envs"]], dtype=np.float64)
            assert np.array_equal(m[:, M_TX_SOLE], sole) and np.array_equal(m[:, M_TX_COLLIDED], N - sole)
            done += 1
    assert done == 10
