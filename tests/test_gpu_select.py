"""`diral_policy_select` / `QPolicy` on the device against the host statement of tests/select_cases.py (which
tests/test_select_cases.py holds against the reference's recorded actions).

GREEDY, EPS_GREEDY and the explore / exploit decision of BOLTZMANN are compared bit for bit.  SOFTMAX and the exploiting
BOLTZMANN rows go through exp(), where the device's libm and NumPy's may differ by ulps: rows on which that could change
the answer (select_cases.margin) are left out of the comparison - the CPU test shows there are none in these cases - and
rows that are exact by construction (all-equal rows with draws on the cdf's entries, rows of {0, -inf}) are compared
in full."""
import ctypes

import numpy as np
import pytest
import torch

from diral_amd.config import STEP_MY_STEP, bench_config
from diral_amd.driver import DriverLoop
from diral_amd.qpolicy import QPolicy
from diral_amd.rollout import SlotClock, no_finalizers_during_capture
from tests import select_cases as H
from tests.gpu_util import make_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def tensor(store, dtype, B, N):
    """The case's storage as the [B, N, A] tensor of `dtype` (bf16: the recorded bit patterns)."""
    t = torch.from_numpy(np.ascontiguousarray(store.view(np.int16) if dtype == "bf16" else store)).to(DEV)
    if dtype == "bf16":
        t = t.view(torch.bfloat16)
    return t.reshape(B, N, -1).contiguous()


def host(t):
    return t.cpu().numpy().reshape(-1)


def policy(B, N, A, kind, **kw):
    return QPolicy(B, N, A, kind, seed=kw.pop("seed", H.POLICY_SEED), device=DEV, **kw)


# ---- every kind on random rows: shapes, dtypes, the device generator ----
@pytest.mark.parametrize("i,dtype", H.GPU_CASES, ids=["%dx%dx%d-%s" % (H.SHAPES[i] + (d,)) for i, d in H.GPU_CASES])
def test_kinds_equal_the_host_statement(i, dtype):
    B, N, A, store, exact = H.random_case(i, dtype)
    q = tensor(store, dtype, B, N)
    assert q.dtype == TORCH[dtype] and np.array_equal(q.double().cpu().numpy().reshape(-1, A), exact)   # the exact f64 values
    u, a = H.case_draws(i)                                          # the generator, restated on the host
    flags = torch.zeros((B, N), dtype=torch.uint8, device=DEV)

    assert np.array_equal(host(policy(B, N, A, "greedy").act(q)), H.greedy(exact))

    pol = policy(B, N, A, "eps_greedy", eps_init=0.4)
    want, wexp = H.eps_greedy(exact, 0.4, u, a)
    assert np.array_equal(host(pol.act(q, explored=flags)), want) and np.array_equal(host(flags) != 0, wexp)
    assert pol.get_epsilon() == 0.4 and (A == 1 or 0 < wexp.sum() < B * N or B * N < 8)

    bz = H.BOLTZ
    pol = policy(B, N, A, "boltzmann", beta=bz["beta"], alpha=bz["alpha"], explore_start=bz["explore_p"],
                 explore_stop=bz["explore_p"])
    want, wexp = H.boltzmann(exact, bz["beta"], bz["alpha"], bz["explore_p"], u, a)
    got = host(pol.act(q, time_slot=1, explored=flags))             # (slot 1: beta stays)
    assert pol.beta == bz["beta"] and pol.explore_p == bz["explore_p"]
    assert np.array_equal(host(flags) != 0, wexp)                   # the decision: bit for bit
    keep = wexp | ~H.boltzmann_ambiguous(exact, bz["beta"], bz["alpha"])
    assert np.array_equal(got[keep], want[keep]) and keep.mean() > 0.99

    pol = policy(B, N, A, "softmax", temperature=H.SOFTMAX_TMP)
    want, bad = H.softmax(exact, H.SOFTMAX_TMP, u)
    got = host(pol.act(q))
    keep = ~H.softmax_ambiguous(exact, H.SOFTMAX_TMP, u)
    assert np.array_equal(got[keep], want[keep]) and keep.mean() > 0.99
    assert int(pol.bad_rows.item()) == int(bad.sum()) == 0 and pol.get_epsilon() == H.SOFTMAX_TMP


# ---- hand-made rows of the arg-max ----
@pytest.mark.parametrize("A", [1, 2, 3, 5, 31, 32, 33, 64, 65, 100, 256, 300, 4096])
def test_argmax_rules_on_hand_made_rows(A):
    rows = H.special_rows(A)
    for dtype in H.DTYPES:
        store, exact = H.quantize(rows, dtype)
        R = len(rows)
        got = host(policy(1, R, A, "greedy").act(tensor(store, dtype, 1, R)))
        want = H.greedy(exact)
        assert np.array_equal(got, want), (dtype, np.argwhere(got != want)[:5].ravel(), got[got != want][:5], want[got != want][:5])
    # the rows do hold what they are for
    assert np.isnan(rows).any() and (rows == np.inf).any() and np.signbit(rows[rows == 0]).any()
    assert A == 1 or (H.greedy(rows) != H.wrong_greedy_last_tie(rows)).any()
    assert A == 1 or (H.greedy(rows) != H.wrong_greedy_nan_ignored(rows)).any()


def test_eps_greedy_draw_corners():
    """draw_u == eps exactly explores (the test is a strict >), eps 0 and 1, draw_a far above A."""
    B, N, A = 3, 64, 5
    rng = np.random.default_rng(77)
    Q = rng.standard_normal((B * N, A))
    q = tensor(Q, "f64", B, N)
    u = rng.random(B * N)
    u[::4] = 0.25
    u[1::8] = np.nextafter(0.25, 1.0)
    u[2::8] = np.nextafter(0.25, 0.0)
    u[3::16] = 0.0
    a = rng.integers(0, 2 ** 31 - 1, B * N).astype(np.int32)
    a[::5] = 2 ** 31 - 1
    flags = torch.zeros((B, N), dtype=torch.uint8, device=DEV)
    for eps in (0.0, 0.25, 1.0):
        pol = policy(B, N, A, "eps_greedy", eps_init=eps)
        got = host(pol.act(q, draw_u=u, draw_a=a, explored=flags))
        want, wexp = H.eps_greedy(Q, eps, u, a.astype(np.int64))
        assert np.array_equal(got, want) and np.array_equal(host(flags) != 0, wexp), eps
        assert (got != H.wrong_eps_greedy_ge(Q, eps, u, a.astype(np.int64))).any() == (eps in (0.0, 0.25))
    assert wexp.all()                                               # eps = 1: every agent explores


def test_device_draws_equal_the_generator_bit_for_bit():
    """draw_a through an always-exploring launch; draw_u through per-env eps values: with eps = u the env explores, with
    eps = the double below u it does not - true of no other u."""
    B, A, off = 200, 7, 11
    Q = np.tile(np.arange(A, dtype=np.float64), (B, 1))              # greedy answers A - 1
    q = tensor(Q, "f64", B, 1)
    clk = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    u, a = H.device_draws(H.policy_seed(H.POLICY_SEED, 3 + 5), B, A, idx0=off)
    pol = QPolicy(B, 1, A, "eps_greedy", seed=H.POLICY_SEED, env_offset=off, device=DEV)
    flags = torch.zeros((B, 1), dtype=torch.uint8, device=DEV)
    got = host(pol.act_clocked(q, clk, offset=3, param=torch.as_tensor(u, device=DEV), explored=flags))
    assert np.array_equal(got, a) and host(flags).all()
    below = torch.as_tensor(np.nextafter(u, -1.0), device=DEV)
    got = host(pol.act_clocked(q, clk, offset=3, param=below, explored=flags))
    assert np.array_equal(got, np.full(B, A - 1)) and not host(flags).any()
    # the call `act` number k draws what the clocked form draws at offset + clock = k
    p2 = QPolicy(B, 1, A, "eps_greedy", seed=H.POLICY_SEED, env_offset=off, device=DEV, eps_init=1.0)
    for _ in range(7):
        p2.act(q)
    assert np.array_equal(host(p2.act(q)), a) and p2._t == 8


# ---- SOFTMAX rows that are exact by construction, and the rows the reference raises on ----
@pytest.mark.parametrize("A", [4, 32, 64, 128, 1024])
def test_softmax_all_equal_rows_with_draws_on_the_cdf(A):
    # p = 1 / A exactly, cdf[j] = (j + 1) / A exactly: u = j / A answers j (side="right"), the double below it j - 1
    for dtype in ("f64", "bf16"):
        store, exact = H.quantize(np.full((2 * A, A), 1.5), dtype)
        u = np.concatenate((np.arange(A) / A, np.nextafter(np.arange(A) / A, -1.0)))
        pol = policy(2, A, A, "softmax", temperature=0.25)
        got = host(pol.act(tensor(store, dtype, 2, A), draw_u=u))
        assert np.array_equal(got, np.concatenate((np.arange(A), np.maximum(np.arange(A) - 1, 0))))
        assert np.array_equal(got, H.softmax(exact, 0.25, u)[0])
        assert (got != H.wrong_softmax(exact, 0.25, u, "left")).any()
    # u = 1.0 (outside [0, 1), injected): clamped to A - 1
    assert host(pol.act(tensor(store, dtype, 2, A), draw_u=np.ones(2 * A))).tolist() == [A - 1] * (2 * A)


@pytest.mark.parametrize("A", [3, 5, 32, 33, 64, 100, 300])
def test_softmax_rows_of_zero_and_minus_inf_and_bad_rows(A):
    rng = np.random.default_rng(A)
    R = 96
    Q = np.where(rng.random((R, A)) < 0.5, 0.0, -np.inf)            # exp gives exactly 1 and 0
    Q[:, 0][np.all(Q == -np.inf, axis=1)] = 0.0
    cdfs = [H.softmax_cdf(r, 0.7)[0] for r in Q]
    u = rng.random(R)
    for r in range(0, R, 2):                                        # every other draw ON an entry of the row's cdf
        u[r] = min(cdfs[r][rng.integers(A)], np.nextafter(1.0, 0.0))
    # rows np.random.choice raises on: a NaN, a +inf, nothing but -inf, a quotient that overflows
    bad_rows = np.zeros((6, A))
    bad_rows[0, A // 2] = np.nan
    bad_rows[1, A - 1] = np.inf
    bad_rows[2, :] = -np.inf
    bad_rows[3, :] = np.nan
    bad_rows[4, 0] = np.nan; bad_rows[4, A - 1] = np.inf
    bad_rows[5, A // 2] = 1.7e308                                   # / 0.7 overflows
    Q = np.concatenate((Q, bad_rows))
    u = np.concatenate((u, rng.random(6)))
    want, bad = H.softmax(Q, 0.7, u)
    assert bad.sum() == 6 and list(want[-6:-1]) == [A // 2, A - 1, 0, 0, 0]
    pol = policy(1, R + 6, A, "softmax", temperature=0.7)
    assert np.array_equal(host(pol.act(tensor(Q, "f64", 1, R + 6), draw_u=u)), want)
    assert int(pol.bad_rows.item()) == 6
    pol.act(tensor(Q, "f64", 1, R + 6), draw_u=u)
    assert int(pol.bad_rows.item()) == 12                           # the counter is added to


def test_boltzmann_overflow_answers_the_first_nan():
    for A in (5, 32, 100):
        Q = np.zeros((4, A))
        Q[0, [A - 2, 1]] = 800.0                                    # exp overflows twice: inf / inf at 1 and A - 2
        Q[1, A - 1] = 800.0
        Q[2] = -800.0                                               # every exp is 0: 0 / 0 everywhere
        Q[3, 2] = 3.0
        want, _ = H.boltzmann(Q, 1.0, 0.25, 0.0, np.full(4, 0.5), np.zeros(4, np.int64))
        assert list(want) == [1, A - 1, 0, 2]
        pol = policy(1, 4, A, "boltzmann", beta=1.0, alpha=0.25, explore_start=0.0, explore_stop=0.0)
        assert np.array_equal(host(pol.act(tensor(Q, "f64", 1, 4), time_slot=3)), want)


def test_schedules_follow_the_reference():
    B, N, A = 2, 4, 3
    q = torch.zeros((B, N, A), dtype=torch.float32, device=DEV)
    pol = policy(B, N, A, "eps_greedy", eps_init=0.5, eps_decay=0.5)
    for episode, eps in ((0, 0.5), (1, 0.25), (1, 0.25), (5, 0.125), (3, 0.125), (6, 0.0625)):   # policies.py:46-48
        pol.act(q, episode=episode)
        assert pol.get_epsilon() == eps
    pol.set_epsilon(0.0015)
    pol.act(q, episode=7)
    assert pol.get_epsilon() == 0.001 and pol._t == 7               # the floor of policies.py:62-63
    pol = policy(B, N, A, "softmax", temperature=0.05, episodes=9)
    want = np.concatenate((np.geomspace(1.0, 0.05, 6), np.repeat(0.05, 3)))
    for episode in (0, 3, 8, 9, 1000, -1):
        pol.act(q, episode=episode)
        assert pol.get_epsilon() == (want[episode] if episode < 9 else 0.05)
    pol = policy(B, N, A, "boltzmann")
    for t, beta in ((0, 0.999), (1, 0.999), (50, 0.998), (5000, 0.998)):                          # policies.py:153-159
        pol.act(q, time_slot=t)
        assert pol.beta == pytest.approx(beta, abs=1e-12) and pol.explore_p == 0.01 + (0.02 - 0.01) * np.exp(-0.0001 * t)
    with pytest.raises(ValueError):
        pol.act(q)
    with pytest.raises(ValueError):
        pol.act(q[:1], time_slot=0)
    assert pol._t == 4                                              # refused calls drew nothing


# ---- the reference's recorded actions, replayed on the device under the recorded draws ----
@pytest.mark.parametrize("A", [3, 32])
def test_reference_fixtures_replay_on_the_device(A):
    g = H.load_fixture("q1_greedy")[A]
    R = len(g["Qs"])
    assert np.array_equal(host(policy(R, 1, A, "greedy").act(tensor(g["Qs"], "f64", R, 1))), g["actions"])
    for name, kind in (("q2_eps_greedy", "eps_greedy"), ("q3_softmax", "softmax")):
        g = H.load_fixture(name)[A]
        R = len(g["Qs"])
        pol = policy(R, 1, A, kind)                                 # one env per recorded call: its parameter per env
        got = host(pol._launch(name, tensor(g["Qs"], "f64", R, 1), None, None, draw_u=g["draw_u"], draw_a=g["draw_a"],
                               param=torch.as_tensor(g["param"], device=DEV)))
        keep = ~H.softmax_ambiguous(g["Qs"], g["param"], g["draw_u"]) if kind == "softmax" else np.ones(R, bool)
        assert keep.all() and np.array_equal(got, g["actions"]), name
    g = H.load_fixture("q4_boltzmann")[A]
    got = np.full(len(g["Qs"]), -1)
    for beta, alpha in sorted(set(zip(g["beta"], g["alpha"]))):     # beta and alpha go by value: one launch per pair
        rows = np.flatnonzero((g["beta"] == beta) & (g["alpha"] == alpha))
        pol = policy(len(rows), 1, A, "boltzmann", beta=beta, alpha=alpha)
        got[rows] = host(pol._launch("q4", tensor(g["Qs"][rows], "f64", len(rows), 1), None, None, draw_u=g["draw_u"][rows],
                                     draw_a=g["draw_a"][rows], param=torch.as_tensor(g["param"][rows], device=DEV)))
    assert np.array_equal(got, g["actions"])


# ---- composition ----
@pytest.mark.parametrize("kind", ["eps_greedy", "softmax", "boltzmann"])
def test_shards_draw_what_the_whole_batch_draws(kind):
    B, N, A = 6, 9, 7
    q = torch.randn((B, N, A), dtype=torch.float32, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    kw = dict(seed=91, eps_init=0.5, explore_start=0.5, explore_stop=0.5)
    whole = policy(B, N, A, kind, **kw)
    parts = [QPolicy(3, N, A, kind, device=DEV, env_offset=off, **kw) for off in (0, 3)]
    for call in range(2):
        want = whole.act(q, time_slot=1)
        got = torch.cat([p.act(q[3 * k:3 * k + 3].contiguous(), time_slot=1) for k, p in enumerate(parts)])
        assert torch.equal(got, want)
        if call:
            assert not torch.equal(want, prev)                      # the draw counter moved on
        prev = want.clone()


@pytest.mark.parametrize("kind", ["eps_greedy", "softmax", "boltzmann"])
def test_parameter_per_env_equals_one_env_calls(kind):
    B, N, A = 5, 9, 33
    q = torch.randn((B, N, A), dtype=torch.float32, device=DEV, generator=torch.Generator(DEV).manual_seed(4))
    par = torch.tensor([0.0, 0.3, 0.6, 0.9, 1.0], dtype=torch.float64, device=DEV) + (0.05 if kind == "softmax" else 0.0)
    clk = SlotClock(DEV, 12)
    flags = torch.zeros((B, N), dtype=torch.uint8, device=DEV)
    got = policy(B, N, A, kind).act_clocked(q, clk, offset=2, param=par, explored=flags)
    for b in range(B):
        one = QPolicy(1, N, A, kind, seed=H.POLICY_SEED, env_offset=b, device=DEV)
        assert torch.equal(one.act_clocked(q[b:b + 1].contiguous(), clk, offset=2, param=par[b:b + 1].clone()), got[b:b + 1]), b
    if kind != "softmax":
        share = flags.double().mean(dim=1).cpu().numpy()
        assert share[0] == 0 and share[4] == 1 and 0 < share[2] < 1   # explore_p / eps 0 never explores, 1 always
    assert not torch.equal(got[1], got[3])
    # one value for every env
    one_val = policy(B, N, A, kind).act_clocked(q, clk, offset=2, param=par[2:3].clone())
    assert torch.equal(one_val[2], got[2])


def test_captured_act_and_step_replay_with_the_clock_and_the_parameter():
    """A graph [act_clocked, env step, clock + 1]: every replay draws afresh, follows a rewritten per-env eps, and equals
    the eager calls at that clock."""
    cfg = bench_config(4, 3, 300.0, communication_range=120.0, State=dict(num_bins=20))
    B, N, A = 8, 4, 3
    env, twin = make_env(cfg, B), make_env(cfg, B)
    for e in (env, twin):
        e.reset_topology(seed=5)
    q = torch.randn((B, N, A), dtype=torch.float32, device=DEV, generator=torch.Generator(DEV).manual_seed(8))
    par = torch.full((B,), 0.5, dtype=torch.float64, device=DEV)
    acts = torch.zeros((B, N), dtype=torch.int32, device=DEV)
    flags = torch.zeros((B, N), dtype=torch.uint8, device=DEV)
    pol, pol_e = policy(B, N, A, "eps_greedy"), policy(B, N, A, "eps_greedy")
    clk = SlotClock(DEV, 0)
    env.set_clock(clk.t)

    def slot():
        pol.act_clocked(q, clk, param=par, out=acts, explored=flags)
        env._step(STEP_MY_STEP, acts, 0)                            # slot number = clock, on the device
        env._ok(env.lib.diral_clock_add(ctypes.c_void_p(clk.ptr()), 1, env._stream()), "diral_clock_add")

    def eager(c):
        a = pol_e.act_clocked(q, torch.full((1,), c, dtype=torch.int64, device=DEV), param=par.clone())
        obs, rew, _ = twin._step(STEP_MY_STEP, a, c)
        return a.clone(), obs.clone(), rew.clone()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        slot()                                                      # eager first (slot 0): buffers and kernel path settle
    torch.cuda.synchronize()
    want = eager(0)
    assert torch.equal(acts, want[0]) and torch.equal(env._rew, want[2])
    g = torch.cuda.CUDAGraph()
    with no_finalizers_during_capture():
        with torch.cuda.graph(g, stream=s):
            slot()
    prev = acts.clone()
    for c in (1, 2, 3):
        if c == 3:
            par.fill_(1.0)                                          # a torch op writes the schedule: everyone explores
        g.replay()
        torch.cuda.synchronize()
        want = eager(c)
        assert torch.equal(acts, want[0]), c
        assert torch.equal(env._obs, want[1]) and torch.equal(env._rew, want[2]), c
        assert not torch.equal(acts, prev), c
        assert bool(flags.all()) == (c == 3)
        prev = acts.clone()
    assert clk.value() == 4
    env.set_clock(None)
    env.check(); twin.check()


def test_driver_loop_act_walks_the_three_phases():
    cfg = bench_config(4, 3, 300.0, communication_range=120.0, State=dict(num_bins=20))
    B, N, A = 5, 4, 3
    env = make_env(cfg, B)
    env.reset_topology(seed=1)
    loop = DriverLoop(env)
    q = torch.randn((B, N, A), dtype=torch.float64, device=DEV, generator=torch.Generator(DEV).manual_seed(6))
    pol, ref = policy(B, N, A, "eps_greedy", eps_init=0.5, eps_decay=0.5), policy(B, N, A, "eps_greedy", eps_init=0.5, eps_decay=0.5)
    greedy = torch.as_tensor(H.greedy(q.cpu().numpy().reshape(-1, A)).reshape(B, N), dtype=torch.int32, device=DEV)
    for t in range(9):                                              # main_test.py:129-136 with explore_step 3, greedy_step 6
        torch.manual_seed(100 + t)
        got = loop.act(q, t, episode=t // 2, policy=pol, explore_step=3, greedy_step=6)
        assert got.dtype == torch.int32 and tuple(got.shape) == (B, N)
        if t < 3:
            torch.manual_seed(100 + t)
            assert torch.equal(got, env.sample()) and pol._t == 0
        elif t < 6:
            assert torch.equal(got, ref.act(q, episode=t // 2)) and pol._t == t - 2
            assert pol.get_epsilon() == ref.get_epsilon()
        else:
            assert torch.equal(got, greedy) and pol._t == 3
    assert pol.get_epsilon() == 0.125
