"""What passes through the device's math library, swept completely against correctly rounded values (tests/libm_cases.py;
tests/test_libm_cases.py shows without a GPU that the inputs hold what they are for):

* exp(): the rewards of `my_step_ch` designs 3 / 4 over every reception ratio R = received / in_range a size can produce
  (design 2 pins the division bit for bit), and `my_step` design 3 over every collision count - on step_fast64 plain and
  RICH, its K-slot form (an open-loop rollout of two slots and `step_policy(slots=2)`), step_wide in both table forms at
  128 and 256 vehicles, the general kernel and the large path, both output types.  Every float64 reward against the
  chain R = k / n, a = 1.0 - R, E = RN(exp(a)), 1.0 - E or -E within `libm_cases.exp_ulp_bound` (the oracle's measured
  error of 1 ulp of E plus one, half an ulp more where 1 - E rounds again, never beyond the exp() bar); every float32 reward
  is the float32 cast of the same path's float64 one; the PRR count exact, the PRR sum within the bound of a sum in any
  order; and ONE device value per (design, argument) over every path, size, table form and slot;
* log10(): `window_from_chobs` on rows built by hand against -40.0 - 30.0 * RN(log10(max(d, 1))) within
  `libm_cases.window_bound`, exactly -40 ... -160 at the powers of ten and below the 1 m clamp, monotone over runs of
  adjacent distances; and the SPS decisions of `step_from_chobs`, `step` and the fused / K-slot launches against
  tests/host_closed_loop.choose_new_resource run on the DEVICE's own window - every env compared, none left out.

Measured on an MI355X (gfx950, ROCm's device library), the argument sets being `libm_cases.exp_arguments()` (3031 values
of 1 - k / n and 1 - 1 / c in [0, 1]) and `libm_cases.window_rows()` (9792 distances per input type):
* exp(): of the 3031 device values E (read back exactly from the design-4 rewards -E / +E and from `my_step` design 3) 2857
  are correctly rounded, 174 are 1 ulp off and none is 2 (histogram {0: 2857, 1: 174}; the worst, 1.00 ulp, first at
  a = 0.0535714285714286); the bound allows 2.  The exp(1.0) the compiler folded for the sole transmitter, the run-time
  one at R == 0 and the correctly rounded value are the same double, 2.718281828459045.  One value per (design, argument)
  on every path: 2986 ratio arguments per `my_step_ch` design, 300 collision counts;
* log10(): every window value is within 1 ulp OF THE WINDOW VALUE of -40.0 - 30.0 * RN(log10 d) - 13 of the 9782 heard
  float64 distances and 8 of the float32 ones differ from it at all, the worst at 0.52 (d = 1523) and 0.68 (d =
  9.99997138977) of the bound -, the powers of ten read exactly -40 ... -160, and no run of adjacent distances rises."""
import collections

import numpy as np
import pytest
import torch

from diral_amd.config import (KERNEL_CH, KERNEL_FAST64, KERNEL_GENERAL, KERNEL_LARGE, KERNEL_PACKED, KERNEL_POLICY, KERNEL_RICH,
                              KERNEL_WIDE, STEP_DESIGN, STEP_MY_STEP, STEP_MY_STEP_CH, bench_config)
from tests import libm_cases as C
from tests.gpu_util import make_env
from tests.oracle_compare import exp_close

ORACLE_EXP_ULPS, HOST_LOG10_ULPS = C.ORACLE_EXP_ULPS, C.HOST_LOG10_ULPS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTS = (torch.float64, torch.float32)
FLAG = dict(rich=KERNEL_RICH, ch=KERNEL_CH, packed=KERNEL_PACKED, policy=KERNEL_POLICY)
SEEN = {}                       # kind -> {bits of the argument: {bits of the float64 reward}}, over every path
EXP_ERR = {}                    # bits of the argument of exp() -> the worst error of a device E, in ulps of RN(E)


def _np(t):
    return t.detach().cpu().numpy().copy()


def ran(env, family, **flags):
    lk = env.last_kernel()
    assert (lk & 15) == family, (lk, family)
    for name, want in flags.items():
        assert bool(lk & FLAG[name]) == want, (name, want, lk)


def note(kind, arg_bits, rew):
    tab = SEEN.setdefault(kind, {})
    pairs = np.unique(np.stack([np.asarray(arg_bits).ravel(), C.bits(rew).ravel()], axis=1), axis=0)
    for a, r in pairs.tolist():
        tab.setdefault(a, set()).add(r)


def note_exp(arg, E_dev, E_ref):
    err = np.abs(E_dev - E_ref) / np.spacing(E_ref)
    for a, e in np.unique(np.stack([C.bits(arg).ravel(), C.bits(err).ravel()], axis=1), axis=0).tolist():
        e = float(np.int64(e).view(np.float64))
        EXP_ERR[a] = max(EXP_ERR.get(a, 0.0), e)


def f32_is_the_cast(r32, r64, tag):
    assert r32.dtype == np.float32 and r64.dtype == np.float64, tag
    assert np.array_equal(r32.view(np.int32), r64.astype(np.float32).view(np.int32)), (tag, np.argwhere(r32 != r64.astype(np.float32))[:4])


PATHS = [("fast64", 64, None), ("fast64", 33, None), ("rollout", 64, None), ("rollout", 33, None), ("slots", 64, None),
         ("slots", 33, None), ("wide", 128, "plane"), ("wide", 128, "packed"), ("wide", 256, "plane"), ("wide", 256, "packed"),
         ("general", 64, None), ("large", 64, None), ("large", 300, None)]


def path_id(p):
    return "%s-N%d%s" % (p[0], p[1], "-" + p[2] if p[2] else "")


def handle(cfg, lay, mode, dt, path, N):
    env = make_env(cfg, len(lay["x"]), mode=mode, dtype=dt)
    env.reset_topology(lay["x"], None, 0.0)                      # a static highway
    if path == "general":
        env.force_general_kernel()
    if path == "large" and N <= 256:
        env.force_large_path()
    return env, torch.as_tensor(lay["acts"], device=DEV)


def runs_of(path, N, form, cfg, lay, mode, dt, with_slots=True):
    """Every (tag, reward [B][N], metrics [B][6], slots) the path produces in one output type, the kernel family asserted.
    fast64 / wide: the plain and the RICH instantiation; rollout: both slots of a two-slot open-loop rollout, which on a
    static highway repeat each other bit for bit; slots: the first slot of `step_policy(slots=2)` with agents that keep."""
    from diral_amd.sps import SpsPolicy
    ch = mode == STEP_MY_STEP_CH
    fam = {"fast64": KERNEL_FAST64, "rollout": KERNEL_FAST64, "slots": KERNEL_FAST64, "wide": KERNEL_WIDE,
           "general": KERNEL_GENERAL, "large": KERNEL_LARGE}[path]
    out = []

    def stepped(rich):
        env, a = handle(cfg, lay, mode, dt, path, N)
        if rich:
            env._step(mode, a, 0, want_chobs=True)
        else:
            env.step(a, 0)
        torch.cuda.synchronize()
        if path in ("fast64", "wide"):
            ran(env, fam, rich=rich, ch=ch, policy=False)
            if path == "wide":
                ran(env, fam, packed=form == "packed")
        else:
            ran(env, fam)
        env.check()
        out.append(("rich" if rich else "plain", _np(env._rew), _np(env.metrics()), 1))
    if path in ("fast64", "wide", "general", "large"):
        stepped(False)
        if path in ("fast64", "wide"):
            stepped(True)
    if mode == STEP_DESIGN or not with_slots:
        return out
    if path == "rollout" or (path == "wide" and not ch):
        env, a = handle(cfg, lay, mode, dt, path, N)
        res = env.rollout(torch.stack([a, a]), 0, mode="my_step_ch" if ch else "my_step", states="all" if N <= 64 else "last")
        torch.cuda.synchronize()
        ran(env, fam, policy=True, ch=ch)
        first, second, last = _np(res["shaped"][0]), _np(res["shaped"][1]), _np(res["reward"])
        assert first.tobytes() == second.tobytes() == last.tobytes(), (path, N, "the second slot repeats the first")
        env.check()
        out.append(("rollout", first, _np(env.metrics()), 2))
    if path == "slots" or (path == "wide" and not ch):
        env, a = handle(cfg, lay, mode, dt, path, N)
        B = len(lay["x"])
        pol = SpsPolicy(B, N, 2, device=DEV, seed=1)
        pol.keep_prob = 1.0                                       # nobody re-selects: the second slot repeats the first
        pol.prev_action.copy_(a)
        nxt = torch.empty_like(a)
        sh = torch.zeros((2, B, N), dtype=dt, device=DEV)
        env.step_policy(a, 0, pol, nxt, shaped_out=sh, global_reward_avg=False, slots=2, mode=mode)
        torch.cuda.synchronize()
        ran(env, fam, policy=True, ch=ch)
        assert torch.equal(nxt, a)
        first = _np(sh[0])
        assert first.tobytes() == _np(sh[1]).tobytes() == _np(env._rew).tobytes(), (path, N)
        env.check()
        out.append(("slots", first, _np(env.metrics()), 2))
    return out


# ---- A. reception ratios ---------------------------------------------------------------------------------------------
def ch_case(path, N, form):
    lay, mod = C.ratio_layout(N), C.ratio_model(N)
    R, coll = mod["R"], mod["coll"]
    arg = np.where(coll, C.bits(R), -1)                           # (a sole transmitter: a key of its own)
    for design in C.CH_DESIGNS:
        cfg = C.ratio_config(N, design)
        ref, bound, E = C.ch_reference(design, R, coll, m=ORACLE_EXP_ULPS)
        orc = C.ratio_oracle(N, design)
        r64 = runs_of(path, N, form, cfg, lay, STEP_MY_STEP_CH, torch.float64)
        r32 = runs_of(path, N, form, cfg, lay, STEP_MY_STEP_CH, torch.float32)
        assert [r[0] for r in r64] == [r[0] for r in r32] and len(r64) > 0
        for (tag, rew, met, slots), (_, rew32, met32, _) in zip(r64, r32):
            tag = (path_id((path, N, form)), design, tag)
            bad = C.reward_failures(design, rew, ref, bound)
            if design != 2:
                err = C.exp_errors(design, rew, ref, E)
                print(tag, "worst error %.2f ulp of E" % float(err.max()))
            assert len(bad) == 0, (tag, len(bad), bad[:4], [(rew[tuple(i)], ref[tuple(i)]) for i in bad[:4]])
            if design == 2:
                assert C.same_bits(rew, orc["rew"]), tag
            else:
                assert exp_close(rew, orc["rew"]), tag
            f32_is_the_cast(rew32, rew, tag)
            for m in (met, met32):
                assert np.array_equal(m[:, 5], np.full(len(m), float(slots * N))), tag          # DIRAL_M_PRR_CNT
                assert np.array_equal(m[:, [0, 2, 3]], slots * orc["metrics"][:, [0, 2, 3]]), tag
                assert len(C.prr_sum_failures(m[:, 4], R, slots)) == 0, tag                     # DIRAL_M_PRR_SUM
            note(("my_step_ch", design), arg, rew)
            if design == 4:
                note_exp(np.where(coll, 1.0 - R, 1.0), np.where(coll, -rew, rew), E)


@pytest.mark.parametrize("p", PATHS, ids=path_id)
def test_reception_ratio_rewards_against_correctly_rounded_exp(p, monkeypatch):
    path, N, form = p
    if form:
        monkeypatch.setenv("DIRAL_TABLE_FORM", form)             # read when the handle is made
    ch_case(path, N, form)


# ---- A. collision counts ---------------------------------------------------------------------------------------------
def count_case(path, N, form):
    lay = C.count_layout(N)
    c = lay["c"]
    ref3, bound3, E3 = C.count_reference(c, m=ORACLE_EXP_ULPS)
    for design, mode in [(d, STEP_MY_STEP) for d in C.MY_STEP_DESIGNS] + [(1, STEP_DESIGN)]:
        if mode == STEP_DESIGN and path in ("rollout", "slots"):
            continue
        cfg = C.count_config(N, design)
        orc = C.count_oracle(N, design, mode)
        r64 = runs_of(path, N, form, cfg, lay, mode, torch.float64)
        r32 = runs_of(path, N, form, cfg, lay, mode, torch.float32)
        assert [r[0] for r in r64] == [r[0] for r in r32] and len(r64) > 0
        for (tag, rew, _, _), (_, rew32, _, _) in zip(r64, r32):
            tag = (path_id((path, N, form)), design, mode, tag)
            if design == 3 and mode == STEP_MY_STEP:
                assert exp_close(rew, orc), tag
                bad = C.reward_failures(3, rew, ref3, bound3)
                assert len(bad) == 0, (tag, bad[:4], [(rew[tuple(i)], ref3[tuple(i)]) for i in bad[:4]])
                note(("my_step", 3), c, rew)
                sel = c > 1
                note_exp((1.0 - 1.0 / np.maximum(c, 1))[sel], -rew[sel], E3[sel])
            else:
                assert C.same_bits(rew, orc), (tag, np.argwhere(C.bits(rew) != C.bits(orc))[:4])
            f32_is_the_cast(rew32, rew, tag)


@pytest.mark.parametrize("p", PATHS, ids=path_id)
def test_collision_count_rewards_against_the_oracle_and_correctly_rounded_exp(p, monkeypatch):
    path, N, form = p
    if form:
        monkeypatch.setenv("DIRAL_TABLE_FORM", form)
    count_case(path, N, form)


def test_one_device_value_per_argument_and_the_measured_exp_error(monkeypatch):
    """The device reward is one function of (design, argument): every path, size, table form and slot that ran in this
    session gave the same bits.  (Run alone, the test sweeps step_fast64 at 64 vehicles itself.)"""
    if ("my_step_ch", 4) not in SEEN:
        ch_case("fast64", 64, None)
    if ("my_step", 3) not in SEEN:
        count_case("fast64", 64, None)
    for kind, tab in SEEN.items():
        many = {a: v for a, v in tab.items() if len(v) != 1}
        assert not many, (kind, len(many), list(many.items())[:3])
        print(kind, "%d arguments, one value each" % len(tab))
    tab = SEEN[("my_step_ch", 4)]
    sole, at0 = tab[-1], tab[int(C.bits(np.array(0.0))[0])]      # the folded exp(1.0) and the run-time one (R == 0)
    e_sole, e_run = (abs(float(np.int64(next(iter(s))).view(np.float64))) for s in (sole, at0))
    print("exp(1.0): folded %r, run time %r, correctly rounded %r" % (e_sole, e_run, C.rn_exp(1.0)))
    hist = collections.Counter(int(round(e)) for e in EXP_ERR.values())
    worst = max(EXP_ERR, key=EXP_ERR.get)
    print("device exp over %d arguments: errors in ulps of RN(E) %s; worst %.2f at a = %r" % (
        len(EXP_ERR), dict(sorted(hist.items())), EXP_ERR[worst], float(np.int64(worst).view(np.float64))))
    assert max(EXP_ERR.values()) <= ORACLE_EXP_ULPS + 1


# ---- B. the RSSI window ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", (False, True), ids=("float64", "float32"))
def test_window_values_against_correctly_rounded_log10(f32):
    from diral_amd.sps import SpsPolicy
    rows = C.window_rows(f32)
    R = len(rows["chobs"])
    pol = SpsPolicy(R, 1, C.WIN_A, device=DEV, seed=0)
    chobs = torch.as_tensor(rows["chobs"], device=DEV).reshape(R, 1, C.WIN_A)
    assert chobs.dtype == (torch.float32 if f32 else torch.float64)
    w = _np(pol.window_from_chobs(chobs, torch.as_tensor(rows["actions"], device=DEV).reshape(R, 1))).reshape(R, C.WIN_A)
    bad, worst = C.window_failures(w, f32, HOST_LOG10_ULPS)
    print("device window over %d %s distances: %r; bound misses %d" % (len(rows["d"]), "float32" if f32 else "float64", worst, len(bad)))
    assert not bad, (len(bad), bad[:6])


def _policy(n, A, thr, prev, seed=5):
    from diral_amd.sps import SpsPolicy
    pol = SpsPolicy(n, 1, A, rssi_threshold=thr, device=DEV, seed=seed)
    pol.keep_prob = 0.0                                           # every agent re-selects:
    pol.counter.zero_()                                           # ... its counter has run out, and it never keeps
    pol.prev_action.copy_(torch.as_tensor(prev, device=DEV).reshape(n, 1))
    return pol


@pytest.mark.parametrize("f32", (False, True), ids=("float64", "float32"))
@pytest.mark.parametrize("A", C.DECISION_A)
def test_stand_alone_decisions_against_the_host_on_the_device_window(A, f32):
    """`step_from_chobs` (injected picks 0 ... need - 1, then the device's own draws against their mirror) and `step` on
    the window `window_from_chobs` gave, at four thresholds; every agent is compared."""
    rows = C.decision_rows(A, f32)
    n = len(rows["chobs"])
    chobs = torch.as_tensor(rows["chobs"], device=DEV).reshape(n, 1, A)
    own = torch.as_tensor(rows["own"], device=DEV).reshape(n, 1)
    for thr in C.THRESHOLDS:
        pol = _policy(n, A, thr, rows["prev"])
        w_t = pol.window_from_chobs(chobs, own)
        w = _np(w_t).reshape(n, A)
        want, _ = C.host_decisions(w, rows["prev"], thr, choice=rows["choice"])
        draws = dict(draw_counter=np.full(n, 7, np.int32), draw_keep=np.ones(n), draw_choice=rows["choice"])
        got = _np(pol.step_from_chobs(chobs, own, **draws)).reshape(-1)
        assert np.array_equal(got, want), (A, thr, "step_from_chobs", np.flatnonzero(got != want)[:6], rows["kind"][got != want][:6])
        assert np.array_equal(_np(pol.prev_action).reshape(-1), want) and (_np(pol.counter) == 7).all()
        pol = _policy(n, A, thr, rows["prev"])
        got = _np(pol.step(w_t, **draws)).reshape(-1)
        assert np.array_equal(got, want), (A, thr, "step", np.flatnonzero(got != want)[:6], rows["kind"][got != want][:6])
        pol = _policy(n, A, thr, rows["prev"])
        want, _ = C.host_decisions(w, rows["prev"], thr, seed=pol.seed * 1000003 + pol._t + 1)
        got = _np(pol.step_from_chobs(chobs, own)).reshape(-1)
        assert np.array_equal(got, want), (A, thr, "device draws", np.flatnonzero(got != want)[:6], rows["kind"][got != want][:6])
        assert (want != rows["prev"]).all()


# ---- B. the fused and K-slot launches ----------------------------------------------------------------------------------
def grid_topology(kind, N, B, seed):
    """grid10: a static 10 m integer grid - integer distances and ties, every resource heard; far: a static 2500 m grid on
    a 30 km highway with a 20 km range - d = 1e4 exactly, and transmitters beyond 5 km.  (cfg kwargs, A, x0 [B][N])."""
    rng = np.random.default_rng(seed)
    u = np.arange(N)
    if kind == "grid10":
        base, L, rc, A = 10.0 * u, 10.0 * N + 100.0, 250.0, 8 if N <= 64 else 16
    else:
        base, L, rc, A = 2500.0 * (u % 12) + 7.0 * (u // 12), 30000.0, 20000.0, 32 if N <= 64 else 64
    x0 = np.stack([rng.permutation(base) for _ in range(B)])
    return dict(communication_range=rc), L, A, x0


FUSED = [("fused", 64, STEP_MY_STEP, 1), ("three", 64, STEP_MY_STEP_CH, 1), ("slots", 64, STEP_MY_STEP, 2),
         ("slots_ch", 64, STEP_MY_STEP_CH, 2), ("wide_slots", 128, STEP_MY_STEP, 2), ("wide_slots", 256, STEP_MY_STEP, 2)]


@pytest.mark.parametrize("topo", ("grid10", "far"))
@pytest.mark.parametrize("case", FUSED, ids=lambda c: "%s-N%d" % (c[0], c[1]))
def test_fused_decisions_against_the_host_on_the_device_window(case, topo):
    """The decision a launch takes behind its first slot against the host's on `window_from_chobs` of that slot's channel
    observation: the launch's own where it has one slot, else a one-slot RICH step of a twin handle.  Every agent
    re-selects in the first slot (counter 0, keep probability 0) and none in the second (its counter is fresh), so the
    actions a two-slot launch hands back ARE the first slot's decisions."""
    from diral_amd.sps import SpsPolicy
    name, N, mode, K = case
    B = 6
    kw, L, A, x0 = grid_topology(topo, N, B, 17 + N)
    cfg = bench_config(N, A, L, reward_design=2, **kw)
    for dt in DTS:
        env = make_env(cfg, B, mode=mode, dtype=dt)
        env.reset_topology(x0, None, 0.0)
        pol = SpsPolicy(B, N, A, device=DEV, seed=11)
        pol.keep_prob = 0.0
        pol.counter.zero_()
        a = pol.prev_action.clone()
        nxt = torch.empty_like(a)
        seed = pol.seed * 1000003 + pol._t + 1
        env.step_policy(a, 0, pol, nxt, slots=K, mode=mode, want_chobs=True)
        torch.cuda.synchronize()
        fam = KERNEL_WIDE if N > 64 else KERNEL_FAST64
        ran(env, fam, policy=name != "three", ch=mode == STEP_MY_STEP_CH)
        if K == 1:
            chobs = env._chobs
        else:
            twin = make_env(cfg, B, mode=mode, dtype=dt)
            twin.reset_topology(x0, None, 0.0)
            twin._step(mode, a, 0, want_chobs=True)
            ran(twin, fam, rich=True, policy=False)
            chobs = twin._chobs
        w = _np(pol.window_from_chobs(chobs, a)).reshape(B * N, A)
        d = _np(chobs).astype(np.float64).reshape(B * N, A)
        if mode == STEP_MY_STEP_CH:                               # (my_step_ch observes occupancy, 0 / 1: the clamp tie)
            assert set(np.unique(d).tolist()) <= {0.0, 1.0} and (w[d == 1.0] == -40.0).all()
        elif topo == "far":
            assert (d == 1e4).any() and ((d > 5000.0) & (d < 100000.0)).any()
            assert (w[d == 1e4] == -160.0).all()
        else:
            assert (d == np.round(d)).all() and ((d > 0) & (d < 100000.0)).mean() > 0.75
        a_np = _np(a).reshape(-1)
        want, log = C.host_decisions(w, a_np, pol.threshold, seed=seed)
        assert len(log) == B * N                                  # every agent of every env decided, none left out
        got = _np(nxt).reshape(-1)
        assert np.array_equal(got, want), (name, N, topo, dt, np.flatnonzero(got != want)[:6])
        assert np.array_equal(_np(pol.prev_action).reshape(-1), want)
        env.check()
