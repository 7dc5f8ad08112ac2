"""Keeps tests/libm_cases.py honest, without a GPU: the layouts hold what the GPU sweep (tests/test_gpu_libm_edges.py) claims
for them, the integer host model and the oracle agree bit for bit where no exp() is involved, the oracle's exp() and the
host's log10 are within the one ulp of the correctly rounded values that the device's bounds are derived from, and every
wrong restatement the sweep is there to catch is told apart by the comparison functions the GPU test calls."""
import math

import numpy as np
import pytest

from diral_amd.config import STEP_DESIGN, STEP_MY_STEP
from tests import libm_cases as C

ORACLE_EXP_ULPS, HOST_LOG10_ULPS = C.ORACLE_EXP_ULPS, C.HOST_LOG10_ULPS


@pytest.mark.parametrize("N", C.RATIO_SIZES)
def test_ratio_layout_holds_every_claimed_pair_and_its_edges(N):
    lay, mod = C.ratio_layout(N), C.ratio_model(N)
    P = len(C.claimed_pairs(N))
    env = np.arange(P)
    got = np.stack([mod["rec"][env, 0], mod["inr"][env, 0]], axis=1)
    assert np.array_equal(got, np.array(C.claimed_pairs(N))), np.argwhere(got != np.array(C.claimed_pairs(N)))[:4]
    assert len(set(C.claimed_pairs(N))) == P == {64: 2016, 33: 528}.get(N, P)
    assert mod["coll"][:2 * P].all()                              # both resources collide in every env of the sweep
    assert lay["sole"].sum() == 2 and not mod["coll"][lay["sole"], lay["marked"][lay["sole"]]].any()
    k, n = lay["kn"][:, 0], lay["kn"][:, 1]
    on_mid, on_edge = (lay["x"] == C.X_MID).sum(1), (lay["x"] == C.X_EDGE).sum(1)
    assert np.array_equal(on_mid == 1, k >= 1) and np.array_equal(on_edge == 1, n < N - 2)      # wherever there is room
    # the swapped variant pays the tie to the transmitter at 1100 (now the lower id)
    sw = env + P
    assert np.array_equal(mod["rec"][sw, N - 1], np.where(k[:P] >= 1, k[:P] - 1, 0)) and np.array_equal(mod["inr"][sw, N - 1], n[:P])
    R = mod["R"]
    assert (mod["inr"] == 0).any() and (R == 0.0).any() and ((R == 1.0) & (mod["inr"] > 0)).any()
    assert ((mod["inr"][:, 2:N - 2] <= 2).all()) and (mod["rec"] <= mod["inr"]).all()


@pytest.mark.parametrize("N", C.RATIO_SIZES)
def test_host_model_equals_the_oracle_bit_for_bit_at_design_2(N):
    mod, orc = C.ratio_model(N), C.ratio_oracle(N, 2)
    ref, bound, _ = C.ch_reference(2, mod["R"], mod["coll"])
    assert len(C.reward_failures(2, orc["rew"], ref, bound)) == 0
    assert np.array_equal(orc["metrics"][:, 5], np.full(len(ref), float(N)))
    assert len(C.prr_sum_failures(orc["metrics"][:, 4], mod["R"])) == 0
    k, n = C.ratio_layout(N)["kn"].T
    sel = np.flatnonzero((n > 0) & ~C.ratio_layout(N)["swapped"] & ~C.ratio_layout(N)["sole"])
    assert C.same_bits(orc["rew"][sel, 0], -1.0 * (1.0 - k[sel] / n[sel]))


def test_oracle_exp_is_within_one_ulp_of_the_correctly_rounded_values():
    worst = 0.0
    for N in C.RATIO_SIZES:
        mod = C.ratio_model(N)
        for design in (3, 4):
            ref, bound, E = C.ch_reference(design, mod["R"], mod["coll"], m=0)
            got = C.ratio_oracle(N, design)["rew"]
            worst = max(worst, float(C.exp_errors(design, got, ref, E).max()))
            assert len(C.reward_failures(design, got, ref, bound)) == 0, (N, design)     # the oracle under m = 0: one ulp
    for N in C.COUNT_SIZES:
        ref, bound, E = C.count_reference(C.count_layout(N)["c"], m=0)
        got = C.count_oracle(N, 3, STEP_MY_STEP)
        err = C.exp_errors(3, got, ref, E)
        worst = max(worst, float(err.max()))
        assert err.max() == 0.0, N                                 # -exp(1 - 1/c): correctly rounded everywhere
    print("oracle exp: worst error %.2f ulp of E over %d arguments" % (worst, len(C.exp_arguments())))
    assert worst <= ORACLE_EXP_ULPS


def test_decimal_and_mpmath_agree():
    try:
        import mpmath  # noqa: F401
    except ImportError:
        return                                                     # (a second opinion, wherever it is installed)
    for a in C.exp_arguments():
        assert C.rn_exp(a) == C.mp_exp(a), a
    d = C.window_rows(False)["d"].astype(np.float64)
    for v in d[C.heard(d) & (d >= 1.0)][::7].tolist() + [10.0, 100.0, 1000.0, 1e4]:
        assert C.rn_log10(v) == C.mp_log10(v), v


def test_wrong_ratio_and_exp_restatements_are_told_apart():
    N = 64
    lay, mod = C.ratio_layout(N), C.ratio_model(N)
    rec, inr, coll, R = mod["rec"], mod["inr"], mod["coll"], mod["R"]
    for design in C.CH_DESIGNS:
        ref, bound, E = C.ch_reference(design, R, coll)
        assert len(C.reward_failures(design, ref, ref, bound)) == 0
        assert len(C.reward_failures(design, C.ratio_oracle(N, design)["rew"], ref, bound)) == 0

        def misses(R2, coll2=coll):
            return len(C.reward_failures(design, C.ch_reference(design, R2, coll2, m=0)[0], ref, bound))
        # the ratio as k * (1 / n): an ulp of R, which design 2 pins (behind exp() it is inside the bound)
        with np.errstate(divide="ignore", invalid="ignore"):
            Rm = np.where(coll, np.where(inr > 0, rec * (1.0 / inr), 1.0), 1.0)
        assert (Rm != R).sum() > 100 and (design != 2 or misses(Rm) > 100)
        # the tie paid to the higher id; d <= Rc; nobody in range -> 0
        for kw in (dict(tie_high=True), dict(closed=True)):
            r2, i2, c2 = C.host_pairs(lay["x"], lay["acts"], 2, C.RC, **kw)
            assert misses(C.ratios(r2, i2, c2)) > 100, kw
        assert misses(C.ratios(rec, inr, coll, empty_is=0.0)) > 0
        if design != 2:                                            # exp() evaluated in float32: 1e9 ulps
            E32 = np.exp((1.0 - R).astype(np.float32)).astype(np.float64)
            wrong = np.where(coll, 1.0 - E32 if design == 3 else -E32, ref)
            assert len(C.reward_failures(design, wrong, ref, bound)) > R.size // 2
            assert C.exp_errors(design, wrong, ref, E).max() > 1e6
    # my_step design 3 from the counts
    ref, bound, E = C.count_reference(C.count_layout(N)["c"])
    wrong = np.where(C.count_layout(N)["c"] > 1, -np.exp((1.0 - 1.0 / np.maximum(C.count_layout(N)["c"], 1)).astype(np.float32)).astype(np.float64), 1.0)
    assert len(C.reward_failures(3, wrong, ref, bound)) > 0 and len(C.reward_failures(3, ref, ref, bound)) == 0


@pytest.mark.parametrize("N", (64, 33))
def test_count_layouts_sit_far_from_the_mean_distance_decision(N):
    lay = C.count_layout(N)
    x = lay["x"]
    half = N + 1
    assert np.abs(x[0][:, None] - x[0][None, :]).max() < C.RC / 2 and np.diff(x[half]).min() > 2 * C.RC
    assert sorted(set(lay["c"].ravel().tolist())) == list(range(1, N + 1))
    for design in C.MY_STEP_DESIGNS:
        assert np.isfinite(C.count_oracle(N, design, STEP_MY_STEP)).all()
    assert np.isfinite(C.count_oracle(N, 1, STEP_DESIGN)).all()
    # the two layouts are paid differently where the mean distance decides (design 1)
    r = C.count_oracle(N, 1, STEP_MY_STEP)
    assert not np.array_equal(r[:half], r[half:])


@pytest.mark.parametrize("f32", (False, True))
def test_host_window_is_within_the_bound_and_wrong_log10_is_told_apart(f32):
    rows = C.window_rows(f32)
    m = C.host_log10_error(f32)
    print("host log10: worst error %.2f ulp on %d distances" % (m, len(rows["d"])))
    assert m <= HOST_LOG10_ULPS
    for p, w in C.POWERS:                                          # the correctly rounded chain is exact at the powers of ten
        assert -40.0 - 30.0 * C.rn_log10(p) == w and -40.0 - 30.0 * math.log10(p) == w
    good = C.host_window(rows["chobs"], rows["actions"])
    bad, worst = C.window_failures(good, f32, HOST_LOG10_ULPS)
    assert not bad, bad[:5]
    chain = C.host_window(rows["chobs"], rows["actions"], log10=C.rn_log10_array)
    assert not C.window_failures(chain, f32, 0)[0]
    if not f32:                                                    # NumPy's chain is the correctly rounded one on (1, 1e5)
        d = rows["d"].astype(np.float64)
        sel = C.heard(d)
        assert np.array_equal(C.window_values(good, rows)[0][sel], C.window_values(chain, rows)[0][sel])
    # one ulp high at 1e4
    high = C.host_window(rows["chobs"], rows["actions"], log10=lambda a: np.where(a == 1e4, np.nextafter(4.0, 5.0), np.log10(a)))
    assert any(b[0] == "exact" and b[3] == -160.0 for b in C.window_failures(high, f32, HOST_LOG10_ULPS)[0])
    # log(d) / log(10)
    quot = C.host_window(rows["chobs"], rows["actions"], log10=lambda a: np.log(a) / math.log(10.0))
    if not np.array_equal(quot, good):
        assert C.window_failures(quot, f32, HOST_LOG10_ULPS)[0]
    # a window that is not monotone over a run of adjacent distances
    s, n = rows["runs"][3]
    swapped = good.copy()
    flat = swapped[:, 1:].reshape(-1)
    assert flat[s] != flat[s + n - 1]
    flat[s], flat[s + n - 1] = flat[s + n - 1], flat[s]
    swapped[:, 1:] = flat.reshape(swapped.shape[0], -1)
    assert any(b[0] == "monotone" for b in C.window_failures(swapped, f32, 4)[0])
    # the own subframe and NaN
    assert (good[:, 0] == -60.0).all() and rows["own_d"] == 777.0


@pytest.mark.parametrize("A", C.DECISION_A)
def test_decision_rows_hold_what_they_are_for(A):
    for f32 in (False, True):
        rows = C.decision_rows(A, f32)
        d, own, prev, choice, kind = (rows[k] for k in ("chobs", "own", "prev", "choice", "kind"))
        w = C.host_window(d, own)
        picks, _ = C.host_decisions(w, prev, -110.0, choice=choice)
        # the host's own judgement of every (row, prev) - the pick does not enter it
        one = np.array([i for i in range(len(d)) if i == 0 or (kind[i], prev[i]) != (kind[i - 1], prev[i - 1])])
        _, log = C.host_decisions(w[one], prev[one], -110.0, choice=choice[one], chobs=d[one], own=own[one])
        assert len(log) == len(one)
        kind1 = kind[one]
        for name, side in rows["label"].items():                   # on the labelled side of the shortcut
            got = {rec["shortcut"] for rec in log if kind1[rec["agent"]] == name}
            assert got == {side}, (A, name, got)
        assert {rec["far"] for rec in log if kind1[rec["agent"]] == "beyond5000"} == {True}
        assert {rec["far"] for rec in log if kind1[rec["agent"]] == "at5000"} == {False}
        assert {rec["shortcut"] for rec in log if kind1[rec["agent"]] == "at5000" and prev[one][rec["agent"]] == own[0]} == {True}
        assert (picks != prev).all() and (picks != own).any()
        # every pick 0 ... need - 1 (or the selection) is asked for
        assert set((choice % rows["need"]).tolist()) >= {0, rows["need"] - 1}
        # d = 1e4 one ulp either way, and a clamp tie broken: decisions change
        at = (d.astype(np.float64) == 1e4) & (np.arange(A)[None, :] != own[:, None])
        assert at.any() and (w[at] == -160.0).all()
        for step in (np.inf, -np.inf):
            moved = np.where(at, np.nextafter(w, step), w)
            assert (C.host_decisions(moved, prev, -110.0, choice=choice)[0] != picks).any(), (A, step)
        cl = (kind == "clamp")
        assert (w[cl][:, :A - 1] == -40.0).all()
        broken = w.copy()
        broken[cl, 0] = np.nextafter(-40.0, 0.0)
        assert (C.host_decisions(broken, prev, -110.0, choice=choice)[0] != picks)[cl].any(), A
        # adjacent pairs: the lower subframe holds the larger distance
        adj = d[kind == "adjacent"][0].astype(np.float64)
        assert (adj[0:A - 2:2] > adj[1:A - 1:2]).all()
        # thresholds below -200 and between -200 and -160 raise
        for thr in (-165.0, -230.0):
            _, lg = C.host_decisions(w, prev, thr, choice=choice)
            assert sum(rec["raises"] for rec in lg) > 0
