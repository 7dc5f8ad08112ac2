"""The three rules every comparison against the CPU oracle (IEEE-square mode) goes by, on NumPy arrays, without a
device: one slot's outputs, the exported tables, the metrics.  Everything is bit for bit except what passes through
exp() (within EXP_ATOL) and the metrics' float sums, whose order of summation differs.  A failed rule raises
AssertionError with `what`, the number of differing elements, their first indices and values."""
import math

import numpy as np

from tests.golden_util import EXP_ATOL

ALL = ("seq", "x", "y", "pos_x", "vel", "age", "la")
F32_EXP_ATOL = 1e-6        # a float32 exp() reward against the oracle's float64
PRR_ATOL = 1e-6            # BASELINE.json north_star: the packet reception ratio


def uses_exp(cfg, mode):
    return cfg.reward_design in (3, 4)


def exp_close(a, b):
    return bool(np.all(np.abs(np.asarray(a) - np.asarray(b)) <= EXP_ATOL))


def exp_atol(on):
    """The tolerance of a value that passes through exp() when `on`, None (exact) otherwise."""
    return EXP_ATOL if on else None


def exp_bounds(N):
    """Rewards built on exp() differ by at most EXP_ATOL each (|reward| <= e).  A sum of N of them in one fixed order
    then differs by at most N * EXP_ATOL plus the rounding of N - 1 additions of partial sums below N * e on either
    side, 2 * N * 2**-53 * N * e; a shaped reward (reward + sum / N) by its own EXP_ATOL, that over N, and the rounding
    of one division and one addition below 8 on either side (4 * 2**-52 * 4)."""
    sum_atol = N * EXP_ATOL + 2.0 * N * N * math.e * 2.0 ** -53
    return sum_atol, EXP_ATOL + sum_atol / N + 16 * 2.0 ** -52


def stored_age(age):
    """The device stores an age as a byte that saturates at 255."""
    return np.minimum(age, 255)


def same(got, want, what, equal_nan=False, atol=None, rtol=0.0):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if atol is None:
        ok = (got == want) | (np.isnan(got) & np.isnan(want)) if equal_nan else got == want
    else:
        ok = np.abs(got.astype(np.float64) - want) <= atol + rtol * np.abs(want)
    assert ok.all(), (what, int((~ok).sum()), np.argwhere(~ok)[:5], got[~ok][:5], want[~ok][:5])


def slot_equal(cfg, mode, got, want, what, dtype=np.float64):
    """One slot: `got` and `want` are (state, reward, chobs or None), `want` the oracle's float64.  Rewards are exact,
    those of the exp() designs within EXP_ATOL; the state is exact, but for the elements that hold such a reward
    (State.add_reward), which share its tolerance; the channel observation is exact.  A float32 handle (`dtype`) gives
    float32 arrays and is held to the float32 cast of `want` by the same rules, its exp() reward to F32_EXP_ATOL of the
    float64 value."""
    exp, f32 = uses_exp(cfg, mode), np.dtype(dtype) == np.float32
    atols = (None, exp_atol(exp), None)
    if exp and cfg.State.add_reward:                  # only the elements that hold the agent's own reward may differ
        atols = (np.where(want[0] == want[1][..., None], EXP_ATOL, 0.0),) + atols[1:]
    for name, g, w, atol in zip(("state", "reward", "chobs"), got, want, atols):
        if g is None:
            continue
        assert g.dtype == dtype, (what, name, g.dtype)
        if f32 and name == "reward" and exp:
            same(g, w, (what, name), atol=F32_EXP_ATOL)
        else:
            same(g, w.astype(np.float32).astype(np.float64) if f32 else w, (what, name), atol=atol)


def tables_equal(st, oe, what, planes=ALL):
    """An export of the handle against the oracle's: every plane exact, ages as the stored byte, the arrival stamps
    (where both sides hold them) as int64."""
    for k in planes:
        if k == "age":
            same(st[k], stored_age(oe[k]), (what, k))
        elif k != "la":
            same(st[k], oe[k], (what, k))
        elif k in st and k in oe:
            same(st[k].astype(np.int64), oe[k], (what, k))


def metrics_equal(m, om, what, prr=False, sums_exact=False):
    """Counts (columns 0, 2, 3) exact; the reward sum (1) within rtol 1e-12, atol 1e-9 - the order of summation differs -
    or exact with `sums_exact` (integer-valued rewards, or two handles that sum in one order); with `prr` the reception
    count (5) exact, the PRR sum (4) held like column 1 and the ratio within PRR_ATOL."""
    tol = {} if sums_exact else dict(rtol=1e-12, atol=1e-9)
    same(m[:, [0, 2, 3]], om[:, [0, 2, 3]], (what, "counts"))
    same(m[:, 1], om[:, 1], (what, "reward sum"), **tol)
    if prr:
        same(m[:, 5], om[:, 5], (what, "receptions"))
        same(m[:, 4], om[:, 4], (what, "PRR sum"), **tol)
        ratio = [x[:, 4] / np.maximum(x[:, 5], 1) for x in (m, om)]
        same(ratio[0], ratio[1], (what, "PRR"), atol=PRR_ATOL)
