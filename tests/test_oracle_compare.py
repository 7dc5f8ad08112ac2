"""tests/oracle_compare.py on real oracle data, without a device: an unmodified copy passes every rule, and every
single-element change is refused except the ones the rules allow - an exp() reward (and the state column that carries
it) within the exp() bar, the metrics' float sums within their summation tolerance, ages beyond the stored byte."""
import copy

import numpy as np
import pytest

from diral_amd.config import STEP_MY_STEP, STEP_MY_STEP_CH, bench_config
from oracle.oracle import Oracle, SQ_IEEE
from tests.oracle_compare import ALL, metrics_equal, slot_equal, tables_equal

B, N, A = 2, 4, 3
CASES = {"rd2_my_step": (2, STEP_MY_STEP), "rd3_my_step": (3, STEP_MY_STEP), "rd3_my_step_ch": (3, STEP_MY_STEP_CH)}


@pytest.fixture(scope="module", params=list(CASES))
def run(request):
    """Three slots of the oracle: (cfg, mode, the last slot's (state, reward, chobs), export, metrics)."""
    rd, mode = CASES[request.param]
    cfg = bench_config(N, A, 100.0, communication_range=40.0, reward_design=rd,
                       State=dict(num_bins=8, add_reward=True)).replace(track_arrival=True)
    rng = np.random.default_rng(1)
    orc = Oracle(cfg, batch=B, sq_mode=SQ_IEEE)
    orc.reset(rng.integers(0, 100, size=(B, N)).astype(np.float64), np.zeros((B, N)), np.full((B, N), 1.7))
    for t in range(3):
        a = rng.integers(0, A, size=(B, N)).astype(np.int32)
        rew, chobs = orc.step(mode, a, t)
        state = orc.obtain_state(a, chobs, rew)
    assert state.shape == (B, N, 12) and np.array_equal(state[..., -1], rew) and len(np.unique(rew)) == 3
    return cfg, mode, (state, rew, chobs), orc.export(), orc.metrics()


def refused(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


def changed(arrays, i, at, delta=None):
    """A copy of `arrays` (tuple or dict) with element `at` of array `i` moved: to the next float, or by `delta`."""
    out = copy.deepcopy(arrays) if isinstance(arrays, dict) else [a.copy() for a in arrays]
    out[i][at] = np.nextafter(out[i][at], np.inf) if delta is None else out[i][at] + delta
    return out


def exact_element(state, rew):
    """A state element that does not hold its agent's reward (one that does shares the reward's tolerance)."""
    return tuple(np.argwhere(state != rew[..., None])[0])


def test_an_unmodified_copy_passes_every_rule(run):
    cfg, mode, slot, exp, m = run
    slot_equal(cfg, mode, [a.copy() for a in slot], slot, "copy")
    slot_equal(cfg, mode, (slot[0].copy(), slot[1].copy(), None), slot, "no chobs")
    tables_equal(copy.deepcopy(exp), exp, "copy")
    assert set(ALL) <= set(exp) and m.shape == (B, 6)
    metrics_equal(m.copy(), m, "copy", prr=True, sums_exact=True)


def test_every_single_element_change_of_a_slot_is_refused_beyond_the_exp_bar(run):
    cfg, mode, slot, _, _ = run
    last = (1, 2, slot[0].shape[-1] - 1)                         # the state's reward column
    for i, at in ((0, exact_element(slot[0], slot[1])), (0, last), (1, (1, 2)), (2, (0, 1, 1))):
        is_reward = i == 1 or at == last
        if not (is_reward and cfg.reward_design == 3):
            refused(slot_equal, cfg, mode, changed(slot, i, at), slot, "next float")
        for delta in (1e-15, -1e-15, 1e-14, -1e-14) if is_reward else ():
            moved = changed(slot, i, at, delta)
            assert moved[i][at] != slot[i][at]
            if cfg.reward_design == 3 and abs(delta) < 2e-15:
                slot_equal(cfg, mode, moved, slot, delta)
            else:
                refused(slot_equal, cfg, mode, moved, slot, delta)


def test_a_float32_handle_is_held_to_the_cast(run):
    cfg, mode, slot, _, _ = run
    cast = [a.astype(np.float32) for a in slot]
    slot_equal(cfg, mode, cast, slot, "cast", dtype=np.float32)
    refused(slot_equal, cfg, mode, cast, slot, "float32 under the float64 rule")
    n_changed = 0
    for i in range(3):
        if not np.array_equal(cast[i], slot[i]):                 # the cast changes this array: the original is refused
            n_changed += 1
            mixed = list(cast)
            mixed[i] = slot[i]
            refused(slot_equal, cfg, mode, mixed, slot, i, dtype=np.float32)
    assert n_changed >= 1
    for d in (np.float32(np.inf), np.float32(-np.inf)):           # the neighbouring float32 of one state element
        off = [a.copy() for a in cast]
        at = exact_element(slot[0], slot[1])
        off[0][at] = np.nextafter(off[0][at], d)
        refused(slot_equal, cfg, mode, off, slot, "next float32", dtype=np.float32)


def test_every_table_plane_is_held_and_ages_as_the_stored_byte(run):
    _, _, _, exp, _ = run
    at = (1, 2, 3)
    for k in ALL:
        for d in (1, -1):
            refused(tables_equal, changed(exp, k, at[:exp[k].ndim], d), exp, k)
        tables_equal(changed(exp, k, at[:exp[k].ndim], 1), exp, "plane left out", planes=[p for p in ALL if p != k])
    want = changed(exp, "age", at, 300 - exp["age"][at])
    tables_equal(changed(exp, "age", at, 255 - exp["age"][at]), want, "saturated")
    refused(tables_equal, changed(exp, "age", at, 254 - exp["age"][at]), want, "254 against 300")
    got = copy.deepcopy(exp)
    got["la"] = got["la"].astype(np.int32)
    tables_equal(got, exp, "int32 stamps")
    del got["la"]
    tables_equal(got, exp, "no stamps on one side")


def test_metric_counts_are_exact_and_float_sums_within_their_tolerance(run):
    _, _, _, _, m = run
    for col in range(6):
        for d in (1.0, -1.0):
            bad = changed((m,), 0, (1, col), d)[0]
            refused(metrics_equal, bad, m, col, prr=True)
            if col < 4:
                refused(metrics_equal, bad, m, col)
    near = changed((m,), 0, (1, 1), 1e-13 * max(abs(m[1, 1]), 1.0))[0]
    assert near[1, 1] != m[1, 1]
    metrics_equal(near, m, "1e-13 relative")
    refused(metrics_equal, near, m, "1e-13 relative", sums_exact=True)
