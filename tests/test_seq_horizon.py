"""The oracle near the 24-bit sequence-number horizon (no GPU).

The table words of the kernels pack a sequence number into 24 bits (include/diral_env.h: DIRAL_MAX_SLOTS); the oracle
keeps plain int32 numbers, as the reference keeps Python ints.  The reference only ever COMPARES two numbers about one
subject (vehicle.py:56-63) and tests a number against 0, "never heard": so a run whose heard entries all carry numbers
shifted by one constant must compute the same rewards, observations, states, ages, xpos, arrival stamps and metrics,
and end on tables whose numbers differ by exactly that constant.  This is what lets tests/test_gpu_seq_horizon.py take
the oracle as the statement of the operation at numbers no fixture of the reference reaches (it would have to run for
8 million slots first).
"""
import numpy as np
import pytest

from diral_amd.config import MAX_SLOTS, STEP_DESIGN, STEP_MY_STEP, STEP_MY_STEP_CH, bench_config
from tests.golden_util import horizon_tables

T = 10
BASE = 1_300_000
STARTS = (BASE, (1 << 23) - 4, (1 << 24) - 2 - T)


def run_oracle(cfg, mode, tab, seq, acts, threads=1):
    """T slots of `mode` from the tables `tab` with the numbers `seq`: everything the run computes, per slot."""
    from oracle.oracle import Oracle, SQ_IEEE
    B, N = tab["pos_x"].shape
    orc = Oracle(cfg, batch=B, sq_mode=SQ_IEEE, threads=threads)
    orc.reset(tab["pos_x"], np.zeros((B, N)), tab["vel"])
    orc.import_state(seq=seq, age=tab["age"], x=tab["x"], y=np.zeros((B, N, N)))
    out = []
    for t in range(len(acts)):
        rew, chobs = orc.step(mode, acts[t], t)
        d = dict(rew=rew, chobs=chobs, state=orc.obtain_state(acts[t], chobs, rew))
        d.update(orc.export())
        out.append(d)
    return out, orc.info_age(len(acts) - 1), orc.metrics()


def shifted(seq, delta):
    return np.where(seq > 0, seq.astype(np.int64) + delta, 0).astype(np.int32)


def test_the_constant_the_header_states():
    assert MAX_SLOTS == (1 << 24) - 2 == 16_777_214


@pytest.mark.parametrize("mode", [STEP_MY_STEP, STEP_MY_STEP_CH, STEP_DESIGN])
@pytest.mark.parametrize("rd", [1, 2, 3, 4, 5])
def test_oracle_is_translation_invariant_in_the_sequence_numbers(mode, rd):
    N, A, L, B = 40, 6, 1500.0, 2
    cfg = bench_config(N, A, L, reward_design=rd, track_arrival=True, track_prr=True,
                       State=dict(add_channel_obs=True, add_reward=True, add_index=True, add_velocity=True, add_position=True))
    rng = np.random.default_rng(77 + 10 * mode + rd)
    tab = horizon_tables(rng, B, N, L, BASE)
    acts = rng.integers(0, A, size=(T, B, N)).astype(np.int32)
    base, base_ia, base_m = run_oracle(cfg, mode, tab, tab["seq"], acts)
    assert any((s["seq"] != base[0]["seq"]).any() for s in base[1:])          # the tables do move
    for own in STARTS[1:]:
        delta = own - BASE
        run, ia, m = run_oracle(cfg, mode, tab, shifted(tab["seq"], delta), acts)
        for t, (a, b) in enumerate(zip(base, run)):
            for k in ("rew", "chobs", "state", "age", "x", "y", "pos_x", "vel", "la", "pf"):
                assert np.array_equal(a[k], b[k]), (k, t, own)
            assert np.array_equal(b["seq"], shifted(a["seq"], delta)), (t, own)
        assert np.array_equal(ia, base_ia) and np.array_equal(m, base_m), own
    assert run[-1]["seq"].max() == MAX_SLOTS                                   # the last run ended on the last legal number
