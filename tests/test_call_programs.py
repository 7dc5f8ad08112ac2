"""What keeps tests/test_gpu_call_programs.py honest, checked on the host model alone (no GPU): the committed programs are
deterministic, walk every ordered pair of op classes a family accepts at least twice, refuse rarely, leave no env out,
and reach the states they are there for - lags above 7 in the sparse families, steps off the y = 0 lane and back on it,
vehicles whose wrap takes the generic branch.  And the wrap itself is pinned to Python's own `%`, not to our C."""
import collections
import functools
import math

import numpy as np
import pytest

from diral_amd.config import STEP_MY_STEP, bench_config
from oracle.oracle import SQ_IEEE, Oracle
from tests import call_programs as P

CASES = [(fam, seed) for fam in P.FAMILIES for seed in P.SEEDS[fam]]


@functools.lru_cache(maxsize=None)
def host(family, seed):
    prog, expected, closing, rec, digest = P.run_host(family, seed)
    return prog, rec, digest


def pair_table(family):
    """Ordered pairs of op classes over the family's committed programs, as counts and as text."""
    count = collections.Counter()
    for seed in P.SEEDS[family]:
        count.update(P.transitions(host(family, seed)[0]))
    classes = P.family_classes(family)
    rows = ["%-13s" % "from \\ to" + " ".join("%5s" % c[:5] for c in classes)]
    for a in classes:
        rows.append("%-13s" % a + " ".join("%5d" % count[(a, b)] for b in classes))
    return count, "\n".join(rows)


def test_six_seeds_with_six_residues_per_family():
    for fam, seeds in P.SEEDS.items():
        assert len(seeds) == 6 and sorted(s % 6 for s in seeds) == list(range(6)), fam


@pytest.mark.parametrize("family,seed", CASES)
def test_same_seed_same_program_and_same_expected_outputs(family, seed):
    prog, rec, digest = host(family, seed)
    again = P.run_host(family, seed)
    assert again[4] == digest
    assert P.MIN_OPS <= len(prog["ops"]) <= P.MAX_OPS, len(prog["ops"])
    assert [P.describe(o) for o in again[0]["ops"]] == [P.describe(o) for o in prog["ops"]]


@pytest.mark.parametrize("family", list(P.FAMILIES))
def test_every_ordered_pair_of_op_classes_occurs_twice(family):
    count, text = pair_table(family)
    print(text)
    classes = P.family_classes(family)
    assert len(classes) == (11 if P.FAMILIES[family]["kslot"] else 10)
    missing = [(a, b, count[(a, b)]) for a in classes for b in classes if count[(a, b)] < 2]
    assert not missing, "%s\n%s" % (missing, text)


def test_refusals_are_rare_and_no_env_is_left_out():
    ops = refused = 0
    for fam, seed in CASES:
        prog, rec, _ = host(fam, seed)
        assert rec["left_out"] == 0, (fam, seed, rec["host_record"])
        ops += rec["ops"]
        refused += rec["refused"]
        assert rec["refused"] == sum(1 for o in prog["ops"] if o.get("refused"))
    print("ops %d, refused %d" % (ops, refused))
    assert 0 < refused <= 0.10 * ops, (refused, ops)


@pytest.mark.parametrize("family", [f for f in P.FAMILIES if P.FAMILIES[f].get("sparse")])
def test_sparse_families_leave_the_ring_before_a_kslot_launch_and_before_an_export(family):
    lag_k = max(host(family, s)[1]["lag_kslot"] for s in P.SEEDS[family])
    lag_e = max(host(family, s)[1]["lag_export"] for s in P.SEEDS[family])
    print(family, "max lag before a K-slot launch", lag_k, "before an export", lag_e)
    assert lag_k > 7 and lag_e > 7, (lag_k, lag_e)


@pytest.mark.parametrize("family,seed", CASES)
def test_flat_flip_and_offroad_reach_what_they_are_for(family, seed):
    prog, rec, _ = host(family, seed)
    names = [o["op"] for o in prog["ops"]]
    if "flat_flip" in names:
        assert rec["steps_off_lane"] >= 1 and rec["steps_after_restore"] >= 1, rec
    for below, above in rec["offroad"]:
        assert below >= 1 and above >= 1, rec["offroad"]


def test_offroad_record_counts_every_import():
    """Two import_offroad ops with no step between them share one next step: the record then holds one entry for both."""
    for fam, seed in CASES:
        prog, rec, _ = host(fam, seed)
        want, open_ = 0, False
        for o in prog["ops"]:
            if o["op"] == "import_offroad":
                open_ = True
            elif o["op"] in P.STEP_LIKE and not o.get("refused") and open_:
                want, open_ = want + 1, False
        assert not open_ and len(rec["offroad"]) == want, (fam, seed)


# ---- the wrap -------------------------------------------------------------------------------------------------------
def _edge_triples(L, rng, n):
    x = rng.uniform(-3.0 * L, 5.0 * L, size=n)
    v = np.where(rng.random(n) < 0.5, rng.uniform(1.1, 2.77, size=n), rng.uniform(-2.0 * L, 2.0 * L, size=n))
    edges_x = [L, 2.0 * L, -0.0, 0.0, -1e-300, 1e-300, -L, -2.0 * L, 3.0 * L, np.nextafter(L, 0.0), np.nextafter(L, 2 * L),
               np.nextafter(-(L + 1.5), -np.inf), np.nextafter(-(L + 1.5), np.inf), -(L + 1.5), 5.0 * L, -3.0 * L]
    edges_v = [1.5, -L, 0.0, -0.0, L, 2.0 * L, -2.0 * L, 1.1, 2.77]
    k = 0
    for ex in edges_x:
        for ev in edges_v:
            x[k], v[k] = ex, ev
            k += 1
    return x, v


@pytest.mark.parametrize("L", [2000.0, 6000.0, 1234.5, 30000.0])
def test_oracle_wrap_is_pythons_own_modulo(L):
    """One oracle slot moves x to Python's `(x + v + L) % L` (network.py:203), bit for bit and sign of zero included, for
    2500 triples per highway length: positions in [-3L, 5L], speeds in [-2L, 2L], and the edges between the branches."""
    B, N = 50, 50
    cfg = bench_config(N, 4, L)
    rng = np.random.default_rng(int(L))
    x, v = _edge_triples(L, rng, B * N)
    orc = Oracle(cfg, batch=B, sq_mode=SQ_IEEE)
    orc.reset(x.reshape(B, N), np.zeros((B, N)), v.reshape(B, N))
    orc.step(STEP_MY_STEP, np.zeros((B, N), np.int32), 0)
    got = orc.export()["pos_x"].reshape(-1)
    s = x + v + L
    assert (s < 0).sum() > 100 and (s > 2 * L).sum() > 100 and ((s >= L) & (s <= 2 * L)).sum() > 100
    bad = [(float(x[i]), float(v[i]), float(got[i]), P.python_wrap(x[i], v[i], L)) for i in range(B * N)
           if not P.same_float_bits(float(got[i]), P.python_wrap(x[i], v[i], L))]
    assert not bad, bad[:5]
    assert any(math.copysign(1.0, float(g)) > 0 and g == 0.0 for g in got)          # a zero result occurs, and it is +0.0
