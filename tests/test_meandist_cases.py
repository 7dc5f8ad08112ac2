"""What keeps tests/test_gpu_meandist_edges.py honest, checked without a GPU: every env of tests/meandist_cases.py holds
what it claims under the plain host statement - the tuned pairs straddle Rc between two neighbouring doubles with ids
that are not in x order, the transmitter sets cross 64-bit words / sit in the top word / take every second id where
they say so, the division layouts sum to the one double at which `s / cnt` and `s * (1.0 / cnt)` decide differently,
the toy-weight, off-lane and design-step envs decide as built -; the C oracle returns the statement's rewards bit for
bit on every env (SQ_IEEE; SQ_POW on every env the construction kept); and each deliberately wrong restatement changes
the reward of at least one env of every (size, family) set it applies to.

Restatements that CANNOT be told apart somewhere, and why:
* every summation order (reversed, descending ids, word-major, fsum, tree) at c == 2: one term;
* word-major at N <= 64: one word, it IS the ascending order;
* the pairwise tree at c == 3: (d0 + d1) + d2 is the serial sum;
* the last index winning the norm's ties on one lane (y == 0 everywhere): the two holders of an extreme are on one
  point, so the norm is the same distance - only the y = 0 / 1 envs of the off-lane handles tell it apart;
* `>=` needs m == Rc exactly: the pair exactly Rc apart (`c2-exact`), the 60-144-156 / 60-221-229 triple, and whichever
  tuned `below` env happens to land on Rc."""
import collections

import numpy as np
import pytest

from diral_amd.config import STEP_DESIGN, STEP_MY_STEP
from tests import meandist_cases as C

SIZES = pytest.mark.parametrize("N", C.SIZES)


def cases_of(envs, family):
    out = collections.OrderedDict()
    for e in envs:
        if e["family"] == family:
            out.setdefault(e["case"], []).append(e)
    return out


def check_others(e):
    """Outside the marked resource (and outside the toy envs, which place everybody by hand): two vehicles of one resource
    are at least 620 m apart - each alone within 2 Rc, the weight plainly 1."""
    for a, ids in C.transmitters(e).items():
        if a != 0:
            xs = sorted(e["x"][u] for u in ids)
            assert all(q - p >= 620.0 for p, q in zip(xs, xs[1:])), (e["case"], a)
            assert all(e["y"][u] == 0.0 for u in ids)


def check_tuned(es, family):
    up, dn = es
    assert (up["role"], dn["role"]) == ("above", "below") and up["ids"] == dn["ids"] and up["y"] == dn["y"]
    ids, rc = up["ids"], up["rc"]
    diff = [u for u in range(up["N"]) if up["x"][u] != dn["x"][u]]
    assert len(diff) == 1 and diff[0] in ids and C.bits(up["x"][diff[0]]) == C.bits(dn["x"][diff[0]]) + 1   # one double
    assert up.get("tuned", diff[0]) == diff[0] and up["x"][diff[0]] == max(up["x"][u] for u in ids)
    m_up, m_dn = C.mean_distance(up, ids), C.mean_distance(dn, ids)
    assert m_up > rc >= m_dn, (up["case"], m_up, m_dn)
    # one double of x moves c - 1 distances by at most ulp(x) each; the cnt additions round by at most ulp(s) / 2 each, either env
    cnt = len(ids) * (len(ids) - 1) // 2
    assert m_up - m_dn <= ((len(ids) - 1) * np.spacing(up["x"][diff[0]]) + cnt * np.spacing(cnt * rc)) / cnt + np.spacing(rc)
    xs = [up["x"][u] for u in ids]
    if len(ids) == 2:
        assert xs[0] > xs[1]
    else:
        assert xs != sorted(xs) and xs != sorted(xs, reverse=True)
    assert C.weight(up, ids) == 1 and C.weight(dn, ids) == 0
    if family == "offlane":
        assert set(up["y"]) <= set(C.LANES) and any(up["y"][u] != 0.0 for u in ids)
    else:
        assert not up["offlane"]


@SIZES
def test_order_pairs_straddle_the_range_with_ids_against_x(N):
    envs = C.layout(N)["envs"]
    seen, pats = collections.Counter(), collections.Counter()
    for case, es in cases_of(envs, "order").items():
        check_tuned(es, "order")
        ids = es[0]["ids"]
        seen[len(ids)] += 1
        pat = es[0]["pattern"]
        pats[pat] += 1
        words = {u // 64 for u in ids}
        if pat == "cross":
            assert len(words) > 1
        if pat == "top":
            assert words == {(N - 1) // 64} and N > 64
        if pat == "alt":
            assert all(b - a == 2 for a, b in zip(ids, ids[1:])) and len(words) > 1
        if pat == "all":
            assert ids == list(range(N))
        for e in es:
            check_others(e)
    assert set(seen) == set(C.ORDER_COUNTS[N]) | {2} and min(seen[c] for c in C.ORDER_COUNTS[N]) >= 2, seen   # (2: `c2-exact`)
    if N in (128, 256):
        assert pats["cross"] >= 4 and pats["top"] >= 3 and pats["alt"] >= 3 and pats["all"] == 2, pats
        assert any(e["pattern"] == "alt" and len(e["ids"]) == 65 for e in envs if e["family"] == "order") == (N == 256)


@SIZES
def test_division_layouts_sum_to_the_double_where_the_reciprocal_decides_differently(N):
    envs = C.layout(N)["envs"]
    got = set()
    for case, (e,) in cases_of(envs, "division").items():
        ids, rc = e["ids"], e["rc"]
        s, cnt = C.pair_sum(e, ids)
        assert cnt == len(ids) * (len(ids) - 1) // 2 and s == e["target"]
        assert abs(C.bits(s) - C.bits(cnt * rc)) <= 6
        assert (s / cnt > rc) != (s * (1.0 / cnt) > rc)
        # the grid: every other order of additions gives the same sum, so only the division is on trial
        for name in ("reversed", "descending_ids", "fsum", "tree"):
            assert C.pair_sum(e, ids, C.WRONG[name][0])[0] == s or len(ids) % 2 == 1, (case, name)
        assert N <= 64 or len({u // 64 for u in ids}) > 1
        got.add((rc, len(ids)))
        check_others(e)
    assert got == {(rc, c) for rc in C.RCS for c in C.DIVISION_COUNTS[rc] if c <= N}


@SIZES
def test_toy_offlane_and_design_envs_decide_as_built(N):
    lay = C.layout(N)
    envs = lay["envs"]
    toy = cases_of(envs, "toy")
    want = {"extremes-%d" % (N // 3): {"equal": 1, "inside": 0}, "extremes-0": {"equal": 1, "inside": 0},
            "shared": {"equal": 1}, "point": {"equal": 1, "moved": 0}, "lanes-01": {"": 0}, "lanes-10": {"": 0}, "lanes-same": {"": 1}}
    assert set(toy) == set(want)
    for case, es in toy.items():
        for e in es:
            assert e["toy"] and C.weight(e, e["ids"]) == want[case][e["role"]], (case, e["role"])
            assert e["offlane"] == case.startswith("lanes")
    for case in ("shared", "lanes-01", "lanes-10", "lanes-same"):   # both extremes held twice, the later holders collide
        e = toy[case][0]
        lo, hi = min(e["x"]), max(e["x"])
        assert [u for u in range(N) if e["x"][u] == lo] == [0, e["ids"][0]] and [u for u in range(N) if e["x"][u] == hi] == [1, e["ids"][1]]
    e, moved = toy["point"]
    assert len(set(e["x"])) == 1 and len(e["ids"]) == 3 and sum(a != b for a, b in zip(e["x"], moved["x"])) == 1
    assert C.my_step_rewards(e, 1)[e["ids"][0]] == -1 * (1 - 1 / 3) and C.my_step_rewards(moved, 1)[e["ids"][0]] == -1.0
    # off-lane
    off = cases_of(envs, "offlane")
    for case, es in off.items():
        if case.startswith("triple"):
            (e,) = es
            assert C.mean_distance(e, e["ids"]) == e["rc"] and C.weight(e, e["ids"]) == 0 and set(e["y"]) == {0.0, 60.0}
            assert sorted(C.dist(e, a, b) for a, b in C.pairs_ascending(e["ids"])) == [156.0, 229.0, 365.0]
        else:
            check_tuned(es, "offlane")
        for e in es:
            check_others(e)
    assert sum(c.startswith("triple") for c in off) == 2 or lay["offlane_dropped"] > 0
    assert {len(es[0]["ids"]) for es in off.values()} >= {2, 3, 4, 5, 8}
    # the condition on the construction: at most 1 % of the off-lane cases decide differently under `** 2`
    print("N = %d: %d off-lane cases, %d dropped because pow() squares decide them differently" % (N, lay["offlane_cases"], lay["offlane_dropped"]))
    assert lay["offlane_dropped"] <= C.MAX_DROPPED * lay["offlane_cases"]
    assert len(off) == lay["offlane_cases"] - lay["offlane_dropped"]
    # design step
    des = cases_of(envs, "design")
    assert len(des) == 4
    for case, es in des.items():
        rc = es[0]["rc"]
        for e in es:
            ids = e["ids"]
            r = C.design_rewards(e)
            if case.startswith("pair"):
                d = C.dist(e, *ids)
                assert C.bits(d) - C.bits(2.0 * rc) == {"exact": 0, "inside": -1, "outside": 1}[e["role"]]
                assert [r[u] for u in ids] == ([-2.0, -2.0] if e["role"] == "inside" else [1.0, 1.0])
            else:
                a, b, c = ids
                assert C.dist(e, a, b) == 2.0 * rc and C.bits(C.dist(e, b, c)) == C.bits(2.0 * rc) - 1 and C.dist(e, a, c) < 1e-9
                assert [r[u] for u in ids] == [-2.0, -2.0, -3.0]
            check_others(e)
    assert {es[0]["rc"] for es in des.values()} == {250.0, 249.7}


@SIZES
def test_oracle_returns_the_statement_bit_for_bit(N):
    from oracle.oracle import SQ_IEEE, SQ_POW
    for key, g in C.groups(N).items():
        for design, mode in C.MODES:
            want = C.host(N, key, design, mode)
            got = C.oracle_steps(N, key, design, mode, SQ_IEEE)[0]
            assert C.same_bits(got, want), (N, key, design, mode, np.argwhere(got != want)[:4])
            # SQ_POW: every env on one lane (sqrt(pow(dx, 2)) is |dx| as well) and every off-lane env that was kept
            got = C.oracle_steps(N, key, design, mode, SQ_POW, steps=1)[0]
            assert C.same_bits(got, want), (N, key, design, mode, "SQ_POW", np.argwhere(got != want)[:4])
    assert sum(len(g["envs"]) for g in C.groups(N).values()) == len(C.layout(N)["envs"])


def flips(N, name):
    """{family: number of envs whose reward the wrong restatement changes} over the envs it applies to."""
    rules, families, needs3, wide_only, kind = C.WRONG[name]
    design, mode = (1, STEP_DESIGN) if kind == "design" else (1, STEP_MY_STEP)
    out = {}
    for e in C.layout(N)["envs"]:
        if e["family"] not in families or (needs3 and len(e["ids"]) < 3) or (wide_only and N <= 64):
            continue
        out.setdefault(e["family"], 0)
        out[e["family"]] += C.rewards(e, design, mode) != C.rewards(e, design, mode, rules)
    return out


@SIZES
@pytest.mark.parametrize("name", sorted(C.WRONG))
def test_wrong_restatement_is_told_apart(name, N):
    got = flips(N, name)
    print("%s at N = %d: rewards changed in %s" % (name, N, got))
    if name == "word_major" and N <= 64:
        assert got == {}
        return
    assert got and all(v > 0 for v in got.values()), (name, N, got)


def test_what_cannot_be_told_apart():
    """The cases of the module docstring, shown."""
    for N in (64, 128):
        for e in C.layout(N)["envs"]:
            if e["family"] == "order" and len(e["ids"]) == 2:
                for name in ("reversed", "descending_ids", "word_major", "fsum", "tree"):
                    assert C.my_step_rewards(e, 1, C.WRONG[name][0]) == C.my_step_rewards(e, 1)
            if e["family"] == "order" and (len(e["ids"]) == 3 or N <= 64):
                name = "tree" if len(e["ids"]) == 3 else "word_major"
                assert C.my_step_rewards(e, 1, C.WRONG[name][0]) == C.my_step_rewards(e, 1)
            if e["family"] == "toy" and not e["offlane"]:
                assert C.my_step_rewards(e, 1, C.WRONG["last_index"][0]) == C.my_step_rewards(e, 1)
