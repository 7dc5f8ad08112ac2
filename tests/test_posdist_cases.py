"""What keeps tests/test_gpu_posdist_edges.py honest, checked without a GPU: on every case of that sweep the oracle's
state equals the plain NumPy statement of the operation bit for bit, the inputs do hold what they are there for (norms
that are exactly the anchor, values exactly on interior edges, viewers with nothing valid, norms of 0, ties, NaN rows),
and three deliberately wrong restatements of the type-1 histogram are each told apart from the right one."""
import numpy as np
import pytest

from tests import posdist_cases as P


@pytest.mark.parametrize("case", P.A15_CASES, ids=P.a15_id)
def test_type1_histogram_oracle_equals_numpy_on_the_edge_tables(case):
    """posdist_piggy1 of the oracle against np.histogram(s, linspace(-1, 1, K + 1), weights=s) itself, every viewer:
    behind one my_step (ages stamped) and on the tables as imported."""
    K, N = case[:2]
    t, o = P.a15_tables(*case[:5]), P.a15_oracle(*case[:5])
    assert np.array_equal(o["pos_x"], np.zeros((t["B"], N)))                 # post-move x == 0: a table distance is the xpos itself
    want = P.a15_expected(t, stamped=True)
    assert np.array_equal(o["state"][:, :, -K:], want), np.argwhere(o["state"][:, :, -K:] != want)[:5]
    assert np.array_equal(o["foreign"][:, :, -K:], want)
    assert np.array_equal(o["observed"][:, :, -K:], P.a15_expected(t, stamped=False))
    assert not np.isnan(o["state"]).any() and not np.isnan(o["observed"]).any()


@pytest.mark.parametrize("case", P.A15_CASES, ids=P.a15_id)
def test_type1_histogram_tables_hold_what_they_are_there_for(case):
    """Conditions, not measurements.  The anchored viewers are those of a non-degenerate env other than the one viewer of
    env 0 whose entries were all aged out."""
    K, N, ylane, ghosts, degenerate, _ = case
    t = P.a15_tables(*case[:5])
    interior = t["edges"][1:-1]
    empty, zero_norm = 0, 0
    for b in range(t["B"]):
        for u in range(N):
            s, norm = P.a15_scaled(t, b, u, stamped=True)
            if s is None:
                empty += 1
                assert (b, u) == (0, t["empty_viewer"])
                continue
            zero_norm += norm == 0
            if b == t["degenerate_env"]:
                assert norm == 0 or (ghosts and ylane != 0 and norm == 1.0), (b, u, norm)
                continue
            if N >= 12:
                assert norm == P.ANCHOR, (b, u, norm)
                if K >= 2:
                    assert np.isin(s, interior).any(), (b, u)
    assert empty == 1
    if degenerate:
        assert zero_norm >= 1
    # the table forms one pass over the stamped table reads: coded entries, the hand-over at lag 7, entries beyond the ring
    off = ~np.eye(N, dtype=bool)
    lag_after = P.T0 + 1 - t["seq"][0][off & (t["seq"][0] > 0)]
    assert (lag_after < 7).any() and (lag_after == 7).any() and (lag_after > 8).any()
    if ghosts:
        assert (t["seq"][:, off] == 0).any()


@pytest.mark.parametrize("case", P.A15_CASES, ids=P.a15_id)
def test_wrong_restatements_of_the_type1_histogram_are_caught(case):
    """Each of them changes at least one viewer's row: the searches in every case, the uncorrected bin estimate wherever
    the edges are not exact (K >= 7 here; at K = 1 and 2 it cannot differ)."""
    K = case[0]
    t = P.a15_tables(*case[:5])
    want = P.a15_expected(t, stamped=True)

    def rows_changed(hist):
        return int((P.a15_expected(t, stamped=True, hist=hist) != want).any(axis=2).sum())
    assert rows_changed(P.hist_interior_right) >= 1
    assert rows_changed(P.hist_last_left) >= 1
    if K >= 7:
        assert rows_changed(P.hist_uncorrected_estimate) >= 1


@pytest.mark.parametrize("N,lanes", P.A16_CASES)
def test_sorted_distances_oracle_equals_numpy_and_the_positions_hold_ties(N, lanes):
    """posdist_full of the oracle against sorted(d * sign) / max(d), NaN rows in exactly the same places; at N >= 5 more
    than half the viewers see two vehicles at the same signed distance and one env has norm 0 throughout."""
    p, o = P.a16_positions(N, lanes), P.a16_oracle(N, lanes)
    want = P.a16_expected(p)
    for key in ("state", "foreign"):
        got = o[key][:, :, P.A:P.A + N - 1]
        assert np.array_equal(got, want, equal_nan=True), (key, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5])
    nan_rows = np.isnan(want).any(axis=2)
    assert np.array_equal(nan_rows, np.isnan(want).all(axis=2))               # a row is NaN throughout or nowhere
    if N >= 5:
        assert nan_rows[P.ONE_POINT_ENV].all()
        ties = sum(len(np.unique(row)) < N - 1 for row in want[~nan_rows])
        assert ties > 0.5 * p["B"] * N, ties
    assert lanes == bool((p["y0"] != 0).any())
