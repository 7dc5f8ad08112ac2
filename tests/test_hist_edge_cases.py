"""What keeps tests/test_gpu_hist_edges.py honest, checked without a GPU: on every row of that sweep the oracle's
histogram equals the plain NumPy statement bit for bit (behind the first and the second step), the vehicles are where
the stamps were aimed from, the inputs hold what they are there for - values exactly on, one grid step below and one
above every interior edge, from own positions at and beyond L / 2 as well as from 0; the range ends; zeros and the
underflow values; every quad form in every env -, the float32 model leaves its bin around every edge where the
screening is on, and five deliberately wrong restatements are each told apart from the right one."""
import numpy as np
import pytest

from tests import hist_edge_cases as H

ROWS = pytest.mark.parametrize("r", H.ROWS, ids=H.row_id)
DYADIC = {(10, 500.0), (20, 500.0), (40, 500.0), (64, 500.0)}      # every edge a float64 with a handful of mantissa bits
# interior edges a value can sit on EXACTLY, per (K, rb).  Dyadic edges: all K - 1, from every position that reaches them
# (npx + e is exact).  The others (e has a full mantissa, npx + e rounds, and x - npx moves on the coarser grid): only
# from the position 0, the edges e > 0 - nine of (20, 123.456) beside its edge 0, three of (7, 250), 32 of (65, 500)
EXACT_EDGES = {(10, 500.0): 9, (20, 500.0): 19, (40, 500.0): 39, (64, 500.0): 63, (20, 123.456): 10, (7, 250.0): 3,
               (65, 500.0): 32}


def near_edges(r, t):
    """(j, kind, v, keep) [B][viewer][subject]: the interior edge nearest to the entry's value and where the value lies:
    0 on it, -1 / +1 within one step of the stamp's grid below / above it, 9 elsewhere."""
    v, keep = H.counted(r, t)
    interior = t["edges"][1:-1]
    i = np.searchsorted(interior, v)
    lo, hi = np.clip(i - 1, 0, len(interior) - 1), np.clip(i, 0, len(interior) - 1)
    j = np.where(np.abs(v - interior[lo]) <= np.abs(interior[hi] - v), lo, hi)
    e = interior[j]
    g = np.spacing(np.abs(t["npx"][:, :, None] + e))
    kind = np.where(v == e, 0, np.where((v < e) & (e - v <= g), -1, np.where((v > e) & (v - e <= g), 1, 9)))
    return j, kind, v, keep


@ROWS
def test_oracle_equals_numpy_and_the_vehicles_are_where_the_stamps_aim(r):
    t, o = H.tables(r), H.oracle(r)
    assert np.array_equal(o["export1"]["pos_x"], t["npx"])                    # the stamps are built from exactly this value
    assert np.array_equal(o["export2"]["pos_x"], t["npx2"])
    want = H.expected(r, t)
    assert np.array_equal(o["state1"][:, :, -r.K:], want), np.argwhere(o["state1"][:, :, -r.K:] != want)[:5]
    assert np.array_equal(o["foreign"][:, :, -r.K:], want)
    assert np.array_equal(o["state2"][:, :, -r.K:], H.expected(r, t, slot=2))
    assert want.any(axis=2).all()                                              # every viewer counts something


@ROWS
def test_tables_hold_what_they_are_there_for(r):
    """Conditions, not measurements."""
    t = H.tables(r)
    K, rb, L, N = r.K, r.rb, r.L, r.N
    interior = t["edges"][1:-1]
    j, kind, v, keep = near_edges(r, t)
    dx, dy, ok = H.values(r, t)
    ptype = np.broadcast_to(t["ptype"][:, :, None], keep.shape)
    cov = np.zeros((3, len(interior), H.NTYPES), bool)                         # [kind + 1][edge][position type]
    m = keep & (kind != 9)
    cov[kind[m] + 1, j[m], ptype[m]] = True
    high = cov[:, :, list(H.HIGH_TYPES)].sum(axis=2)
    # one step below and one above every interior edge: from two positions at or beyond L / 2, and from 0 where a stamp
    # in [0, L] can: e > 0 (just above the edge 0 a value from x == 0 underflows to 0 itself)
    assert (high[0] >= 2).all() and (high[2] >= 2).all(), (high[0], high[2])
    assert cov[0, interior > 0, 0].all() and cov[2, interior > 0, 0].all()
    # exactly on the edge, where it is reachable
    if (K, rb) in DYADIC:
        assert (high[1] >= 2).all(), high[1]
        assert (cov[1].any(axis=1)).sum() == EXACT_EDGES[(K, rb)] == K - 1
    assert cov[1, interior >= 0, 0].all()
    assert cov[1, interior >= 0, 0].sum() <= EXACT_EDGES[(K, rb)] <= cov[1].any(axis=1).sum()
    assert (t["npx"][t["ptype"] == 0] == 0).all() and (t["npx"][np.isin(t["ptype"], H.HIGH_TYPES)] >= L / 2).all()
    m32 = np.float32(t["npx"][t["ptype"] == 1]).astype(np.float64)            # ... and one loses half a float32 ulp
    assert (np.abs(m32 - t["npx"][t["ptype"] == 1]) == 0.5 * np.spacing(np.float32(t["npx"][t["ptype"] == 1]))).all()
    # the range ends: on them and not counted (the reference's d < Rb), one step inside and counted
    grb = np.spacing(np.abs(t["npx"][:, :, None] + np.where(v > 0, rb, -rb)))
    # (x - npx == -rb needs npx - rb to be a float64: with the positions of these cases that is so where rb is an integer)
    assert (ok & (v == rb) & ~keep).any() and ((ok & (v == -rb) & ~keep).any() or rb != int(rb))
    assert (keep & (v < rb) & (rb - v <= grb)).any() and (keep & (v > -rb) & (v + rb <= grb)).any()
    # v == 0 and the values whose square underflows: each of the three stamps dealt from the position 0 is there and counts
    assert (keep & (dx == 0)).any()
    for xx in H.UNDERFLOW_STAMPS:
        there = (t["x"] == xx) & (np.signbit(t["x"]) == np.signbit(xx)) & (t["npx"][:, :, None] == 0)
        assert (keep & there).any(), xx
    # every quad form holds counted values on an edge, one step below and one step above (so do the bodies the form runs)
    fq = np.stack([np.broadcast_to(t["form"][b][np.arange(N) // 4], (N, N)) for b in range(H.B)])   # [B][viewer][subject]
    for f, name in enumerate(H.FORMS):
        for kd in (0, -1, 1):
            assert (keep & (fq == f) & (kind == kd)).any(), (name, kd)
    # every quad form in every env, told from the tables themselves
    lag = np.where(t["seq"] > 0, H.T0 - t["seq"], -1)
    off = ~np.eye(N, dtype=bool)
    for b in range(H.B):
        seen = set()
        for q in range((N + 3) // 4):
            cols = slice(4 * q, min(4 * q + 4, N))
            lg, ag = lag[b][:, cols][off[:, cols]], t["age"][b][:, cols][off[:, cols]]
            ghost = lg < 0
            if not ghost.any() and lg.max() <= 5:
                seen.add("fast")
            elif not ghost.any() and lg.max() == 6:
                seen.add("handover")
            elif not ghost.any() and lg.max() == 9:
                seen.add("beyond")
            elif ghost.any() and ag[ghost].max() <= H.AGE_LIMIT - 2 and (ag[ghost] == H.AGE_LIMIT - 2).any():
                seen.add("ghost")
            elif ghost.any() and ag[ghost].min() >= H.AGE_LIMIT - 1 and (ag[ghost] == H.AGE_LIMIT - 1).any():
                seen.add("oldghost")
        assert seen == set(H.FORMS), (b, seen)
        heard_ages = t["age"][b][off & (t["seq"][b] > 0)]
        assert (heard_ages == H.AGE_LIMIT - 2).any() and (heard_ages == H.AGE_LIMIT - 1).any()   # ages straddle the limit - 1
    # young never-heard entries carry aimed values that count
    assert (keep & (t["seq"] == 0) & (kind != 9)).any()
    assert (keep & t["filler"]).sum() <= 0.5 * keep.sum()
    if r.lanes == 2:
        assert (dy != 0).any() and (keep & (dy != 0)).any()
        if (K, rb) in ((10, 500.0), (20, 500.0)):                             # 3-4-5: exactly on the edges +-100
            assert (keep & (dy != 0) & (dx == 80.0) & (v == 100.0)).any() and (keep & (dy != 0) & (dx == -80.0) & (v == -100.0)).any()
        # ... and one step below and one above every edge beyond the lane distance (no stamp brings +-sqrt(dx^2 + 60^2)
        # nearer to 0 than 60), from the stamps searched around dx = +-sqrt(e^2 - 60^2)
        beyond = np.flatnonzero(np.abs(interior) > H.LANE_Y)
        for kd in (-1, 1):
            assert np.array_equal(np.unique(j[keep & (dy != 0) & (kind == kd)]), beyond), (kd, beyond)
    else:
        assert (dy == 0).all()


@pytest.mark.parametrize("r", [r for r in H.ROWS if H.screening_on(r)], ids=H.row_id)
def test_the_float32_model_leaves_its_bin_around_every_edge_where_the_screening_is_on(r):
    """Existence only: the inputs reach into the band the kernel must hand to float64 - around every interior edge, and
    inside the fast quads, the only ones that are screened.  Whether the host's band is wide enough is for the GPU test
    to decide."""
    t = H.tables(r)
    j, kind, v, keep = near_edges(r, t)
    t16 = H.f32_model_t16(r, t["x"], t["npx"][:, :, None])
    wrong = keep & (kind != 9) & ((t16 >> 16) != H.true_bins(r, v))
    assert np.array_equal(np.unique(j[wrong]), np.arange(r.K - 1)), np.setdiff1d(np.arange(r.K - 1), j[wrong])
    fast = np.stack([np.broadcast_to(t["form"][b][np.arange(r.N) // 4] == H.FORMS.index("fast"), (r.N, r.N)) for b in range(H.B)])
    assert (wrong & fast).any()


@ROWS
def test_wrong_restatements_are_caught(r):
    """Each of them changes at least one viewer's row (the float32 model: on the one-lane rows, where it is defined)."""
    t = H.tables(r)
    want = H.expected(r, t)

    def rows_changed(got):
        return int((got != want).any(axis=2).sum())
    assert rows_changed(H.wrong_floor_estimate(r, t)) >= 1
    assert rows_changed(H.wrong_right_closed(r, t)) >= 1
    assert rows_changed(H.wrong_closed_range(r, t)) >= 1
    assert rows_changed(H.wrong_own_at_zero(r, t)) >= 1
    if r.lanes == 1:
        assert rows_changed(H.wrong_f32_no_band(r, t)) >= 1
