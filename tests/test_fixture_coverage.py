"""What the reference fixtures from g10 on (tests/golden/gen_golden.py `curated`, and the driver loops d3 / d4) must
cover, computed from the committed files: a cell that no fixture fills fails, so a deleted or regenerated-away fixture is
noticed.  Where a cell is about something that has to HAPPEN during the run (a highway that breaks apart and re-merges,
a wrap at the end of the highway, a table age past the device's byte, a proportional-fairness penalty), the recorded
data must show that it did.  CPU only; the reference is not needed."""
import json
import os

import numpy as np
import pytest

from tests.golden_util import GOLDEN_DIR, Golden, golden_names

RICH = ("add_reward", "add_index", "add_velocity", "add_position", "add_channel_obs")


def _new():
    return [Golden(n) for n in golden_names() if int(n[1:n.index("_")]) >= 10]


@pytest.fixture(scope="module")
def fx():
    return _new()


def _modes(g):
    return {str(m) for m in g["modes"]}


def _slots(g, mode):
    return int(np.sum(g["modes"] == mode))


def _wide(g):
    return 65 <= g.N <= 256


def _default_flags(g):
    st, c = g.cfg.State, g.cfg
    return (st.type == 2 and st.add_action and st.action_index == "binary" and st.add_positional_dist_piggy
            and st.add_positional_dist_type == 2 and not (st.add_reward or st.add_index or st.add_velocity
            or st.add_position or st.add_positional_dist or st.add_channel_obs)
            and c.mobility and not c.proportional_fair and not c.enable_fingerprint)


def _components(x, y, rc):
    """Connected components of the "closer than the communication range" graph (network.py:389, 604)."""
    n = len(x)
    adj = np.sqrt((x[:, None] - x[None, :]) ** 2 + (y[:, None] - y[None, :]) ** 2) < rc
    seen = np.zeros(n, bool)
    comps = 0
    for s in range(n):
        if seen[s]:
            continue
        comps += 1
        front = np.zeros(n, bool)
        front[s] = True
        while front.any():
            seen |= front
            front = adj[front].any(axis=0) & ~seen
    return comps


def _splits_and_merges(g):
    c = [_components(px, g["y0"], g.cfg.communication_range) for px in g["pos_x"]]
    d = np.diff(c)
    rises = np.flatnonzero(d > 0)
    return max(c) > 1 and len(rises) > 0 and bool(np.any(d[rises[0]:] < 0))


def _wraps(g):
    return bool(np.any(np.diff(g["pos_x"], axis=0) < 0))


@pytest.mark.parametrize("rd", [2, 3, 4])
def test_wide_ch_mode_every_reward_design(fx, rd):
    assert [g.name for g in fx if _wide(g) and g.cfg.reward_design == rd and _slots(g, "ch") >= 20]


def test_wide_design_mode(fx):
    assert [g.name for g in fx if _wide(g) and "design" in _modes(g)]


@pytest.mark.parametrize("rd", [1, 3, 4, 5])
def test_wide_step_mode_every_other_reward_design(fx, rd):
    assert [g.name for g in fx if _wide(g) and g.cfg.reward_design == rd and "step" in _modes(g)]


@pytest.mark.parametrize("lo,hi", [(1, 64), (65, 128), (129, 256)])
def test_sparse_highway_splits_and_remerges(fx, lo, hi):
    hit = [g for g in fx if lo <= g.N <= hi and g.T >= 150 and len(g.vel_updates) > 0
           and np.any(g["vel"][-1] != g["v0"]) and _wraps(g) and _splits_and_merges(g)]
    assert hit, (lo, hi)


def test_a_sparse_highway_runs_on_the_default_flags(fx):
    assert [g.name for g in fx if g.T >= 150 and _default_flags(g) and _wraps(g) and _splits_and_merges(g)]


def test_a_table_age_passes_255_before_the_last_readouts(fx):
    hit = []
    for g in fx:
        ck = g.table_checkpoints()
        over = [s for s, j in ck.items() if g["tab_age"][j].max() > 255]
        if not over or g.kept is not None:
            continue
        s = min(over)
        # after that checkpoint: an information-age readout that counts something, a histogram readout
        K = g.cfg.State.num_bins
        if s < g.T - 1 and g["ia"][s + 1:].sum() > 0 and g.cfg.State.add_positional_dist_piggy \
                and np.any(g["state"][s + 1:, :, -K:] != 0):
            hit.append(g.name)
    assert hit


@pytest.mark.parametrize("wide", [False, True])
def test_off_lane_vehicles(fx, wide):
    assert [g.name for g in fx if (g.N > 64) == wide and set(np.unique(g["y0"])) == {0.0, 1.0, 2.0}]


@pytest.mark.parametrize("mode", ["step", "ch"])
def test_more_than_64_resources(fx, mode):
    assert [g.name for g in fx if g.A > 64 and mode in _modes(g)]


def test_more_than_256_vehicles(fx):
    big = [g for g in fx if g.N > 256]
    assert {300, 512} <= {g.N for g in big}
    assert set().union(*[_modes(g) for g in big]) == {"step", "ch", "design"}


def test_rich_state_flags_beyond_64_vehicles(fx):
    rich = [g for g in fx if g.N > 64 and all(getattr(g.cfg.State, k) for k in RICH) and g.cfg.enable_fingerprint]
    assert len(rich) >= 2
    assert [g.name for g in rich if g.cfg.State.type == 1 and g.cfg.State.action_index == "real"]
    assert [g.name for g in rich if g.cfg.State.type == 2 and g.cfg.State.action_index == "binary"]


def test_secondary_observation_modes_at_64_vehicles_or_more(fx):
    assert [g.name for g in fx if g.N >= 64 and g.cfg.State.add_positional_dist]
    assert [g.name for g in fx if g.N >= 64 and g.cfg.State.add_positional_dist_piggy
            and g.cfg.State.add_positional_dist_type == 1]


def test_proportional_fairness_changes_the_recorded_rewards(fx):
    """test_env.py:215-222: the recorded rewards differ from what the same actions earn without proportional_fair
    (the oracle, which reproduces the fixture bit for bit with the flag on)."""
    from oracle.oracle import Oracle, SQ_POW
    hit = []
    for g in fx:
        if not (g.cfg.proportional_fair and g.N >= 32 and _slots(g, "step") >= 30):
            continue
        o = Oracle(g.cfg.replace(proportional_fair=False), sq_mode=SQ_POW)
        o.reset(g["x0"], g["y0"], g["v0"])
        plain = np.array([o.step(mode, acts, t)[0][0] for _, mode, acts, t, _ in g.steps()])
        paid = g["rews"] != plain
        if paid.any() and np.all(g["rews"][paid] == -10.0):
            hit.append(g.name)
    assert hit


def test_odd_histograms(fx):
    assert len([g for g in fx if g.cfg.bin_range != 500 and g.cfg.State.num_bins not in (10, 20, 40)
                and g.cfg.State.add_positional_dist_piggy]) >= 2


def test_static_topology(fx):
    assert [g.name for g in fx if g.N >= 32 and not g.cfg.mobility and g.cfg.enable_design_topology
            and np.all(g["pos_x"] == g["x0"])]


def test_congestion_test_weights_beyond_the_toy(fx):
    assert [g.name for g in fx if g.cfg.congestion_test and g.N > 4 and g.cfg.reward_design in (1, 2, 5)]


def test_trace_replay_beyond_64_vehicles(fx):
    assert [g.name for g in fx if g.N > 64 and g.trace is not None and 0 <= g.trace_after < g.T - 1]


def test_piggybacking_with_16_resources(fx):
    assert [g.name for g in fx if g.cfg.State.piggybacking and g.A >= 16]


def test_slot_numbers_start_late_and_jump_back(fx):
    assert [g.name for g in fx if g["tsteps"][0] >= 10 ** 6 and np.any(np.diff(g["tsteps"]) < 0)
            and np.any(np.diff(g["tsteps"]) > 1)]


def _driver(name):
    d = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    return d, json.loads(str(d["cfg"])), json.loads(str(d["opts"]))


def test_driver_loop_fixtures():
    d, cfg, o = _driver("d3_driver_ch_c2")
    assert (cfg["num_users"], cfg["num_channels"]) == (64, 32) and o["enable_channel"] and o["n_prefill"] >= 25
    assert int(d["episode"][-1]) >= 2 and not o["ia_averaging"]
    d, cfg, o = _driver("d4_driver_ch_n100")
    assert 65 <= cfg["num_users"] <= 256 and o["ia_averaging"] and o["ia_penalty_enable"]
    assert np.any(d["ia_pen"] != 0) and np.any(d["shaped_reward"] == o["ia_penalty_value"])


def test_new_fixtures_stay_small():
    sizes = {n: os.path.getsize(os.path.join(GOLDEN_DIR, n + ".npz")) for n in golden_names() + golden_names("d")}
    new = [v for n, v in sizes.items() if n[0] == "d" and n[1] in "34" or n[0] == "g" and int(n[1:n.index("_")]) >= 10]
    assert len(new) == 29 and max(new) <= 314507 and sum(new) < 5_000_000     # (314507: g6_c5_vary, the largest before)
