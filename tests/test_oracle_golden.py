"""Pin the CPU oracle (oracle/diral_oracle.c) to the reference.

Every fixture under tests/golden/ was recorded from the real reference
(tests/golden/gen_golden.py).  The oracle in its reference-faithful mode
(sq_mode=SQ_POW) must reproduce every recorded output BIT FOR BIT: rewards,
channel observations, state vectors, positions, velocities, neighbour-table
planes, arrival stamps and the information-age histogram.
"""
import numpy as np
import pytest

from oracle.oracle import Oracle, SQ_IEEE, SQ_POW
from tests.golden_util import Golden, compare_with_reference, golden_names, replay, ulp_diff


@pytest.mark.parametrize("name", golden_names())
def test_oracle_reproduces_reference_bit_exact(name):
    g = Golden(name)
    o = compare_with_reference(g)
    if g.cfg.State.piggybacking:
        # TestEnv.prev_obs after the last slot (test_env.py:260-261)
        assert np.array_equal(o.prev_obs()[0], g["prev_obs"])
        if "keyerror_actions" in g.d.files:
            # the slot the reference left with KeyError (`self.prev_obs[None]`, test_env.py:243)
            with pytest.raises(KeyError):
                o.step(0, g["keyerror_actions"], int(g["keyerror_t"]))


@pytest.mark.parametrize("name", ["g4_c2_step", "g4_c2_ch", "g4_c2_vary_rd1", "g6_c5_vary",
                                  "g5_c3_step", "g8_n70_a5", "g3_design6_rc100"])
def test_ieee_square_mode_matches_on_indices(name):
    """sq_mode=SQ_IEEE (x*x, what the GPU computes) vs the reference-faithful
    pow(): every integer/index output identical, distances within 1 ulp."""
    g = Golden(name)
    _, a = replay(g, SQ_POW)
    _, b = replay(g, SQ_IEEE)
    for i in range(g.T):
        assert np.array_equal(a["state"][i], b["state"][i]) or \
            ulp_diff(a["state"][i], b["state"][i]) <= 1
        # histogram sections / one-hot are index work: exactly equal
        K = g.cfg.State.num_bins
        if g.cfg.State.add_positional_dist_piggy and not g.cfg.State.add_reward:
            assert np.array_equal(a["state"][i][..., -K:], b["state"][i][..., -K:])
        assert ulp_diff(a["chobs"][i], b["chobs"][i]) <= 1
        assert ulp_diff(a["rews"][i], b["rews"][i]) <= 1
        assert np.array_equal(a["pos_x"][i], b["pos_x"][i])
        ea, eb = a["exp"][i], b["exp"][i]
        for k in ("seq", "age", "x", "y", "la"):
            assert np.array_equal(ea[k], eb[k]), (k, i)


def test_batch_envs_are_independent():
    """B copies of the same env give B identical results (batch plumbing)."""
    g = Golden("g8_n5_a9_ch")
    _, one = replay(g, SQ_POW, batch=1)
    _, many = replay(g, SQ_POW, batch=3)
    for i in range(g.T):
        for b in range(3):
            assert np.array_equal(many["state"][i][b], one["state"][i][0])
            assert np.array_equal(many["rews"][i][b], one["rews"][i][0])


def test_histogram_edges_match_numpy():
    from diral_amd.config import bench_config
    for K in (1, 7, 10, 20, 33, 40, 64):
        for rb in (500, 250, 123.456, 0.3):
            cfg = bench_config(8, 4, 100.0, bin_range=rb, State=dict(num_bins=K))
            e = Oracle(cfg).edges()
            ref = np.linspace(-rb, rb, K + 1)
            assert np.array_equal(e, ref), (K, rb)


def test_histogram_bin_edges_sweep():
    """G7: distances exactly on / 1 ulp around every bin edge, checked against
    NumPy itself (np.histogram is the third-party routine the reference calls at
    network.py:500)."""
    from diral_amd.config import bench_config
    for K, rb in ((10, 500), (20, 500), (40, 500), (20, 123.456), (7, 250.0)):
        N = 6
        cfg = bench_config(N, 4, 100000.0, bin_range=rb, State=dict(num_bins=K))
        edges = np.linspace(-rb, rb, K + 1)
        cand = []
        for ed in edges:
            cand += [ed, np.nextafter(ed, -np.inf), np.nextafter(ed, np.inf)]
        cand = [c for c in cand if abs(c) < rb and c != 0.0]
        own_x = 5000.0
        for start in range(0, len(cand), N - 1):
            chunk = cand[start:start + N - 1]
            o = Oracle(cfg)
            px = np.full(N, own_x)
            o.reset(px, np.zeros(N), np.ones(N))
            seq = np.zeros((1, N, N), np.int32)
            age = np.full((1, N, N), 99, np.int32)
            x = np.zeros((1, N, N))
            for j, c in enumerate(chunk):
                k = j + 1
                seq[0, 0, k] = 1
                age[0, 0, k] = 0
                x[0, 0, k] = own_x + c          # exact: |c| << 2**52 ulp(own_x)? checked below
            o.import_state(seq=seq, age=age, x=x, y=np.zeros((1, N, N)))
            st = o.obtain_state(np.zeros(N, np.int32), np.zeros((1, N, 4)), np.zeros((1, N)))
            hist = st[0, 0, -K:]
            vals = []
            for j, c in enumerate(chunk):
                dx = (own_x + c) - own_x
                d = np.sqrt(dx * dx)
                if d < rb:
                    vals.append(d * (1 if dx > 0 else -1))
            ref = np.histogram(sorted(vals), K, range=(-rb, rb))[0] / float(len(vals)) \
                if vals else np.zeros(K)
            assert np.array_equal(hist, ref), (K, rb, chunk)


def test_oracle_under_sanitizers():
    """the CPU restatement built with -fsanitize=address,undefined
    and driven through every step kind / reward design / observation mode."""
    import os
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    odir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
    subprocess.check_call(["make", "-C", odir, "san_check"], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(odir, "san_check")], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-3000:]
    assert "san_check ok" in out.stdout


def test_fixtures_carry_the_keys_the_generator_writes():
    """tests/golden/gen_golden.py and the committed .npz files stay in step: every env
    fixture has the full key set of run_case / run_driver_case, every SPS fixture that of
    run_sps_case (recorded from algorithms/v2x_sps.py)."""
    import glob
    import os
    gdir = os.path.join(os.path.dirname(__file__), "golden")
    case_keys = {"cfg", "x0", "y0", "v0", "modes", "actions", "tsteps", "vel_update_steps", "vel_update_draws",
                 "episode_eps", "state_space", "table_sha", "trace", "trace_after", "rews", "chobs", "state", "pos_x",
                 "vel", "ia", "tab_step", "tab_seq", "tab_age", "tab_x", "tab_y", "tab_la"}
    sps_keys = {"A", "threshold", "tie_step", "init_prev", "init_counter", "codes", "draw_counter", "draw_keep",
                "draw_choice", "actions", "counters", "prev_actions", "reselections"}
    names = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(gdir, "*.npz")))
    assert len([n for n in names if n[0] == "g"]) == 65 and len([n for n in names if n[0] == "s"]) == 7
    assert len([n for n in names if n[0] == "d"]) == 4
    for n in names:
        keys = set(np.load(os.path.join(gdir, n + ".npz")).files)
        if n[0] == "g":
            # State.piggybacking fixtures also hold TestEnv.prev_obs; the KeyError one the slot that raised
            more = {"prev_obs"} if "piggyback" in n else set()
            more |= {"keyerror_actions", "keyerror_t"} if n.endswith("keyerror") else set()
            # a thinned fixture (run_case(record_every=...)): the slots whose outputs it keeps, and every slot's hashes
            thinned = n in ("g11_sparse_n100", "g11_sparse_n200")
            more |= {"rec_step", "out_sha"} if thinned else set()
            assert keys == case_keys | more, (n, keys ^ (case_keys | more))
            g = np.load(os.path.join(gdir, n + ".npz"))
            T = len(g["modes"])
            assert g["table_sha"].shape == (T, 5)
            if thinned:
                rs = g["rec_step"]
                assert g["out_sha"].shape == (T, 6) and 1 < len(rs) < T and rs[0] == 0 and rs[-1] == T - 1
                assert all(len(g[k]) == len(rs) for k in ("rews", "chobs", "state", "pos_x", "vel", "ia"))
            else:
                assert all(len(g[k]) == T for k in ("rews", "chobs", "state", "pos_x", "vel", "ia"))
        elif n[0] == "s":
            assert keys == sps_keys, (n, keys ^ sps_keys)
            g = np.load(os.path.join(gdir, n + ".npz"))
            A = int(g["A"])
            assert g["actions"].min() >= 0 and g["actions"].max() < A and g["counters"].min() >= 0
            assert g["counters"].max() <= 16 and int(g["reselections"]) >= 40
            # a kept resource repeats the previous action (v2x_sps.py:85-96)
            same = g["actions"][1:] == g["prev_actions"][:-1]
            changed = g["prev_actions"][1:] != g["prev_actions"][:-1]
            assert np.all(same | changed)
