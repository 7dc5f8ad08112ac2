"""Inputs and plain NumPy expectations for the edge sweeps of the two secondary observation modes (no GPU needed):

* a15, the type-1 weighted histogram (State.add_positional_dist_type == 1, network.py:432-471): imported tables whose
  scaled distances sit exactly on / one ulp around every edge of np.linspace(-1, 1, K + 1), several values per edge,
  +-0 and subnormals, viewers with nothing valid, envs whose norm is 0, never-heard entries;
* a16, the sorted true distances (State.add_positional_dist, network.py:409-430): positions with exact ties across the
  x ranking, both extremes equally far, everybody on one point.

tests/test_posdist_cases.py keeps the generators honest against the oracle; tests/test_gpu_posdist_edges.py runs them
through the HIP kernels of csrc/posdist_kernel.hpp."""
import functools

import numpy as np

from diral_amd.config import bench_config

A = 4
AGE_LIMIT = 20                                   # an entry of age >= 20 is not used (dist_piggy, network.py:538-558)

# ---- a15 ----------------------------------------------------------------------------------------------------------
A15_L, A15_V, A15_B = 100000.0, 1.0, 3           # x = L - v: the post-move x is exactly 0, a table distance is the xpos itself
ANCHOR = 1024.0                                  # the norm of every anchored viewer: scaling by it is exact
T0 = 50                                          # every subject's own sequence number at the import
LAGS = (1, 2, 3, 4, 5, 6, 9, 14)                 # behind T0; one more after the slot's stamp: coded entries (2..6), the hand-over
NL = len(LAGS)                                   # to the plane (7), and entries beyond the ring (10, 15)
ANCHOR_SLOT, EDGE_SLOT = 0, 1                    # lag slot 0: +-ANCHOR, age 0; lag slot 1: exactly on an interior edge, valid

# (K, N, ylane, ghosts, degenerate, DIRAL_TABLE_FORM or None): the smallest shapes that reach every implementation of
# posdist_kernel.hpp and every form of the table it reads
A15_CASES = [
    (1, 64, 0.0, False, False, None),            # posdist_type1_n64_kernel; no interior edge
    (2, 6, 0.0, False, True, None),              # ... masked lanes; some viewers unanchored: the scale is no power of two
    (7, 64, 0.0, False, True, None),             # ... edges that are not exact
    (20, 40, 0.0, True, False, None),
    (64, 64, 1.0, True, True, None),             # ... off y = 0: a never-heard entry's sequence number decides its distance
    (33, 65, 0.0, False, True, None),            # posdist_type1_lanes_kernel<4, 32>, the plane form of step_wide
    (10, 128, 0.0, True, False, None),           # ... every lane full
    (20, 130, 1.0, True, False, None),           # posdist_type1_lanes_kernel<8, 32>, off y = 0 (the step is the general kernel's)
    (20, 200, 0.0, False, True, "plane"),
    (20, 200, 0.0, False, True, "packed"),       # (communication_range 0: the density rule alone would always pick the plane)
    (64, 256, 0.0, False, False, "plane"),
    (64, 256, 0.0, False, False, "packed"),
    (20, 257, 0.0, False, True, None),           # posdist_kernel, the literal statement: N > 256
    (12, 300, 1.0, True, False, None),
    (65, 40, 0.0, False, True, None),            # ... K > 64
    (300, 100, 0.0, True, False, None),
]


def a15_id(case):
    K, N, ylane, ghosts, degenerate, form = case
    return "K%d-N%d%s%s%s%s" % (K, N, "-y1" if ylane else "", "-ghosts" if ghosts else "", "-degenerate" if degenerate else "",
                                "-" + form if form else "")


def a15_config(K, N):
    return bench_config(N, A, A15_L, communication_range=0.0, State=dict(add_positional_dist_type=1, num_bins=K))


def a15_candidates(K, rng, count):
    """`count` xpos values in [-ANCHOR, ANCHOR]: every edge of linspace(-1, 1, K + 1) times ANCHOR and its two neighbours
    first, then +-0 and values whose square underflows, then walks of 0-3 ulps around random edges (duplicates intended:
    several values on one edge is a case) and some uniform values."""
    edges = np.linspace(-1.0, 1.0, K + 1)
    c = []
    for e in edges:
        c += [s * ANCHOR for s in (e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)) if abs(s) <= 1.0]
    c += [0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300]
    while len(c) < count:
        if rng.random() < 0.75:
            s = edges[rng.integers(0, K + 1)]
            for _ in range(int(rng.integers(0, 4))):
                s = np.nextafter(s, np.inf if rng.random() < 0.5 else -np.inf)
            c.append(min(max(s, -1.0), 1.0) * ANCHOR)
        else:
            c.append(rng.uniform(-ANCHOR, ANCHOR))
    return np.array(c[:count])


@functools.lru_cache(maxsize=None)
def a15_tables(K, N, ylane=0.0, ghosts=False, degenerate=False):
    """The import of one case: dict(seq, age, x [B][viewer][subject], pos_x, pos_y, vel [B][N], acts, empty_viewer,
    degenerate_env).  Entries about one subject with equal sequence numbers carry equal xpos (the import contract of
    include/diral_env.h): a subject has NL values, one per lag, and viewer u holds lag slot (u + k) % NL about subject k.
    Never-heard entries (`ghosts`) are what a fresh table holds: sequence number 0, xpos 0."""
    B = A15_B
    rng = np.random.default_rng(150000 + K * 1000 + N + (7 if ylane else 0) + (11 if ghosts else 0) + (13 if degenerate else 0))
    edges = np.linspace(-1.0, 1.0, K + 1)
    pool = a15_candidates(K, rng, B * N * NL)
    pool = np.stack([rng.permutation(pool[b * N * NL:(b + 1) * N * NL]).reshape(N, NL) for b in range(B)])   # [B][subject][lag slot]
    pool[:, :, ANCHOR_SLOT] = np.where(rng.random((B, N)) < 0.5, ANCHOR, -ANCHOR)
    if K >= 2:
        pool[:, :, EDGE_SLOT] = edges[rng.integers(1, K, size=(B, N))] * ANCHOR
    deg_env = B - 1 if degenerate else -1
    if degenerate:                                   # every distance 0 (the square of a subnormal underflows): norm 0
        pool[deg_env] = rng.choice(np.array([0.0, -0.0, 5e-324, -5e-324]), size=(N, NL))
    uu, kk = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")   # [viewer][subject]
    slot = (uu + kk) % NL
    x = np.stack([pool[b][kk, slot] for b in range(B)])
    seq = np.broadcast_to((T0 - np.array(LAGS))[slot].astype(np.int32), (B, N, N)).copy()
    age = rng.integers(0, AGE_LIMIT, size=(B, N, N)).astype(np.int32)      # 19 -> 20 under the stamp: invalid
    age[:, slot == ANCHOR_SLOT] = 0
    age[:, slot == EDGE_SLOT] = np.minimum(age[:, slot == EDGE_SLOT], AGE_LIMIT - 2)
    empty_viewer = N // 2                            # of env 0: nothing valid after the stamp, the reference returns zeros
    age[0, empty_viewer, :] = AGE_LIMIT - 1
    if ghosts:
        # 10 % of all entries, none of them in the anchor or the edge slot; the even viewers of the degenerate env keep
        # none either (off y = 0 a ghost is at distance 1: those viewers keep the norm 0)
        g = (rng.random((B, N, N)) < 0.1 * NL / (NL - 2)) & (slot >= 2)[None]
        if degenerate:
            g[deg_env, 0::2, :] = False
        seq[g], x[g] = 0, 0.0
    for u in range(N):                               # own entries: what a run would hold
        x[:, u, u], age[:, u, u], seq[:, u, u] = A15_L - A15_V, 0, T0
    return dict(K=K, N=N, B=B, ylane=ylane, edges=edges, seq=seq, age=age, x=x,
                pos_x=np.full((B, N), A15_L - A15_V), pos_y=np.full((B, N), ylane), vel=np.full((B, N), A15_V),
                acts=rng.integers(0, A, size=(B, N)).astype(np.int32), empty_viewer=empty_viewer, degenerate_env=deg_env)


def a15_entry_y(t):
    """The ypos the oracle's import takes: the subject's lane once heard, 0 in a fresh table."""
    return np.where(t["seq"] > 0, t["ylane"], 0.0)


def a15_scaled(t, b, u, stamped=True):
    """Viewer u of env b at x = 0: (s, norm) - the sorted signed distances of its valid entries over their inf-norm
    (NaN where the norm is 0) - or (None, None) when nothing is valid.  `stamped`: one my_step aged every entry by one."""
    age = t["age"][b, u] + (1 if stamped else 0)
    ok = age < AGE_LIMIT
    ok[u] = False
    if not ok.any():
        return None, None
    dx = t["x"][b, u, ok] - 0.0
    dy = np.where(t["seq"][b, u, ok] > 0, t["ylane"], 0.0) - t["ylane"]
    d = np.sqrt(dx * dx + dy * dy)                   # Network.dist (network.py:318-332): tiny dx underflow to 0
    v = np.where(dx > 0, d, -d)                      # dist_piggy's sign: + iff x1 - x2 > 0 (network.py:552-556)
    norm = np.linalg.norm(v, np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sort(v) / norm, norm


def hist_numpy(s, edges):
    return np.histogram(s, edges, weights=s)[0]


def _hist_from_counts(s, idx):
    cw = np.concatenate(([0.0], np.cumsum(s)))       # NumPy's own path for explicit edges + weights (_histograms_impl.py)
    return np.diff(cw[idx])


def hist_interior_right(s, edges):
    """WRONG on purpose: every edge but the last searched 'right' - a value on an edge falls into the bin below."""
    return _hist_from_counts(s, np.concatenate((np.searchsorted(s, edges[:-1], "right"), np.searchsorted(s, edges[-1:], "right"))))


def hist_last_left(s, edges):
    """WRONG on purpose: the last edge searched 'left' like the others - s == 1 falls into no bin."""
    return _hist_from_counts(s, np.searchsorted(s, edges, "left"))


def hist_uncorrected_estimate(s, edges):
    """WRONG on purpose: the bin taken from clip(int((s + 1) * K / 2), 0, K - 1) without the step against the real edges."""
    K = len(edges) - 1
    est = np.clip(((s + 1.0) * (0.5 * K)).astype(np.int64), 0, K - 1)
    return _hist_from_counts(s, np.searchsorted(est, np.arange(K + 1), "left"))


def a15_expected(t, stamped=True, hist=hist_numpy):
    """[B][N][K]: `hist` of every viewer's scaled distances; zeros when nothing is valid (network.py:432-471).  A norm of
    0 goes through np.histogram as it is - the NaNs fall into no bin -; the wrong restatements take finite values only."""
    out = np.zeros((t["B"], t["N"], t["K"]))
    for b in range(t["B"]):
        for u in range(t["N"]):
            s, norm = a15_scaled(t, b, u, stamped)
            if s is not None and (hist is hist_numpy or norm > 0):
                out[b, u] = hist(s, t["edges"])
    return out


# ---- a16 ----------------------------------------------------------------------------------------------------------
A16_L, A16_V, A16_B = 1000.0, 1.0, 6
A16_CASES = [(N, lanes) for N in (2, 5, 64, 65, 200, 256, 300) for lanes in (False, True)]
ONE_POINT_ENV = 1


def a16_config(N):
    return bench_config(N, A, A16_L, State=dict(add_positional_dist=True))


@functools.lru_cache(maxsize=None)
def a16_positions(N, lanes=False):
    """dict(x0, y0, v0 [B][N], acts): integer-valued x, one speed - every difference of two positions is exact and ties
    are exact ties.  `lanes`: y drawn from {0, 1.5} (a16 then runs on the literal kernel); the env with everybody on one
    point keeps one lane, so that its norm is 0 there too."""
    B, L = A16_B, int(A16_L)
    rng = np.random.default_rng(160000 + N * 2 + int(lanes))
    x = np.empty((B, N))
    nc = min(8, max(1, N // 2))                                                               # eight clusters of equal x (N // 2 below 16)
    x[0] = rng.choice(np.arange(5, L - 5), size=nc, replace=False)[np.arange(N) % nc]
    x[ONE_POINT_ENV] = 417.0                                                                  # everybody at one point: norm 0
    x[2] = np.array([250.0, 700.0])[rng.permutation(np.arange(N) % 2)]                       # two points only
    x[3] = rng.integers(0, L, size=N)                                                         # random, with both ends taken
    x[3, 0], x[3, -1] = 0.0, L - 2.0
    x[4] = rng.integers(L - 12, L - 2, size=N)                                                # a dense tail of ties ...
    x[4, :2] = L - 1.0                                                                        # ... beside two that wrap to 0
    x[5] = 500.0 - N // 2 + np.arange(N)                                                      # consecutive integers around 500,
    x[5, 0] = x[5, -1] = 500.0                                                                # two of them on 500
    y = np.zeros((B, N))
    if lanes:
        y = rng.choice(np.array([0.0, 1.5]), size=(B, N))
        y[:, 0], y[:, -1] = 0.0, 1.5                 # (both lanes in every env, whatever N)
        y[ONE_POINT_ENV] = 1.5
    return dict(N=N, B=B, x0=x, y0=y, v0=np.full((B, N), A16_V), acts=rng.integers(0, A, size=(B, N)).astype(np.int32))


def a16_expected(p):
    """[B][N][N - 1]: sorted(d * sign) / max(d) over the other vehicles at the post-move positions (network.py:409-430,
    dist_sign :334-349); NaN where every distance is 0."""
    B, N = p["B"], p["N"]
    x = (p["x0"] + p["v0"] + A16_L) % A16_L
    out = np.empty((B, N, N - 1))
    for b in range(B):
        for u in range(N):
            o = np.arange(N) != u
            dx, dy = x[b, o] - x[b, u], p["y0"][b, o] - p["y0"][b, u]
            d = np.sqrt(dx * dx + dy * dy)
            with np.errstate(invalid="ignore", divide="ignore"):
                out[b, u] = np.array(sorted(d * np.where(dx > 0, 1.0, -1.0))) / d.max()
    return out


# ---- the oracle's side, computed once per case and shared by the CPU and the GPU tests ------------------------------
def foreign_args(cfg, B, seed):
    """Arguments of a stand-alone obtain_state that no step produced: (actions, channel observation, rewards)."""
    rng = np.random.default_rng(seed)
    N = cfg.num_users
    return (rng.integers(0, A, size=(B, N)).astype(np.int32), rng.uniform(0.0, 300.0, size=(B, N, cfg.chobs_width)),
            rng.uniform(-3.0, 1.0, size=(B, N)))


FOREIGN_EPISODE, FOREIGN_EPS = 3.0, 0.25


@functools.lru_cache(maxsize=None)
def a15_oracle(K, N, ylane=0.0, ghosts=False, degenerate=False):
    """dict(rew, state: one my_step on the imported tables; foreign: a stand-alone obtain_state behind it; pos_x: where
    the step left the vehicles; observed: obtain_state of vehicles at x = 0 on the tables as imported, no step)."""
    from diral_amd.config import STEP_MY_STEP
    from oracle.oracle import SQ_IEEE, Oracle
    t, cfg = a15_tables(K, N, ylane, ghosts, degenerate), a15_config(K, N)
    fa, fc, fr = foreign_args(cfg, t["B"], 1500 + K + N)
    tabs = dict(seq=t["seq"], age=t["age"], x=t["x"], y=a15_entry_y(t))
    orc = Oracle(cfg, batch=t["B"], sq_mode=SQ_IEEE, threads=4)
    orc.reset(t["pos_x"], t["pos_y"], t["vel"])
    orc.import_state(**tabs)
    rew, chobs = orc.step(STEP_MY_STEP, t["acts"], 0)
    out = dict(rew=rew, state=orc.obtain_state(t["acts"], chobs, rew),
               foreign=orc.obtain_state(fa, fc, fr, FOREIGN_EPISODE, FOREIGN_EPS), pos_x=orc.export()["pos_x"])
    still = Oracle(cfg, batch=t["B"], sq_mode=SQ_IEEE, threads=4)
    still.reset(np.zeros_like(t["pos_x"]), t["pos_y"], t["vel"])
    still.import_state(**tabs)
    out["observed"] = still.obtain_state(fa, fc, fr, FOREIGN_EPISODE, FOREIGN_EPS)
    return out


@functools.lru_cache(maxsize=None)
def a16_oracle(N, lanes=False):
    """dict(rew, state: one my_step from the case's positions; foreign: a stand-alone obtain_state behind it)."""
    from diral_amd.config import STEP_MY_STEP
    from oracle.oracle import SQ_IEEE, Oracle
    p, cfg = a16_positions(N, lanes), a16_config(N)
    fa, fc, fr = foreign_args(cfg, p["B"], 1600 + N)
    orc = Oracle(cfg, batch=p["B"], sq_mode=SQ_IEEE, threads=4)
    orc.reset(p["x0"], p["y0"], p["v0"])
    rew, chobs = orc.step(STEP_MY_STEP, p["acts"], 0)
    return dict(rew=rew, state=orc.obtain_state(p["acts"], chobs, rew),
                foreign=orc.obtain_state(fa, fc, fr, FOREIGN_EPISODE, FOREIGN_EPS))
