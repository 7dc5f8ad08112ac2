"""Inputs, a plain integer host model and correctly rounded references for the two places where the device's math library
decides a value: the exp() rewards (my_step reward_design 3: -exp(1 - 1/c); my_step_ch reward_design 3 / 4: 1 - exp(1 - R) /
-exp(1 - R) with R = received / in_range) and the log10 of the SPS window (-40 - 30 log10(max(d, 1))).  No GPU needed;
tests/test_libm_cases.py keeps the builders honest, tests/test_gpu_libm_edges.py runs them on every kernel path.

Both domains are small enough to sweep completely:

* reception ratios: one env per (k, n) = (received, in_range) of a marked transmitter (and two with a sole one).  A static one-lane highway
  (v = 0: the positions the reward reads are the ones given), Rc = 250, two resources.  The marked transmitter sits at
  x = 1000 and a second one at x = 1100, both on resource 0; everyone else transmits on resource 1.  k of the others sit
  at x <= 1050 - nearer to the marked transmitter, the first of them exactly on the midpoint 1050: a tie, which the lower
  id wins -, n - k in (1050, 1250) - in its range, nearer to the other -, the rest at x >= 1250, the first exactly at
  1250 = Rc away: out of range under the strict `<`.  Resource 1 then carries N - 2 colliding transmitters with the two
  receivers 0 and 1; what they are paid comes out of the host model.  A second variant gives the two transmitters the ids
  N - 2 and N - 1 with their positions swapped: the lower id sits on the other side of the tie;
* collision counts: one env per c = 0 ... N, the first c vehicles on resource 0 and the rest on resource 1, as a cluster
  (mean pair distance far below Rc) and as a spread (far above).

The host model (`host_pairs`) is integer counting over |dx| - on these positions (at most two fractional bits below 2^13)
sqrt(dx * dx) is |dx| exactly.  Correctly rounded values come from `decimal` at 60 digits, then float()."""
import decimal
import functools
import math

import numpy as np

from diral_amd.config import bench_config
from tests.golden_util import EXP_ATOL   # tests/test_gpu_parity.py: the project's bar for exp()-based rewards; no bound here exceeds it
ORACLE_EXP_ULPS = 1             # the oracle's exp() and the host's log10 against the correctly rounded values, in ulps: the
HOST_LOG10_ULPS = 1             # conditions tests/test_libm_cases.py asserts, which the device's bounds are derived from
RC = 250.0
X_MARKED, X_OTHER, X_MID, X_EDGE = 1000.0, 1100.0, 1050.0, 1250.0
CH_DESIGNS = (2, 3, 4)

_CTX = decimal.Context(prec=60)


# ---- correctly rounded references --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rn_exp(a):
    """RN(exp(a)): 60 decimal digits, rounded once more to the nearest float64."""
    return float(_CTX.exp(decimal.Decimal(float(a))))


@functools.lru_cache(maxsize=None)
def rn_log10(d):
    return float(_CTX.log10(decimal.Decimal(float(d))))


def mp_exp(a):
    import mpmath
    with mpmath.workprec(200):
        return float(mpmath.exp(mpmath.mpf(float(a))))


def mp_log10(d):
    import mpmath
    with mpmath.workprec(200):
        return float(mpmath.log10(mpmath.mpf(float(d))))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- the ratio layout ----------------------------------------------------------------------------------------------------
def subset_k(n):
    return sorted({0, 1, n // 3, n // 2, n - 1, n} & set(range(n + 1)))


def claimed_pairs(N):
    """The (received, in_range) pairs of the marked transmitter the sweep claims for a size: every pair at 64 and 33
    vehicles; every n with k in {0, 1, n // 3, n // 2, n - 1, n} at 128 and 256; the same with n <= 64 at 300."""
    if N in (64, 33):
        return [(k, n) for n in range(N - 1) for k in range(n + 1)]
    top = 64 if N == 300 else N - 2
    return [(k, n) for n in range(top + 1) for k in subset_k(n)]


RATIO_SIZES = (64, 33, 128, 256, 300)


def ratio_config(N, design, **kw):
    return bench_config(N, 2, 6000.0, reward_design=design, communication_range=RC, **kw)


@functools.lru_cache(maxsize=None)
def ratio_layout(N):
    """dict(x [B][N], acts [B][N], kn [B][2], swapped [B], marked [B]: the id of the transmitter at x = 1000).  The envs of
    the plain variant first, then the same pairs with the two transmitters at ids N - 2, N - 1 and swapped positions."""
    pairs = claimed_pairs(N)
    P = len(pairs)
    x, acts = np.empty((2 * P, N)), np.ones((2 * P, N), np.int32)
    for v in range(2):
        for e, (k, n) in enumerate(pairs):
            others = ([X_MID - 1.0 * j for j in range(k)] + [X_MID + 1.0 + 0.75 * j for j in range(n - k)]
                      + [X_EDGE + 10.0 * j for j in range(N - 2 - n)])
            assert len(others) == N - 2 and all(X_MARKED - RC < p for p in others[:n]) and all(p < X_EDGE for p in others[:n])
            row = [X_MARKED, X_OTHER] + others if v == 0 else others + [X_OTHER, X_MARKED]
            x[v * P + e] = row
            acts[v * P + e, [0, 1] if v == 0 else [N - 2, N - 1]] = 0
    assert x.max() < 6000.0
    # ... and one env per variant whose marked transmitter is alone on resource 0 (the other one moved to resource 1): a
    # sole transmitter is paid 1, or the exp(1.0) the compiler folded
    e12 = pairs.index((1, 2))
    xs, as_ = x[[e12, P + e12]].copy(), acts[[e12, P + e12]].copy()
    as_[0, 1] = as_[1, N - 2] = 1
    B = 2 * P + 2
    return dict(x=np.concatenate([x, xs]), acts=np.concatenate([acts, as_]), kn=np.array(pairs * 2 + [(1, 2)] * 2),
                swapped=(np.arange(B) >= P) & (np.arange(B) != 2 * P), marked=np.where((np.arange(B) >= P) & (np.arange(B) != 2 * P), N - 1, 0),
                sole=np.arange(B) >= 2 * P, P=P)


def host_pairs(x, acts, A, rc, tie_high=False, closed=False):
    """The integer host model: per transmitter (received, in_range) over the receivers of its resource - the vehicles that
    transmit elsewhere and are closer than rc (strict) -, a receiver counted as received by the nearest transmitter in its
    range, the first minimum in id order; and whether it shares its resource.  tie_high / closed: WRONG on purpose (the tie
    paid to the higher id; d <= rc)."""
    B, N = x.shape
    rec, inr, coll = np.zeros((B, N), np.int64), np.zeros((B, N), np.int64), np.zeros((B, N), bool)
    ids = np.arange(N)
    for s in range(0, B, 64):
        xs, a = x[s:s + 64], acts[s:s + 64]
        d = np.abs(xs[:, :, None] - xs[:, None, :])                        # [env][transmitter][receiver]
        near = (d <= rc) if closed else (d < rc)
        for i in range(A):
            tx = a == i
            ok = near & tx[:, :, None] & ~tx[:, None, :]
            dd = np.where(ok, d, np.inf)
            best = (N - 1 - np.argmin(dd[:, ::-1, :], axis=1)) if tie_high else np.argmin(dd, axis=1)
            won = ok & (ids[None, :, None] == best[:, None, :])
            inr[s:s + 64][tx] = ok.sum(2)[tx]
            rec[s:s + 64][tx] = won.sum(2)[tx]
            coll[s:s + 64] |= tx & (tx.sum(1, keepdims=True) > 1)
    return rec, inr, coll


def ratios(rec, inr, coll, empty_is=1.0):
    """R per transmitter: received / in_range as one float64 division, 1 with nobody in range and for a sole transmitter."""
    with np.errstate(divide="ignore", invalid="ignore"):
        R = np.where(inr > 0, rec.astype(np.float64) / inr.astype(np.float64), empty_is)
    return np.where(coll, R, 1.0)


@functools.lru_cache(maxsize=None)
def ratio_model(N):
    lay = ratio_layout(N)
    rec, inr, coll = host_pairs(lay["x"], lay["acts"], 2, RC)
    return dict(rec=rec, inr=inr, coll=coll, R=ratios(rec, inr, coll))


def exp_ulp_bound(E, minus_from_one, m):
    """The bound on a reward built on E = RN(exp(a)), E in [1, e]: (m + 1) ulps of E - m the oracle's measured worst error,
    one more because two libraries within an ulp may sit on opposite sides of the true value -, half an ulp of E more
    where `1 - E` rounds again (E > 2; below, the subtraction is exact); never beyond EXP_ATOL."""
    E = np.asarray(E, dtype=np.float64)
    u = np.spacing(E)
    return np.minimum((m + 1) * u + np.where(minus_from_one & (E > 2.0), 0.5 * u, 0.0), EXP_ATOL)


def ch_reference(design, R, coll, m=1):
    """(reference reward, bound, E) of my_step_ch from the ratios: design 2 `-1.0 * (1.0 - R)` (bound 0: bit for bit),
    3 `1.0 - RN(exp(1.0 - R))`, 4 `-RN(exp(1.0 - R))`; a sole transmitter 1, 1, RN(exp(1))."""
    R = np.asarray(R, dtype=np.float64)
    a = 1.0 - R
    if design == 2:
        return np.where(coll, -1.0 * a, 1.0), np.zeros(R.shape), np.ones(R.shape)
    E = np.vectorize(rn_exp, otypes=[np.float64])(a)
    e1 = rn_exp(1.0)
    if design == 3:
        return np.where(coll, 1.0 - E, 1.0), np.where(coll, exp_ulp_bound(E, True, m), 0.0), E
    return np.where(coll, -1.0 * E, e1), np.where(coll, exp_ulp_bound(E, False, m), exp_ulp_bound(e1, False, m)), np.where(coll, E, e1)


def exp_errors(design, got, ref, E):
    """Errors of exp()-based rewards in ulps of the correctly rounded E (one per element)."""
    return np.abs(np.asarray(got, np.float64) - ref) / np.spacing(E)


def reward_failures(design, got, ref, bound):
    """What the GPU and the CPU tests both call: indices where a float64 reward misses its reference - by bits where the
    bound is 0, else by the bound."""
    got = np.asarray(got, dtype=np.float64)
    exact = bound == 0.0
    bad = np.where(exact, bits(got) != bits(ref), ~(np.abs(got - ref) <= bound))
    return np.argwhere(bad)


def prr_sum_failures(got_sum, R, slots=1):
    """DIRAL_M_PRR_SUM of every env against the exact sum of its ratios over `slots` equal slots, within the bound of a
    float64 sum in any order: (terms - 1) * 2^-53 * sum |R|."""
    want = np.array([math.fsum(row.tolist() * slots) for row in R])
    terms = slots * R.shape[1]
    return np.argwhere(~(np.abs(np.asarray(got_sum) - want) <= (terms - 1) * 2.0 ** -53 * want))


@functools.lru_cache(maxsize=None)
def ratio_oracle(N, design):
    """One my_step_ch of the oracle on the layout: dict(rew [B][N], metrics [B][6])."""
    from diral_amd.config import STEP_MY_STEP_CH
    from oracle.oracle import SQ_IEEE, Oracle
    lay = ratio_layout(N)
    B = lay["x"].shape[0]
    orc = Oracle(ratio_config(N, design), batch=B, sq_mode=SQ_IEEE, threads=8)
    orc.reset(lay["x"], np.zeros((B, N)), np.zeros((B, N)))
    rew, _ = orc.step(STEP_MY_STEP_CH, lay["acts"], 0)
    return dict(rew=rew, metrics=orc.metrics())


# ---- collision counts --------------------------------------------------------------------------------------------------
COUNT_SIZES = (64, 33, 128, 256, 300)
MY_STEP_DESIGNS = (1, 2, 3, 4, 5)


def count_config(N, design, **kw):
    return bench_config(N, 2, 600.0 * N + 2000.0, reward_design=design, communication_range=RC, **kw)


@functools.lru_cache(maxsize=None)
def count_layout(N):
    """dict(x, acts [2 (N + 1)][N], c [B][N]: the number of transmitters on each vehicle's resource).  Env c of the first
    half is a cluster half a metre apart, env c of the second a spread 600 m apart."""
    u = np.arange(N)
    acts = (u[None, :] >= np.arange(N + 1)[:, None]).astype(np.int32)       # the first c on resource 0
    acts = np.concatenate([acts, acts])
    x = np.concatenate([np.broadcast_to(1000.0 + 0.5 * u, (N + 1, N)), np.broadcast_to(600.0 * u, (N + 1, N))])
    on0 = (acts == 0).sum(1, keepdims=True)
    return dict(x=np.ascontiguousarray(x), acts=acts, c=np.where(acts == 0, on0, N - on0))


def count_reference(c, m=1):
    """my_step design 3 from the counts: 1 for a sole transmitter, else -RN(exp(1.0 - 1.0 / c)); (reward, bound, E)."""
    c = np.asarray(c)
    E = np.vectorize(lambda cc: rn_exp(1.0 - 1.0 / float(cc)), otypes=[np.float64])(np.maximum(c, 1))
    return np.where(c > 1, -1.0 * E, 1.0), np.where(c > 1, exp_ulp_bound(E, False, m), 0.0), E


@functools.lru_cache(maxsize=None)
def count_oracle(N, design, mode):
    from oracle.oracle import SQ_IEEE, Oracle
    lay = count_layout(N)
    B = lay["x"].shape[0]
    orc = Oracle(count_config(N, design), batch=B, sq_mode=SQ_IEEE, threads=8)
    orc.reset(lay["x"], np.zeros((B, N)), np.zeros((B, N)))
    rew, _ = orc.step(mode, lay["acts"], 0)
    return rew


def exp_arguments():
    """Every argument the sweep hands to exp(): 1 - k / n of every claimed pair of every size, 1 - 1 / c up to 300, 0, 1."""
    args = {0.0, 1.0}
    for N in RATIO_SIZES:
        args |= {1.0 - k / n for k, n in claimed_pairs(N) if n > 0}
        args |= set((1.0 - ratio_model(N)["R"]).ravel().tolist())
    args |= {1.0 - 1.0 / c for c in range(2, 301)}
    return sorted(args)


# ---- the RSSI window -----------------------------------------------------------------------------------------------------
WIN_A = 64                      # a window row: subframe 0 is the agent's own, 63 values behind it
POWERS = ((1.0, -40.0), (10.0, -70.0), (100.0, -100.0), (1000.0, -130.0), (1e4, -160.0))
RUN = 64
ANCHORS = (1.0, 2.0, 9.999, 10.0, 31.6227766, 100.0, 999.5, 1000.0, 5000.0, 1e4, 65536.0, 99990.0)


def _walk(x, n, dt):
    x = dt(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, dt(np.inf if n > 0 else -np.inf))
    return x


@functools.lru_cache(maxsize=None)
def window_rows(f32=False):
    """dict(d: the flat list of distances in the input type; chobs [R][64], actions [R]; runs: (start, length) of the runs
    of adjacent values; exact {index: value}: what a distance MUST read; own_d: what the own subframes hold)."""
    dt = np.float32 if f32 else np.float64
    rng = np.random.default_rng(95 + f32)
    d, exact, runs = [], {}, []

    def put(v, must=None):
        if must is not None:
            exact[len(d)] = must
        d.append(dt(v))
    for i in range(1, 5001):
        put(i)
    for p, w in POWERS:
        put(_walk(p, -1, dt), -40.0 if p == 1.0 else None)
        put(p, w)
        put(_walk(p, 1, dt))
    put(0.5, -40.0)
    put(1e-40 if f32 else 5e-324, -40.0)                           # a subnormal of the input type
    put(_walk(100000.0, -1, dt))
    put(100000.0, -160.0)
    put(5000.0)
    put(_walk(5000.0, 1, dt))
    put(np.nan, -200.0)
    put(0.0, -200.0)
    put(250000.0, -160.0)
    for v in np.exp(rng.uniform(0.0, math.log(1e5), 2000)):
        put(min(max(dt(v), _walk(1.0, 1, dt)), _walk(100000.0, -1, dt)))
    for v in np.exp(rng.uniform(0.0, math.log(1e5), 2000)).astype(np.float32):
        put(min(max(v, np.float32(1.0000001)), np.float32(99999.99)))
    for a in ANCHORS:
        v = _walk(a, -(RUN // 2) if a > 1.0 else 0, dt)
        runs.append((len(d), RUN))
        for _ in range(RUN):
            put(v)
            v = np.nextafter(v, dt(np.inf))
    d = np.array(d, dtype=dt)
    assert (d[np.isfinite(d)] >= 0).all()
    per = WIN_A - 1
    R = -(-len(d) // per)
    own_d = dt(777.0)
    chobs = np.full((R, WIN_A), own_d, dtype=dt)
    flat = np.full(R * per, 3.0, dtype=dt)
    flat[:len(d)] = d
    chobs[:, 1:] = flat.reshape(R, per)
    return dict(d=d, chobs=chobs, actions=np.zeros(R, np.int32), runs=runs, exact=exact, own_d=own_d)


def window_values(w, rows):
    """The values of `rows`' flat distance list out of a window [R][64], and the own column."""
    w = np.asarray(w, dtype=np.float64)
    return w[:, 1:].reshape(-1)[:len(rows["d"])], w[:, 0]


def heard(d):
    return (d > 0) & (d < 100000.0)


@functools.lru_cache(maxsize=None)
def window_reference(f32=False):
    """(w_ref, bound per ulp of host error m -> see window_bound, l) over the flat list: -40.0 - 30.0 * RN(log10(max(d, 1)))
    where a transmitter is heard, -160 at or beyond 100000, -200 for 0 and NaN."""
    d = window_rows(f32)["d"].astype(np.float64)
    l = np.array([rn_log10(max(v, 1.0)) if hv else 0.0 for v, hv in zip(d.tolist(), heard(d).tolist())])
    w = np.where(heard(d), -40.0 - 30.0 * l, np.where(d >= 100000.0, -160.0, -200.0))
    return w, l


def host_log10_error(f32=False):
    """m: the worst error of the host's log10 (math's and NumPy's) on the rows, in ulps of the correctly rounded value."""
    d = window_rows(f32)["d"].astype(np.float64)
    _, l = window_reference(f32)
    h = heard(d) & (d > 1.0)
    dm = np.maximum(d[h], 1.0)
    e_np = np.abs(np.log10(dm) - l[h]) / np.spacing(l[h])
    e_m = np.abs(np.array([math.log10(v) for v in dm.tolist()]) - l[h]) / np.spacing(l[h])
    return float(max(e_np.max(), e_m.max()))


def window_bound(f32, m):
    """|w_dev - w_ref| <= 30 (m + 1) ulp(l) + ulp(w_ref): m the host library's measured error, one ulp more for the two
    sides of the true value; the last term the chain's own two roundings.  0 where no log10 is taken."""
    d = window_rows(f32)["d"].astype(np.float64)
    w, l = window_reference(f32)
    return np.where(heard(d) & (d > 1.0), 30.0 * (m + 1) * np.spacing(l) + np.spacing(np.abs(w)), 0.0)


def window_failures(w, f32, m):
    """What the GPU and the CPU tests both call on a window [R][64] built from window_rows(f32): a list of (what, index,
    got, wanted) - the own subframes -60, the required exact values, every value within window_bound of the correctly
    rounded chain, every run of adjacent distances monotone non-increasing - and the worst error: in ulps of the reference value, as a fraction of the bound, where, and how
    many values differ from the reference at all."""
    rows = window_rows(f32)
    got, own = window_values(w, rows)
    ref, l = window_reference(f32)
    bad = [("own", int(i), float(own[i]), -60.0) for i in np.flatnonzero(own != -60.0)]
    for i, must in rows["exact"].items():
        if not got[i] == must:
            bad.append(("exact", i, float(got[i]), must))
    bound = window_bound(f32, m)
    for i in np.flatnonzero(~(np.abs(got - ref) <= bound)):
        bad.append(("bound", int(i), float(got[i]), float(ref[i])))
    for s, n in rows["runs"]:
        seg = got[s:s + n]
        for i in np.flatnonzero(seg[1:] > seg[:-1]):
            bad.append(("monotone", int(s + i + 1), float(seg[i + 1]), float(seg[i])))
    d = rows["d"].astype(np.float64)
    h = heard(d) & (d > 1.0)
    err = np.abs(got[h] - ref[h])
    i = int(np.argmax(err / bound[h]))
    worst = dict(ulps_of_w=float((err / np.spacing(np.abs(ref[h]))).max()), of_bound=float((err / bound[h]).max()),
                 at=float(d[h][i]), differ=int((err > 0).sum()), heard=int(h.sum()))
    return bad, worst


def host_window(chobs, actions, log10=np.log10):
    """The documented map with a given log10 (NumPy's: tests/host_closed_loop.window_from_chobs)."""
    d = np.asarray(chobs, dtype=np.float64)
    h = heard(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(h, -40.0 - 30.0 * log10(np.where(h, np.maximum(d, 1.0), 1.0)), -200.0)
    w = np.where(d >= 100000.0, -160.0, w)
    return np.where(np.arange(d.shape[-1])[None, :] == np.asarray(actions)[:, None], -60.0, w)


def rn_log10_array(a):
    return np.vectorize(rn_log10, otypes=[np.float64])(a)


# ---- decisions ----------------------------------------------------------------------------------------------------------
DECISION_A = (3, 8, 10, 64, 65, 256)
THRESHOLDS = (-110.0, -150.0, -165.0, -230.0)      # the default; close above -160; between -200 and -160; below -200
OOR, IDLE, LOUD = 100000.0, 0.0, 10.0
ADJ = (3.0, 10.0, 47.5, 100.0, 999.9, 1000.0, 2500.0, 4999.0, 7000.0, 1e4, 31622.7, 99999.0)
CLAMPED = (0.5, 0.99999, 1.0, 1e-30, 0.25)


def need_of(A):
    return max(1, math.ceil(A / 5))


@functools.lru_cache(maxsize=None)
def decision_rows(A, f32=False):
    """dict(chobs [agents][A], own, prev, choice [agents], kind [agents]: the row's name, label {kind: True (shortcut) /
    False (general path)} for the rows whose side is fixed at the default threshold).  The agent's own subframe is A - 1;
    every row runs with prev == own and with prev == A - 2, each with the picks 0 ... need - 1 (a selection of them beyond
    eight).  Rows: `unheard_exact` / `unheard_less` - exactly ceil(A / 5) idle or out-of-range candidates, and one fewer;
    `at5000` / `beyond5000` - a heard transmitter at exactly 5000 m and one step of the input type beyond, every other
    candidate unheard; `tie_after` / `tie_first` / `tie_mid` - d = 1e4 (exactly -160) behind, in front of and between
    out-of-range subframes, everything else loud; `clamp` - every subframe below or on the 1 m clamp (all -40: ordered by
    subframe); `adjacent` - pairs of adjacent distances, the larger one in the lower subframe; `mixed*` - random rows."""
    dt = np.float32 if f32 else np.float64
    need, own, alt = need_of(A), A - 1, A - 2
    rng = np.random.default_rng(1000 + A)
    rows, label = [], {}

    def row(kind, fill, vals=(), side=None):
        r = np.full(A, fill, dtype=dt)
        r[:len(vals)] = np.array(vals, dtype=dt)
        r[own] = dt(0.0)                                             # half duplex: the own subframe reads 0
        rows.append((kind, r))
        if side is not None:
            label[kind] = side
    mix = [OOR if i % 2 == 0 else IDLE for i in range(A)]
    row("unheard_exact", LOUD, mix[:need], True)
    row("unheard_less", LOUD, mix[:need - 1], False)
    row("at5000", IDLE, mix[:A - 3] + [5000.0] if A > 3 else [5000.0], None)
    row("beyond5000", IDLE, mix[:A - 3] + [_walk(5000.0, 1, dt)] if A > 3 else [_walk(5000.0, 1, dt)], False)
    row("tie_after", LOUD, [OOR, 1e4], False)
    row("tie_first", LOUD, [1e4, OOR], False)
    if A >= 5:
        row("tie_mid", LOUD, [OOR, 1e4, OOR], False)
    row("clamp", 0.5, [CLAMPED[i % len(CLAMPED)] for i in range(A)], False)
    adj = []
    for i in range(A // 2):
        v = dt(ADJ[i % len(ADJ)]) + dt(i // len(ADJ))
        adj += [np.nextafter(v, dt(np.inf)), v]
    row("adjacent", 20.0, adj, False)
    for j in range(4):
        v = np.exp(rng.uniform(math.log(0.5), math.log(2e5), A))
        v = np.where(rng.random(A) < 0.2, 0.0, v)
        row("mixed%d" % j, 0.0, v.tolist())
    picks = list(range(need)) if need <= 8 else sorted({0, 1, 2, need // 2, need - 2, need - 1})
    chobs, owns, prevs, choice, kind = [], [], [], [], []
    for name, r in rows:
        for prev in (own, alt):
            for pk in picks:
                chobs.append(r); owns.append(own); prevs.append(prev); kind.append(name)
                choice.append(pk + need * int(rng.integers(0, 1000)))            # (r % need is the pick)
    return dict(chobs=np.stack(chobs), own=np.array(owns, np.int32), prev=np.array(prevs, np.int32),
                choice=np.array(choice, np.int32), kind=np.array(kind), label=label, need=need)


def host_decisions(window, prev, thr, choice=None, seed=None, chobs=None, own=None):
    """tests/host_closed_loop.HostSps on a READY window with every agent re-selecting (counter 0, keep probability 0): the
    picks, and - where the observation is given too - the host's own record of every decision (`_judge`).  Draws: the
    injected `choice`, or the mirror's from `seed`."""
    from tests import host_closed_loop as H
    n, A = np.asarray(window).shape
    sps = H.HostSps(n, A, threshold=thr, keep_prob=0.0, prev_action=prev, counter=np.zeros(n, np.int32))
    kw = dict(seed=seed) if choice is None else dict(draw_counter=np.full(n, 7, np.int32), draw_keep=np.ones(n), draw_choice=choice)
    out = sps.step(window=window, **kw)
    if chobs is not None:
        w = np.asarray(window, dtype=np.float64)
        d = np.asarray(chobs, dtype=np.float64)
        for rec in sps.log:
            i = rec["agent"]
            hv = heard(d[i]) & (np.arange(A) != own[i])
            _, _, tried = H.choose_new_resource(w[i].tolist(), int(prev[i]), thr, sps.inc_db, 0)
            rec.update(sps._judge(d[i], w[i].tolist(), hv, int(prev[i]), int(own[i]), tried))
    return out, sps.log
