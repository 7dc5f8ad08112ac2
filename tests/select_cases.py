"""Host statement of `diral_policy_select` (include/diral_env.h) in NumPy float64, the device generator restated, and the
case builders shared by tests/test_select_cases.py (CPU) and tests/test_gpu_select.py.

The four kinds are written with the very calls the reference makes (algorithms/policies.py): np.argmax, np.sum, np.exp,
np.cumsum, searchsorted(side="right").  The `wrong_*` functions are restatements with ONE rule changed; the CPU test shows
that each of them is told apart from the statement by some case, so a device kernel that passes against the statement
cannot carry that mistake."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GREEDY, EPS_GREEDY, SOFTMAX, BOLTZMANN = 0, 1, 2, 3
STREAM_U, STREAM_A = 10, 11
M64 = (1 << 64) - 1


# ---- the device generator (csrc/policy_device.hpp: mix64, rng_u64, rng_unit) ----
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def rng_u64(seed, stream, idx):
    return mix64((mix64((seed ^ (stream * 0xD1342543DE82EF95)) & M64) + idx) & M64)


def policy_seed(seed, k):
    return (int(seed) * 1000003 + int(k)) & M64


def device_draws(seed, agents, A, idx0=0):
    """(draw_u [agents] float64, draw_a [agents] int64 already mod A) of a launch seeded `seed`."""
    u = np.array([(rng_u64(seed, STREAM_U, idx0 + i) >> 11) * (1.0 / 9007199254740992.0) for i in range(agents)])
    a = np.array([rng_u64(seed, STREAM_A, idx0 + i) % A for i in range(agents)], dtype=np.int64)
    return u, a


# ---- the statement ----
def greedy(Q):
    return np.argmax(Q, axis=1)                                     # policies.py:30


def eps_greedy(Q, eps, u, a):
    """-> (actions, explored); eps scalar or [R]."""
    A = Q.shape[1]
    g = greedy(Q)
    exploit = u > eps                                               # :50 (strict)
    return np.where(exploit, g, a % A), ~exploit


def softmax_cdf(q, tmp):
    """-> (cdf or None for a row np.random.choice raises on, the row's sum)."""
    with np.errstate(all="ignore"):
        x = q / tmp                                                 # :98
        x = x - x.max()                                             # :110
        y = np.exp(x)
        S = y.sum()
        if not np.isfinite(S) or not S > 0:
            return None, S
        p = y / S                                                   # :112
        cdf = np.cumsum(p)                                          # np.random.choice(p=)
        cdf /= cdf[-1]
    return cdf, S


def softmax(Q, tmp, u):
    """-> (actions, bad): a row the reference raises on takes the greedy answer."""
    R, A = Q.shape
    tmp = np.broadcast_to(np.asarray(tmp, np.float64), (R,))
    act, bad = np.zeros(R, np.int64), np.zeros(R, bool)
    for r in range(R):
        cdf, _ = softmax_cdf(Q[r], tmp[r])
        if cdf is None:
            act[r], bad[r] = np.argmax(Q[r]), True
        else:
            act[r] = min(int(np.searchsorted(cdf, u[r], side="right")), A - 1)
    return act, bad


def boltzmann_prob(q, beta, alpha):
    A = len(q)
    with np.errstate(all="ignore"):
        prob1 = (1 - alpha) * np.exp(beta * q)                      # :171
        return prob1 / np.sum(np.exp(beta * q)) + alpha / A         # :172


def boltzmann(Q, beta, alpha, explore_p, u, a):
    """-> (actions, explored); beta, alpha, explore_p scalars or [R]."""
    R, A = Q.shape
    beta, alpha, explore_p = (np.broadcast_to(np.asarray(v, np.float64), (R,)) for v in (beta, alpha, explore_p))
    explored = explore_p > u                                        # :162
    act = np.zeros(R, np.int64)
    for r in range(R):
        act[r] = a[r] % A if explored[r] else np.argmax(boltzmann_prob(Q[r], beta[r], alpha[r]))   # :175
    return act, explored


# ---- np.sum's order as the kernel walks it (csrc/policy_device.hpp np_pairwise_sum, csrc/select_kernel.hpp) ----
def pairwise_sum(a):
    n = len(a)
    if n < 8:
        res = np.float64(0.0)
        for v in a:
            res = res + v
        return res
    if n <= 128:
        r = [a[j] for j in range(8)]
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] = r[j] + a[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res = res + a[i]
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_sum(a[:n2]) + pairwise_sum(a[n2:])


def pairwise_depth(n):
    """Splits above the deepest leaf: the kernel's lane walk covers six."""
    if n <= 128:
        return 0
    n2 = n // 2
    n2 -= n2 % 8
    return 1 + max(pairwise_depth(n2), pairwise_depth(n - n2))


# ---- restatements with one rule wrong ----
def wrong_greedy_last_tie(Q):
    A = Q.shape[1]
    return A - 1 - np.argmax(Q[:, ::-1], axis=1)


def wrong_greedy_nan_ignored(Q):
    return np.array([np.nanargmax(r) if not np.all(np.isnan(r)) else 0 for r in Q])


def wrong_eps_greedy_ge(Q, eps, u, a):
    return np.where(u >= eps, greedy(Q), a % Q.shape[1])


def wrong_softmax(Q, tmp, u, rule):
    act = np.zeros(len(Q), np.int64)
    for r in range(len(Q)):
        q = Q[r]
        if rule == "max_first":
            x = (q - q.max()) / tmp
        else:
            x = q / tmp
            x = x - x.max()
        y = np.exp(x)
        p = y / y.sum()
        if rule == "tree_cumsum":                                   # a Hillis-Steele scan: re-associates the additions
            cdf, d = p.copy(), 1
            while d < len(cdf):
                cdf[d:] = cdf[d:] + cdf[:-d].copy()
                d *= 2
        else:
            cdf = np.cumsum(p)
        cdf = cdf / cdf[-1]
        act[r] = min(int(np.searchsorted(cdf, u[r], side="left" if rule == "left" else "right")), len(q) - 1)
    return act


# ---- ambiguity: rows on which two correct implementations may differ because their exp differs by ulps ----
def margin(A):
    """Two implementations' cdf entries differ relatively by at most (2A + 16) * 2^-52: the exp errors (2 ulps each side),
    A rounded additions on each side, the two divisions."""
    return (2 * A + 16) * 2.0 ** -52


def softmax_ambiguous(Q, tmp, u):
    R, A = Q.shape
    tmp = np.broadcast_to(np.asarray(tmp, np.float64), (R,))
    m = margin(A)
    amb = np.zeros(R, bool)
    for r in range(R):
        cdf, _ = softmax_cdf(Q[r], tmp[r])
        if cdf is not None:
            amb[r] = bool(np.any(np.abs(u[r] - cdf) <= m * cdf))
    return amb


def boltzmann_ambiguous(Q, beta, alpha):
    """An exploiting row is ambiguous when two actions with DIFFERENT Q-values (equal ones give equal exp on any one
    implementation) have probabilities within the margin of the row's maximum, or when an exp argument is within 2 of
    the overflow threshold."""
    R, A = Q.shape
    beta, alpha = (np.broadcast_to(np.asarray(v, np.float64), (R,)) for v in (beta, alpha))
    m = margin(A)
    amb = np.zeros(R, bool)
    for r in range(R):
        with np.errstate(all="ignore"):
            z = beta[r] * Q[r]
            pr = boltzmann_prob(Q[r], beta[r], alpha[r])
        if np.any(np.abs(z - 709.78) < 2.0):
            amb[r] = True
        elif not np.any(np.isnan(pr)):
            top = pr.max()
            near = np.abs(pr - top) <= 4 * m * top
            amb[r] = len(np.unique(Q[r][near])) > 1
    return amb


# ---- case builders ----
DTYPES = ("f64", "f32", "f16", "bf16")


def quantize(Q, dtype):
    """-> (store, exact): `store` the array as the tensor holds it (bf16: the uint16 bit patterns), `exact` its float64
    values - what the kernel converts to."""
    if dtype == "f64":
        return Q.copy(), Q.copy()
    if dtype == "f32":
        s = Q.astype(np.float32)
        return s, s.astype(np.float64)
    if dtype == "f16":
        with np.errstate(over="ignore"):
            s = Q.astype(np.float16)
        return s, s.astype(np.float64)
    bits = (Q.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)      # truncated: any bf16 value will do
    return bits, (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


# (B, N, A): every B of {1, 3, 17}, N of {4, 9, 33, 64}, A of {1, 2, 3, 5, 31, 32, 33, 64, 65, 100, 256, 300} and 4096 at
# one small batch; A <= 64 runs G lanes per row, above one wave per row with a 64-lane stride
SHAPES = [(1, 4, 1), (3, 9, 2), (17, 33, 3), (3, 64, 5), (17, 4, 31), (17, 64, 32), (3, 33, 33), (1, 9, 64), (3, 4, 65),
          (17, 9, 100), (1, 33, 256), (3, 9, 300), (1, 4, 4096)]
CASE_SEED = 20261019


def random_case(i, dtype):
    """Case i of SHAPES in `dtype`: Q (store, exact) with coarse rows (ties) and, for the arg-max kinds, NaN / inf rows."""
    B, N, A = SHAPES[i]
    rng = np.random.default_rng(CASE_SEED + 100 * i + DTYPES.index(dtype))
    R = B * N
    Q = rng.standard_normal((R, A))
    Q[::3] = np.round(Q[::3] * 2.0) / 2.0
    store, exact = quantize(Q, dtype)
    return B, N, A, store, exact


# (shape index, dtype) of the GPU comparisons: every shape with the dtypes taken in turn, every dtype at the flagship
# A = 32, at a strided A = 100 and at A = 4096
GPU_CASES = [(i, DTYPES[i % 4]) for i in range(len(SHAPES))] + \
            [(i, d) for i in (5, 9, 12) for d in DTYPES if d != DTYPES[i % 4]]
POLICY_SEED = 4242            # QPolicy(seed=POLICY_SEED): its first call draws with policy_seed(POLICY_SEED, 1)
SOFTMAX_TMP = 0.5
BOLTZ = dict(beta=1.5, alpha=0.125, explore_p=0.3)


def case_draws(i):
    """The device's draws of the first `act` of a QPolicy(seed=POLICY_SEED) over case i."""
    B, N, A = SHAPES[i]
    return device_draws(policy_seed(POLICY_SEED, 1), B * N, A)


def special_rows(A):
    """Hand-made rows for the arg-max: all equal, ties first / last / across lane-group and 64-lane-stride boundaries,
    -0.0 against +0.0, a NaN in front of and behind the maximum, +-inf, all -inf."""
    rows = [np.zeros(A), np.full(A, -np.inf), np.full(A, np.inf), np.full(A, np.nan), np.full(A, -0.0)]
    ks = sorted({k for k in (0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 65, 127, 128, 129, 255, 256, A // 2, A - 2, A - 1)
                 if 0 <= k < A})
    for k in ks:
        k2 = (k + 64) % A if A > 64 else (A - 1 - k)
        r = np.zeros(A); r[k] = 3.0; r[k2] = 3.0; rows.append(r)                       # a tie between k and k2
        r = np.zeros(A); r[k] = 3.0; r[A - 1] = 3.0; r[0] = 3.0; rows.append(r)        # ... first and last
        r = np.full(A, 0.0); r[k] = -0.0; rows.append(r)
        r = np.full(A, -0.0); r[k] = 0.0; rows.append(r)
        r = np.arange(A, dtype=np.float64); r[k] = np.nan; rows.append(r)              # NaN in front of / at the maximum
        r = -np.arange(A, dtype=np.float64); r[k] = np.nan; rows.append(r)             # NaN behind the maximum
        r = np.zeros(A); r[k] = np.nan; r[k2] = np.nan; rows.append(r)                 # two NaNs: the first
        r = np.zeros(A); r[k] = np.inf; r[k2] = np.inf; rows.append(r)
        r = np.full(A, -np.inf); r[k] = -65504.0; rows.append(r)
        r = np.full(A, -np.inf); r[k] = np.nan; rows.append(r)
    return np.array(rows)


def load_fixture(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {A: {k[len("A%d_" % A):]: g[k] for k in g.files if k.startswith("A%d_" % A)} for A in (3, 32)}
