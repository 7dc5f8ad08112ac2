"""Host statement of `diral_td_head` and `diral_memory_history` (include/diral_env.h) in NumPy, shared by
tests/test_td_cases.py (CPU) and tests/test_gpu_td.py / tests/test_gpu_history.py.

`calc_target` restates ``DRQN._calc_target`` (algorithms/drl_drqn.py:267-292) with the dtypes NumPy gives its steps said
out loud; `td_head` adds the loss head (:76-80) and its gradient in float32, and the loss in the fixed order the device
sums in.  `deque_window` is the driver's ``history_input`` said literally; `ring_window` the rows the device reads.  Every
`wrong=` switch changes ONE rule; the CPU test shows that each is told apart by some case.  Q-values travel as float32
arrays holding values the case's dtype represents exactly."""
import math
import os
from collections import deque

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {"td1": "td1_double_lstm", "td2": "td2_double_dqn", "td3": "td3_plain_lstm", "td4": "td4_plain_dqn",
            "h1": "h1_history_feeds"}
F32 = np.float32
LOSS_THREADS = 256


def load_fixture(key):
    z = np.load(os.path.join(GOLDEN, FIXTURES[key] + ".npz"))
    return {k: z[k] for k in z.files}


# ---- number formats ----
def bf16_round(x):
    """float32 -> the float32 value of the nearest bfloat16, ties to even (a NaN stays one)."""
    u = np.asarray(x, F32).view(np.uint32).astype(np.uint64)
    r = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(F32)
    return np.where(np.isnan(x), F32(np.nan), r).astype(F32)


def quantize(x, dtype):
    """float32 array -> float32 array of the values `dtype` ("f32" / "f16" / "bf16") holds after one rounding to nearest even."""
    x = np.asarray(x, F32)
    if dtype == "f32":
        return x.copy()
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(F32)
    return bf16_round(x)


def same_bits(got, want):
    """float32 arrays equal bit for bit, but that any NaN equals any NaN."""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]))


# ---- the targets ----
def argmax_rows(index, wrong=None):
    if wrong == "last_tie":                                         # the last index between equals
        A = index.shape[1]
        return (A - 1 - np.argmax(index[:, ::-1], axis=1)).astype(np.int64)
    return np.argmax(index, axis=1)


def calc_target(qn_target, qn_eval, rewards, gamma, double, wrong=None):
    """-> (targets float32 [rows], next actions [rows]).  `qn_target` / `qn_eval` float32 [rows, A] (`qn_eval` may be None
    when `double` is False), `rewards` [rows] float64 or float32."""
    qn_target = np.asarray(qn_target, F32)
    rows = len(qn_target)
    use_eval = double != (wrong == "plain_index_eval")
    index = np.asarray(qn_eval, F32) if use_eval else qn_target
    j = argmax_rows(index, wrong)
    source = np.asarray(qn_eval, F32) if wrong == "double_from_eval" and double else qn_target
    nv = source[np.arange(rows), j]                                 # np.max(qn_target, axis=1) in the plain case
    with np.errstate(invalid="ignore", over="ignore"):
        if wrong == "gamma_f64":
            return (np.asarray(rewards, np.float64) + gamma * nv.astype(np.float64)).astype(F32), j
        if wrong == "fma":                                          # the product never rounded to float32
            return (np.asarray(rewards, np.float64) + np.float64(F32(gamma)) * nv.astype(np.float64)).astype(F32), j
        disc = F32(gamma) * nv                                      # a Python float times a float32 array: float32
        assert disc.dtype == F32
        if wrong == "add_f32":
            return np.asarray(rewards).astype(F32) + disc, j
        total = np.asarray(rewards).astype(np.float64) + disc.astype(np.float64)   # float64 rewards: a float64 sum
        return total.astype(F32), j                                 # the feed into the float32 placeholder rounds once


# ---- the loss head ----
def fixed_order_loss(hl):
    """mean(hl^2) as the device sums it: thread t of 256 adds (double)hl * (double)hl of the rows t, t + 256, ... in turn,
    the 256 partial sums are added in index order, the loss is float32(sum / rows)."""
    rows = len(hl)
    sq = np.asarray(hl, np.float64) ** 2                            # (exact: the square of a float32 fits a float64)
    pad = np.zeros((-rows) % LOSS_THREADS)
    part = np.zeros(LOSS_THREADS)
    with np.errstate(invalid="ignore", over="ignore"):
        for chunk in np.concatenate([sq, pad]).reshape(-1, LOSS_THREADS):
            part = part + chunk                                     # (+ 0.0 behind a thread's last row changes nothing)
        total = 0.0
        for v in part:
            total = total + float(v)
        return F32(total / rows)


def td_head(q, actions, rewards, qn_target, qn_eval, gamma, double, hysteretic, wrong=None):
    """-> dict(targets, next_actions, td (hl), grad (float32 [rows, A], before the rounding to the Q dtype), loss, bad)."""
    q = np.asarray(q, F32)
    rows, A = q.shape
    targets, j = calc_target(qn_target, qn_eval, rewards, gamma, double, wrong)
    a = np.asarray(actions, np.int64)
    inside = (a >= 0) & (a < A)
    Q = np.where(inside, q[np.arange(rows), np.where(inside, a, 0)], F32(0.0)).astype(F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        h = Q - targets
        damped = (h < 0) & bool(hysteretic)
        tenth = h * F32(0.1) if wrong == "mul_tenth" else h / F32(10.0)
        hl = np.where(damped, tenth, h).astype(F32)
        g = (F32(2.0) * hl) / F32(rows)
        g = np.where(damped, g * F32(0.1) if wrong == "mul_tenth" else g / F32(10.0), g).astype(F32)
    grad = np.zeros((rows, A), F32)
    grad[np.arange(rows)[inside], a[inside]] = g[inside]
    return dict(targets=targets, next_actions=j.astype(np.int32), td=hl, grad=grad, loss=fixed_order_loss(hl),
                bad=int((~inside).sum()))


def fsum_loss(hl):
    """float32(the exactly rounded float64 sum of hl^2 / rows)."""
    return F32(math.fsum(float(v) * float(v) for v in hl) / len(hl))


# ---- the acting window ----
def deque_window(states, step):
    """np.array(history_input) after the driver appended every state of `states` [T][B, N, S] (main_test.py:86, 114, 219)."""
    history = deque(maxlen=step)
    for s in states:
        history.append(s)
    return np.array(history)                                        # [step, B, N, S]


def agent_feeds(window):
    """state_vector[:, user].reshape(1, step, S) of every agent of every env (drl_drqn.py:172), env-major: [B * N, step, S]."""
    step, B, N, S = window.shape
    return np.array([window[:, b, n].reshape(step, S) for b in range(B) for n in range(N)])


def ring_window(ring, count, C, step, wrong=None):
    """The device's rows: ring [C + 1, B, N, S] with logical state j in row j mod (C + 1); step s of the window is state
    count - step + 1 + s.  -> [B * N, step, S]."""
    last = count - (1 if wrong == "ends_before_newest" else 0)
    rows = [(last - step + 1 + s) % (C + 1) for s in range(step)]
    return agent_feeds(np.array([ring[r] for r in rows]))


# ---- case generators ----
# A <= 64 runs G lanes per row (G = 4, 32, 64, 64 here), above one wave per row; rows: one, a part-filled group and wave,
# one past a workgroup's worth at A = 3 (256 / 4 * 4 = 256 rows), several partial sums per thread in the loss
SMALL_A, WIDE_A = (3, 32, 33, 64), (65, 200, 4096)
ROWS = (1, 15, 17, 257, 1000)
DTYPES = ("f32", "f16", "bf16")
CASE_SEED = 20261021


def random_case(rows, A, dtype="f32", seed=0, f32_rewards=False):
    """Q-values of the dtype's grid with coarse rows (ties), rewards float64 that float32 does not hold (or float32),
    actions inside [0, A); |h| stays within about [1e-3, 1e3] but for accidents."""
    rng = np.random.default_rng(CASE_SEED + 7919 * seed + 31 * A + rows)
    def table(scale):
        t = (rng.standard_normal((rows, A)) * scale).astype(F32)
        t[::3] = np.round(t[::3] * 2.0) / 2.0
        return quantize(t, dtype)
    q, qn_target, qn_eval = table(4.0), table(4.0), table(4.0)
    rewards = rng.standard_normal(rows) * 3.0
    rewards[::5] = 0.1
    if f32_rewards:
        rewards = rewards.astype(F32)
    actions = rng.integers(0, A, rows).astype(np.int32)
    return dict(q=q, qn_target=qn_target, qn_eval=qn_eval, rewards=rewards, actions=actions)


def special_index_rows(A):
    """Hand-made rows for the arg-max and the value taken: ties first / last / across a group's halves and the 64-lane
    stride, -0.0 against +0.0, NaN rows, rows of -inf, +inf."""
    rows = [np.zeros(A), np.full(A, -0.0), np.full(A, -np.inf), np.full(A, np.inf), np.full(A, np.nan)]
    ks = sorted({k for k in (0, 1, 2, 15, 16, 31, 32, 63, 64, 65, 128, A // 2, A - 1) if 0 <= k < A})
    for k in ks:
        k2 = (k + 64) % A if A > 64 else A - 1 - k
        r = np.full(A, -1.0); r[k] = 3.0; r[k2] = 3.0; rows.append(r)                 # an exact tie
        r = np.full(A, 0.0); r[k] = -0.0; rows.append(r)
        r = np.full(A, -0.0); r[k] = 0.0; rows.append(r)                              # the first zero is -0.0 (k > 0)
        r = np.arange(A, dtype=np.float64); r[k] = np.nan; rows.append(r)
        r = np.zeros(A); r[k] = np.nan; r[k2] = np.nan; rows.append(r)
        r = np.full(A, -np.inf); r[k] = -65504.0; rows.append(r)
        r = np.full(A, -1.0); r[k] = np.inf; r[k2] = np.inf; rows.append(r)
    return np.array(rows, F32)


def special_case(A, dtype="f32", double=True, gamma=0.99):
    """`special_index_rows` as the index rows of a double head (and, eight of them, of a plain one), then value rows: h == 0
    exactly (placed for `double`), the tiniest negative and positive h, a tiny negative h whose tenth is subnormal, -0.0
    chosen, an inf and a NaN in a column that was not chosen, and actions of -1 and A."""
    idx = quantize(special_index_rows(A), dtype)
    n = len(idx)
    rng = np.random.default_rng(CASE_SEED + A)
    other = quantize((rng.standard_normal((n, A)) * 2.0).astype(F32), dtype)
    qn_eval = np.concatenate([idx, other[:16]])
    qn_target = np.concatenate([other, idx[:8], other[8:16]])       # rows n ... n + 7: the plain head sees special rows too
    rows = n + 16                                                   # rows n + 8 ...: the value rows below
    rewards = rng.standard_normal(rows) * 2.0
    rewards[::4] = 0.1
    actions = rng.integers(0, A, rows).astype(np.int32)
    q = quantize((rng.standard_normal((rows, A)) * 2.0).astype(F32), dtype)
    case = dict(q=q, qn_target=qn_target, qn_eval=qn_eval, rewards=rewards, actions=actions)
    if dtype == "f32":                                              # values placed on the float32 grid around the target
        t, _ = calc_target(qn_target, qn_eval, rewards, gamma, double)
        r0, a = n + 8, actions
        q[r0, a[r0]] = t[r0]                                        # h == 0: no division, a zero gradient
        q[r0 + 1, a[r0 + 1]] = np.nextafter(t[r0 + 1], F32(-np.inf))          # the tiniest negative h at the target
        q[r0 + 2, a[r0 + 2]] = np.nextafter(t[r0 + 2], F32(np.inf))
        rewards[r0 + 3] = 0.0                                       # target 0, Q a few subnormal steps below it:
        qn_target[r0 + 3] = 0.0
        qn_eval[r0 + 3] = 0.0
        q[r0 + 3, a[r0 + 3]] = F32(-1e-44)                          # h / 10 rounds to the smallest subnormal
    r1 = n + 12
    q[r1, actions[r1]] = F32(-0.0)                                  # a chosen -0.0 stays -0.0 (target 0 there)
    rewards[r1] = 0.0
    qn_target[r1] = 0.0
    qn_eval[r1] = 0.0
    q[r1 + 1, (actions[r1 + 1] + 1) % A if A > 1 else 0] = F32(np.inf)       # not chosen (A > 1): does not poison the row
    q[r1 + 2, (actions[r1 + 2] + 1) % A if A > 1 else 0] = F32(np.nan)
    actions[r1 + 3] = -1                                            # outside [0, A): Q = 0, a zero gradient row, counted
    actions[0] = A
    return case


def rounding_cases(n=64, gamma=0.99, seed=1):
    """Rows of A = 3 on which float32(r + float64(gamma32 * nv)) differs from the sum done in float32: -> a case dict."""
    rng = np.random.default_rng(CASE_SEED + seed)
    qn = (rng.standard_normal((40 * n, 3)) * 4.0).astype(F32)
    r = rng.standard_normal(40 * n) * 3.0
    right, _ = calc_target(qn, None, r, gamma, False)
    wrong, _ = calc_target(qn, None, r, gamma, False, wrong="add_f32")
    keep = np.flatnonzero(right != wrong)[:n]
    assert len(keep) == n
    rows = len(keep)
    return dict(q=(rng.standard_normal((rows, 3)) * 4.0).astype(F32), qn_target=qn[keep], qn_eval=qn[keep][:, ::-1].copy(),
                rewards=r[keep], actions=rng.integers(0, 3, rows).astype(np.int32))


# ---- what the reference's loss head is, as a torch expression (CPU autograd, and the composition the launch replaces) ----
def torch_loss(torch, q, actions, targets, hysteretic):
    """drl_drqn.py:76-80 on float32 tensors: reduce_sum(q * one_hot), the TD error, where(h < 0, h / 10, h), the mean of squares."""
    one_hot = torch.nn.functional.one_hot(actions.long(), q.shape[1]).to(q.dtype)
    h = (q * one_hot).sum(dim=1) - targets
    if hysteretic:
        h = torch.where(h < 0, h / 10, h)
    return h.square().mean()
