"""Host statement of `diral_memory_add` / `diral_memory_sample` (include/diral_env.h) in NumPy, shared by
tests/test_memory_cases.py (CPU) and tests/test_gpu_memory.py.

`DequeMemory` is the reference's Memory said literally - one ``deque(maxlen=capacity)`` of (state, action, reward,
next_state) tuples per env, fed the way the driver feeds it (``state = next_state``) - and `regroup` is
``DRQN.get_states_user`` and the three like it (algorithms/drl_drqn.py:294-377) restated as one loop nest, followed by
the reshapes of ``train`` (:234-243).  `RingMemory` is the layout the device keeps (three rings of capacity + 1 rows, each
state once) with the index arithmetic of the kernels.  Every `wrong=` switch changes ONE rule; the CPU test shows that each
is told apart by some fixture.  `permute` restates the device's window draw."""
import os
from collections import deque

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M64 = (1 << 64) - 1
FIXTURES = {"m1": "m1_memory_wrapped", "m2": "m2_memory_dqn", "m3": "m3_memory_batches"}
FIXTURE_SEEDS = {"m1": 8100, "m2": 8101, "m3": 8102}     # np.random.seed of tests/golden/gen_memory_golden.py


def load_fixture(key):
    z = np.load(os.path.join(GOLDEN, FIXTURES[key] + ".npz"))
    d = {k: z[k] for k in z.files}
    N, S, C, adds, step = (int(v) for v in d["meta"])
    d.update(N=N, S=S, C=C, adds=adds, step=step, lstm=key != "m2",
             batches=sorted(int(k[1:].split("_")[0]) for k in z.files if k.endswith("_idx")))
    return d


# ---- the device generator (csrc/policy_device.hpp) and the window permutation (csrc/memory_kernel.hpp) ----
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def rng_u64(seed, stream, idx):
    return mix64((mix64((seed ^ (stream * 0xD1342543DE82EF95)) & M64) + idx) & M64)


def policy_seed(seed, k):
    return (int(seed) * 1000003 + int(k)) & M64


def memory_seed(seed, call, env_offset=0):
    """Seed of ReplayMemory(seed=, env_offset=)'s `sample` call number `call` (1, 2, ...)."""
    return policy_seed(policy_seed(seed, env_offset), call)


def half_bits(R):
    cl = 0 if R <= 1 else (R - 1).bit_length()                      # ceil_log2(R)
    return max(1, (cl + 1) // 2)


def permute(x, R, seed):
    """P(x) for x in [0, R): a 4-round Feistel network on 2 w bits, walked again while the value is >= R."""
    w = half_bits(R)
    mask = (1 << w) - 1
    while True:
        left, right = x >> w, x & mask
        for k in range(4):
            left, right = right, left ^ (rng_u64(seed, k, right) & mask)
        x = (left << w) | right
        if x < R:
            return x


def _mix64_np(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def permute_all(R, seed):
    """[P(0), ..., P(R - 1)] as `permute` gives them, on uint64 arrays (wrapping arithmetic)."""
    w = np.uint64(half_bits(R))
    mask = np.uint64((1 << int(w)) - 1)
    keys = [np.uint64(mix64((seed ^ (k * 0xD1342543DE82EF95)) & M64)) for k in range(4)]
    out = np.empty(R, np.uint64)
    pending, cur = np.arange(R), np.arange(R, dtype=np.uint64)
    with np.errstate(over="ignore"):
        while pending.size:
            left, right = cur >> w, cur & mask
            for k in range(4):
                left, right = right, left ^ (_mix64_np(keys[k] + right) & mask)
            cur = (left << w) | right
            done = cur < np.uint64(R)
            out[pending[done]] = cur[done]
            pending, cur = pending[~done], cur[~done]
    return out.astype(np.int64)


def drawn_windows(M, B, L, seed):
    """-> (idx [M], env [M]) of a drawn sample: v = P(m), env = v mod B, start = v div B."""
    v = np.array([permute(m, B * L, seed) for m in range(M)], dtype=np.int64)
    return (v // B).astype(np.int32), (v % B).astype(np.int32)


def reference_idx(length, step, M, wrong=None):
    """Memory.sample's draw (utils/memory.py:184) from the global np.random."""
    pop = length - step + (1 if wrong == "last_start" else 0)
    return np.random.choice(np.arange(pop), size=M, replace=False)


# ---- the reference, literally ----
class DequeMemory:
    def __init__(self, capacity, B):
        self.buffers = [deque(maxlen=capacity) for _ in range(B)]
        self.state = None

    def begin(self, state):                                         # [B, N, S]
        for b in self.buffers:
            b.clear()
        self.state = np.array(state)

    def add(self, action, reward, next_state):                      # [B, N], [B, N], [B, N, S]
        for b, buf in enumerate(self.buffers):
            buf.append((self.state[b], action[b], reward[b], next_state[b]))
        self.state = np.array(next_state)                           # state = next_state (main_test.py:113, 217)

    def __len__(self):
        return len(self.buffers[0])

    def windows(self, idx, env, step):                              # Memory.sample's res (utils/memory.py:187-194)
        return [[self.buffers[b][i + j] for j in range(step)] for i, b in zip(idx, env)]


def regroup(batch, field, N, wrong=None):
    """get_states_user (field 0), get_actions_user (1), get_rewards_user (2), get_next_states_user (3)."""
    if wrong == "same_row" and field == 3:
        field = 0
    out = []
    for n in range(N):                                              # user-major: all of user 0's windows, then user 1's, ...
        rows = []
        for window in batch:
            rows.append([entry[field][n] for entry in window])
        out.append(rows)
    out = np.array(out)                                             # [N, M, step, ...]
    if wrong == "sample_major":
        out = np.swapaxes(out, 0, 1)
    return out


def train_batch(batch, N, lstm=True, last_only=False, wrong=None):
    """-> (states, actions, rewards, next_states) as `train` holds them (drl_drqn.py:218-243, 255, 288)."""
    s, a, r, n = (regroup(batch, f, N, wrong) for f in range(4))
    if lstm:
        s, n = np.reshape(s, [-1, s.shape[2], s.shape[3]]), np.reshape(n, [-1, n.shape[2], n.shape[3]])
        a, r = np.reshape(a, [-1, a.shape[2]]), np.reshape(r, [-1, r.shape[2]])
        if last_only:
            a, r = a[:, -1], r[:, -1]
    else:
        s, n = np.reshape(s, [-1, s.shape[3]]), np.reshape(n, [-1, n.shape[3]])
        a, r = np.reshape(a, [-1]), np.reshape(r, [-1])
    return s, a, r, n


def host_sample(mem, idx, env, step, N, last_only=False):
    """The batch a DequeMemory gives for the windows; a window outside [0, len - step) x [0, B) is zeros (the device's rule).
    -> (states, actions, rewards, next_states, bad count)."""
    L, B = len(mem) - step, len(mem.buffers)
    good = [(0 <= i < L) and (0 <= b < B) for i, b in zip(idx, env)]
    batch = mem.windows([i if g else 0 for i, g in zip(idx, good)], [b if g else 0 for b, g in zip(env, good)], step)
    s, a, r, n = train_batch(batch, N)
    M = len(idx)
    for m, g in enumerate(good):
        if not g:
            for x in (s, a, r, n):
                x[m::M] = 0
    if last_only:
        a, r = a[:, -1], r[:, -1]
    return s, a, r, n, M - sum(good)


# ---- the device's layout ----
class RingMemory:
    """states [C + 1, B, N, S], actions / rewards [C + 1, B, N]; logical state j in row j mod (C + 1), transition j's
    action and reward in row j mod (C + 1)."""

    def __init__(self, capacity, B, N, S, dtype=np.float64, wrong=None):
        self.C, self.B, self.N, self.S, self.wrong = capacity, B, N, S, wrong
        self.rows = capacity + (0 if wrong == "wrap_at_C" else 1)
        self.states = np.zeros((self.rows, B, N, S), dtype)
        self.actions = np.zeros((self.rows, B, N), np.int32)
        self.rewards = np.zeros((self.rows, B, N), dtype)
        self.count = 0

    def begin(self, state):
        self.count = 0
        self.states[0] = state

    def add_many(self, actions, rewards, next_states):
        K = len(actions)
        assert K <= self.C
        for k in range(K):
            self.states[(self.count + 1 + k) % self.rows] = next_states[k]
            self.actions[(self.count + k) % self.rows] = actions[k]
            self.rewards[(self.count + k) % self.rows] = rewards[k] if np.ndim(rewards) == 3 else rewards
        self.count += K

    def __len__(self):
        return min(self.count, self.C)

    def sample(self, idx, env, step, last_only=False):
        N, S, M = self.N, self.S, len(idx)
        first = self.count - len(self)
        s = np.zeros((N * M, step, S), self.states.dtype)
        n = np.zeros_like(s)
        a = np.zeros((N * M, step), np.int32)
        r = np.zeros((N * M, step), self.rewards.dtype)
        for m, (i, b) in enumerate(zip(idx, env)):
            for sp in range(step + 1):
                j = first + int(i) + sp
                blk = self.states[j % self.rows, b]                 # [N, S]: one contiguous block
                if sp < step:
                    s[m::M, sp] = blk
                    a[m::M, sp] = self.actions[j % self.rows, b]
                    r[m::M, sp] = self.rewards[(j + (1 if self.wrong == "reward_next" else 0)) % self.rows, b]
                if sp >= 1:
                    n[m::M, sp - 1] = blk
        if last_only:
            a, r = a[:, -1], r[:, -1]
        return s, a, r, n


def replay_fixture(fx, mem, env=0, B=1, others=None):
    """Feed the fixture's trajectory as env `env` of a B-env memory (`others`: an rng for the other envs' data)."""
    def widen(x):
        full = np.zeros((B,) + x.shape, x.dtype) if others is None else \
            (others.standard_normal((B,) + x.shape).astype(np.float32).astype(x.dtype) if x.dtype != np.int32
             else others.integers(0, 32, size=(B,) + x.shape).astype(np.int32))
        full[env] = x
        return full
    mem.begin(widen(fx["state0"]))
    for j in range(fx["adds"]):
        a, r, s = widen(fx["actions"][j]), widen(fx["rewards"][j]), widen(fx["next_states"][j])
        if isinstance(mem, DequeMemory):
            mem.add(a, r, s)
        else:
            mem.add_many(a[None], r[None], s[None])


def fixture_expected(fx, M):
    """The recorded batch in the [N * M, step, S] form (m2's DQN reshapes are the step = 1 case of it)."""
    s, a, r, n = (fx["b%d_%s" % (M, k)] for k in ("states", "actions", "rewards", "next_states"))
    if not fx["lstm"]:
        s, n, a, r = s[:, None, :], n[:, None, :], a[:, None], r[:, None]
    return s, a, r, n
