"""`diral_memory_add` / `diral_memory_sample` / `ReplayMemory` on the device against the host statement of
tests/memory_cases.py - a literal deque of tuples plus the reference's four regrouping loops, which
tests/test_memory_cases.py holds against the reference's recorded batches.  Everything is compared bit for bit: the
launches copy and round, nothing more; the 16-bit outputs are compared with ``tensor.to(dtype)``."""
import functools

import numpy as np
import pytest
import torch

from diral_amd.config import bench_config, c2_config
from diral_amd.memory import ReplayMemory
from diral_amd.rollout import no_finalizers_during_capture
from diral_amd.vec_env import DiralError
from tests import memory_cases as H
from tests.gpu_util import make_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 31
RING = {"f32": torch.float32, "f64": torch.float64}
OUTS = {"f32": (torch.float32, torch.float16, torch.bfloat16), "f64": (torch.float64, torch.float32)}

# (B, N, S, C, step): every B of {1, 3}, N of {1, 4, 9, 64, 65}, S of {1, 23, 52, 85}, C of {step + 1, 7, 16}, step of {1, 6};
# N * S a multiple of 4 with S one (wide loads and stores), a multiple of 4 with odd S (wide loads, single stores), odd
# (single loads), and blocks off 16-byte alignment; a wave per block and a workgroup per block
CASES = [(1, 1, 1, 2, 1), (3, 4, 23, 16, 6), (3, 9, 23, 7, 6), (1, 64, 52, 16, 6), (3, 65, 85, 7, 1), (3, 64, 85, 16, 6),
         (1, 65, 52, 7, 6), (3, 1, 52, 2, 1), (1, 4, 85, 16, 1), (3, 9, 52, 16, 6), (1, 9, 1, 7, 1), (3, 64, 1, 7, 6),
         (1, 65, 23, 16, 6), (3, 4, 52, 7, 6)]
IDS = ["B%d-N%d-S%d-C%d-step%d" % c for c in CASES]


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def f32_values(rng, shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32).astype(np.float64)


def add_plan(C):
    """K = 1, K = C, then Ks that straddle the wrap of the C + 1 rows (the count ends well past it)."""
    return [1, C] + [max(1, C // 2), C - 1 if C > 1 else 1, 2 if C >= 2 else 1, max(1, C // 2)]


@functools.lru_cache(maxsize=None)
def filled(case, ring):
    """(device memory, host deque) after the same adds; data float64 that float32 holds exactly, so both rings hold it."""
    B, N, S, C, step = case
    rng = np.random.default_rng(hash(case) % 1000 + len(ring))
    mem = ReplayMemory(C, B, N, S, dtype=RING[ring], seed=SEED, device=DEV)
    dq = H.DequeMemory(C, B)
    s0 = f32_values(rng, (B, N, S))
    mem.begin(dev(s0))
    dq.begin(s0)
    for n, K in enumerate(add_plan(C)):
        a = rng.integers(0, 32, (K, B, N)).astype(np.int32)
        s = f32_values(rng, (K, B, N, S))
        bcast = n == 2
        r = f32_values(rng, (B, N) if bcast else (K, B, N), 3.0)
        src = torch.float32 if n % 2 else torch.float64             # the source dtype alternates, the rewards' against it
        mem.add_many(dev(a), dev(r, torch.float64 if n % 2 else torch.float32), dev(s, src))
        for k in range(K):
            dq.add(a[k], r if bcast else r[k], s[k])
    torch.cuda.synchronize()
    assert len(mem) == len(dq) == C and mem.count == sum(add_plan(C)) > C + 1
    return mem, dq


def guarded(shape, dtype, guard=16):
    """An output inside a larger buffer of sentinels: (the view, check()) - check() says the guards are untouched."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard,), 77, dtype=dtype, device=DEV)
    return buf[guard:guard + n].view(shape), lambda: bool((buf[:guard] == 77).all() and (buf[guard + n:] == 77).all())


def outputs(mem, M, step, out_dtype, last_only=False, keys=("states", "actions", "rewards", "next_states"),
            guard=16):
    rows = mem.N * M
    shapes = dict(states=((rows, step, mem.S), out_dtype), next_states=((rows, step, mem.S), out_dtype),
                  actions=((rows,) if last_only else (rows, step), torch.int32),
                  rewards=((rows,) if last_only else (rows, step), mem.dtype))
    out, checks = {}, []
    for k in keys:
        out[k], chk = guarded(*shapes[k], guard=guard)
        checks.append(chk)
    return out, lambda: all(c() for c in checks)


def expect(want, ring, out_dtype):
    """The host batch as the device should hold it: (states, actions, rewards, next_states) tensors on the CPU."""
    s, a, r, n = want[:4]
    cast = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(RING[ring]).to(out_dtype)   # noqa: E731
    plain = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dt)                   # noqa: E731
    return cast(s), plain(a, torch.int32), plain(r, RING[ring]), cast(n)


def same(got, want):
    return all(g is not None and g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.cpu(), w) for g, w in zip(got, want))


def window_sets(B, L, rng):
    """M = 1, a prime, R: (idx, env) lists; the M = R one holds every window once, shuffled."""
    R = B * L
    every = rng.permutation(R)
    sets = [([int(rng.integers(0, L))], [int(rng.integers(0, B))])]
    prime = max(p for p in (2, 3, 5, 7, 11, 13) if p <= max(R, 2))
    sets.append(([int(v) for v in rng.integers(0, L, prime)], [int(v) for v in rng.integers(0, B, prime)]))
    sets.append(([int(v) // B for v in every], [int(v) % B for v in every]))
    return sets


# ---- add + injected windows: shapes, dtypes, wrap, widths ----
@pytest.mark.parametrize("ring", ["f32", "f64"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_injected_windows_equal_the_host_statement(case, ring):
    B, N, S, C, step = case
    mem, dq = filled(case, ring)
    rng = np.random.default_rng(5)
    L = C - step
    for idx, env in window_sets(B, L, rng):
        M = len(idx)
        want = H.host_sample(dq, idx, env, step, N)
        assert want[4] == 0
        for od in OUTS[ring]:
            out, intact = outputs(mem, M, step, od)
            got = mem.sample(M, step, out_dtype=od, idx=idx, env=env, out=out)
            assert same(got, expect(want, ring, od)) and intact(), (M, od)
            assert torch.equal(mem.last_idx.cpu(), torch.tensor(idx, dtype=torch.int32))
            assert torch.equal(mem.last_env.cpu(), torch.tensor(env, dtype=torch.int32))
    # last_only and NULL outputs equal the full call (M = R)
    full = mem.sample(M, step, idx=idx, env=env)
    out, intact = outputs(mem, M, step, RING[ring], last_only=True)
    s, a, r, n = mem.sample(M, step, idx=idx, env=env, last_only=True, out=out)
    assert torch.equal(s, full[0]) and torch.equal(n, full[3]) and intact()
    assert torch.equal(a, full[1][:, -1]) and torch.equal(r, full[2][:, -1])
    for keys in (("states",), ("next_states",), ("actions", "rewards"), ("next_states", "rewards")):
        out, intact = outputs(mem, M, step, RING[ring], keys=keys)
        got = mem.sample(M, step, idx=idx, env=env, out=out)
        for k, g, f in zip(("states", "actions", "rewards", "next_states"), got, full):
            assert (g is None) if k not in keys else torch.equal(g, f), (keys, k)
        assert intact()
    assert int(mem.bad_samples.item()) == 0


def test_outputs_off_16_byte_alignment():
    """Output tensors that start one element into their allocation: the wide stores are not used, the batch is the same."""
    case = (1, 64, 52, 16, 6)
    mem, dq = filled(case, "f32")
    idx, env = [3, 0, 9, 5, 1], [0] * 5
    want = H.host_sample(dq, idx, env, 6, 64)
    for od in OUTS["f32"]:
        out, intact = outputs(mem, 5, 6, od, guard=1)
        assert out["states"].data_ptr() % 16 != 0
        assert same(mem.sample(5, 6, out_dtype=od, idx=idx, env=env, out=out), expect(want, "f32", od)) and intact()


# ---- windows outside the population ----
@pytest.mark.parametrize("case", [(3, 4, 23, 16, 6), (3, 65, 85, 7, 1)], ids=["toy", "odd"])
def test_bad_windows_are_zeros_and_counted(case):
    B, N, S, C, step = case
    mem, dq = filled(case, "f32")
    L = C - step
    idx = [0, L, L - 1, -1, 2, 2 ** 31 - 1, 1, 0]
    env = [0, 0, B - 1, 0, B, 1, -1, -(2 ** 31)]
    want = H.host_sample(dq, idx, env, step, N)
    assert want[4] == 6
    before = int(mem.bad_samples.item())
    for last_only in (False, True):
        w = H.host_sample(dq, idx, env, step, N, last_only)
        out, intact = outputs(mem, 8, step, torch.float32, last_only=last_only)
        assert same(mem.sample(8, step, idx=idx, env=env, last_only=last_only, out=out), expect(w, "f32", torch.float32)) and intact()
    assert int(mem.bad_samples.item()) == before + 12
    mem.bad_samples.zero_()


# ---- drawn windows ----
@pytest.mark.parametrize("case", [(1, 1, 1, 2, 1), (3, 4, 23, 16, 6), (3, 64, 85, 16, 6), (1, 65, 52, 7, 6)],
                         ids=["R1", "toy", "N64", "N65"])
def test_drawn_windows_equal_the_host_permutation(case):
    B, N, S, C, step = case
    mem, dq = filled(case, "f32")
    L = C - step
    R = B * L
    t0 = mem._t
    for n, M in enumerate(sorted({1, max(p for p in (1, 2, 3, 5, 7, 11, 13) if p <= R), R})):
        got = mem.sample(M, step)
        idx, env = mem.last_idx.cpu().numpy(), mem.last_env.cpu().numpy()
        widx, wenv = H.drawn_windows(M, B, L, H.memory_seed(SEED, t0 + n + 1))
        assert np.array_equal(idx, widx) and np.array_equal(env, wenv), M
        assert len(set(zip(idx.tolist(), env.tolist()))) == M and 0 <= idx.min() and idx.max() < L and 0 <= env.min() and env.max() < B
        assert same(got, expect(H.host_sample(dq, idx, env, step, N), "f32", torch.float32))
        again = mem.sample(M, step, idx=mem.last_idx, env=mem.last_env)          # replayed by injection
        assert all(torch.equal(g, a) for g, a in zip(got, again))
    assert mem._t == t0 + n + 1 and int(mem.bad_samples.item()) == 0
    with pytest.raises(DiralError):
        mem.sample(R + 1, step)                                     # more windows than pairs
    with pytest.raises(DiralError):
        mem.sample(1, C)                                            # len <= step
    assert mem._t == t0 + n + 1


def test_shards_draw_other_windows():
    a = ReplayMemory(16, 2, 4, 3, seed=SEED, device=DEV, env_offset=0)
    b = ReplayMemory(16, 2, 4, 3, seed=SEED, device=DEV, env_offset=2)
    for m in (a, b):
        m.begin(torch.zeros((2, 4, 3), device=DEV))
        m.add_many(torch.zeros((12, 2, 4), dtype=torch.int32, device=DEV), torch.zeros((2, 4), device=DEV),
                   torch.zeros((12, 2, 4, 3), device=DEV))
        m.sample(8, 4)
    assert not (torch.equal(a.last_idx, b.last_idx) and torch.equal(a.last_env, b.last_env))
    widx, wenv = H.drawn_windows(8, 2, 8, H.memory_seed(SEED, 1, env_offset=2))
    assert np.array_equal(b.last_idx.cpu().numpy(), widx) and np.array_equal(b.last_env.cpu().numpy(), wenv)


# ---- add: rounding, the broadcast row ----
def test_float64_into_a_float32_ring_is_rounded_once_and_float32_widens_exactly():
    B, N, S, C, K = 3, 9, 23, 7, 5
    g = torch.Generator(DEV).manual_seed(2)
    s0 = torch.randn((B, N, S), dtype=torch.float64, device=DEV, generator=g)
    s = torch.randn((K, B, N, S), dtype=torch.float64, device=DEV, generator=g) * 1e-3
    # ties to even, just above a tie, a subnormal of float32
    s[0, 0, 0, :4] = torch.tensor([1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 + 3 * 2.0 ** -24, 1e-42], device=DEV)
    r = torch.randn((K, B, N), dtype=torch.float64, device=DEV, generator=g)
    a = torch.randint(0, 32, (K, B, N), dtype=torch.int32, device=DEV, generator=g)
    lo, hi = ReplayMemory(C, B, N, S, torch.float32, device=DEV), ReplayMemory(C, B, N, S, torch.float64, device=DEV)
    lo.begin(s0)
    lo.add_many(a, r, s)
    assert torch.equal(lo.states[0].cpu(), s0.cpu().float()) and torch.equal(lo.states[1:K + 1].cpu(), s.cpu().float())
    assert torch.equal(lo.rewards[:K].cpu(), r.cpu().float()) and torch.equal(lo.actions[:K], a)
    hi.begin(s0.float())
    hi.add_many(a, r.float(), s.float())
    assert torch.equal(hi.states[0], s0.float().double()) and torch.equal(hi.states[1:K + 1], s.float().double())
    assert torch.equal(hi.rewards[:K], r.float().double())
    # float64 ring -> float32 output: one rounding
    hi2 = ReplayMemory(C, B, N, S, torch.float64, device=DEV)
    hi2.begin(s0)
    hi2.add_many(a, r, s)
    st, _, rw, nx = hi2.sample(2, 3, out_dtype=torch.float32, idx=[0, 1], env=[0, 2])
    full = hi2.sample(2, 3, idx=[0, 1], env=[0, 2])
    assert torch.equal(st.cpu(), full[0].cpu().float()) and torch.equal(nx.cpu(), full[3].cpu().float()) and rw.dtype == torch.float64


def test_broadcast_reward_row_equals_the_expanded_rewards():
    B, N, S, C, K = 3, 4, 23, 7, 6
    g = torch.Generator(DEV).manual_seed(4)
    s0 = torch.randn((B, N, S), device=DEV, generator=g)
    s = torch.randn((K, B, N, S), device=DEV, generator=g)
    r = torch.randn((B, N), dtype=torch.float64, device=DEV, generator=g)
    a = torch.randint(0, 3, (K, B, N), dtype=torch.int32, device=DEV, generator=g)
    one, many = ReplayMemory(C, B, N, S, device=DEV), ReplayMemory(C, B, N, S, device=DEV)
    for m in (one, many):
        m.begin(s0)
        m.add_many(a[:4], r.expand(4, B, N).contiguous(), s[:4])    # count 4: the next add crosses the wrap of 8 rows
    one.add_prefill(s, a, r)
    many.add_many(a, r.expand(K, B, N).contiguous(), s)
    for k in ("states", "actions", "rewards"):
        assert torch.equal(getattr(one, k), getattr(many, k)), k
    assert torch.equal(one.rewards[(4 + 5) % 8], r.float()) and len(one) == C and one.count == 10
    with pytest.raises(ValueError):
        one.add_many(torch.zeros((C + 1, B, N), dtype=torch.int32, device=DEV), r, torch.zeros((C + 1, B, N, S), device=DEV))


# ---- the reference's recorded batches ----
@pytest.mark.parametrize("B, env", [(1, 0), (3, 2)], ids=["B1", "env2-of-3"])
@pytest.mark.parametrize("key", ["m1", "m2", "m3"])
@pytest.mark.parametrize("ring", ["f32", "f64"])
def test_fixtures_replayed(key, ring, B, env):
    fx = H.load_fixture(key)
    mem = ReplayMemory(fx["C"], B, fx["N"], fx["S"], dtype=RING[ring], device=DEV)

    class Feed:                                                     # replay_fixture's protocol onto the device memory
        def begin(self, s):
            mem.begin(dev(s))

        def add_many(self, a, r, s):
            mem.add_many(dev(a), dev(r), dev(s))
    H.replay_fixture(fx, Feed(), env=env, B=B, others=np.random.default_rng(6))
    for M in fx["batches"]:
        got = mem.sample(M, fx["step"], idx=fx["b%d_idx" % M], env=[env] * M)
        assert same(got, expect(H.fixture_expected(fx, M), ring, RING[ring])), M
    assert int(mem.bad_samples.item()) == 0 and len(mem) == min(fx["adds"], fx["C"])


# ---- a real K-slot rollout ----
@pytest.mark.parametrize("which", ["toy", "N64"])
def test_add_rollout_equals_adding_the_slots_one_by_one(which):
    if which == "toy":
        cfg, B, K = bench_config(4, 3, 300.0, communication_range=120.0, State=dict(num_bins=20)), 5, 6
    else:
        cfg, B, K = c2_config(), 3, 6
    env, twin = make_env(cfg, B, dtype=torch.float32), make_env(cfg, B, dtype=torch.float32)
    for e in (env, twin):
        if which == "toy":
            e.use_subwave_path(slots=True)
        e.reset_topology(seed=3)
    N, A, S = env.N, env.A, env.S
    seq = torch.randint(0, A, (K, B, N), dtype=torch.int32, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    s0 = torch.randn((B, N, S), device=DEV, generator=torch.Generator(DEV).manual_seed(2))
    whole, single = ReplayMemory(4, B, N, S, device=DEV), ReplayMemory(4, B, N, S, device=DEV)
    whole.begin(s0)
    single.begin(s0)
    for lap in range(2):                                            # the second lap (K = 3) crosses the wrap of the 5 rows
        part = seq[:3 + lap].contiguous()
        out = env.rollout(part, states="all")
        whole.add_rollout(part, out)
        assert out["states"].shape == (3 + lap, B, N, S) and out["shaped"].abs().sum() > 0
        for k in range(3 + lap):
            o = twin.rollout(part[k:k + 1].contiguous(), states="all")
            single.add(part[k], o["shaped"][0], o["states"][0])
            assert torch.equal(o["states"][0], out["states"][k])
    for k in ("states", "actions", "rewards"):
        assert torch.equal(getattr(whole, k), getattr(single, k)), k
    assert whole.count == 7 and len(whole) == 4
    st, ac, rw, nx = whole.sample(2 * B, 2, idx=[0, 1] * B, env=[b for b in range(B) for _ in range(2)])
    # state = next_state inside a window; the last window ends one short of the newest state
    assert torch.equal(nx[:, 0], st[:, 1]) and torch.equal(nx[1, 1], out["states"][-2, 0, 0])
    env.check(); twin.check()


# ---- captured: [add, count + K, sample_clocked] ----
def test_captured_add_and_sample_replay_three_times():
    B, N, S, C, K, M, step = 3, 4, 23, 7, 4, 5, 2
    g = torch.Generator(DEV).manual_seed(9)
    mem = ReplayMemory(C, B, N, S, seed=SEED, device=DEV, count_on_device=True)
    ref = ReplayMemory(C, B, N, S, seed=SEED, device=DEV)
    a_in = torch.zeros((K, B, N), dtype=torch.int32, device=DEV)
    r_in = torch.zeros((K, B, N), dtype=torch.float64, device=DEV)
    s_in = torch.zeros((K, B, N, S), device=DEV)
    out, intact = outputs(mem, M, step, torch.bfloat16)

    def fresh():
        a_in.copy_(torch.randint(0, 9, a_in.shape, dtype=torch.int32, device=DEV, generator=g))
        r_in.copy_(torch.randn(r_in.shape, dtype=torch.float64, device=DEV, generator=g))
        s_in.copy_(torch.randn(s_in.shape, device=DEV, generator=g))

    def round_():
        mem.add_many(a_in, r_in, s_in)                              # ... and count_dev += K behind it
        mem.sample_clocked(M, step, mem.count_dev, out_dtype=torch.bfloat16, out=out)

    def eager():
        ref.add_many(a_in, r_in, s_in)
        ref._t = ref.count - 1                                      # the call number the clocked form draws with: the count
        return ref.sample(M, step, out_dtype=torch.bfloat16)

    s0 = torch.randn((B, N, S), device=DEV, generator=g)
    mem.begin(s0)
    ref.begin(s0)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    fresh()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        round_()                                                    # eagerly first: it takes state0
    torch.cuda.synchronize()
    want = eager()
    assert all(torch.equal(out[k], w) for k, w in zip(("states", "actions", "rewards", "next_states"), want))
    graph = torch.cuda.CUDAGraph()
    with no_finalizers_during_capture():
        with torch.cuda.graph(graph, stream=stream):
            round_()
    torch.cuda.synchronize()
    # (the capture itself ran nothing: the count is still K)
    assert int(mem.count_dev.item()) == K
    seen = []
    for n in range(3):
        fresh()
        graph.replay()
        torch.cuda.synchronize()
        want = eager()
        assert all(torch.equal(out[k], w) for k, w in zip(("states", "actions", "rewards", "next_states"), want)), n
        assert torch.equal(mem.last_idx, ref.last_idx) and torch.equal(mem.last_env, ref.last_env) and intact()
        seen.append(tuple(mem.last_idx.tolist()) + tuple(mem.last_env.tolist()))
    assert len(set(seen)) == 3 and int(mem.count_dev.item()) == 4 * K == ref.count and len(mem) == C
    for k in ("states", "actions", "rewards"):
        assert torch.equal(getattr(mem, k), getattr(ref, k)), k
    assert int(mem.bad_samples.item()) == 0
    # with the count on the device the kernel itself refuses what the host cannot see: zeros, every window counted
    small = ReplayMemory(C, B, N, S, device=DEV, count_on_device=True)
    small.begin(s0)
    small.add_many(a_in[:2], r_in[:2], s_in[:2])                    # len = 2 = step
    st, ac, rw, nx = small.sample(M, 2)
    assert not st.any() and not nx.any() and not ac.any() and not rw.any() and int(small.bad_samples.item()) == M
    small.add_many(a_in[:1], r_in[:1], s_in[:1])                    # len = 3: R = 3 < M
    small.sample(M, 2)
    assert int(small.bad_samples.item()) == 2 * M
    st, _, _, _ = small.sample(3, 2)
    assert st.any() and int(small.bad_samples.item()) == 2 * M


def test_state_dict_round_trip():
    case = (3, 9, 23, 7, 6)
    mem, dq = filled(case, "f32")
    sd = mem.state_dict()
    for dev_count in (False, True):
        other = ReplayMemory(7, 3, 9, 23, seed=SEED, device=DEV, count_on_device=dev_count)
        other.load_state_dict(sd)
        assert len(other) == len(mem) == 7
        idx, env = [0], [2]
        assert all(torch.equal(a, b) for a, b in zip(other.sample(1, 6, idx=idx, env=env), mem.sample(1, 6, idx=idx, env=env)))
        if not dev_count:
            t0 = mem._t
            other.sample(3, 6)
            mem.sample(3, 6)
            assert torch.equal(other.last_idx, mem.last_idx) and torch.equal(other.last_env, mem.last_env) and mem._t == t0 + 1
    sd["states"].zero_()                                            # a copy, not a view of the rings
    assert mem.states.abs().sum() > 0
