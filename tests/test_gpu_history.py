"""`diral_memory_history` / `ReplayMemory.history` on the device against a literal ``deque(maxlen=step)`` fed the same
states, with ``np.array(d)[:, b, n]`` per agent (tests/td_cases.py, which tests/test_td_cases.py holds against the feeds the
reference's ``infer_action`` recorded).  Compared bit for bit: the launch copies and rounds, nothing more; the 16-bit
outputs are compared with ``tensor.to(dtype)``."""
import numpy as np
import pytest
import torch

from diral_amd.config import bench_config
from diral_amd.memory import ReplayMemory
from diral_amd.rollout import no_finalizers_during_capture
from diral_amd.vec_env import DiralError
from tests import td_cases as H
from tests.gpu_util import make_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RING = {"f32": torch.float32, "f64": torch.float64}
OUTS = {"f32": (torch.float32, torch.float16, torch.bfloat16), "f64": (torch.float64, torch.float32)}
# odd sizes - every vector-width tail, a wave per item - and the wide path (N * S a multiple of 4, a workgroup per item)
SHAPES = [(3, 5, 7), (2, 64, 52)]
IDS = ["B3-N5-S7", "B2-N64-S52"]


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def f32_values(rng, shape):
    return rng.standard_normal(shape).astype(np.float32).astype(np.float64)


def guarded(shape, dtype, guard=16):
    """An output inside a larger buffer of sentinels: (the view, check()) - check() says the guards are untouched."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard,), 77, dtype=dtype, device=DEV)
    return buf[guard:guard + n].view(shape), lambda: bool((buf[:guard] == 77).all() and (buf[guard + n:] == 77).all())


def expect(states, step, ring, out_dtype):
    """The deque's window of the states so far as the device should hold it (a CPU tensor)."""
    return torch.from_numpy(H.agent_feeds(H.deque_window(states, step))).to(RING[ring]).to(out_dtype)


def check(mem, states, step, ring, out_dtype=None, guard=16):
    od = RING[ring] if out_dtype is None else out_dtype
    out, intact = guarded((mem.B * mem.N, step, mem.S), od, guard)
    got = mem.history(step, out_dtype=od, out=out)
    assert got is out and torch.equal(got.cpu(), expect(states, step, ring, od)) and intact(), (len(states), step, od)


@pytest.mark.parametrize("ring", ["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_window_equals_the_deque_before_at_and_across_the_wrap(shape, ring):
    B, N, S = shape
    C = 5
    rng = np.random.default_rng(B + N)
    mem = ReplayMemory(C, B, N, S, dtype=RING[ring], device=DEV)
    states = [f32_values(rng, (B, N, S))]
    mem.begin(dev(states[0]))
    check(mem, states, 1, ring)                                     # right after begin: the begin state ...
    with pytest.raises(DiralError):
        mem.history(2)                                              # ... and nothing in front of it
    for count in range(1, 13):                                      # adds 1 ... 12
        states.append(f32_values(rng, (B, N, S)))
        mem.add(dev(rng.integers(0, 9, (B, N)).astype(np.int32)), dev(f32_values(rng, (B, N))), dev(states[-1]))
        largest = min(count, C) + 1
        for step in sorted({1, min(3, largest), largest}):
            check(mem, states, step, ring)
        with pytest.raises(DiralError):
            mem.history(largest + 1)
    for od in OUTS[ring]:                                           # every dtype pair; an output off 16-byte alignment
        check(mem, states, 3, ring, od)
        check(mem, states, 6, ring, od, guard=1)
    assert int(mem.bad_samples.item()) == 0
    with pytest.raises(ValueError):
        mem.history(0)
    with pytest.raises(ValueError):
        mem.history(3, out_dtype=torch.float16 if ring == "f64" else torch.float64,
                    out=torch.zeros((B * N, 3, S), device=DEV))     # (the out tensor's dtype is checked first)


def test_window_after_add_many_and_sample_is_left_alone():
    B, N, S, C, K = 3, 5, 7, 7, 5
    rng = np.random.default_rng(2)
    mem = ReplayMemory(C, B, N, S, device=DEV)
    states = [f32_values(rng, (B, N, S))]
    mem.begin(dev(states[0]))
    for _ in range(2):                                              # the second add crosses the wrap of the 8 rows
        nxt = f32_values(rng, (K, B, N, S))
        mem.add_many(dev(rng.integers(0, 9, (K, B, N)).astype(np.int32)), dev(f32_values(rng, (K, B, N))), dev(nxt))
        states += list(nxt)
        for step in (1, 4, K + 1):
            check(mem, states, step, "f32")
    idx, env = [0, 2, 1], [0, 1, 2]
    before = mem.sample(3, 4, idx=idx, env=env)
    rings = [getattr(mem, k).clone() for k in ("states", "actions", "rewards")]
    check(mem, states, C + 1, "f32", torch.bfloat16)
    after = mem.sample(3, 4, idx=idx, env=env)
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert all(torch.equal(getattr(mem, k), r) for k, r in zip(("states", "actions", "rewards"), rings))
    # the window's last row is the one state no sampled window holds: the newest
    assert torch.equal(mem.history(1).view(B, N, S), mem.states[mem.count % (C + 1)])


def test_window_after_a_rollout_into_the_memory():
    cfg, B, K = bench_config(4, 3, 300.0, communication_range=120.0, State=dict(num_bins=20)), 5, 3
    env = make_env(cfg, B, dtype=torch.float32)
    env.use_subwave_path(slots=True)
    env.reset_topology(seed=3)
    N, A, S = env.N, env.A, env.S
    g = torch.Generator(DEV).manual_seed(1)
    mem = ReplayMemory(4, B, N, S, device=DEV)
    s0 = torch.randn((B, N, S), device=DEV, generator=g)
    mem.begin(s0)
    states = [s0.cpu().numpy()]
    for lap in range(2):                                            # the second lap crosses the wrap of the 5 rows
        seq = torch.randint(0, A, (K, B, N), dtype=torch.int32, device=DEV, generator=g)
        env.rollout(seq, memory=mem)
        rows = [(mem.count - K + 1 + k) % 5 for k in range(K)]
        states += [mem.states[r].cpu().numpy() for r in rows]
        assert np.abs(states[-1]).sum() > 0
        for step in (1, 2, min(mem.count, 4) + 1):
            check(mem, states, step, "f32")
    env.check()


def test_counted_on_the_device_a_captured_window_moves_on_at_every_replay():
    B, N, S, C, step = 3, 5, 7, 5, 3
    g = torch.Generator(DEV).manual_seed(9)
    mem = ReplayMemory(C, B, N, S, device=DEV, count_on_device=True)
    a_in = torch.zeros((B, N), dtype=torch.int32, device=DEV)
    r_in = torch.zeros((B, N), device=DEV)
    s_in = torch.zeros((B, N, S), device=DEV)
    out, intact = guarded((B * N, step, S), torch.float32)
    states = [torch.randn((B, N, S), device=DEV, generator=g)]
    mem.begin(states[0])

    def fresh():
        s_in.copy_(torch.randn(s_in.shape, device=DEV, generator=g))
        states.append(s_in.clone())

    def round_():
        mem.add(a_in, r_in, s_in)                                   # ... and count_dev += 1 behind it
        mem.history(step, out=out)

    def want():
        return expect([s.cpu().numpy() for s in states], step, "f32", torch.float32)

    # a window longer than the live states: zeros, counted once, with the count where the host cannot see it
    assert not mem.history(2).any() and int(mem.bad_samples.item()) == 1
    assert torch.equal(mem.history(1).cpu(), expect([states[0].cpu().numpy()], 1, "f32", torch.float32))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        fresh()
        mem.add(a_in, r_in, s_in)                                   # the first add takes state0: two live states ...
        fresh()
        round_()                                                    # ... and the third: the window fits
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want())
    graph = torch.cuda.CUDAGraph()
    with no_finalizers_during_capture():
        with torch.cuda.graph(graph, stream=stream):
            round_()
    torch.cuda.synchronize()
    assert int(mem.count_dev.item()) == 2                           # (the capture itself ran nothing)
    seen = []
    for n in range(5):                                              # past the wrap of the 6 rows
        fresh()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want()) and intact(), n
        seen.append(out.clone())
    assert int(mem.count_dev.item()) == 7 and int(mem.bad_samples.item()) == 1
    assert torch.equal(seen[1][:, :2], seen[0][:, 1:]) and not torch.equal(seen[1], seen[0])   # the window slid by one
    assert not mem.history(C + 2).any() and int(mem.bad_samples.item()) == 2


def test_the_reference_s_feeds():
    fx = H.load_fixture("h1")
    T, N, S, step = (int(v) for v in fx["meta"])
    for B, env in ((1, 0), (3, 2)):
        rng = np.random.default_rng(6)
        mem = ReplayMemory(4, B, N, S, dtype=torch.float64, device=DEV)
        full = rng.standard_normal((T, B, N, S))
        full[:, env] = fx["states"]
        mem.begin(dev(rng.standard_normal((B, N, S))))
        for s in full:                                              # history_input.append(state) behind every add
            mem.add(dev(np.zeros((B, N), np.int32)), dev(np.zeros((B, N))), dev(s))
        got = mem.history(step).view(B, N, step, S)[env].cpu().numpy()
        assert np.array_equal(got, fx["feeds_lstm"])
        assert np.array_equal(mem.history(1).view(B, N, S)[env].cpu().numpy(), fx["feeds_dqn"])
