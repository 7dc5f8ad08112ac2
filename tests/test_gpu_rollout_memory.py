"""`VecV2VEnv.rollout(memory=)` / `prefill(memory=)` - the K-slot launches write the replay memory's ring rows themselves
(`diral_env_rollout_memory` / `diral_env_prefill_memory`) - against the two-call form they stand for: a twin handle runs
``rollout(states="all")`` + ``add_rollout`` (``prefill`` + ``add_prefill``) into a second memory.  Both memories start from
the same sentinel fill and the same ``begin(state)``; everything is compared bit for bit - the three whole rings (so rows
the launch must not write are seen untouched), the counts, sampled windows, the launches' other outputs and the envs."""
import ctypes

import pytest
import torch

from diral_amd.config import DT_F32, DT_F64, ERR_BAD_ARG, ERR_UNSUPPORTED, KERNEL_FAST64, KERNEL_POLICY, KERNEL_SUBWAVE, bench_config
from diral_amd.driver import DriverLoop
from diral_amd.memory import ReplayMemory
from diral_amd.rollout import no_finalizers_during_capture
from diral_amd.vec_env import DiralError, VecV2VEnv
from tests.kslots_harness import DEV, VEL_SEED, assert_equal, assert_same_envs, chain_cfg, start, stuck_penalty_state, twins

pytestmark = pytest.mark.gpu
C = 7
PLAN = [1, 7, 3, 6, 2, 3]          # add_plan(7) of tests/test_gpu_memory.py: K = 1, K = C, then across the wrap of the 8 rows
F = {"f32": torch.float32, "f64": torch.float64}


def toy(N, A):
    return bench_config(N, A, 300.0, communication_range=120.0, State=dict(num_bins=20))


def pair(cfg, B, dtype, seed=31, subwave=False):
    env, twin = twins(cfg, B, dtype, start(cfg, B, seed))
    if subwave:
        for e in (env, twin):
            e.use_subwave_path(slots=True)
    return env, twin


def memories(env, capacity=C, **kw):
    """(the launches' memory, the two-call form's): sentinels in every ring row, the same begin(state)."""
    g = torch.Generator(DEV).manual_seed(5)
    s0 = torch.randn((env.B, env.N, env.S), dtype=torch.float64, device=DEV, generator=g)      # (cast to the rings' dtype)
    mems = []
    for n in range(2):
        m = ReplayMemory(capacity, env.B, env.N, env.S, dtype=env.out_dtype, seed=3, device=DEV, **(kw if n == 0 else {}))
        m.states.fill_(-7.0); m.actions.fill_(-7); m.rewards.fill_(-7.0)
        m.begin(s0)
        mems.append(m)
    return mems


def same_memories(mem, ref, what):
    for key in ("states", "actions", "rewards"):
        assert_equal(getattr(ref, key), getattr(mem, key), (what, key))
    count = mem.count if mem.count_dev is None else int(mem.count_dev.item())
    assert count == ref.count and len(mem) == len(ref), (what, count, ref.count)


def same_windows(mem, ref, step=2):
    """Injected windows: every start of the live range on every env."""
    L = len(ref) - step
    if L < 1:
        return
    idx = [i for i in range(L) for _ in range(ref.B)]
    env = [b for _ in range(L) for b in range(ref.B)]
    got, want = mem.sample(len(idx), step, idx=idx, env=env), ref.sample(len(idx), step, idx=idx, env=env)
    for k, (g, w) in enumerate(zip(got, want)):
        assert_equal(w, g, ("window", k))
    assert int(mem.bad_samples.item()) == 0 == int(ref.bad_samples.item())


def rollouts(env, twin, mem, ref, plan, mode="my_step", avg=False, pen=False, sticky=False, **extra):
    """The launches of `plan` (slots per launch) into `mem`, the two calls on the twin into `ref`, compared behind each."""
    B, N = env.B, env.N
    pens = [stuck_penalty_state(B, N) if pen else None for _ in range(2)]
    prev = [torch.zeros((B,), dtype=torch.int64, device=DEV) for _ in range(2)] if extra.pop("ia_avg", False) else None
    t = 0
    for n, K in enumerate(plan):
        seq = torch.stack([env.sample(700 + 10 * n + (k // 4 if sticky else k)) for k in range(K)])
        kw = dict(mode=mode, global_reward_avg=avg, vel_seed=VEL_SEED, **extra)
        got = env.rollout(seq, t, stuck_penalty=pens[0], memory=mem, **dict(kw, **(dict(sum_ia_prev=prev[0]) if prev else {})))
        want = twin.rollout(seq, t, states="all", stuck_penalty=pens[1], **dict(kw, **(dict(sum_ia_prev=prev[1]) if prev else {})))
        ref.add_rollout(seq, want)
        torch.cuda.synchronize()
        assert set(got) == set(want) and got["shaped"] is None and want["shaped"] is not None
        if mem.count_dev is None:
            assert_equal(want["states"][-1], got["states"], (n, "states"))
            assert got["states"].data_ptr() == mem.states[mem.count % (mem.C + 1)].data_ptr()
        else:
            assert got["states"] is None
        for key in set(want) - {"states", "shaped"}:
            assert_equal(want[key], got[key], (n, key))
        same_memories(mem, ref, n)
        assert env.last_kernel() == twin.last_kernel() and (env.last_kernel() & KERNEL_POLICY)
        t += K
        assert env.t == t == twin.t
    if pen:
        assert torch.equal(pens[0][2], pens[1][2]) and torch.equal(pens[0][3], pens[1][3])
    if prev:
        assert torch.equal(prev[0], prev[1])
    same_windows(mem, ref)
    assert_same_envs(env, twin)
    env.check(); twin.check()
    return pens[0]


def prefills(env, twin, mem, ref, plan, mode="my_step_design"):
    g = torch.Generator(DEV).manual_seed(8)
    rews0 = torch.randn((env.B, env.N), dtype=torch.float64, device=DEV, generator=g)   # (float32 rings round it once, both ways)
    seed = 40
    a0 = env.sample(seed)
    for n, K in enumerate(plan):
        last, none, a_next = env.prefill(a0, K, seed, rew_in=rews0, mode=mode, memory=mem)
        st, a_all, w_next = twin.prefill(a0, K, seed, rew_in=rews0, mode=mode)
        ref.add_prefill(st, a_all, rews0)
        torch.cuda.synchronize()
        assert none is None
        assert_equal(w_next, a_next, (n, "next actions"))
        assert_equal(st[-1], last, (n, "last state"))
        same_memories(mem, ref, n)
        assert env.last_kernel() == twin.last_kernel() and (env.last_kernel() & KERNEL_POLICY)
        a0, seed = a_next, seed + K
    same_windows(mem, ref)
    assert_same_envs(env, twin)
    env.check(); twin.check()


# ---- the fast64 slot loop: full and partial wave, both dtypes, both modes, plain and rich state vectors ----
@pytest.mark.parametrize("N,A,dt,mode,rich", [(64, 32, "f32", "my_step", False), (64, 32, "f64", "my_step_ch", True),
                                              (9, 5, "f32", "my_step_ch", True), (9, 5, "f64", "my_step", False),
                                              (9, 5, "f32", "my_step", False), (64, 32, "f32", "my_step", True)],
                         ids=lambda v: str(v))
def test_fast64_rollout_into_the_rings(N, A, dt, mode, rich):
    cfg = chain_cfg(N, A, 2, vary=True, rich=rich)
    env, twin = pair(cfg, 3, F[dt], seed=N + A)
    mem, ref = memories(env)
    rollouts(env, twin, mem, ref, PLAN, mode=mode)
    assert (env.last_kernel() & 15) == KERNEL_FAST64


def test_fast64_stuck_penalty_and_global_average():
    """Actions held for four slots with 3 resources for 9 vehicles: the penalty counters pass the threshold."""
    cfg = chain_cfg(9, 3, 2, rich=True)
    env, twin = pair(cfg, 3, torch.float32)
    mem, ref = memories(env)
    pn = rollouts(env, twin, mem, ref, PLAN, avg=True, pen=True, sticky=True)
    assert int(pn[2].max()) > 2


@pytest.mark.parametrize("N,A,dt", [(64, 32, "f32"), (9, 5, "f64")])
def test_fast64_with_the_information_age_block(N, A, dt):
    cfg = chain_cfg(N, A, 2, track=True)
    env, twin = pair(cfg, 3, F[dt])
    mem, ref = memories(env)
    rollouts(env, twin, mem, ref, PLAN, mode="my_step_ch", info_age=True, ia_avg=True)


@pytest.mark.parametrize("N,A,dt", [(9, 5, "f32"), (64, 32, "f64")])
def test_fast64_with_the_position_log(N, A, dt):
    cfg = chain_cfg(N, A, 2, vary=True)
    env, twin = pair(cfg, 3, F[dt])
    mem, ref = memories(env)
    rollouts(env, twin, mem, ref, PLAN, log_positions=True)


@pytest.mark.parametrize("N,A,dt,mode", [(64, 32, "f32", "my_step_design"), (9, 5, "f64", "my_step_ch"),
                                         (9, 5, "f32", "my_step_design"), (64, 32, "f64", "my_step_ch")])
def test_fast64_prefill_into_the_rings(N, A, dt, mode):
    cfg = chain_cfg(N, A, 2, rich=(N == 9))
    env, twin = pair(cfg, 3, F[dt])
    mem, ref = memories(env)
    prefills(env, twin, mem, ref, PLAN, mode=mode)
    assert (env.last_kernel() & 15) == KERNEL_FAST64


def test_capacity_equal_to_the_slots_rewrites_every_action_row():
    cfg = chain_cfg(9, 5, 2)
    env, twin = pair(cfg, 3, torch.float32)
    mem, ref = memories(env, capacity=5)
    rollouts(env, twin, mem, ref, [5, 5, 5])
    env2, twin2 = pair(cfg, 3, torch.float32)
    mem2, ref2 = memories(env2, capacity=5)
    prefills(env2, twin2, mem2, ref2, [5, 5])


# ---- the sub-wave slot loop: G = 4 and G = 8, a partly filled second block ----
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("N,A", [(4, 3), (8, 5)])
def test_subwave_rollout_and_prefill_into_the_rings(N, A, dt):
    cfg = toy(N, A)
    env, twin = pair(cfg, 70, F[dt], subwave=True)
    mem, ref = memories(env)
    rollouts(env, twin, mem, ref, PLAN, avg=True)
    assert (env.last_kernel() & 15) == KERNEL_SUBWAVE
    env2, twin2 = pair(cfg, 70, F[dt], subwave=True)
    mem2, ref2 = memories(env2)
    prefills(env2, twin2, mem2, ref2, PLAN)
    assert (env2.last_kernel() & 15) == KERNEL_SUBWAVE


# ---- the count in device memory: eagerly, and as a captured [rollout into the rings, count + K, sample_clocked] ----
def nodes_and_edges(graph):
    """(number of nodes, [(from, to)]) of a captured graph kept by torch (``CUDAGraph(keep_graph=True)``), read through the
    HIP runtime the process already holds."""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    g = ctypes.c_void_p(graph.raw_cuda_graph())
    n, m = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, ctypes.byref(n)) == 0 and hip.hipGraphGetEdges(g, None, None, ctypes.byref(m)) == 0
    src, dst = (ctypes.c_void_p * max(m.value, 1))(), (ctypes.c_void_p * max(m.value, 1))()
    assert hip.hipGraphGetEdges(g, src, dst, ctypes.byref(m)) == 0
    return n.value, [(src[i], dst[i]) for i in range(m.value)]


@pytest.mark.parametrize("which", ["fast64", "subwave"])
def test_device_count_eager_and_captured(which):
    if which == "fast64":
        cfg, B, sub = chain_cfg(9, 5, 2, rich=True), 3, False
    else:
        cfg, B, sub = toy(4, 3), 70, True
    env, twin = pair(cfg, B, torch.float32, subwave=sub)
    mem, ref = memories(env, count_on_device=True)
    K, M, step = 3, 3, 2                                           # (M <= B windows: the first round has one start per env)
    seq = torch.zeros((K, B, env.N), dtype=torch.int32, device=DEV)
    outs = {k: None for k in ("states", "actions", "rewards", "next_states")}

    def fresh(n):
        seq.copy_(torch.stack([env.sample(300 + 10 * n + k) for k in range(K)]))

    def round_():
        got = env.rollout(seq, 0, global_reward_avg=True, memory=mem)             # ... and count_dev += K behind it
        assert got["states"] is None and got["shaped"] is None
        res = mem.sample_clocked(M, step, mem.count_dev)
        for k, r in zip(outs, res):
            outs[k] = r

    def eager():
        ref.add_rollout(seq, twin.rollout(seq, 0, states="all", global_reward_avg=True))
        ref._t = ref.count - 1                                      # the call number the clocked form draws with: the count
        return ref.sample(M, step)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    for n in range(2):                                              # eagerly first (the first takes state0; len 6 > step)
        fresh(n)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            round_()
        torch.cuda.synchronize()
        want = eager()
        assert all(torch.equal(outs[k], w) for k, w in zip(outs, want)), n
        same_memories(mem, ref, ("eager", n))
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with no_finalizers_during_capture():
        with torch.cuda.graph(graph, stream=stream):
            round_()
    torch.cuda.synchronize()
    assert int(mem.count_dev.item()) == 2 * K                      # (the capture itself ran nothing)
    # one linear chain: rollout -> count + K -> sample, no node with two successors or two predecessors
    nodes, edges = nodes_and_edges(graph)
    assert nodes >= 3 and len(edges) == nodes - 1, (nodes, edges)
    assert len({a for a, _ in edges}) == len(edges) == len({b for _, b in edges}), edges
    for n in range(3):                                              # the launches cross the wrap of the 8 rows
        fresh(2 + n)
        graph.replay()
        torch.cuda.synchronize()
        want = eager()
        assert all(torch.equal(outs[k], w) for k, w in zip(outs, want)), n
        assert torch.equal(mem.last_idx, ref.last_idx) and torch.equal(mem.last_env, ref.last_env)
        same_memories(mem, ref, ("replay", n))
    assert int(mem.count_dev.item()) == 5 * K > C + 1 and int(mem.bad_samples.item()) == 0
    assert_same_envs(env, twin)
    env.check(); twin.check()


# ---- refusals: the env and the rings as they were ----
def untouched(env, twin, mem, ref):
    same_memories(mem, ref, "refused")
    assert mem._state0 is not None and bool((mem.states == -7).all()) and bool((mem.actions == -7).all())
    assert_same_envs(env, twin)


def test_refusals_leave_env_and_rings_untouched():
    # N = 65: the wide slot loop does not take the block
    cfg = chain_cfg(65, 32, 2)
    env, twin = pair(cfg, 2, torch.float32)
    mem, ref = memories(env)
    seq = torch.stack([env.sample(k) for k in range(3)])
    with pytest.raises(DiralError) as ei:
        env.rollout(seq, 0, memory=mem)
    assert ei.value.status == ERR_UNSUPPORTED
    with pytest.raises(DiralError) as ei:
        env.prefill(env.sample(1), 3, 1, rew_in=torch.zeros((2, 65), device=DEV), memory=mem)
    assert ei.value.status == ERR_UNSUPPORTED
    untouched(env, twin, mem, ref)
    # a toy handle pinned without slots=True
    cfg = toy(4, 3)
    env, twin = pair(cfg, 5, torch.float32)
    for e in (env, twin):
        e.use_subwave_path()
    mem, ref = memories(env)
    seq = torch.stack([env.sample(k) for k in range(3)])
    with pytest.raises(DiralError) as ei:
        env.rollout(seq, 0, memory=mem)
    assert ei.value.status == ERR_UNSUPPORTED
    untouched(env, twin, mem, ref)
    # ring dtype != out dtype, K > C, other shapes: Python says so; the C-ABI says DIRAL_ERR_BAD_ARG
    cfg = chain_cfg(9, 5, 2)
    env, twin = pair(cfg, 3, torch.float32)
    mem, ref = memories(env)
    seq = torch.stack([env.sample(k) for k in range(C + 1)])
    other = ReplayMemory(C, 3, 9, env.S, dtype=torch.float64, device=DEV)
    other.begin(torch.zeros((3, 9, env.S), device=DEV))
    for m, s in ((other, seq[:3].contiguous()), (mem, seq), (ReplayMemory(C, 3, 9, env.S + 1, device=DEV), seq[:3].contiguous())):
        with pytest.raises(ValueError):
            env.rollout(s, 0, memory=m)
        with pytest.raises(ValueError):
            env.prefill(env.sample(1), int(s.shape[0]), 1, rew_in=torch.zeros((3, 9), device=DEV), memory=m)
    with pytest.raises(ValueError):
        env.prefill(env.sample(1), 3, 1, memory=mem)                # no rew_in
    untouched(env, twin, mem, ref)


def test_c_abi_bad_arguments_on_a_live_handle():
    """Every DIRAL_ERR_BAD_ARG of the block on an otherwise valid call (the same call with a good block is taken last)."""
    from diral_amd._tensors import _ptr
    from diral_amd.config import STEP_DESIGN, STEP_MY_STEP, DiralRollout
    cfg = chain_cfg(9, 5, 2)
    env, twin = pair(cfg, 3, torch.float32)
    mem, ref = memories(env)
    K = 3
    seq = torch.stack([env.sample(k) for k in range(K)])
    ro = DiralRollout()
    ro.struct_bytes = ctypes.sizeof(DiralRollout)
    scratch = torch.zeros((K, 3, 9, env.S), device=DEV)
    shaped = torch.zeros((K, 3, 9), device=DEV)
    a_next = torch.zeros((3, 9), dtype=torch.int32, device=DEV)
    rin = torch.zeros((3, 9), dtype=torch.float64, device=DEV)

    def roll(m, states=None, ro=ro, dt=DT_F32, slots=K):
        return env.lib.diral_env_rollout_memory(env._h, STEP_MY_STEP, _ptr(seq), slots, 0, _ptr(states), 0, _ptr(env._rew),
                                                _ptr(env._done), dt, ctypes.byref(ro), None, None, ctypes.byref(m), env._stream())

    def fill(m, states=None, a_all=None, rew=rin, slots=K):
        return env.lib.diral_env_prefill_memory(env._h, STEP_DESIGN, _ptr(seq[0]), slots, 1, _ptr(states), DT_F32, _ptr(a_all),
                                                _ptr(a_next), _ptr(rew), 0.0, 1.0, ctypes.byref(m), env._stream())

    def block(**kw):
        m = mem._desc()
        for k, v in kw.items():
            setattr(m, k, v)
        return m
    bad = [dict(struct_bytes=8), dict(states=None), dict(actions=None), dict(rewards=None), dict(capacity=0), dict(capacity=K - 1),
           dict(count=-1), dict(batch=4), dict(num_users=8), dict(state_space=env.S + 1), dict(dtype=DT_F64)]
    for kw in bad:
        assert roll(block(**kw)) == ERR_BAD_ARG, kw
        assert fill(block(**kw)) == ERR_BAD_ARG, kw
    assert roll(block(), states=scratch) == ERR_BAD_ARG
    ro2 = DiralRollout()
    ro2.struct_bytes = ctypes.sizeof(DiralRollout)
    ro2.shaped_out = _ptr(shaped)
    assert roll(block(), ro=ro2) == ERR_BAD_ARG
    assert roll(block(), dt=DT_F64) == ERR_BAD_ARG                  # ring dtype != out dtype
    assert fill(block(), states=scratch) == ERR_BAD_ARG
    assert fill(block(), a_all=seq) == ERR_BAD_ARG
    assert fill(block(), rew=None) == ERR_BAD_ARG
    torch.cuda.synchronize()
    untouched(env, twin, mem, ref)
    assert roll(block()) == 0                                       # the good block: taken
    torch.cuda.synchronize()
    assert not bool((mem.states[1:K + 1] == -7).any()) and bool((mem.states[K + 1:] == -7).all()) and bool((mem.states[0] == -7).all())
    env.check()


# ---- the driver: the same rings where the launch is refused ----
@pytest.mark.parametrize("N,A", [(65, 32), (9, 5)], ids=["N65-falls-back", "N9-direct"])
def test_driver_loop_fills_the_same_rings_either_way(N, A):
    cfg = chain_cfg(N, A, 2)
    env, twin = pair(cfg, 2, torch.float32)
    mem, ref = memories(env)
    d1, d2 = DriverLoop(env, global_reward_avg=True), DriverLoop(twin, global_reward_avg=True)
    for d in (d1, d2):                                              # (the bootstrap's stale rewards)
        d._rews0 = torch.randn((2, N), device=DEV, generator=torch.Generator(DEV).manual_seed(6))
    # prefill, then two rollouts across the wrap
    d1.prefill(4, 11, memory=mem)
    st, acts = d2.prefill(4, 11)
    ref.add_prefill(st, acts, d2._rews0)
    same_memories(mem, ref, "prefill")
    t = 0
    for K in (5, 3):
        seq = torch.stack([env.sample(100 + t + k) for k in range(K)])
        got = d1.rollout(seq, t, memory=mem)
        want = d2.rollout(seq, t, states="all")
        ref.add_rollout(seq, want)
        assert got["shaped"] is None
        assert_equal(want["states"][-1], got["states"], "last state")
        for key in ("reward", "done", "sum_r", "collision"):
            assert_equal(want[key], got[key], key)
        same_memories(mem, ref, ("rollout", K))
        t += K
    same_windows(mem, ref)
    assert_same_envs(env, twin)
    env.check(); twin.check()
