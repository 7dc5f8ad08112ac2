#!/usr/bin/env python3
"""A Q-network against the env with its actions chosen on the device: QPolicy.act (diral_policy_select) turns Q[B, N, A]
into actions[B, N] in one launch - epsilon-greedy, softmax or Boltzmann exploration as in the reference's
algorithms/policies.py, drawn from (seed, call number, global agent index) instead of torch's generator.

  python examples/act_from_q_values.py --envs 4096 --slots 100 --kind eps_greedy
  python examples/act_from_q_values.py --config toy --envs 65536 --kind softmax

Two loops over the same two-layer MLP (untrained: the point is the plumbing, not the return):
  eager     q = mlp(state); a = policy.act(q, episode); DriverLoop.slot(a, t) -> next state, shaped reward
  captured  a torch.cuda.graph holding [mlp, policy.act_clocked, env step]; diral_clock_add between the replays moves the
            slot number and the seed of the draws on, and a torch op writes the per-env epsilon the graph reads
"""
import argparse
import ctypes
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diral_amd import QPolicy, c2_config  # noqa: E402
from diral_amd.config import STEP_MY_STEP, bench_config  # noqa: E402
from diral_amd.driver import DriverLoop  # noqa: E402
from diral_amd.rollout import SlotClock, no_finalizers_during_capture  # noqa: E402
from diral_amd.vec_env import VecV2VEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--slots", type=int, default=100)
    ap.add_argument("--kind", choices=["eps_greedy", "softmax", "boltzmann"], default="eps_greedy")
    ap.add_argument("--config", choices=["c2", "toy"], default="c2", help="c2: 64 UE / 32 res; toy: 4 UE / 3 res")
    ap.add_argument("--hidden", type=int, default=64)
    args = ap.parse_args()
    cfg = c2_config() if args.config == "c2" else bench_config(4, 3, 100.0, communication_range=250.0, State=dict(num_bins=20))
    dev = torch.device("cuda:0")
    B, N, A, T = args.envs, cfg.num_users, cfg.num_channels, args.slots
    env = VecV2VEnv(cfg, batch=B, device=dev, out_dtype=torch.float32)
    env.reset_topology(seed=1)
    torch.manual_seed(0)
    mlp = torch.nn.Sequential(torch.nn.Linear(env.S, args.hidden), torch.nn.ReLU(), torch.nn.Linear(args.hidden, A)).to(dev)
    policy = QPolicy(B, N, A, args.kind, seed=11, device=dev, eps_init=0.5, eps_decay=0.9, temperature=0.5)
    explored = torch.zeros((B, N), dtype=torch.uint8, device=dev)

    # ---- eager: the reference's slot loop, actions from the network's Q-values ----
    loop = DriverLoop(env, global_reward_avg=True, episode_interval=cfg.episode_interval, fused=True)
    state = loop.bootstrap(env.sample(seed=3))
    total = torch.zeros((), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        for t in range(T):
            q = mlp(state)                                             # [B, N, A] float32
            a = policy.act(q, episode=loop.episode, time_slot=t, explored=explored)
            out = loop.slot(a, t)
            state = out["next_state"]
            total += out["reward"].sum()
            if out["episode_end"]:
                loop.end_episode()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("%s, %s: %d envs x %d agents, %d slots eager: %.1f us per slot, mean shaped reward %.4f, parameter now %.4g, "
          "%.1f %% of the last slot's agents explored" % (args.config, args.kind, B, N, T, dt / T * 1e6, float(total) / (T * B * N),
                                                          policy.get_epsilon() or 0.0, 100.0 * float(explored.float().mean())))

    # ---- captured: [mlp, act_clocked, step] replayed, the clock and the per-env parameter moved between replays ----
    clock = SlotClock(dev, T)
    env.set_clock(clock.t)
    s_in = state.clone()
    acts = torch.empty((B, N), dtype=torch.int32, device=dev)
    par = torch.linspace(0.05, 0.5, B, dtype=torch.float64, device=dev)    # population-style exploration: one value per env

    def slot():
        with torch.no_grad():
            policy.act_clocked(mlp(s_in), clock, param=par, out=acts)
        obs, rew, _ = env._step(STEP_MY_STEP, acts, 0)                 # slot number = clock, read on the device
        s_in.copy_(obs)
        return rew

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        slot()                                                         # once eagerly: buffers and kernel path settle
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with no_finalizers_during_capture():
        with torch.cuda.graph(graph, stream=side):
            rew = slot()
    tick = lambda: env._ok(env.lib.diral_clock_add(ctypes.c_void_p(clock.ptr()), 1, env._stream()), "diral_clock_add")  # noqa: E731
    tick()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for r in range(T):
        graph.replay()
        tick()
        if r % 25 == 24:
            par.mul_(0.9)                                              # the schedule, written by a torch op
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("captured [mlp, act_clocked, step]: %.1f us per slot, mean reward of the last slot %.4f, clock %d, per-env parameter now %.3f ... %.3f"
          % (dt / T * 1e6, float(rew.double().mean()), clock.value(), float(par[0]), float(par[-1])))
    env.set_clock(None)
    env.check()


if __name__ == "__main__":
    main()
