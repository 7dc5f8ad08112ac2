#!/usr/bin/env python3
"""Collect -> store -> sample with the store inside the collecting launch: the K-slot prefill and rollout write their
transitions straight into the ReplayMemory's rings (diral_env_prefill_memory / diral_env_rollout_memory), next to the
two-call form (rollout(states="all") + add_rollout) they stand for.

  python examples/rollout_into_memory.py --envs 4096 --slots 25
  python examples/rollout_into_memory.py --config toy --envs 65536

  bootstrap -> memory.begin(state)
  prefill   -> loop.prefill(K, seed, memory=memory)             K random slots: states, actions and the stale rewards land in ring rows
  rollout   -> loop.rollout(seq, t, memory=memory)              K slots of given actions: states, actions, shaped rewards
  sample    -> memory.sample(batch, step)                        one launch, [num_users * batch, step, S]
A second env and memory run the same slots as two calls each; the rings are compared bit for bit and both forms are timed.
Where the env does not take the launch (N > 64, a toy handle that is not pinned with slots=True) DriverLoop runs the two
calls itself: the rings are the same.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diral_amd import ReplayMemory, c2_config  # noqa: E402
from diral_amd.config import bench_config  # noqa: E402
from diral_amd.driver import DriverLoop  # noqa: E402
from diral_amd.vec_env import VecV2VEnv  # noqa: E402


def timed(body):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = body()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--slots", type=int, default=25, help="K of the prefill and of the rollout")
    ap.add_argument("--capacity", type=int, default=60)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--step", type=int, default=6)
    ap.add_argument("--config", choices=["c2", "toy"], default="c2", help="c2: 64 UE / 32 res; toy: 4 UE / 3 res")
    args = ap.parse_args()
    cfg = c2_config() if args.config == "c2" else bench_config(4, 3, 100.0, communication_range=250.0, State=dict(num_bins=20))
    dev = torch.device("cuda:0")
    B, N, A, K = args.envs, cfg.num_users, cfg.num_channels, args.slots
    sides = []
    for _ in range(2):                                   # [0]: the launches write the rings; [1]: two calls each
        env = VecV2VEnv(cfg, batch=B, device=dev, out_dtype=torch.float32)
        if N <= 8:
            env.use_subwave_path(slots=True)
        env.reset_topology(seed=1)
        loop = DriverLoop(env, global_reward_avg=True, episode_interval=cfg.episode_interval)
        memory = ReplayMemory(args.capacity, B, N, env.S, dtype=torch.float32, seed=5, device=dev)
        memory.begin(loop.bootstrap(env.sample(seed=3)))
        sides.append((env, loop, memory))
    (env, loop, memory), (env2, loop2, memory2) = sides
    seq = torch.randint(0, A, (K, B, N), dtype=torch.int32, device=dev, generator=torch.Generator(dev).manual_seed(2))

    # main_test.py:99-114: K random slots into the memory
    _, us_fill = timed(lambda: loop.prefill(K, seed=100, memory=memory))

    def fill_two_calls():
        states, actions = loop2.prefill(K, seed=100)
        memory2.add_prefill(states, actions, loop2._rews0)
    _, us_fill2 = timed(fill_two_calls)
    # K slots of a given action sequence: every slot's state, actions and shaped reward
    out, us_roll = timed(lambda: loop.rollout(seq, 1 + K, memory=memory))
    _, us_roll2 = timed(lambda: memory2.add_rollout(seq, loop2.rollout(seq, 1 + K, states="all")))
    for ring in ("states", "actions", "rewards"):
        assert torch.equal(getattr(memory, ring), getattr(memory2, ring)), ring
    assert memory.count == memory2.count == 2 * K and out["shaped"] is None
    assert out["states"].data_ptr() == memory.states[memory.count % (args.capacity + 1)].data_ptr()   # a view of the newest row
    print("%s: %d envs x %d agents, S = %d, K = %d (first calls, enqueue included): prefill into the rings %.0f us / prefill + "
          "add_prefill %.0f us; rollout into the rings %.0f us / rollout + add_rollout %.0f us; the rings are equal"
          % (args.config, B, N, env.S, K, us_fill, us_fill2, us_roll, us_roll2))
    s, a, r, n = memory.sample(args.batch, args.step, out_dtype=torch.bfloat16, last_only=True)
    print("batch: states %s %s, actions %s, rewards %s, next_states %s; len(memory) = %d of %d"
          % (tuple(s.shape), s.dtype, tuple(a.shape), tuple(r.shape), tuple(n.shape), len(memory), args.capacity))
    assert torch.equal(n[:, :-1], s[:, 1:]) and int(memory.bad_samples.item()) == 0      # state = next_state inside a window
    env.check(); env2.check()


if __name__ == "__main__":
    main()
