#!/usr/bin/env python3
"""The driver's experience store on the device: ReplayMemory (diral_memory_add / diral_memory_sample) takes what the
K-slot launches write and hands a training step its batch in the layout the reference's DRQN builds with four Python
loops (algorithms/drl_drqn.py:294-377): [num_users * batch, step, S], user-major.

  python examples/replay_memory_batch.py --envs 4096 --slots 25 --batch 512
  python examples/replay_memory_batch.py --config toy --envs 65536 --batch 4096

  bootstrap -> memory.begin(state)
  prefill   -> memory.add_prefill(states, actions, rews0)       K random slots, one launch each way
  rollout   -> memory.add_rollout(actions_seq, out)             K slots with QPolicy's actions, the shaped rewards stored
  sample    -> (states, actions, rewards, next_states)          one launch; here bfloat16 states for a small LSTM
The LSTM is untrained and nothing is optimised: the point is that the shapes fit.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diral_amd import QPolicy, ReplayMemory, c2_config  # noqa: E402
from diral_amd.config import bench_config  # noqa: E402
from diral_amd.driver import DriverLoop  # noqa: E402
from diral_amd.vec_env import VecV2VEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--slots", type=int, default=25, help="K of the prefill and of the rollout")
    ap.add_argument("--capacity", type=int, default=60)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--step", type=int, default=6)
    ap.add_argument("--config", choices=["c2", "toy"], default="c2", help="c2: 64 UE / 32 res; toy: 4 UE / 3 res")
    ap.add_argument("--hidden", type=int, default=32)
    args = ap.parse_args()
    cfg = c2_config() if args.config == "c2" else bench_config(4, 3, 100.0, communication_range=250.0, State=dict(num_bins=20))
    dev = torch.device("cuda:0")
    B, N, A, K = args.envs, cfg.num_users, cfg.num_channels, args.slots
    env = VecV2VEnv(cfg, batch=B, device=dev, out_dtype=torch.float32)
    if N <= 8:
        env.use_subwave_path(slots=True)
    env.reset_topology(seed=1)
    S = env.S
    loop = DriverLoop(env, global_reward_avg=True, episode_interval=cfg.episode_interval)
    memory = ReplayMemory(args.capacity, B, N, S, dtype=torch.float32, seed=5, device=dev)
    policy = QPolicy(B, N, A, "eps_greedy", seed=11, device=dev, eps_init=0.3)
    torch.manual_seed(0)
    qnet = torch.nn.Sequential(torch.nn.Linear(S, 64), torch.nn.ReLU(), torch.nn.Linear(64, A)).to(dev)

    # main_test.py:89-114: the bootstrap slot, then K random slots into the memory
    state = loop.bootstrap(env.sample(seed=3))
    memory.begin(state)
    states, actions = loop.prefill(K, seed=100)
    memory.add_prefill(states, actions, loop._rews0)
    # K slots with the exploration policy's actions over the network's Q-values of the newest state (one decision per
    # slot from the same Q: an open-loop stretch), as ONE launch; the shaped rewards are what the driver stores
    with torch.no_grad():
        q = qnet(states[-1])
        seq = torch.stack([policy.act(q, episode=0) for _ in range(K)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = loop.rollout(seq, 1 + K, states="all")
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    memory.add_rollout(seq, out)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    s, a, r, n = memory.sample(args.batch, args.step, out_dtype=torch.bfloat16, last_only=True)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    print("%s: %d envs x %d agents, S = %d; %d-slot rollout %.0f us, add_rollout %.0f us, sample(%d, %d) %.0f us (first calls, "
          "enqueue included); len(memory) = %d of %d" % (args.config, B, N, S, K, (t1 - t0) * 1e6, (t2 - t1) * 1e6, args.batch,
                                                        args.step, (t3 - t2) * 1e6, len(memory), args.capacity))
    print("batch: states %s %s, actions %s, rewards %s, next_states %s; windows drawn: %d distinct (env, start) pairs"
          % (tuple(s.shape), s.dtype, tuple(a.shape), tuple(r.shape), tuple(n.shape),
             len(set(zip(memory.last_env.tolist(), memory.last_idx.tolist())))))
    assert torch.equal(n[:, :-1], s[:, 1:]) and int(memory.bad_samples.item()) == 0      # state = next_state inside a window

    # the training step's forward pass: an LSTM over the windows, Q-values of the last step, the TD target's ingredients
    lstm = torch.nn.LSTM(S, args.hidden, batch_first=True).to(dev).to(torch.bfloat16)
    head = torch.nn.Linear(args.hidden, A).to(dev).to(torch.bfloat16)
    with torch.no_grad():
        qs = head(lstm(s)[0][:, -1])                                   # [N * batch, A]
        q_next = head(lstm(n)[0][:, -1])
        target = r + 0.9 * q_next.float().max(dim=1).values            # rewards[:, -1] + gamma * max Q(next) (drl_drqn.py:288)
        chosen = qs.float().gather(1, a.long().unsqueeze(1)).squeeze(1)
    print("LSTM forward: Q %s, target %s, mean TD error %.4f (untrained)" % (tuple(qs.shape), tuple(target.shape),
                                                                         float((target - chosen).mean())))
    env.check()


if __name__ == "__main__":
    main()
