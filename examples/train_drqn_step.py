#!/usr/bin/env python3
"""A whole DRQN iteration with nothing but launches between the env and a torch network - the reference's driver loop
(main_test.py:119-236) and ``DRQN.train`` (algorithms/drl_drqn.py:199-265) for B envs at once, no host round trip inside
the loop:

  python examples/train_drqn_step.py --envs 256 --iters 20
  python examples/train_drqn_step.py --config toy --envs 4096

  prefill    -> loop.prefill(K, seed, memory=memory)             random slots into the replay memory's rings
  window     -> memory.history(step)                             np.array(history_input), state_vector[:, user]: one launch
  Q-values   -> net(window)                                      a small torch LSTM (the network is PyTorch's job)
  actions    -> policy.act(q.view(B, N, A))                      one launch
  slot       -> loop.rollout(actions[None], t, memory=memory)    env step + store: one launch
  batch      -> memory.sample(batch, step, last_only=True)       one launch, [N * batch, step, S]
  loss       -> qloss.loss(net(states), a, r, target(next), net(next)).backward()    targets, hysteretic loss, dL/dQ: one launch
  Adam, and the target copy every `--target-update` iterations.
The loss is read once, behind the loop.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diral_amd import QLoss, QPolicy, ReplayMemory, c2_config  # noqa: E402
from diral_amd.config import bench_config  # noqa: E402
from diral_amd.driver import DriverLoop  # noqa: E402
from diral_amd.vec_env import VecV2VEnv  # noqa: E402


class Drqn(torch.nn.Module):
    """An LSTM over the window, its last output through one hidden layer (drl_drqn.py:116-121, 130-153 in outline)."""

    def __init__(self, state_space, hidden, num_actions):
        super().__init__()
        self.lstm = torch.nn.LSTM(state_space, hidden, batch_first=True)
        self.head = torch.nn.Sequential(torch.nn.Linear(hidden, hidden), torch.nn.ReLU(), torch.nn.LayerNorm(hidden),
                                        torch.nn.Linear(hidden, num_actions))

    def forward(self, x):
        out, _ = self.lstm(x)
        return self.head(out[:, -1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--capacity", type=int, default=60)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--n-batch", type=int, default=1, help="training steps per slot (the reference's n_batch)")
    ap.add_argument("--step", type=int, default=6)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--target-update", type=int, default=5)
    ap.add_argument("--config", choices=["c2", "toy"], default="c2", help="c2: 64 UE / 32 res; toy: 4 UE / 3 res")
    args = ap.parse_args()
    cfg = c2_config() if args.config == "c2" else bench_config(4, 3, 100.0, communication_range=250.0, State=dict(num_bins=20))
    dev = torch.device("cuda:0")
    B, N, A, step = args.envs, cfg.num_users, cfg.num_channels, args.step
    env = VecV2VEnv(cfg, batch=B, device=dev, out_dtype=torch.float32)
    if N <= 8:
        env.use_subwave_path(slots=True)
    env.reset_topology(seed=1)
    loop = DriverLoop(env, global_reward_avg=True, episode_interval=cfg.episode_interval)
    memory = ReplayMemory(args.capacity, B, N, env.S, dtype=torch.float32, seed=5, device=dev)
    policy = QPolicy(B, N, A, "eps_greedy", seed=7, device=dev, eps_init=0.3)
    qloss = QLoss(gamma=0.99, double=True, hysteretic=True, device=dev)
    torch.manual_seed(0)
    net, target = Drqn(env.S, args.hidden, A).to(dev), Drqn(env.S, args.hidden, A).to(dev)
    target.load_state_dict(net.state_dict())
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)

    memory.begin(loop.bootstrap(env.sample(seed=3)))
    K = 2 * step
    loop.prefill(K, seed=100, memory=memory)                         # main_test.py:99-114
    losses = torch.zeros((args.iters,), device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(args.iters):
        with torch.no_grad():                                        # main_test.py:125-136, drl_drqn.py:171-182
            q = net(memory.history(step)).view(B, N, A)
            actions = policy.act(q, episode=0)
        loop.rollout(actions.unsqueeze(0), 1 + K + it, memory=memory)           # :144-217: the slot and memory.add
        for _ in range(args.n_batch):                                # drl_drqn.py:208-261
            states, acts, rewards, nxt = memory.sample(args.batch, step, last_only=True)
            with torch.no_grad():                                    # _calc_target's two sess.run
                q_next_target, q_next_eval = target(nxt), net(nxt)
            loss = qloss.loss(net(states), acts, rewards, q_next_target, q_next_eval)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        losses[it] = loss.detach()
        if (it + 1) % args.target_update == 0:                       # :263-265
            target.load_state_dict(net.state_dict())
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.iters
    first, last = float(losses[0].item()), float(losses[-1].item())
    assert torch.isfinite(losses).all() and int(qloss.bad_rows.item()) == 0 and int(memory.bad_samples.item()) == 0
    env.check()
    print("%s: %d envs x %d agents, S = %d, window %d, batch %d x %d rows: %d iterations, %.2f ms each (enqueue and the first calls' warm-up included); "
          "loss %.4f -> %.4f; len(memory) = %d of %d"
          % (args.config, B, N, env.S, step, args.batch, N, args.iters, ms, first, last, len(memory), args.capacity))


if __name__ == "__main__":
    main()
