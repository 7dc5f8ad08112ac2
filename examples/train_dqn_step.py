#!/usr/bin/env python3
"""A whole DQN iteration of the feed-forward agent (``use_lstm_input: false``) with nothing but launches between the env
and the optimiser - the reference's driver loop (main_test.py:119-236) and ``DRQN.train`` (algorithms/drl_drqn.py:199-265)
for B envs at once, no host round trip inside the loop.  The Q-network is the reference's dense chain
(``_create_network``, drl_drqn.py:124-153) held by `QNet`: its three evaluations that never see a gradient are ONE launch
each, the fourth goes through torch on the same parameters.

  python examples/train_dqn_step.py --envs 256 --iters 20
  python examples/train_dqn_step.py --config toy --envs 4096

  prefill    -> loop.prefill(K, seed, memory=memory)             random slots into the replay memory's rings
  state      -> memory.history(1).view(B * N, S)                 state_vector[-1:, user] of every agent: one launch
  Q-values   -> net.forward(state)                               the acting pass: one launch
  actions    -> policy.act(q.view(B, N, A))                      one launch
  slot       -> loop.rollout(actions[None], t, memory=memory)    env step + store: one launch
  batch      -> memory.sample(batch, step, last_only=True)       one launch; states[:, -1] goes in as a strided view
  targets    -> target.forward(next), net.forward(next)          _calc_target's two sess.run: one launch each
  loss       -> qloss.loss(module(states), a, r, ...).backward() net(states) through torch_module(), the gradient path
  Adam on the module's parameters - views of net.params, so the next launch reads the new weights -, and
  target.copy_from(net) every `--target-update` iterations.
The loss is read once, behind the loop.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diral_amd import QLoss, QNet, QPolicy, ReplayMemory, c2_config  # noqa: E402
from diral_amd.config import bench_config  # noqa: E402
from diral_amd.driver import DriverLoop  # noqa: E402
from diral_amd.vec_env import VecV2VEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--capacity", type=int, default=60)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--n-batch", type=int, default=1, help="training steps per slot (the reference's n_batch)")
    ap.add_argument("--step", type=int, default=6, help="window length of the sampled batch; the agent sees its last state")
    ap.add_argument("--hidden", type=int, nargs="+", default=[256, 256])
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
    S = env.S
    loop = DriverLoop(env, global_reward_avg=True, episode_interval=cfg.episode_interval)
    memory = ReplayMemory(args.capacity, B, N, S, dtype=torch.float32, seed=5, device=dev)
    policy = QPolicy(B, N, A, "eps_greedy", seed=7, device=dev, eps_init=0.3)
    qloss = QLoss(gamma=0.99, double=True, hysteretic=True, device=dev)
    net = QNet(S, args.hidden, A, device=dev, seed=0)
    target = QNet(S, args.hidden, A, device=dev, init="zeros")
    target.copy_from(net)
    module = net.torch_module()
    opt = torch.optim.Adam(module.parameters(), lr=1e-4)

    memory.begin(loop.bootstrap(env.sample(seed=3)))
    K = 2 * step
    loop.prefill(K, seed=100, memory=memory)                         # main_test.py:99-114
    losses = torch.zeros((args.iters,), device=dev)
    q_act = torch.empty((B * N, A), device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(args.iters):
        state = memory.history(1).view(B * N, S)                     # main_test.py:125-136, drl_drqn.py:173-182
        actions = policy.act(net.forward(state, out=q_act).view(B, N, A), episode=0)
        loop.rollout(actions.unsqueeze(0), 1 + K + it, memory=memory)           # :144-217: the slot and memory.add
        for _ in range(args.n_batch):                                # drl_drqn.py:208-261
            states, acts, rewards, nxt = memory.sample(args.batch, step, last_only=True)
            s_last, n_last = states[:, -1], nxt[:, -1]               # [N * batch, S] views with a row stride of step * S
            q_next_target, q_next_eval = target.forward(n_last), net.forward(n_last)      # _calc_target's two sess.run
            loss = qloss.loss(module(s_last), acts, rewards, q_next_target, q_next_eval)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
        losses[it] = loss.detach()
        if (it + 1) % args.target_update == 0:                       # :263-265
            target.copy_from(net)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.iters
    host_losses = losses.cpu()                                       # the one read of the losses, behind the loop
    assert bool(torch.isfinite(host_losses).all()) and bool(torch.isfinite(net.params).all())
    assert int(qloss.bad_rows.item()) == 0 and int(memory.bad_samples.item()) == 0
    env.check()
    print("%s: %d envs x %d agents, S = %d, chain %s, batch %d x %d rows: %d iterations, %.2f ms each (enqueue and the first calls' warm-up included); "
          "loss %.4f -> %.4f; len(memory) = %d of %d"
          % (args.config, B, N, S, " -> ".join(str(w) for w in net.widths), args.batch, N, args.iters, ms,
             float(host_losses[0]), float(host_losses[-1]), len(memory), args.capacity))


if __name__ == "__main__":
    main()
