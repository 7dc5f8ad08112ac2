#!/usr/bin/env python3
"""The reference's toy configuration (configs/4ue_3r_toy: 4 vehicles, 3 resources) rolled out K slots per launch: the
driver's random prefill and a held random schedule on B parallel envs, on a handle pinned to the sub-wave step kernel
with its slot loop (`use_subwave_path(slots=True)`, csrc/step_subwave_slots.hpp): 16 envs share a wavefront and keep
their tables, positions and counters in registers from slot to slot.  `--loop` runs the same slots as one-slot calls
(`use_subwave_path()` alone refuses the K-slot calls, DriverLoop loops) for comparison.

  python examples/rollout_toy.py --envs 65536 --slots 25 --launches 40
  python examples/rollout_toy.py --loop
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diral_amd.config import KERNEL_POLICY, M_TX_COLLIDED, M_TX_SOLE, bench_config  # noqa: E402
from diral_amd.driver import DriverLoop  # noqa: E402
from diral_amd.vec_env import VecV2VEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--slots", type=int, default=25, help="K: slots per launch")
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--hold", type=int, default=5, help="slots a vehicle keeps the resource it drew")
    ap.add_argument("--loop", action="store_true", help="one-slot calls instead of the slot loop")
    args = ap.parse_args()
    cfg = bench_config(4, 3, 100.0, communication_range=250.0, reward_design=2, congestion_test=True, State=dict(num_bins=20))
    dev = torch.device("cuda:0")
    B, N, K = args.envs, cfg.num_users, args.slots
    env = VecV2VEnv(cfg, batch=B, device=dev, out_dtype=torch.float32)
    env.use_subwave_path(slots=not args.loop)
    env.reset_topology(seed=1)
    # (DriverLoop: the launch where the env takes the K-slot call, the loop of slots where it refuses)
    loop = DriverLoop(env, global_reward_avg=True, episode_interval=cfg.episode_interval)
    loop.bootstrap(env.sample(1))
    states, acts = loop.prefill(K, 1000)                             # main_test.py:99-114: K random slots, every state kept
    print("prefill: states %s, actions %s, one launch: %s" % (tuple(states.shape), tuple(acts.shape), bool(env.last_kernel() & KERNEL_POLICY)))

    def schedule(i):
        draws = [env.sample(2000 + i * K + k // max(args.hold, 1)) for k in range(K)]
        return torch.stack(draws)
    t = 0
    loop.rollout(schedule(0), t, states="last")                      # warm-up
    t += K
    env.metrics(clear=True)
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    for i in range(args.launches):
        loop.rollout(schedule(1 + i), t, states="last")
        t += K
    torch.cuda.synchronize()
    dt = time.perf_counter() - t_start
    m = env.metrics().sum(0)
    tx = float(m[M_TX_SOLE] + m[M_TX_COLLIDED])
    print("%d envs x %d slots in %.3f s: %.2f us per slot, %.3e agent-steps/s, %.1f %% of the transmissions collided (%s)" % (
        B, args.launches * K, dt, dt * 1e6 / (args.launches * K), B * N * args.launches * K / dt,
        100.0 * float(m[M_TX_COLLIDED]) / max(tx, 1.0), "one-slot calls" if args.loop else "K slots per launch"))
    env.check()


if __name__ == "__main__":
    main()
