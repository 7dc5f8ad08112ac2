#!/usr/bin/env python3
"""A fixed schedule evaluated open-loop: K slots of round-robin resource use on B parallel envs in ONE launch per K
slots (VecV2VEnv.rollout -> diral_env_rollout), the collision-free-by-construction baseline a learned policy is compared
with.  Vehicle u uses resource (u + k * stride) mod A in slot k: with N <= A nobody ever shares a resource; with N > A the
vehicles that do are N / A apart in index, not on the road, so some of them collide.

  python examples/rollout_fixed_schedule.py --envs 1024 --slots 25 --launches 40
  python examples/rollout_fixed_schedule.py --config c3 --envs 8192           # 256 UE / 64 res
  python examples/rollout_fixed_schedule.py --enable-channel --states all     # my_step_ch, every slot's state vector
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diral_amd import c2_config  # noqa: E402
from diral_amd.config import M_SLOTS, M_TX_COLLIDED, M_TX_SOLE, bench_config  # noqa: E402
from diral_amd.driver import DriverLoop  # noqa: E402
from diral_amd.vec_env import VecV2VEnv  # noqa: E402


def round_robin(K, B, N, A, t0, stride, device):
    """[K, B, N] int32: vehicle u's resource in slot t0 + k."""
    u = torch.arange(N, device=device, dtype=torch.int64).view(1, 1, N)
    k = torch.arange(t0, t0 + K, device=device, dtype=torch.int64).view(K, 1, 1)
    return ((u + k * stride) % A).to(torch.int32).expand(K, B, N).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--slots", type=int, default=25, help="K: slots per launch")
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--stride", type=int, default=1, help="resources a vehicle moves on by per slot (0: it keeps its resource)")
    ap.add_argument("--config", choices=["c2", "c5", "c3"], default="c2",
                    help="c2: 64 UE / 32 res (the default); c5: 128 UE / 64 res with mobility_vary; c3: 256 UE / 64 res")
    ap.add_argument("--enable-channel", action="store_true", help="my_step_ch (the PRR reward) instead of my_step; 64 UE only")
    ap.add_argument("--states", choices=["last", "all", "none"], default="none")
    args = ap.parse_args()
    cfg = {"c2": lambda: c2_config(), "c5": lambda: bench_config(128, 64, 4000.0, mobility_vary=True),
           "c3": lambda: bench_config(256, 64, 4000.0)}[args.config]()
    dev = torch.device("cuda:0")
    B, N, A, K = args.envs, cfg.num_users, cfg.num_channels, args.slots
    env = VecV2VEnv(cfg, batch=B, device=dev)
    env.reset_topology(seed=1)
    # (DriverLoop.rollout: the launch where the slot loops take the configuration, the loop of slots elsewhere)
    loop = DriverLoop(env, enable_channel=args.enable_channel, global_reward_avg=True, episode_interval=cfg.episode_interval)
    states = None if args.states == "none" else args.states
    t = 0
    loop.rollout(round_robin(K, B, N, A, t, args.stride, dev), t, states=states)          # warm-up
    t += K
    env.metrics(clear=True)
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    coll = torch.zeros((), dtype=torch.float64, device=dev)
    for _ in range(args.launches):
        out = loop.rollout(round_robin(K, B, N, A, t, args.stride, dev), t, states=states)
        coll += out["collision"].sum(dtype=torch.float64)
        t += K
    torch.cuda.synchronize()
    dt = time.perf_counter() - t_start
    m = env.metrics().sum(0).cpu()
    tx = float(m[M_TX_SOLE] + m[M_TX_COLLIDED])
    slots = args.launches * K
    print("%s: %d envs x %d vehicles, %d slots (%d per launch), round-robin over %d resources" % (args.config, B, N, slots, K, A))
    print("collision rate      %.4f of the transmissions (%d of %d)" % (float(m[M_TX_COLLIDED]) / max(tx, 1.0), int(m[M_TX_COLLIDED]), int(tx)))
    print("A - sum(reward)     %.3f per env and slot (main_test.py:178)" % (float(coll) / (B * slots)))
    print("agent-steps/s       %.3e (%.1f us per slot of %d envs)" % (B * N * slots / dt, dt / slots * 1e6, B))
    assert int(m[M_SLOTS]) == B * slots
    env.check()


if __name__ == "__main__":
    main()
