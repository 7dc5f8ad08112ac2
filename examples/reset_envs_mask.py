#!/usr/bin/env python3
"""Domain randomisation driven from the device: after every K-slot rollout the envs with the lowest reward sums get a
fresh topology (VecV2VEnv.reset_envs -> diral_env_reset_envs) while the others go on.  Which envs those are is decided
on the GPU - a reduction over the rollout's `sum_r`, a k-th value, a comparison - and handed over as a bool mask [B]: no
`nonzero()`, no copy to the host, no synchronisation between the rollout and the reset.

  python examples/reset_envs_mask.py --envs 4096 --slots 25 --rounds 20 --fraction 0.125
  python examples/reset_envs_mask.py --config toy --envs 65536

What a reset env gets is what `reset_topology(seed=...)` would give it: zeroed tables, arrival stamps, counters and
metric sums, and the positions and speeds drawn for its global env index.  The slot counter is the handle's and runs on.
A policy that keeps state per env outside the handle (an SpsPolicy's counters) re-initialises those rows itself.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diral_amd import c2_config  # noqa: E402
from diral_amd.config import M_SLOTS, bench_config  # noqa: E402
from diral_amd.vec_env import VecV2VEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--slots", type=int, default=25, help="K: slots per rollout launch")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--fraction", type=float, default=0.125, help="share of the envs re-drawn after each rollout")
    ap.add_argument("--config", choices=["c2", "toy"], default="c2", help="c2: 64 UE / 32 res; toy: 4 UE / 3 res")
    args = ap.parse_args()
    cfg = c2_config() if args.config == "c2" else bench_config(4, 3, 100.0, communication_range=250.0, State=dict(num_bins=20))
    dev = torch.device("cuda:0")
    B, N, A, K = args.envs, cfg.num_users, cfg.num_channels, args.slots
    k_low = max(1, min(B, int(round(B * args.fraction))))
    env = VecV2VEnv(cfg, batch=B, device=dev)
    if args.config == "toy":
        env.use_subwave_path(slots=True)                               # (K-slot launches below 8 vehicles: the sub-wave slot loop)
    env.reset_topology(seed=1)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)

    def actions():
        return torch.randint(0, A, (K, B, N), device=dev, dtype=torch.int32, generator=gen)

    env.rollout(actions(), states=None)                                # warm-up
    resets = torch.zeros(B, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    for r in range(args.rounds):
        out = env.rollout(actions(), states=None)
        total = out["sum_r"].sum(0)                                    # [B] reward of the K slots, on the device
        cut = torch.kthvalue(total, k_low).values                      # ... the k-th lowest, still on the device
        mask = total <= cut                                            # bool [B]: at least k_low envs (ties included)
        env.reset_envs(mask=mask, seed=1000 + r)                       # enqueue-only: one launch, the mask read on the device
        resets += mask
    torch.cuda.synchronize()
    dt = time.perf_counter() - t_start
    slots = env.metrics()[:, M_SLOTS].cpu()
    n_reset = resets.cpu()
    print("%s: %d envs x %d vehicles, %d rollouts of %d slots, the %d lowest re-drawn after each" % (args.config, B, N, args.rounds, K, k_low))
    print("envs re-drawn       %d in all, %d never, at most %d times one env" % (int(n_reset.sum()), int((n_reset == 0).sum()), int(n_reset.max())))
    print("slots since reset   min %d  median %d  max %d (metric sums restart with the env)" % (int(slots.min()), int(slots.median()), int(slots.max())))
    print("agent-steps/s       %.3e (%.1f us per rollout + reset of %d envs)" % (B * N * K * args.rounds / dt, dt / args.rounds * 1e6, B))
    assert int(slots.max()) <= (args.rounds + 1) * K and int(slots.min()) == 0
    env.check()


if __name__ == "__main__":
    main()
