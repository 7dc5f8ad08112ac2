#!/usr/bin/env python3
"""A random-shooting planner on B parallel envs: every K slots each env is forked into C candidates, each candidate runs a
random K-slot action sequence, and the env goes on from the best one (diral_amd.search.CandidateSearch: a gather of the env
into the work handle, ONE rollout launch of B * C envs, a gather of the winners back - VecV2VEnv.copy_envs_from ->
diral_env_copy_envs).  The baseline is what the planner draws from: uniform random actions, no choice.

  python examples/search_candidates.py --envs 256 --candidates 16 --slots 5 --rounds 20
  python examples/search_candidates.py --config c5 --envs 128 --candidates 8
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diral_amd import c2_config  # noqa: E402
from diral_amd.config import bench_config  # noqa: E402
from diral_amd.search import CandidateSearch  # noqa: E402
from diral_amd.vec_env import VecV2VEnv  # noqa: E402


def random_sequences(K, B, C, N, A, gen):
    """[K, B, C, N] int32: C uniform random K-slot sequences per env."""
    return torch.randint(0, A, (K, B, C, N), device=gen.device, generator=gen, dtype=torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--candidates", type=int, default=16, help="C: sequences tried per env and round")
    ap.add_argument("--slots", type=int, default=5, help="K: slots per sequence")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--config", choices=["c2", "c5", "c3"], default="c2",
                    help="c2: 64 UE / 32 res (the default); c5: 128 UE / 64 res with mobility_vary; c3: 256 UE / 64 res")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    cfg = {"c2": lambda: c2_config(), "c5": lambda: bench_config(128, 64, 4000.0, mobility_vary=True),
           "c3": lambda: bench_config(256, 64, 4000.0)}[args.config]()
    dev = torch.device("cuda:0")
    B, C, K, N, A = args.envs, args.candidates, args.slots, cfg.num_users, cfg.num_channels
    gen = torch.Generator(device=dev)
    gen.manual_seed(args.seed)
    env = VecV2VEnv(cfg, batch=B, device=dev)
    env.reset_topology(seed=args.seed)
    baseline = env.twin()                                            # the same topology, driven by uniform random actions
    baseline.copy_envs_from(env)
    search = CandidateSearch(env, candidates=C)
    search.evaluate(random_sequences(K, B, C, N, A, gen))            # warm-up: nothing is committed
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    planned = torch.zeros((), dtype=torch.float64, device=dev)
    uniform = torch.zeros((), dtype=torch.float64, device=dev)
    for _ in range(args.rounds):
        out = search.evaluate(random_sequences(K, B, C, N, A, gen))
        choice = out["returns"].argmax(dim=1)                        # [B], on the device: no synchronisation
        search.commit(choice)
        planned += out["collision"].gather(2, choice.view(1, B, 1).expand(K, B, 1)).sum(dtype=torch.float64)
        uniform += baseline.rollout(random_sequences(K, B, 1, N, A, gen)[:, :, 0], states=None)["collision"].sum(dtype=torch.float64)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t_start
    slots = args.rounds * K
    print("%s: %d envs x %d vehicles, %d slots; %d candidates of %d slots per env and round" % (args.config, B, N, slots, C, K))
    print("collisions per slot   %.3f with the best of %d random sequences" % (float(planned) / (B * slots), C))
    print("                      %.3f with uniform random actions (A - sum(reward), main_test.py:178)" % (float(uniform) / (B * slots)))
    print("env-slots/s           %.3e evaluated (%.1f us per round of %d x %d envs x %d slots)" % (
        B * C * slots / dt, dt / args.rounds * 1e6, B, C, K))
    assert env.t == slots
    env.check()
    search.work.check()


if __name__ == "__main__":
    main()
