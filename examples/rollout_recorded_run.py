#!/usr/bin/env python3
"""Record a run and replay it: 25 slots of the velocity model on B parallel envs as ONE launch that also writes the position
log (VecV2VEnv.rollout(log_positions=True) -> diral_env_rollout_replay), then the recorded positions and actions on a fresh
env, again as one launch (rollout(positions=...)) - the reference's `save_positions` / `load_saved_positions` pair
(main_test.py:118, 140-142) without leaving the device - and the equality of the two runs.  Last, the SPS baseline over the
recorded positions (step_policy(slots=25, positions=...)): another policy on the same mobility trace.

  python examples/rollout_recorded_run.py --envs 1024
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diral_amd import c2_config  # noqa: E402
from diral_amd.config import KERNEL_POLICY  # noqa: E402
from diral_amd.sps import SpsPolicy  # noqa: E402
from diral_amd.vec_env import VecV2VEnv  # noqa: E402

K = 25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = c2_config(reward_design=2, mobility_vary=True)
    B, N, A = args.envs, cfg.num_users, cfg.num_channels

    def fresh():
        env = VecV2VEnv(cfg, batch=B, device=dev, out_dtype=torch.float32)
        env.reset_topology(seed=args.seed)
        return env

    # record: the velocity model, random actions, the position log of every slot
    env = fresh()
    actions = torch.stack([env.sample(100 + k) for k in range(K)])                 # the `actions` log, [K, B, N]
    rec = env.rollout(actions, 0, states="last", global_reward_avg=True, vel_seed=7, log_positions=True)
    assert env.last_kernel() & KERNEL_POLICY                                        # one launch, not the loop
    positions = rec["xpos"].transpose(0, 1).contiguous()                            # one sequence per env, [B, T = K, N]

    # replay both on a fresh env
    env2 = fresh()
    rep = env2.rollout(actions, 0, states="last", global_reward_avg=True, vel_seed=7, positions=positions)
    assert env2.last_kernel() & KERNEL_POLICY
    same = all(torch.equal(rec[k], rep[k]) for k in ("states", "reward", "shaped", "sum_r", "collision"))
    s1, s2 = env.export_state(), env2.export_state()
    same = same and all(torch.equal(s1[k], s2[k]) for k in s1)
    print("replayed run equals the recorded one (states, rewards, tables, positions, velocities): %s" % same)

    # the SPS baseline on the recorded mobility
    env3 = fresh()
    pol = SpsPolicy(B, N, A, device=dev, seed=5)
    o = dict(dtype=torch.float32, device=dev)
    sum_r, coll = torch.empty((K, B), **o), torch.empty((K, B), **o)
    env3.step_policy(pol.prev_action.clone(), 0, pol, torch.empty_like(pol.prev_action), shaped_out=torch.empty((K, B, N), **o),
                     sum_r_out=sum_r, collision_out=coll, slots=K, vel_seed=7, want_obs=False, positions=positions)
    assert env3.last_kernel() & KERNEL_POLICY
    for e in (env, env2, env3):
        e.check()
    print("same positions:            random actions   SPS")
    print("mean successful agents     %14.2f  %5.2f" % (float(rec["sum_r"].mean()), float(sum_r.mean())))
    print("mean collision count       %14.2f  %5.2f" % (float(rec["collision"].mean()), float(coll.mean())))


if __name__ == "__main__":
    main()
