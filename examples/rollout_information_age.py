#!/usr/bin/env python3
"""The information-age curve of a fixed schedule: 25 slots of round-robin resource use in `my_step_ch` on B parallel envs
with arrival stamps, as ONE launch (VecV2VEnv.rollout(info_age=True) -> diral_env_rollout_ia).  The launch keeps the stamps
from slot to slot and returns Network.get_information_age behind every slot and utils/misc.calculate_ia_penalty of it -
the quantity the reference's `enable_channel` experiments report next to the packet reception ratio - and, with
--ia-averaging, the -1 / 0 / +1 reward term of main_test.py:151-160.

  python examples/rollout_information_age.py --envs 1024
  python examples/rollout_information_age.py --stride 0 --ia-averaging      # everybody keeps its resource
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diral_amd import c2_config  # noqa: E402
from diral_amd.config import KERNEL_POLICY, M_PRR_CNT, M_PRR_SUM  # noqa: E402
from diral_amd.vec_env import VecV2VEnv  # noqa: E402

K = 25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--stride", type=int, default=1, help="resources a vehicle moves on by per slot (0: it keeps its resource)")
    ap.add_argument("--ia-averaging", action="store_true", help="add the information-age term to the shaped rewards")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = c2_config(reward_design=2, track_arrival=True)
    B, N, A = args.envs, cfg.num_users, cfg.num_channels
    env = VecV2VEnv(cfg, batch=B, device=dev, out_dtype=torch.float32)
    env.reset_topology(seed=args.seed)
    u = torch.arange(N, device=dev, dtype=torch.int64).view(1, 1, N)
    k = torch.arange(K, device=dev, dtype=torch.int64).view(K, 1, 1)
    seq = ((u + k * args.stride) % A).to(torch.int32).expand(K, B, N).contiguous()
    prev = torch.zeros((B,), dtype=torch.int64, device=dev) if args.ia_averaging else None
    out = env.rollout(seq, 0, mode="my_step_ch", states=None, global_reward_avg=True, info_age=True, sum_ia_prev=prev)
    assert env.last_kernel() & KERNEL_POLICY                        # one launch, not the loop
    env.check()
    ia_sum = out["ia_sum"].to(torch.float64).mean(1).cpu()
    received = out["ia"].sum(-1).to(torch.float64).mean(1).cpu()
    print("slot  mean ia_sum  mean pairs counted" + ("  mean term" if args.ia_averaging else ""))
    for s in range(K):
        line = "%4d  %11.1f  %18.1f" % (s, ia_sum[s], received[s])
        if args.ia_averaging:
            line += "  %9.3f" % float(out["ia_penalty"][s].to(torch.float64).mean())
        print(line)
    m = env.metrics().sum(0).cpu()
    print("packet reception ratio over the %d slots: %.4f" % (K, float(m[M_PRR_SUM] / m[M_PRR_CNT])))


if __name__ == "__main__":
    main()
