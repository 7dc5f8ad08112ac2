"""What a launch with the recorded-mobility block costs against the same launch without it: C2, states=None, K = 25, the forms
interleaved as in profiles/kslots_replay_bench.py, us per slot.
  none      rollout without the block
  log       rollout with the position log only (the RP instantiation on the velocity model)
  exact     rollout with positions = the velocity model's own (the recorded log of the whole run: the same topologies as `none`)
  wrap      rollout with the bench's T = 25 sequence per env (it jumps back at every launch)
for each library given (tuning variants next to the tree's own): --libs name=path,...   (path `this`: the tree's own)

  python profiles/kslots_replay_cost.py [--mode my_step_ch] [--batches 4096,64]
"""
import argparse
import json
import os

import torch

import ab  # noqa: E402  (puts the repository's root on sys.path)
from diral_amd import _lib  # noqa: E402
from diral_amd.config import c2_config  # noqa: E402
from diral_amd.vec_env import VecV2VEnv  # noqa: E402

K = 25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", default="this=this")
    ap.add_argument("--batches", default="4096,64")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--mode", default="my_step")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = c2_config(reward_design=2)
    libs = [(n, _lib.load() if p == "this" else _lib.bind(os.path.abspath(p))) for n, p in (x.split("=") for x in args.libs.split(","))]
    total = K * (args.rounds + args.warm)
    for B in (int(b) for b in args.batches.split(",")):
        # the velocity model's own positions over the whole run
        rec = VecV2VEnv(cfg, batch=B, device=dev, out_dtype=torch.float32)
        rec.reset_topology(seed=1234)
        seq = torch.stack([rec.sample(4000 + k) for k in range(K)])
        s0 = rec.export_state(tables=False)                           # [B, K, N]: where the velocity model takes the envs in K slots
        k = torch.arange(1, K + 1, dtype=torch.float64, device=dev).view(1, K, 1)
        wrap = torch.remainder(s0["pos_x"].unsqueeze(1) + s0["vel"].unsqueeze(1) * k, float(cfg.highway_length)).contiguous()
        logs = []
        for r in range(args.rounds + args.warm):
            logs.append(rec.rollout(seq, r * K, mode=args.mode, states=None, global_reward_avg=True, log_positions=True)["xpos"])
        exact = torch.cat(logs).transpose(0, 1).contiguous()          # [B, total, N]
        del logs
        forms = []
        for name, lib in libs:
            for kind in ("none", "log", "exact", "wrap"):
                with _lib.use(lib):
                    env = VecV2VEnv(cfg, batch=B, device=dev, out_dtype=torch.float32)
                env.reset_topology(seed=1234)
                forms.append(dict(form=name + ":" + kind, kind=kind, env=env, t=0, ms=[]))

        def body(f):
            kw = {"none": {}, "log": dict(log_positions=True), "exact": dict(positions=exact), "wrap": dict(positions=wrap)}[f["kind"]]
            f["out"] = f["env"].rollout(seq, f["t"], mode=args.mode, states=None, global_reward_avg=True, **kw)
            f["t"] += K
        ab.timed_rounds(forms, body, args.rounds, args.warm)
        us, _ = ab.summary(forms, K)
        same = {f["form"]: bool(torch.equal(f["env"].export_state()["pos_x"], rec.export_state()["pos_x"])) for f in forms}
        print(json.dumps({"B": B, "us_per_slot": us, "ends_where_the_velocity_model_ends": same}), flush=True)
        assert total == exact.shape[1]
        del forms, exact, wrap, rec, s0
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
