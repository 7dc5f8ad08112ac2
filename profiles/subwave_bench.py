"""The sub-wave step kernel (csrc/step_subwave.hpp, `use_subwave_path()`) against the paths a toy-size env runs on today,
timed interleaved in one process, one env per form, median of the rounds:
  AUTO      what a handle runs without any option: step_fast64, one 256-thread workgroup per env (the baseline: every
            existing kernel's resource-usage line is the parent's, profiles/subwave/resource_usage.txt);
  general   `force_general_kernel()`: step_kernel.hpp, the same shape;
  SUBWAVE   4 lanes per env, 16 envs per wavefront.
Configuration: configs/4ue_3r_toy (4 UE / 3 resources, L = 100, Rc = 250, 20 bins, congestion_test, reward_design 2,
add_action + the type-2 piggybacked histogram), float32 outputs.  my_step with a state vector at B = 4096, 65 536 and
262 144, my_step_ch at B = 65 536.  A round is SLOTS one-slot `diral_env_step` calls between two device events.

  python profiles/subwave_bench.py [--rounds 7] [--warm 2] [--slots 50] [--batches 4096,65536,262144] [--out FILE]
"""
import argparse

import torch

import ab  # noqa: E402  (puts the repository's root on sys.path)
from diral_amd.config import (KERNEL_FAST64, KERNEL_GENERAL, KERNEL_SUBWAVE, STEP_MY_STEP, STEP_MY_STEP_CH,  # noqa: E402
                              bench_config)
from diral_amd.vec_env import VecV2VEnv  # noqa: E402

MODES = {"my_step": STEP_MY_STEP, "my_step_ch": STEP_MY_STEP_CH}
FAMILY = {"AUTO": KERNEL_FAST64, "general": KERNEL_GENERAL, "SUBWAVE": KERNEL_SUBWAVE}


def toy_config():
    return bench_config(4, 3, 100.0, communication_range=250.0, reward_design=2, congestion_test=True, State=dict(num_bins=20))


def run(B, mode, slots, rounds, warm):
    cfg = toy_config()
    dev = torch.device("cuda:0")
    forms = []
    for form in ("AUTO", "general", "SUBWAVE"):
        env = VecV2VEnv(cfg, batch=B, device=dev, out_dtype=torch.float32)
        if form == "general":
            env.force_general_kernel()
        elif form == "SUBWAVE":
            env.use_subwave_path()
        env.reset_topology(seed=1234)
        forms.append(dict(form=form, env=env, t=0, ms=[]))
    acts = [forms[0]["env"].sample(4000 + k).clone() for k in range(slots)]

    def body(f):
        for k in range(slots):
            f["obs"], f["rew"], _ = f["env"]._step(MODES[mode], acts[k], f["t"])
            f["t"] += 1
    ab.timed_rounds(forms, body, rounds, warm)
    for f in forms:
        assert (f["env"].last_kernel() & 15) == FAMILY[f["form"]], (f["form"], f["env"].last_kernel())
    us, rnd = ab.summary(forms, slots)
    base = forms[0]
    sa = base["env"].export_state()
    steps, equal = {}, {}
    for f in forms:
        steps[f["form"]] = round(B * cfg.num_users / (us[f["form"]] * 1e-6))
        sb = f["env"].export_state()
        equal[f["form"]] = bool(all(torch.equal(sa[k], sb[k]) for k in sa) and torch.equal(base["obs"], f["obs"]) and
                                torch.equal(base["rew"], f["rew"]))
        f["env"].check()
    out = {"config": "4ue_3r_toy %s" % mode, "B": B, "slots_per_round": slots, "rounds": rounds, "us_per_slot": us,
           "agent_steps_per_s": steps, "us_per_slot_rounds": rnd, "equal_to_auto": equal,
           "subwave_vs_auto": round(us["SUBWAVE"] / us["AUTO"], 4)}
    del forms
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,65536,262144")
    ap.add_argument("--ch-batch", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--slots", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    with ab.report(args.out) as emit:
        def show(r):
            emit("%s B=%d: %s us/slot  |  %s agent-steps/s  |  SUBWAVE / AUTO = %.3f  equal %s" % (
                r["config"], r["B"], "  ".join("%s %.2f" % kv for kv in r["us_per_slot"].items()),
                "  ".join("%s %.3e" % kv for kv in r["agent_steps_per_s"].items()), r["subwave_vs_auto"], all(r["equal_to_auto"].values())), r)
        for b in args.batches.split(","):
            show(run(int(b), "my_step", args.slots, args.rounds, args.warm))
        show(run(args.ch_batch, "my_step_ch", args.slots, args.rounds, args.warm))


if __name__ == "__main__":
    main()
