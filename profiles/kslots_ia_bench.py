"""Information age inside the K-slot my_step_ch launches (VecV2VEnv.rollout(info_age=...) -> diral_env_rollout_ia) against
the loop they replace, timed as profiles/rollout_bench.py times: one box, the forms interleaved in one process, one env per
form, K = 25 slots a round, median of the rounds, us per slot; C2 shapes (64 UE / 32 resources) in my_step_ch, reward_design
2, float32, B = 64 / 1024 / 4096, handles with track_arrival.
  loop+ia (parent)   25 x (one-slot my_step_ch step + diral_env_info_age + diral_driver_shape with `ia`, flags 1 | 2) on a
                     library built from the PARENT commit (--parent-lib): what a build without the block runs;
  launch hist+term   one launch with every slot's histogram, its sum and the ia_averaging term;
  loop (parent)      25 x (step + diral_driver_shape without `ia`) on the parent's library: the stamps are kept, nothing reads them;
  launch stamps      one launch with info_age="stamps";
  launch hist        one launch with the histogram and its sum, no term: against `launch stamps` the cost of the histogram pass.
Every launch is checked against the parent's loop (`equal_to_parent_loop`: exported state with the stamps, metrics, shaped
rewards, sums, the histograms).

The guard for what existed (the two CH K-slot instantiations gained run-time branches): step_policy(slots=25,
mode=STEP_MY_STEP_CH) and rollout(mode="my_step_ch") on a handle WITHOUT track_arrival, without the block, at C2, B = 4096, on
the parent's library and on this one, interleaved in the same way (`slower_than_parent`, `equal_to_parent`).

  python profiles/kslots_ia_bench.py --parent-lib /path/to/parent/libdiral_env.so [--rounds 7] [--warm 2] [--only c2,guard]
"""
import argparse
import os

import torch

import ab  # noqa: E402  (puts the repository's root on sys.path)
from diral_amd import _lib  # noqa: E402
from diral_amd.config import KERNEL_POLICY, STEP_MY_STEP_CH, c2_config  # noqa: E402
from diral_amd.sps import SpsPolicy  # noqa: E402
from diral_amd.vec_env import VecV2VEnv, driver_shape  # noqa: E402

K = 25
FORMS = (("loop+ia (parent)", True, "loop_ia"), ("launch hist+term", False, "term"), ("loop (parent)", True, "loop"),
         ("launch stamps", False, "stamps"), ("launch hist", False, "hist"))


def run_feature(B, parent, rounds, warm):
    cfg = c2_config(reward_design=2, track_arrival=True)
    N = cfg.num_users
    dev = torch.device("cuda:0")
    forms = []
    for form, on_parent, kind in FORMS:
        with _lib.use(parent if on_parent else _lib.load()):
            env = VecV2VEnv(cfg, batch=B, device=dev, out_dtype=torch.float32)
        env.reset_topology(seed=1234)
        f = dict(form=form, kind=kind, env=env, t=0, ms=[], prev=torch.zeros((B,), dtype=torch.int64, device=dev))
        if kind.startswith("loop"):
            f.update(sh=torch.empty((K, B, N), dtype=torch.float32, device=dev), sr=torch.empty((K, B), dtype=torch.float32, device=dev),
                     co=torch.empty((K, B), dtype=torch.float32, device=dev), ia=torch.empty((K, B, 100), dtype=torch.int32, device=dev),
                     ia_sum=torch.empty((K, B), dtype=torch.int64, device=dev), pen=torch.empty((K, B), dtype=torch.int32, device=dev))
        forms.append(f)
    seq = torch.stack([forms[0]["env"].sample(4000 + k) for k in range(K)])

    def body(f):
        env, kind = f["env"], f["kind"]
        if not kind.startswith("loop"):
            out = env.rollout(seq, f["t"], mode="my_step_ch", states=None, global_reward_avg=True,
                              info_age="stamps" if kind == "stamps" else True, sum_ia_prev=f["prev"] if kind == "term" else None)
            assert env.last_kernel() & KERNEL_POLICY
            f["sh"], f["sr"], f["co"] = out["shaped"], out["sum_r"], out["collision"]
            f["ia"], f["ia_sum"], f["pen"] = out.get("ia"), out.get("ia_sum"), out.get("ia_penalty")
            f["t"] += K
            return
        for k in range(K):
            _, rew, _ = env._step(STEP_MY_STEP_CH, seq[k], f["t"], want_obs=False)
            if kind == "loop_ia":
                st = env.lib.diral_env_info_age(env._h, f["t"], f["ia"][k].data_ptr(), env._stream())
                assert st == 0
                driver_shape(env, rew, seq[k], shaped=f["sh"][k], sum_r=f["sr"][k], collision=f["co"][k], global_reward_avg=True,
                             ia=f["ia"][k], sum_ia_prev=f["prev"], ia_sum=f["ia_sum"][k], ia_penalty=f["pen"][k])
            else:
                driver_shape(env, rew, seq[k], shaped=f["sh"][k], sum_r=f["sr"][k], collision=f["co"][k], global_reward_avg=True)
            f["t"] += 1

    ab.timed_rounds(forms, body, rounds, warm)
    us, rnd = ab.summary(forms, K)
    by = {f["kind"]: f for f in forms}
    equal = {}
    for kind, ref, keys in (("term", "loop_ia", ("sh", "sr", "co", "ia", "ia_sum", "pen", "prev")), ("stamps", "loop", ("sh", "sr", "co")),
                            ("hist", "loop", ("sr", "co"))):
        x, p = by[kind], by[ref]
        equal[x["form"]] = bool(ab.same_env(p["env"], x["env"]) and all(torch.equal(p[k], x[k]) for k in keys))
    equal["launch hist (histograms)"] = bool(torch.equal(by["hist"]["ia"], by["loop_ia"]["ia"]))
    saving = {"launch hist+term vs loop+ia (parent)": round(1.0 - us["launch hist+term"] / us["loop+ia (parent)"], 4),
              "launch stamps vs loop (parent)": round(1.0 - us["launch stamps"] / us["loop (parent)"], 4)}
    hist_cost = round(us["launch hist"] - us["launch stamps"], 2)
    for f in forms:
        f["env"].check()
    out = {"config": "c2 my_step_ch track_arrival", "N": N, "A": cfg.num_channels, "B": B, "slots_per_round": K, "rounds": rounds,
           "us_per_slot": us, "us_per_slot_rounds": rnd, "equal_to_parent_loop": equal, "saving": saving,
           "histogram_pass_us_per_slot": hist_cost}
    del forms, by
    torch.cuda.empty_cache()
    return out


def run_guard(B, parent, rounds, warm):
    """step_policy(slots=25, my_step_ch) and rollout(my_step_ch) without arrival stamps, on the parent's library and on this one."""
    cfg = c2_config(reward_design=2)
    N, A = cfg.num_users, cfg.num_channels
    dev = torch.device("cuda:0")
    forms = []
    for what in ("step_policy K=25", "rollout K=25"):
        for tag, lib in ((" (parent)", parent), ("", _lib.load())):
            with _lib.use(lib):
                env = VecV2VEnv(cfg, batch=B, device=dev, out_dtype=torch.float32)
            env.reset_topology(seed=1234)
            f = dict(form=what + tag, what=what, env=env, t=0, i=0, ms=[])
            if what.startswith("step_policy"):
                pol = SpsPolicy(B, N, A, device=dev, seed=5)
                f.update(pol=pol, acts=[pol.prev_action.clone(), torch.empty_like(pol.prev_action)],
                         sh=torch.empty((K, B, N), dtype=torch.float32, device=dev), sr=torch.empty((K, B), dtype=torch.float32, device=dev),
                         co=torch.empty((K, B), dtype=torch.float32, device=dev))
            forms.append(f)
    seq = torch.stack([forms[0]["env"].sample(4000 + k) for k in range(K)])

    def body(f):
        env = f["env"]
        if f["what"].startswith("step_policy"):
            i = f["i"]
            env.step_policy(f["acts"][i], f["t"], f["pol"], f["acts"][i ^ 1], shaped_out=f["sh"], sum_r_out=f["sr"],
                            collision_out=f["co"], global_reward_avg=True, slots=K, want_obs=False, mode=STEP_MY_STEP_CH)
            f["i"] ^= 1
        else:
            out = env.rollout(seq, f["t"], mode="my_step_ch", states=None, global_reward_avg=True)
            f["sh"] = out["shaped"]
        f["t"] += K
        assert env.last_kernel() & KERNEL_POLICY

    ab.timed_rounds(forms, body, rounds, warm)
    us, rnd = ab.summary(forms, K)
    s0, s1, r0, r1 = forms
    equal = {"step_policy K=25": bool(ab.same_env(s0["env"], s1["env"]) and torch.equal(s0["sh"], s1["sh"]) and torch.equal(s0["pol"].counter, s1["pol"].counter)),
             "rollout K=25": bool(ab.same_env(r0["env"], r1["env"]) and torch.equal(r0["sh"], r1["sh"]))}
    slower = {w: round(us[w] / us[w + " (parent)"] - 1.0, 4) for w in ("step_policy K=25", "rollout K=25")}
    out = {"config": "guard: c2 my_step_ch, no arrival stamps", "B": B, "slots_per_round": K, "rounds": rounds, "us_per_slot": us,
           "us_per_slot_rounds": rnd, "equal_to_parent": equal, "slower_than_parent": slower}
    del forms
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--batches", default="64,1024,4096")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--only", default="c2,guard")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "kslots_ia", "kslots_ia_bench.txt"))
    args = ap.parse_args()
    parent, _ = ab.two_libraries(args.parent_lib, lacking=("diral_env_rollout_ia", "diral_env_step_policy_ia"))
    only = args.only.split(",")
    with ab.report(args.out) as emit:
        def show(r, key):
            emit("%s B=%d: %s  %s" % (r["config"], r["B"], "  ".join("%s %.1f" % kv for kv in r["us_per_slot"].items()), r[key]), r)
        if "c2" in only:
            for b in args.batches.split(","):
                show(run_feature(int(b), parent, args.rounds, args.warm), "saving")
        if "guard" in only:
            show(run_guard(4096, parent, args.rounds, args.warm), "slower_than_parent")


if __name__ == "__main__":
    main()
