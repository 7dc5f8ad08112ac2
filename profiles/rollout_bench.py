"""An open-loop rollout of K = 25 given slots (VecV2VEnv.rollout -> diral_env_rollout) against the loop it replaces, timed
interleaved in one process, one env per form, median of the rounds:
  loop (parent)   25 x (diral_env_step + diral_driver_shape [+ update_velocity at an episode end]) on a library built from
                  the PARENT commit (--parent-lib): the code a build without the rollout entry point runs;
  loop            the same calls on this build (recorded: it leaves what the parent's loop leaves);
  rollout         one launch.
"last": the state vector of the last slot only (the loop asks its last step for it); "all": every slot's (the loop copies
each step's state into a [K, B, N, S] buffer, the launch writes that buffer itself; N <= 64 only).
Shapes: C2 (64 UE / 32 res) at B = 64 / 1024 / 4096, my_step and my_step_ch; C5 (128 UE / 64 res, mobility_vary, 16384 envs)
and C3 (256 UE / 64 res, 8192 envs), my_step, "last".

The guard for what already exists (the slot loop gained a run-time branch): step_policy(slots=25) and prefill(slots=25) at
C2, B = 4096, on the parent's library and on this one, interleaved in the same way.

  python profiles/rollout_bench.py --parent-lib /path/to/parent/libdiral_env.so [--rounds 7] [--warm 2] [--only c2,wide,guard]
"""
import argparse

import torch

import ab  # noqa: E402  (puts the repository's root on sys.path)
from diral_amd import _lib  # noqa: E402
from diral_amd.config import KERNEL_POLICY, STEP_MY_STEP, STEP_MY_STEP_CH, bench_config, c2_config  # noqa: E402
from diral_amd.driver import DriverLoop  # noqa: E402
from diral_amd.sps import SpsPolicy  # noqa: E402
from diral_amd.vec_env import VecV2VEnv  # noqa: E402

K = 25
VEL_SEED = 77
WIDE = {"c5": (128, 64, 4000.0, 16384, True), "c3": (256, 64, 4000.0, 8192, False)}
MODES = {"my_step": STEP_MY_STEP, "my_step_ch": STEP_MY_STEP_CH}


def shape(env, rew, a, sh, sr, co):
    st = env.lib.diral_driver_shape(env.B, env.N, env.A, rew.data_ptr(), 0, a.data_ptr(), None, None, None, None, 1, 0, 0.0,
                                    sh.data_ptr(), sr.data_ptr(), co.data_ptr(), None, None, env._stream())
    assert st == 0


def run_rollout(name, cfg, B, mode, kinds, parent, rounds, warm):
    N = cfg.num_users
    dev = torch.device("cuda:0")
    vary = cfg.mobility_vary
    EI = cfg.episode_interval
    forms, branch = [], _lib.load()
    for kind in kinds:
        for form, lib in (("loop (parent) " + kind, parent), ("loop " + kind, branch), ("rollout " + kind, branch)):
            with _lib.use(lib):
                env = VecV2VEnv(cfg, batch=B, device=dev, out_dtype=torch.float32)
            env.reset_topology(seed=1234)
            f = dict(form=form, kind=kind, env=env, t=0, ms=[], launch=form.startswith("rollout"))
            if not f["launch"]:
                f.update(sh=torch.empty((K, B, N), dtype=torch.float32, device=dev), sr=torch.empty((K, B), dtype=torch.float32, device=dev),
                         co=torch.empty((K, B), dtype=torch.float32, device=dev))
                if kind == "all":
                    f["states"] = torch.empty((K, B, N, env.S), dtype=torch.float32, device=dev)
            forms.append(f)
    seq = torch.stack([forms[0]["env"].sample(4000 + k) for k in range(K)])

    def body(f):
        env = f["env"]
        if f["launch"]:
            out = env.rollout(seq, f["t"], mode=mode, states=f["kind"], global_reward_avg=True, vel_seed=VEL_SEED)
            assert env.last_kernel() & KERNEL_POLICY
            f["sh"], f["sr"], f["co"], f["states"] = out["shaped"], out["sum_r"], out["collision"], out["states"]
            f["t"] += K
            return
        every = f["kind"] == "all"
        for k in range(K):
            obs, rew, _ = env._step(MODES[mode], seq[k], f["t"], want_obs=every or k == K - 1)
            shape(env, rew, seq[k], f["sh"][k], f["sr"][k], f["co"][k])
            if every:
                f["states"][k].copy_(obs)
            if vary and f["t"] % EI == EI - 1:
                env.update_velocity(seed=VEL_SEED + f["t"] // EI)
            f["t"] += 1
        if not every:
            f["states"] = obs

    ab.timed_rounds(forms, body, rounds, warm)
    us, rnd = ab.summary(forms, K)
    equal, saving = {}, {}
    for i in range(0, len(forms), 3):
        p, l, r = forms[i:i + 3]
        for x in (l, r):
            equal[x["form"]] = bool(ab.same_env(p["env"], x["env"]) and all(torch.equal(p[k], x[k]) for k in ("sh", "sr", "co", "states")))
        saving["rollout %s vs loop (parent)" % p["kind"]] = round(1.0 - us[r["form"]] / us[p["form"]], 4)
        saving["loop %s vs loop (parent)" % p["kind"]] = round(1.0 - us[l["form"]] / us[p["form"]], 4)
    for f in forms:
        f["env"].check()
    out = {"config": "%s %s" % (name, mode), "N": N, "A": cfg.num_channels, "B": B, "slots_per_round": K, "rounds": rounds,
           "us_per_slot": us, "us_per_slot_rounds": rnd, "equal_to_parent_loop": equal, "saving": saving}
    del forms
    torch.cuda.empty_cache()
    return out


def run_guard(B, parent, rounds, warm):
    """step_policy(slots=25) and prefill(slots=25) at C2 on the parent's library and on this one."""
    cfg = c2_config(reward_design=2)
    N, A = cfg.num_users, cfg.num_channels
    dev = torch.device("cuda:0")
    forms = []
    for what in ("step_policy K=25", "prefill K=25"):
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
                else:
                    f["loop"] = DriverLoop(env)
                    f["loop"].bootstrap(env.sample(99))
                    f["seed"] = 5000
            forms.append(f)

    def body(f):
        env = f["env"]
        if f["what"].startswith("step_policy"):
            i = f["i"]
            env.step_policy(f["acts"][i], f["t"], f["pol"], f["acts"][i ^ 1], shaped_out=f["sh"], sum_r_out=f["sr"],
                            collision_out=f["co"], global_reward_avg=True, slots=K, want_obs=False)
            f["i"] ^= 1
            f["t"] += K
        else:
            f["states"], _, _ = env.prefill(env.sample(f["seed"]), K, f["seed"], rew_in=f["loop"]._rews0)
            f["seed"] += K
        assert env.last_kernel() & KERNEL_POLICY

    ab.timed_rounds(forms, body, rounds, warm)
    us, rnd = ab.summary(forms, K)
    s0, s1, p0, p1 = forms
    equal = {"step_policy K=25": bool(ab.same_env(s0["env"], s1["env"]) and torch.equal(s0["sh"], s1["sh"]) and torch.equal(s0["pol"].counter, s1["pol"].counter)),
             "prefill K=25": bool(ab.same_env(p0["env"], p1["env"]) and torch.equal(p0["states"], p1["states"]))}
    slower = {w: round(us[w] / us[w + " (parent)"] - 1.0, 4) for w in ("step_policy K=25", "prefill K=25")}
    out = {"config": "guard: c2 my_step", "B": B, "slots_per_round": K, "rounds": rounds, "us_per_slot": us,
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
    ap.add_argument("--only", default="c2,wide,guard")
    args = ap.parse_args()
    parent, _ = ab.two_libraries(args.parent_lib, lacking=("diral_env_rollout",))
    only = args.only.split(",")
    with ab.report() as emit:
        def show(r, key="saving"):
            emit("%s B=%d: %s  %s" % (r["config"], r["B"], "  ".join("%s %.1f" % kv for kv in r["us_per_slot"].items()), r[key]), r)
        if "c2" in only:
            for b in args.batches.split(","):
                for mode in ("my_step", "my_step_ch"):
                    show(run_rollout("c2", c2_config(reward_design=2), int(b), mode, ("last", "all"), parent, args.rounds, args.warm))
        if "wide" in only:
            for name, (N, A, L, B, vary) in WIDE.items():
                show(run_rollout(name, bench_config(N, A, L, mobility_vary=vary), B, "my_step", ("last",), parent, args.rounds, args.warm))
        if "guard" in only:
            show(run_guard(4096, parent, args.rounds, args.warm), "slower_than_parent")


if __name__ == "__main__":
    main()
