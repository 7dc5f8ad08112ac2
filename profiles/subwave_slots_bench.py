"""The sub-wave slot loop (csrc/step_subwave_slots.hpp, `use_subwave_path(slots=True)`) against the loop of one-slot calls it
replaces, timed interleaved in one process, median of the rounds, microseconds per slot (the method of
profiles/subwave_bench.py and DESIGN.md 3.2 item 16):
  loop (parent)   K x [one-slot sub-wave `diral_env_step` + `diral_driver_shape`] on a library built from the PARENT commit
                  (--parent-lib), handle pinned with `use_subwave_path()`; a state vector is built where the launch builds
                  one (every slot / the last slot / never);
  launch          `VecV2VEnv.rollout` of K slots on this library, handle pinned with `use_subwave_path(slots=True)`.
Configuration: configs/4ue_3r_toy (4 UE / 3 resources, L = 100, Rc = 250, 20 bins, congestion_test, reward_design 2,
add_action + the type-2 piggybacked histogram), float32 outputs, K = 25, global_reward_avg.  my_step with states last / all
/ none and my_step_ch with states last at B = 4096, 65 536 and 262 144; the random prefill (my_step_design) against the loop
of sample + step + observe.  Every launch must leave what the parent's loop leaves (`equal_to_parent_loop`: exported state,
metrics, shaped rewards, sums, states).

The guards for what exists, the parent's library against this one, interleaved, at B = 65 536 (`slower_than_parent`; the
2 % band of item 16; `equal_to_parent`: exported state, metrics and every output): the one-slot sub-wave step, and the
K-slot launch itself - `rollout` of K = 25 `my_step` slots with states last, and `prefill` - on two handles pinned with
`use_subwave_path(slots=True)`.

  python profiles/subwave_slots_bench.py --parent-lib /path/to/parent/libdiral_env.so [--rounds 7] [--warm 2] [--out FILE]
"""
import argparse

import torch

import ab  # noqa: E402  (puts the repository's root on sys.path)
from diral_amd import _lib  # noqa: E402
from diral_amd.config import KERNEL_POLICY, KERNEL_SUBWAVE, STEP_DESIGN, STEP_MY_STEP, STEP_MY_STEP_CH, bench_config  # noqa: E402
from diral_amd.vec_env import VecV2VEnv, driver_shape  # noqa: E402

MODES = {"my_step": STEP_MY_STEP, "my_step_ch": STEP_MY_STEP_CH}
K = 25


def toy_config():
    return bench_config(4, 3, 100.0, communication_range=250.0, reward_design=2, congestion_test=True, State=dict(num_bins=20))


def make_env(B, lib, slots):
    with _lib.use(lib or _lib.load()):
        env = VecV2VEnv(toy_config(), batch=B, device=torch.device("cuda:0"), out_dtype=torch.float32)
    if slots:
        env.use_subwave_path(slots=True)
    else:
        env.use_subwave_path()
    env.reset_topology(seed=1234)
    return env


def own_body(f):
    f["body"](f)


def run_rollout(B, mode, states, parent, rounds, warm):
    loop, one = make_env(B, parent, False), make_env(B, None, True)
    seq = torch.stack([one.sample(4000 + k) for k in range(K)])
    o = dict(dtype=torch.float32, device=one.device)

    def loop_body(f):
        env = f["env"]
        for k in range(K):
            want = states == "all" or (states == "last" and k == K - 1)
            obs, rew, _ = env._step(MODES[mode], seq[k], f["t"], want_obs=want)
            driver_shape(env, rew, seq[k], shaped=f["sh"][k], sum_r=f["sr"][k], collision=f["co"][k], global_reward_avg=True)
            if states == "all":
                f["st"][k].copy_(obs)                                # (the loop's caller keeps every slot's state vector)
            f["t"] += 1
        f["last"] = obs

    def launch_body(f):
        out = f["env"].rollout(seq, f["t"], mode=mode, states=states, global_reward_avg=True)
        f["t"] += K
        f["sh"], f["sr"], f["co"], f["last"] = out["shaped"], out["sum_r"], out["collision"], out["states"]

    forms = [dict(form="loop (parent)", env=loop, t=0, ms=[], body=loop_body, sh=torch.empty((K, B, 4), **o), sr=torch.empty((K, B), **o),
                  co=torch.empty((K, B), **o), st=torch.empty((K, B, 4, loop.S), **o) if states == "all" else None),
             dict(form="launch", env=one, t=0, ms=[], body=launch_body)]
    ab.timed_rounds(forms, own_body, rounds, warm)
    assert (loop.last_kernel() & 15) == KERNEL_SUBWAVE and not (loop.last_kernel() & KERNEL_POLICY)
    assert one.last_kernel() == (KERNEL_SUBWAVE | KERNEL_POLICY), one.last_kernel()
    us, rnd = ab.summary(forms, K)
    p, x = forms
    equal = ab.same_env(loop, one) and all(torch.equal(p[k], x[k]) for k in ("sh", "sr", "co"))
    if states == "all":
        equal = equal and torch.equal(p["st"], x["last"])
    elif states == "last":
        equal = equal and torch.equal(p["last"], x["last"])
    loop.check(); one.check()
    out = {"config": "4ue_3r_toy %s states=%s" % (mode, states), "B": B, "slots_per_round": K, "rounds": rounds, "us_per_slot": us,
           "us_per_slot_rounds": rnd, "equal_to_parent_loop": bool(equal), "launch_vs_loop": round(us["launch"] / us["loop (parent)"], 4)}
    del forms, loop, one
    torch.cuda.empty_cache()
    return out


def run_prefill(B, parent, rounds, warm):
    loop, one = make_env(B, parent, False), make_env(B, None, True)
    a0 = one.sample(123)
    rews0 = None
    for env in (loop, one):
        _, rew, _ = env._step(STEP_MY_STEP, a0, 0)
        rews0 = rew.to(torch.float64).clone()
    o = dict(dtype=torch.float32, device=one.device)

    def loop_body(f):
        env = f["env"]
        for k in range(K):
            a = env.sample(f["seed"] + k)
            env._step(STEP_DESIGN, a, 0, want_chobs=True, want_obs=False)
            f["st"][k].copy_(env.obtain_state(env._chobs, a, rews0))
        f["seed"] += K

    def launch_body(f):
        env = f["env"]
        f["st"], _, _ = env.prefill(env.sample(f["seed"]), K, f["seed"], rew_in=rews0)
        f["seed"] += K

    forms = [dict(form="loop (parent)", env=loop, seed=77001, ms=[], body=loop_body, st=torch.empty((K, B, 4, loop.S), **o)),
             dict(form="launch", env=one, seed=77001, ms=[], body=launch_body)]
    ab.timed_rounds(forms, own_body, rounds, warm)
    assert one.last_kernel() == (KERNEL_SUBWAVE | KERNEL_POLICY), one.last_kernel()
    us, rnd = ab.summary(forms, K)
    equal = ab.same_env(loop, one) and torch.equal(forms[0]["st"], forms[1]["st"])
    loop.check(); one.check()
    out = {"config": "4ue_3r_toy prefill my_step_design", "B": B, "slots_per_round": K, "rounds": rounds, "us_per_slot": us,
           "us_per_slot_rounds": rnd, "equal_to_parent_loop": bool(equal), "launch_vs_loop": round(us["launch"] / us["loop (parent)"], 4)}
    del forms, loop, one
    torch.cuda.empty_cache()
    return out


def run_guard(B, parent, rounds, warm, slots=50):
    """The one-slot sub-wave step, the parent's library against this one."""
    envs = [("one-slot step (parent)", make_env(B, parent, False)), ("one-slot step", make_env(B, None, False))]
    acts = [envs[0][1].sample(4000 + k).clone() for k in range(slots)]

    def body(f):
        for k in range(slots):
            f["obs"], f["rew"], _ = f["env"]._step(STEP_MY_STEP, acts[k], f["t"])
            f["t"] += 1

    forms = [dict(form=name, env=env, t=0, ms=[], body=body) for name, env in envs]
    ab.timed_rounds(forms, own_body, rounds, warm)
    us, rnd = ab.summary(forms, slots)
    p, x = forms
    equal = ab.same_env(p["env"], x["env"]) and torch.equal(p["obs"], x["obs"]) and torch.equal(p["rew"], x["rew"])
    out = {"config": "4ue_3r_toy my_step one slot per call (guard)", "B": B, "slots_per_round": slots, "rounds": rounds, "us_per_slot": us,
           "us_per_slot_rounds": rnd, "equal_to_parent": bool(equal),
           "slower_than_parent": round(us["one-slot step"] / us["one-slot step (parent)"] - 1.0, 4)}
    del forms, envs
    torch.cuda.empty_cache()
    return out


def run_guard_slots(B, parent, rounds, warm, what):
    """The K-slot launch (`what`: "rollout" of my_step with states last, or "prefill"), the parent's library against this one."""
    envs = [("launch (parent)", make_env(B, parent, True)), ("launch", make_env(B, None, True))]
    if what == "rollout":
        seq = torch.stack([envs[1][1].sample(4000 + k) for k in range(K)])

        def body(f):
            out = f["env"].rollout(seq, f["t"], mode="my_step", states="last", global_reward_avg=True)
            f["t"] += K
            f["out"] = [out[k] for k in ("shaped", "sum_r", "collision", "states", "reward", "done") if out[k] is not None]
    else:
        a0 = envs[1][1].sample(123)
        for _, env in envs:
            _, rew, _ = env._step(STEP_MY_STEP, a0, 0)
            rews0 = rew.to(torch.float64).clone()

        def body(f):
            env = f["env"]
            f["out"] = list(env.prefill(env.sample(f["t"]), K, f["t"], rew_in=rews0))   # states, actions of every slot, next draw
            f["t"] += K

    forms = [dict(form=name, env=env, t=0 if what == "rollout" else 77001, ms=[], body=body) for name, env in envs]
    ab.timed_rounds(forms, own_body, rounds, warm)
    for f in forms:
        assert f["env"].last_kernel() == (KERNEL_SUBWAVE | KERNEL_POLICY), f["env"].last_kernel()
        f["env"].check()
    us, rnd = ab.summary(forms, K)
    p, x = forms
    equal = ab.same_env(p["env"], x["env"]) and all(torch.equal(a, b) for a, b in zip(p["out"], x["out"]))
    name = "my_step states=last rollout" if what == "rollout" else "prefill my_step_design"
    out = {"config": "4ue_3r_toy %s, K slots per launch (guard)" % name, "B": B, "slots_per_round": K, "rounds": rounds,
           "us_per_slot": us, "us_per_slot_rounds": rnd, "equal_to_parent": bool(equal),
           "slower_than_parent": round(us["launch"] / us["launch (parent)"] - 1.0, 4)}
    del forms, envs
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--batches", default="4096,65536,262144")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    parent, _ = ab.two_libraries(args.parent_lib)                       # (the option adds no symbol: the parent has them all)
    with ab.report(args.out) as emit:
        def show(r, key):
            emit("%s B=%d: %s us/slot  |  %s = %s  equal %s" % (
                r["config"], r["B"], "  ".join("%s %.2f" % kv for kv in r["us_per_slot"].items()), key, r[key],
                r.get("equal_to_parent_loop", r.get("equal_to_parent"))), r)
        for b in args.batches.split(","):
            for mode, states in (("my_step", "last"), ("my_step", "all"), ("my_step", None), ("my_step_ch", "last")):
                show(run_rollout(int(b), mode, states, parent, args.rounds, args.warm), "launch_vs_loop")
            show(run_prefill(int(b), parent, args.rounds, args.warm), "launch_vs_loop")
        show(run_guard(65536, parent, args.rounds, args.warm), "slower_than_parent")
        for what in ("rollout", "prefill"):
            show(run_guard_slots(65536, parent, args.rounds, args.warm, what), "slower_than_parent")


if __name__ == "__main__":
    main()
