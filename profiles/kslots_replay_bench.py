"""Recorded mobility inside the K-slot launches (VecV2VEnv.rollout / step_policy(positions=...) -> diral_env_rollout_replay /
diral_env_step_policy_replay) against the loops they replace, timed as profiles/kslots_ia_bench.py times: one box, the forms
interleaved in one process, one env per form, K = 25 slots a round, median of the rounds, us per slot; C2 shapes (64 UE / 32
resources), reward_design 2, float32, B = 64 / 1024 / 4096.  The sequence is one per env, [B, T = 25, N]: the positions of
the velocity model from the envs' start, so that the topologies are C2's.
  loop (parent)      25 x one-slot call on a library built from the PARENT commit (--parent-lib) with the sequence on the
                     handle (diral_env_set_trace): step + diral_driver_shape; the closed loop: the three launches of
                     diral_env_step_policy; the information age: + diral_env_info_age, the shaping with `ia` (flags 1 | 2);
  launch             one launch that carries the sequence; `+log`: and writes the position log.
states=last: the loop asks only its last step for a state vector; states=all: the loop copies every step's state into
[K, B, N, S], the launch writes that buffer itself (as profiles/rollout_bench.py).
Every launch is checked against the parent's loop (`equal_to_parent_loop`: exported state, metrics, shaped rewards, sums).

The guard for what existed: step_policy(slots=25) in my_step and my_step_ch, rollout in both modes and rollout(info_age=True),
all WITHOUT the block, at C2, B = 4096, on the parent's library and on this one, interleaved in the same way
(`slower_than_parent`, `equal_to_parent`).

  python profiles/kslots_replay_bench.py --parent-lib /path/to/parent/libdiral_env.so [--rounds 7] [--warm 2] [--only c2,guard]
"""
import argparse
import os

import torch

import ab  # noqa: E402  (puts the repository's root on sys.path)
from diral_amd import _lib  # noqa: E402
from diral_amd.config import KERNEL_POLICY, STEP_MY_STEP, STEP_MY_STEP_CH, c2_config  # noqa: E402
from diral_amd.sps import SpsPolicy  # noqa: E402
from diral_amd.vec_env import VecV2VEnv, driver_shape  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
K = 25
MODES = {"my_step": STEP_MY_STEP, "my_step_ch": STEP_MY_STEP_CH}
# (name of the pair, mode, states, closed loop, information age, position log)
PAIRS = (("rollout my_step", "my_step", None, False, False, False),
         ("rollout my_step +log", "my_step", None, False, False, True),
         ("rollout my_step states=last", "my_step", "last", False, False, False),
         ("rollout my_step states=all", "my_step", "all", False, False, False),
         ("rollout my_step_ch", "my_step_ch", None, False, False, False),
         ("step_policy my_step", "my_step", None, True, False, False),
         ("step_policy my_step_ch", "my_step_ch", None, True, False, False),
         ("rollout my_step_ch info_age", "my_step_ch", None, False, True, False))


def make_form(name, cfg, B, lib, dev, **kw):
    with _lib.use(lib):
        env = VecV2VEnv(cfg, batch=B, device=dev, out_dtype=torch.float32)
    env.reset_topology(seed=1234)
    N = cfg.num_users
    o = dict(dtype=torch.float32, device=dev)
    f = dict(form=name, env=env, t=0, i=0, ms=[], sh=torch.empty((K, B, N), **o), sr=torch.empty((K, B), **o),
             co=torch.empty((K, B), **o), prev=torch.zeros((B,), dtype=torch.int64, device=dev),
             ia=torch.empty((K, B, 100), dtype=torch.int32, device=dev), ia_sum=torch.empty((K, B), dtype=torch.int64, device=dev),
             pen=torch.empty((K, B), dtype=torch.int32, device=dev), **kw)
    if kw.get("closed"):
        pol = SpsPolicy(B, N, cfg.num_channels, device=dev, seed=5)
        f.update(pol=pol, acts=[pol.prev_action.clone(), torch.empty_like(pol.prev_action)])
    return f


def sequence(cfg, B, dev):
    """[B, K, N]: where the velocity model takes the envs of reset_topology(seed=1234) in K slots."""
    env = VecV2VEnv(cfg, batch=B, device=dev, out_dtype=torch.float32)
    env.reset_topology(seed=1234)
    s = env.export_state(tables=False)
    k = torch.arange(1, K + 1, dtype=torch.float64, device=dev).view(1, K, 1)
    return torch.remainder(s["pos_x"].unsqueeze(1) + s["vel"].unsqueeze(1) * k, float(cfg.highway_length)).contiguous()


def body(f, seq, tr):
    env, mode = f["env"], f["mode"]
    if f["launch"]:
        pos = tr if f["block"] else None
        if f["closed"]:
            i = f["i"]
            env.step_policy(f["acts"][i], f["t"], f["pol"], f["acts"][i ^ 1], shaped_out=f["sh"], sum_r_out=f["sr"], collision_out=f["co"],
                            global_reward_avg=True, slots=K, want_obs=False, mode=MODES[mode], positions=pos)
            f["i"] ^= 1
        else:
            kw = dict(info_age=True, sum_ia_prev=f["prev"]) if f["ia_on"] else {}
            if f["block"]:
                kw.update(positions=pos, log_positions=f["log"])
            out = env.rollout(seq, f["t"], mode=mode, states=f["states"], global_reward_avg=True, **kw)
            f["sh"], f["sr"], f["co"] = out["shaped"], out["sum_r"], out["collision"]
            f["xpos"] = out.get("xpos")
            if f["states"] == "all":
                f["st_all"] = out["states"]
        assert env.last_kernel() & KERNEL_POLICY
        f["t"] += K
        return
    for k in range(K):
        if f["closed"]:
            i = f["i"]
            env.step_policy(f["acts"][i], f["t"], f["pol"], f["acts"][i ^ 1], shaped_out=f["sh"][k], sum_r_out=f["sr"][k],
                            collision_out=f["co"][k], global_reward_avg=True, want_obs=False, mode=MODES[mode])
            f["i"] ^= 1
        else:
            want = f["states"] == "all" or (f["states"] == "last" and k == K - 1)
            obs, rew, _ = env._step(MODES[mode], seq[k], f["t"], want_obs=want)
            if f["states"] == "all":
                if "st_all" not in f:
                    f["st_all"] = torch.empty((K,) + tuple(obs.shape), dtype=obs.dtype, device=obs.device)
                f["st_all"][k].copy_(obs)
            if f["ia_on"]:
                assert env.lib.diral_env_info_age(env._h, f["t"], f["ia"][k].data_ptr(), env._stream()) == 0
                driver_shape(env, rew, seq[k], shaped=f["sh"][k], sum_r=f["sr"][k], collision=f["co"][k], global_reward_avg=True,
                             ia=f["ia"][k], sum_ia_prev=f["prev"], ia_sum=f["ia_sum"][k], ia_penalty=f["pen"][k])
            else:
                driver_shape(env, rew, seq[k], shaped=f["sh"][k], sum_r=f["sr"][k], collision=f["co"][k], global_reward_avg=True)
        f["t"] += 1


def run_feature(B, parent, rounds, warm):
    dev = torch.device("cuda:0")
    cfgs = {False: c2_config(reward_design=2), True: c2_config(reward_design=2, track_arrival=True)}
    tr = sequence(cfgs[False], B, dev)
    forms = []
    for name, mode, states, closed, ia_on, log in PAIRS:
        kw = dict(mode=mode, states=states, closed=closed, ia_on=ia_on, log=log, block=True, pair=name)
        if not log:                                                  # (the +log launch is measured against the loop of its pair)
            lp = make_form(name + ": loop (parent)", cfgs[ia_on], B, parent, dev, launch=False, **kw)
            lp["env"].load_saved_positions(tr)
            forms.append(lp)
        forms.append(make_form(name + ": launch", cfgs[ia_on], B, _lib.load(), dev, launch=True, **kw))
    seq = torch.stack([forms[0]["env"].sample(4000 + k) for k in range(K)])
    ab.timed_rounds(forms, lambda f: body(f, seq, tr), rounds, warm)
    us, rnd = ab.summary(forms, K)
    by = {f["form"]: f for f in forms}
    equal, saving = {}, {}
    for name, mode, states, closed, ia_on, log in PAIRS:
        ref = by[(name[:-5] if log else name) + ": loop (parent)"]
        x = by[name + ": launch"]
        keys = ("sh", "sr", "co") + (("prev",) if ia_on else ())
        ok = ab.same_env(ref["env"], x["env"]) and all(torch.equal(ref[k], x[k]) for k in keys)
        if closed:
            ok = ok and torch.equal(ref["pol"].counter, x["pol"].counter) and torch.equal(ref["pol"].prev_action, x["pol"].prev_action)
        if log:
            ok = ok and torch.equal(x["xpos"], tr.transpose(0, 1))
        if states == "all":
            ok = ok and torch.equal(ref["st_all"], x["st_all"])
        equal[name] = bool(ok)
        saving[name] = round(1.0 - us[x["form"]] / us[ref["form"]], 4)
    log_cost = round(us["rollout my_step +log: launch"] - us["rollout my_step: launch"], 2)
    for f in forms:
        f["env"].check()
    out = {"config": "c2 recorded positions", "B": B, "slots_per_round": K, "rounds": rounds, "us_per_slot": us,
           "us_per_slot_rounds": rnd, "equal_to_parent_loop": equal, "saving": saving, "position_log_us_per_slot": log_cost}
    del forms, by
    torch.cuda.empty_cache()
    return out


def run_guard(B, parent, rounds, warm):
    """The five calls WITHOUT the block, on the parent's library and on this one."""
    dev = torch.device("cuda:0")
    calls = (("step_policy my_step", "my_step", True, False), ("step_policy my_step_ch", "my_step_ch", True, False),
             ("rollout my_step", "my_step", False, False), ("rollout my_step_ch", "my_step_ch", False, False),
             ("rollout info_age", "my_step_ch", False, True))
    forms = []
    for name, mode, closed, ia_on in calls:
        cfg = c2_config(reward_design=2, track_arrival=ia_on)
        for tag, lib in ((" (parent)", parent), ("", _lib.load())):
            forms.append(make_form(name + tag, cfg, B, lib, dev, launch=True, block=False, mode=mode, states=None, closed=closed,
                                   ia_on=ia_on, log=False))
    seq = torch.stack([forms[0]["env"].sample(4000 + k) for k in range(K)])
    ab.timed_rounds(forms, lambda f: body(f, seq, None), rounds, warm)
    us, rnd = ab.summary(forms, K)
    by = {f["form"]: f for f in forms}
    equal, slower = {}, {}
    for name, mode, closed, ia_on in calls:
        p, x = by[name + " (parent)"], by[name]
        ok = ab.same_env(p["env"], x["env"]) and torch.equal(p["sh"], x["sh"]) and torch.equal(p["prev"], x["prev"])
        if closed:
            ok = ok and torch.equal(p["pol"].counter, x["pol"].counter)
        equal[name] = bool(ok)
        slower[name] = round(us[name] / us[name + " (parent)"] - 1.0, 4)
    out = {"config": "guard: c2, calls without the block", "B": B, "slots_per_round": K, "rounds": rounds, "us_per_slot": us,
           "us_per_slot_rounds": rnd, "equal_to_parent": equal, "slower_than_parent": slower}
    del forms, by
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--batches", default="64,1024,4096")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--only", default="c2,guard")
    ap.add_argument("--out", default=os.path.join(HERE, "kslots_replay", "kslots_replay_bench.txt"))
    args = ap.parse_args()
    parent, _ = ab.two_libraries(args.parent_lib, lacking=("diral_env_rollout_replay", "diral_env_step_policy_replay"))
    only = args.only.split(",")
    with ab.report(args.out) as emit:
        def show(r, key):
            emit("%s B=%d: %s" % (r["config"], r["B"], r[key]), r)
        if "c2" in only:
            for b in args.batches.split(","):
                show(run_feature(int(b), parent, args.rounds, args.warm), "saving")
        if "guard" in only:
            show(run_guard(4096, parent, args.rounds, args.warm), "slower_than_parent")


if __name__ == "__main__":
    main()
