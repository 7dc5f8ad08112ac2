"""The parent-against-branch guard: bench.py's own functions under the parent's library and under the branch's, alternating
in one session on one box, every measurement a fresh process (parent, branch, parent, ...), reported in the format and with
the criterion of profiles/slot_request/bench_guard.txt (ab.verdict).

  python profiles/bench_guard.py --parent-lib P [--branch-lib Q] [--rounds 6] [--lines c2,rollout_sps_fused,...]
      [--workload-steps 200 --warmup 50] [--dump-outputs] [--lacking SYMBOL,...] [--out FILE]

`--lacking`: the entry points the branch adds - the parent's library predates them and is bound without (`_lib.bind`).

One child is alive at a time, under the time limit of its line; a child that fails or runs into its limit ends the run: what
was collected is printed and the exit status is 1.  Nothing is tried twice.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import ab

# line -> (seconds a child may take: a cold process start is most of it, the measurement itself takes a few seconds;
#          {key of the child's JSON object: heading in the report})
LINES = {
    "c2": (120, {"c2": "c2 headline, us per step (%(steps)d timed steps, %(warmup)d warm-up)"}),
    "rollout_sps_fused": (120, {"first": "rollout_sps_fused, us per slot, first call of the process",
                                "second": "rollout_sps_fused, us per slot, second call of the process"}),
    "rollout_sps_kslots": (90, {"kslots": "rollout_sps_kslots, us per slot"}),
    "prefill_kslots": (120, {"envs_1024": "prefill_kslots one launch, 1024 envs, us per slot",
                             "envs_4096": "prefill_kslots one launch, 4096 envs, us per slot"}),
}
DUMP_LIMIT = 120


def child(line, steps, warmup, lacking=()):
    """One measurement in this process, under the library DIRAL_LIB names: one JSON object on stdout."""
    import torch

    if lacking:
        with ab._lib.use(ab._lib.bind(ab._lib.LIB_PATH, lacking)):
            return child(line, steps, warmup)
    import bench
    dev = torch.device("cuda:0")
    if line == "c2":
        out = {"c2": bench.run_workload("c2", dev, 0, 1, steps, warmup, emit_chobs=True)[1]["ms_per_step"] * 1e3}
    elif line == "rollout_sps_fused":
        out = {k: bench.rollout_sps_fused(dev)["ms_per_slot"] * 1e3 for k in ("first", "second")}
    elif line == "rollout_sps_kslots":
        out = {"kslots": bench.rollout_sps_kslots(dev)["ms_per_slot"] * 1e3}
    elif line == "prefill_kslots":
        out = {k: v["one_launch_us_per_slot"] for k, v in bench.prefill_kslots(dev).items() if k.startswith("envs_")}
    else:                                                           # "dump": what bench.py --dump-outputs writes, hashed
        env, _ = bench.run_workload("c2", dev, 0, 1, steps, warmup, emit_chobs=True)
        with tempfile.TemporaryDirectory() as tmp:
            out = {}
            for name in sorted(bench.dump_outputs(env, tmp, True)):
                with open(os.path.join(tmp, name + ".npy"), "rb") as fh:
                    out[name] = hashlib.sha256(fh.read()).hexdigest()
    print(json.dumps(out), flush=True)


def measure(lib, line, limit, args, lacking=None):
    """The child's JSON object, or None where it failed or ran into its limit."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", line, "--workload-steps", str(args.workload_steps),
           "--warmup", str(args.warmup)] + (["--lacking", lacking] if lacking else [])
    try:
        done = subprocess.run(cmd, env=dict(os.environ, DIRAL_LIB=lib), stdout=subprocess.PIPE, timeout=limit)
    except subprocess.TimeoutExpired:
        print("bench_guard: `%s` under %s ran into its limit of %d s" % (line, lib, limit), flush=True)
        return None
    if done.returncode != 0:
        print("bench_guard: `%s` under %s exited with status %d" % (line, lib, done.returncode), flush=True)
        return None
    return json.loads(done.stdout.decode().strip().splitlines()[-1])


def collect(libs, lines, args, got):
    for r in range(args.rounds):
        for line in lines:
            for side, lib in libs:
                res = measure(lib, line, LINES[line][0], args, args.lacking if side == "parent" else None)
                if res is None:
                    return False
                for key, us in res.items():
                    got.setdefault((line, key), {"parent": [], "branch": []})[side].append(us)
    if args.dump_outputs:
        for side, lib in libs:
            got[side] = measure(lib, "dump", DUMP_LIMIT, args, args.lacking if side == "parent" else None)
            if got[side] is None:
                return False
    return True


def report(got, lines, args):
    fmt = dict(steps=args.workload_steps, warmup=args.warmup)
    text = []
    for line in lines:
        for key, heading in LINES[line][1].items():
            v = got.get((line, key))
            if v and v["parent"]:
                text += [heading % fmt] + ["  %s rounds: %s" % (s, " ".join("%.3f" % x for x in v[s])) for s in ("parent", "branch")]
                if len(v["branch"]) == len(v["parent"]):
                    text.append(ab.verdict(v["parent"], v["branch"]))
                text.append("")
    if got.get("parent") and got.get("branch"):
        p, b = got["parent"], got["branch"]
        differ = [k for k in p if p[k] != b.get(k)]
        text.append("bench.py --dump-outputs (--steps %d --warmup %d): %s %s (sha256) between the two libraries." % (
            args.workload_steps, args.warmup, ", ".join(p), "byte-identical" if not differ else "DIFFER in " + ", ".join(differ)))
    return "\n".join(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--branch-lib", default=ab._lib.LIB_PATH)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--lines", default=",".join(LINES))
    ap.add_argument("--workload-steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--dump-outputs", action="store_true")
    ap.add_argument("--lacking", default=None, help="comma-separated entry points the parent's library predates")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help="(what a child process of this script measures)")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.workload_steps, args.warmup, tuple(args.lacking.split(",")) if args.lacking else ())
    if not args.parent_lib:
        ap.error("--parent-lib is required")
    libs = (("parent", os.path.abspath(args.parent_lib)), ("branch", os.path.abspath(args.branch_lib)))
    lines = args.lines.split(",")
    got = {}
    ok = collect(libs, lines, args, got)
    text = "%d alternating rounds, each measurement a process of its own (parent, branch, parent, ...).  Times in microseconds.\n" \
           "Criterion: the branch's median lies within min ... max of the parent's rounds.\n\n%s" % (args.rounds, report(got, lines, args))
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
