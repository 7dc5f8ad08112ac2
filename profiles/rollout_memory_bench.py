"""The K-slot rollout / prefill that writes the replay memory's ring rows itself (`rollout(memory=)`, `prefill(memory=)`)
against the two-call form it replaces, timed interleaved in one process on one box (the method of
profiles/replay_memory_bench.py): every round times `--reps` back-to-back calls of every form between two device
events, the figure is the median round's time per call (enqueue included).

  a, a'   the PARENT library's rollout(states="all") alone - two series of the same form, interleaved with the others: their
          difference is the run-to-run spread the other comparisons are read against
  b       the parent library's rollout(states="all") + add_rollout          (prefill: prefill + add_prefill)
  c       this library's rollout(memory=)                                   (prefill: prefill(memory=))
  a new   this library's rollout(states="all") alone: the launch (c) would be without the block

Every form has a handle of its own, all reset alike and called alike, so every form times the same slots of the same envs.

The parent library is loaded next to this tree's from `--parent-lib` (the parent commit's libdiral_env.so): both sit in
one process, each behind its own handles.  Shapes: C2 (N = 64, A = 32, float32) at B = 64 / 1024 / 4096 in my_step and
my_step_ch, the toy config (N = 4) at B = 4096 / 65536; K = 25 slots, capacity 60.

  python profiles/rollout_memory_bench.py --parent-lib PATH [--rounds 7] [--warm 2] [--reps 5] > profiles/rollout_memory/rollout_memory_bench.txt
"""
import argparse

import torch

import ab  # noqa: E402  (puts the repository's root on sys.path)
from diral_amd import _lib  # noqa: E402
from diral_amd.config import bench_config, c2_config  # noqa: E402
from diral_amd.memory import ReplayMemory  # noqa: E402
from diral_amd.vec_env import VecV2VEnv  # noqa: E402

CAPACITY, K = 60, 25


def handle(lib, cfg, B):
    with _lib.use(lib):
        env = VecV2VEnv(cfg, batch=B, device="cuda:0", out_dtype=torch.float32)
        mem = ReplayMemory(CAPACITY, B, env.N, env.S, seed=1, device="cuda:0")
    if env.N <= 8:
        env.use_subwave_path(slots=True)
    env.reset_topology(seed=1)
    return env, mem


def run(emit, name, cfg, B, mode, libs, rounds, warm, reps):
    parent, new = libs
    # a handle (and a memory) per form, all from one topology: every form makes the same calls in the same order, so the
    # five envs move in lockstep and every form times the same slots
    forms = [("a", parent), ("b", parent), ("c", new), ("a'", parent), ("a new", new)]
    env, mem = {}, {}
    for form, lib in forms:
        env[form], mem[form] = handle(lib, cfg, B)
    N, S, A = env["c"].N, env["c"].S, env["c"].A
    seq = torch.randint(0, A, (K, B, N), dtype=torch.int32, device="cuda:0")
    s0 = torch.zeros((B, N, S), device="cuda:0")
    for form, _ in forms:
        mem[form].begin(s0)
        for _ in range(3):                                          # 75 adds: the rings have wrapped
            mem[form].add_rollout(seq, env[form].rollout(seq, mode=mode, states="all"))
    count0 = mem["b"].count
    rews0 = torch.randn((B, N), dtype=torch.float64, device="cuda:0")
    pmode = "my_step_ch" if mode == "my_step_ch" else "my_step_design"
    a0 = env["c"].sample(1)

    def alone(form):
        return lambda: env[form].rollout(seq, mode=mode, states="all")

    def two_calls():
        mem["b"].count = count0                                     # the same rows every time
        mem["b"].add_rollout(seq, env["b"].rollout(seq, mode=mode, states="all"))

    def into_ring():
        mem["c"].count = count0
        env["c"].rollout(seq, mode=mode, memory=mem["c"])

    def fill_alone(form):
        return lambda: env[form].prefill(a0, K, 1, rew_in=rews0, mode=pmode)

    def fill_two_calls():
        mem["b"].count = count0
        st, acts, _ = env["b"].prefill(a0, K, 1, rew_in=rews0, mode=pmode)
        mem["b"].add_prefill(st, acts, rews0)

    def fill_into_ring():
        mem["c"].count = count0
        env["c"].prefill(a0, K, 1, rew_in=rews0, mode=pmode, memory=mem["c"])

    bodies = dict(rollout={"a": alone("a"), "b": two_calls, "c": into_ring, "a'": alone("a'"), "a new": alone("a new")},
                  prefill={"a": fill_alone("a"), "b": fill_two_calls, "c": fill_into_ring, "a'": fill_alone("a'"),
                           "a new": fill_alone("a new")})
    for what in ("rollout", "prefill"):
        timing = [dict(form=form, body=bodies[what][form]) for form, _ in forms]
        ab.timed_rounds(timing, ab.own_body, rounds, warm, reps=reps)
        us, _ = ab.summary(timing, reps)
        spread = abs(us["a"] - us["a'"]) / min(us["a"], us["a'"])
        rec = dict(shape=name, what=what, mode=mode, B=B, N=N, S=S, K=K, capacity=CAPACITY, us_per_call=us,
                   c_over_b=round(us["c"] / us["b"], 3), c_over_a=round(us["c"] / min(us["a"], us["a'"]), 3),
                   a_new_over_a=round(us["a new"] / min(us["a"], us["a'"]), 3), a_spread=round(spread, 4),
                   us_rounds=ab.summary(timing, reps, digits=1)[1])
        emit("%s %s %s B=%d: us per call  a %.1f  a' %.1f  a new %.1f  b %.1f  c %.1f;  c / b = %.3f,  c / a = %.3f  (a against a': %.2f %%)"
             % (name, what, mode, B, us["a"], us["a'"], us["a new"], us["b"], us["c"], rec["c_over_b"], rec["c_over_a"], 100.0 * spread), rec)
    for form, _ in forms:
        env[form].check()
        env[form].close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    libs = ab.two_libraries(args.parent_lib, lacking=("diral_env_rollout_memory", "diral_env_prefill_memory"))
    print("device: %s" % torch.cuda.get_device_name(0), flush=True)
    toy = bench_config(4, 3, 100.0, communication_range=250.0, State=dict(num_bins=20))
    with ab.report() as emit:
        for mode in ("my_step", "my_step_ch"):
            for B in (64, 1024, 4096):
                run(emit, "c2", c2_config(reward_design=2), B, mode, libs, args.rounds, args.warm, args.reps)
        for B in (4096, 65536):
            run(emit, "toy", toy, B, "my_step", libs, args.rounds, args.warm, args.reps)


if __name__ == "__main__":
    main()
