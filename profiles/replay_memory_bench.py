"""ReplayMemory (diral_memory_add / diral_memory_sample) against the torch composition it replaces, timed interleaved in
one process on one box: every round times `--reps` back-to-back calls of every form between two device events, the
figure is the median round's time per call (enqueue included, as a training loop pays it).

  sample          one launch, windows drawn on the device
  sample idx      one launch, the same windows injected
  torch           advanced indexing of the same rings ([M, step + 1, N, S]), permute + contiguous for both state outputs,
                  the casts, and the same for actions and rewards of the last step
  add_many        one launch for K = 25 slots          torch: ring.index_copy_(0, rows, x) for the three rings
  rollout         the 25-slot rollout launch (states="all") that an add_many follows: the add as a share of it

Shapes: C2 (B = 4096, N = 64, S = 52; float32 -> float32 and -> bfloat16, step 6, M = 512 and 4096) and the toy config
(N = 4) at B = 65536.  `sample_tb_per_s` counts the ring rows read once and both state outputs written, next to the
6.29 TB/s of the flat copy in profiles/copy_envs/copy_bench.txt.

  python profiles/replay_memory_bench.py [--rounds 7] [--warm 2] [--reps 20] > profiles/replay_memory/memory_bench.txt
"""
import argparse

import torch

import ab  # noqa: E402  (puts the repository's root on sys.path)
from diral_amd.config import bench_config, c2_config  # noqa: E402
from diral_amd.memory import ReplayMemory  # noqa: E402
from diral_amd.vec_env import VecV2VEnv  # noqa: E402

FLAT_COPY_TB_S = 6.29
CAPACITY, K, STEP = 60, 25, 6


def torch_sample(mem, idx, env, step, out_dtype):
    rows = (mem.count - len(mem) + idx.long()[:, None] + torch.arange(step + 1, device=idx.device)) % (mem.C + 1)   # [M, step + 1]
    e = env.long()[:, None]
    blk = mem.states[rows, e]                                       # [M, step + 1, N, S]
    M = idx.shape[0]
    s = blk[:, :step].permute(2, 0, 1, 3).contiguous().view(mem.N * M, step, mem.S).to(out_dtype)
    n = blk[:, 1:].permute(2, 0, 1, 3).contiguous().view(mem.N * M, step, mem.S).to(out_dtype)
    a = mem.actions[rows[:, step - 1], env.long()].t().contiguous().view(-1)
    r = mem.rewards[rows[:, step - 1], env.long()].t().contiguous().view(-1)
    return s, a, r, n


def run(emit, name, cfg, B, Ms, out_dtypes, rounds, warm, reps):
    dev = torch.device("cuda:0")
    env = VecV2VEnv(cfg, batch=B, device=dev, out_dtype=torch.float32)
    if env.N <= 8:
        env.use_subwave_path(slots=True)
    env.reset_topology(seed=1)
    N, S, A = env.N, env.S, env.A
    mem = ReplayMemory(CAPACITY, B, N, S, seed=1, device=dev)
    seq = torch.randint(0, A, (K, B, N), dtype=torch.int32, device=dev)
    out = env.rollout(seq, states="all")
    mem.begin(out["states"][0].clone())
    for _ in range(3):                                              # 75 adds: the rings have wrapped
        mem.add_rollout(seq, out)
    st, sh = out["states"], out["shaped"]
    rows = (torch.arange(K, device=dev) + 7) % (CAPACITY + 1)
    twin_s, twin_a, twin_r = torch.empty_like(mem.states), torch.empty_like(mem.actions), torch.empty_like(mem.rewards)
    count0 = mem.count

    def add():
        mem.count = count0                                          # the same rows every time
        mem.add_many(seq, sh, st)

    def torch_add():
        twin_s.index_copy_(0, (rows + 1) % (CAPACITY + 1), st)
        twin_a.index_copy_(0, rows, seq)
        twin_r.index_copy_(0, rows, sh)

    forms = [dict(form="add_many", body=add), dict(form="torch index_copy", body=torch_add),
             dict(form="rollout", body=lambda: env.rollout(seq, states="all"))]
    ab.timed_rounds(forms, ab.own_body, rounds, warm, reps=max(2, reps // 4))
    us, _ = ab.summary(forms, max(2, reps // 4))
    add_bytes = 2 * (K * B * N * S * 4 + 2 * K * B * N * 4)
    rec = dict(shape=name, B=B, N=N, S=S, K=K, capacity=CAPACITY, us_per_call=us, add_bytes=add_bytes,
               add_tb_per_s=round(add_bytes / (us["add_many"] * 1e-6) / 1e12, 3),
               add_share_of_rollout=round(us["add_many"] / us["rollout"], 3), state_row_mb=round(B * N * S * 4 / 1e6, 1))
    emit("%s add: B=%d N=%d S=%d K=%d, us per call: %s; add_many = %.1f %% of the %d-slot rollout" % (
        name, B, N, S, K, "  ".join("%s %.1f" % kv for kv in us.items()), 100.0 * rec["add_share_of_rollout"], K), rec)
    mem.count = count0 + K
    del twin_s, twin_a, twin_r, out, st
    for M in Ms:
        for od in out_dtypes:
            outs = dict(states=torch.empty((N * M, STEP, S), dtype=od, device=dev),
                        next_states=torch.empty((N * M, STEP, S), dtype=od, device=dev),
                        actions=torch.empty((N * M,), dtype=torch.int32, device=dev),
                        rewards=torch.empty((N * M,), dtype=torch.float32, device=dev))
            mem.sample(M, STEP, out_dtype=od, last_only=True, out=outs)
            idx, e = mem.last_idx.clone(), mem.last_env.clone()
            got = mem.sample(M, STEP, out_dtype=od, last_only=True, idx=idx, env=e)
            want = torch_sample(mem, idx, e, STEP, od)
            agree = all(torch.equal(g, w) for g, w in zip(got, want))    # what was timed is what the tests compare
            forms = [dict(form="sample", body=lambda: mem.sample(M, STEP, out_dtype=od, last_only=True, out=outs)),
                     dict(form="sample idx", body=lambda: mem.sample(M, STEP, out_dtype=od, last_only=True, idx=idx, env=e, out=outs)),
                     dict(form="torch", body=lambda: torch_sample(mem, idx, e, STEP, od))]
            ab.timed_rounds(forms, ab.own_body, rounds, warm, reps=reps)
            us, rnd = ab.summary(forms, reps)
            nbytes = M * (STEP + 1) * N * S * 4 + 2 * M * STEP * N * S * outs["states"].element_size()
            rec = dict(shape=name, B=B, N=N, S=S, M=M, step=STEP, out_dtype=str(od), us_per_call=us, equals_torch=agree,
                       sample_bytes=nbytes,
                       sample_tb_per_s={k: round(nbytes / (v * 1e-6) / 1e12, 3) for k, v in us.items() if k != "torch"},
                       flat_copy_tb_per_s=FLAT_COPY_TB_S, us_rounds=rnd)
            emit("%s sample: M=%d -> %s, us per call: %s (equals torch: %s)"
                 % (name, M, od, "  ".join("%s %.1f" % kv for kv in us.items()), agree), rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    print("device: %s" % torch.cuda.get_device_name(0), flush=True)
    toy = bench_config(4, 3, 100.0, communication_range=250.0, State=dict(num_bins=20))
    with ab.report() as emit:
        run(emit, "c2", c2_config(), 4096, (512, 4096), (torch.float32, torch.bfloat16), args.rounds, args.warm, args.reps)
        run(emit, "toy", toy, 65536, (512, 4096), (torch.float32,), args.rounds, args.warm, args.reps)


if __name__ == "__main__":
    main()
