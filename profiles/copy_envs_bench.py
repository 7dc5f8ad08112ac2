"""Env copies (VecV2VEnv.copy_envs_from -> diral_env_copy_envs) against what they replace and against their ceiling, timed
interleaved in one process on one box, median of the rounds.  Between two rounds the source handle steps once (untimed): it
is in ring form, as it is inside a search, whenever a copy or an export meets it.

  copy            dst.copy_envs_from(src): every env, no index arrays
  copy perm       ... through a random permutation (src_index and dst_index given)
  broadcast       ... env 7 of src into every env of dst (C2 only)
  export+import   the only route before: src.export_state() -> dst.import_state(...), tables and positions only
  flat copy_      ONE torch.Tensor.copy_ of a uint8 buffer with the byte count of the handles' state slabs: the ceiling
  rollout         work.rollout of 25 given slots (C2, B = 4096)
  fork+rollout    work.copy_envs_from(env, gather) (512 envs x 8 candidates) + the same rollout

  python profiles/copy_envs_bench.py [--rounds 9] [--warm 2] [--only c2,c5,fork] > profiles/copy_envs/copy_bench.txt
"""
import argparse

import torch

import ab  # noqa: E402  (puts the repository's root on sys.path)
from diral_amd.config import bench_config, c2_config  # noqa: E402
from diral_amd.search import candidate_index  # noqa: E402
from diral_amd.vec_env import VecV2VEnv  # noqa: E402

K = 25
SHAPES = {"c2": (lambda: c2_config(), 4096), "c5": (lambda: bench_config(128, 64, 4000.0, mobility_vary=True), 16384)}


def state_bytes_per_env(env):
    """The slabs diral_env_copy_envs moves for one env of a packed-form handle without arrival stamps, proportional-fair
    counters or prev_obs (csrc/diral_env.hip, the `own` calls of diral_env_create)."""
    N = env.N
    NR = (N + 15) // 16 * 16
    NV = 64 if N <= 64 else NR
    planes = NR * NV * (4 + 8)
    packed = 2 * (NR // 4) * NV * 4 + NR * 4 + (NR // 4) * 4
    return 3 * N * 8 + planes + NR * 8 * 8 + packed + 6 * 8, planes


def show(emit, config, B, forms, rounds, extra):
    us, rnd = ab.summary(forms, digits=1)
    out = dict(config=config, B=B, rounds=rounds, us=us, us_rounds=rnd)
    out.update(extra)
    emit("%s B=%d: %s" % (config, B, "  ".join("%s %.1f" % kv for kv in us.items())), out)


def run_copy(emit, name, rounds, warm):
    make, B = SHAPES[name]
    cfg = make()
    dev = torch.device("cuda:0")
    src, dst, dst2 = (VecV2VEnv(cfg, batch=B, device=dev) for _ in range(3))
    src.reset_topology(seed=1234)
    acts = src.sample(7)
    for t in range(10):
        src.step(acts, t)
    per_env, planes = state_bytes_per_env(src)
    flat_a = torch.empty(per_env * B, dtype=torch.uint8, device=dev)
    flat_b = torch.zeros(per_env * B, dtype=torch.uint8, device=dev)
    perm_s = torch.randperm(B, device=dev).to(torch.int32)
    perm_d = torch.randperm(B, device=dev).to(torch.int32)
    one = torch.full((B,), 7, dtype=torch.int32, device=dev)

    def export_import():
        st = src.export_state()
        dst2.import_state(st["pos_x"], st["pos_y"], st["vel"], seq=st["seq"], age=st["age"], x=st["x"])

    forms = [dict(form="copy", body=lambda: dst.copy_envs_from(src)),
             dict(form="copy perm", body=lambda: dst.copy_envs_from(src, perm_s, perm_d)),
             dict(form="export+import", body=export_import),
             dict(form="flat copy_", body=lambda: flat_a.copy_(flat_b))]
    if name == "c2":
        forms.insert(2, dict(form="broadcast", body=lambda: dst.copy_envs_from(src, src_index=one)))
    clock = [10]

    def between(_):
        src.step(acts, clock[0])
        clock[0] += 1
    ab.timed_rounds(forms, ab.own_body, rounds, warm, between=between)
    # the copy did what the old route does, and more: tables and positions agree, metrics only on the copied handle
    dst.copy_envs_from(src)
    export_import()
    a, b, c = src.export_state(), dst.export_state(), dst2.export_state()
    equal = bool(all(torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) for k in a) and torch.equal(src.metrics(), dst.metrics()))
    for e in (src, dst, dst2):
        e.check()
    moved = 2 * per_env * B
    us = {f["form"]: ab.per_unit(ab.median(f["ms"]), 1) for f in forms}
    show(emit, "%s copy" % name, B, forms, rounds,
           dict(N=cfg.num_users, A=cfg.num_channels, bytes_per_env=per_env, plane_bytes_per_env=planes, equal=equal,
                tb_per_s={k: round(moved / (v * 1e-6) / 1e12, 2) for k, v in us.items() if k != "export+import"},
                copy_vs_flat=round(us["copy"] / us["flat copy_"], 3), export_import_vs_copy=round(us["export+import"] / us["copy"], 2)))
    del forms, src, dst, dst2, flat_a, flat_b
    torch.cuda.empty_cache()


def run_fork(emit, rounds, warm):
    cfg = c2_config()
    dev = torch.device("cuda:0")
    B, C = 512, 8
    env = VecV2VEnv(cfg, batch=B, device=dev)
    env.reset_topology(seed=1234)
    acts = env.sample(7)
    for t in range(10):
        env.step(acts, t)
    alone, work = env.twin(B * C), env.twin(B * C)
    gather = candidate_index(B, C, dev)
    alone.copy_envs_from(env, src_index=gather)
    seq = torch.stack([work.sample(4000 + k) for k in range(K)])
    forms = [dict(form="rollout", body=lambda: alone.rollout(seq, 0, states=None)),
             dict(form="fork+rollout", body=lambda: (work.copy_envs_from(env, src_index=gather), work.rollout(seq, 0, states=None)))]
    clock = [10]

    def between(_):
        env.step(acts, clock[0])
        clock[0] += 1
    ab.timed_rounds(forms, ab.own_body, rounds, warm, between=between)
    for e in (env, alone, work):
        e.check()
    us = {f["form"]: ab.per_unit(ab.median(f["ms"]), 1) for f in forms}
    show(emit, "c2 fork %d x %d + %d slots" % (B, C, K), B * C, forms, rounds,
           dict(us_per_slot={k: round(v / K, 2) for k, v in us.items()}, fork_share=round(us["fork+rollout"] / us["rollout"] - 1.0, 4)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--only", default="c2,c5,fork")
    args = ap.parse_args()
    only = args.only.split(",")
    print("device: %s" % torch.cuda.get_device_name(0), flush=True)
    with ab.report() as emit:
        for name in ("c2", "c5"):
            if name in only:
                run_copy(emit, name, args.rounds, args.warm)
        if "fork" in only:
            run_fork(emit, args.rounds, args.warm)


if __name__ == "__main__":
    main()
