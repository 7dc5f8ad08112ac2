"""Subset resets (VecV2VEnv.reset_envs -> diral_env_reset_envs) against the whole-batch reset and against the workaround
they replace, timed interleaved in one process on one box, median of the rounds.  Between two timed calls the handle steps
once (untimed): it is in ring form with live tables, as it is in a training loop, whenever a reset meets it.

  index n         E.reset_envs(idx, seed): n distinct envs as an int32 device tensor          n = 1, B/64, B/8, B
  mask n          E.reset_envs(mask=m, seed): a bool device tensor [B] with n envs set (grid.y covers all B envs)
  workaround n    the only route before: T.reset_topology(seed) on a twin + E.copy_envs_from(T, idx, idx)
  reset           E.reset_topology(seed) as a user calls it: the memsets of diral_env_reset + reset_kernel, through the
                  Python wrapper (its host time is inside the bracket where the device is done sooner than the host enqueues)
  reset raw       diral_env_reset of THIS library through raw ctypes on a handle of its own
  reset parent    diral_env_reset of a library built from the PARENT commit (--parent-lib), loaded next to this one, through
                  the same raw ctypes path: `reset raw` against `reset parent` is the like-for-like pair

  python profiles/reset_envs_bench.py [--rounds 7] [--warm 2] [--only c2,toy] [--parent-lib PATH] \
      > profiles/reset_envs/reset_envs_bench.txt
"""
import argparse
import ctypes

import torch

import ab  # noqa: E402  (puts the repository's root on sys.path)
from diral_amd import _lib  # noqa: E402
from diral_amd.config import bench_config, c2_config  # noqa: E402
from diral_amd.vec_env import VecV2VEnv  # noqa: E402

COPY_PEAK_TB_S = 6.29       # what copy_envs_kernel reaches (profiles/copy_envs/copy_bench.txt)
SEED = 20241


def toy_config():
    """configs/4ue_3r_toy's shape: 4 vehicles, 3 resources, L = 100, Rc = 250, 20 bins."""
    return bench_config(4, 3, 100.0, communication_range=250.0, State=dict(num_bins=20))


SHAPES = {"c2": (c2_config, 4096), "toy": (toy_config, 65536)}


def state_bytes_per_env(N):
    """What diral_env_reset_envs writes for one env of a packed-form handle without arrival stamps, proportional-fair
    counters or prev_obs (csrc/diral_env.hip, the `own` calls of diral_env_create): the slabs of copy_envs."""
    NR = (N + 15) // 16 * 16
    NV = 64 if N <= 64 else NR
    planes = NR * NV * (4 + 8)
    packed = 2 * (NR // 4) * NV * 4 + NR * 4 + (NR // 4) * 4
    return 3 * N * 8 + planes + NR * 8 * 8 + packed + 6 * 8


class RawLib:
    """`diral_env_reset` of a build of the library - this one or another - on a handle of its own, through raw ctypes: the
    same calling path for both, none of the Python wrapper's host time inside the timed bracket."""

    def __init__(self, lib, cfg, B):
        self.lib = lib                                              # (from _lib.load() or _lib.bind(): the prototypes are set)
        self.ccfg = cfg.to_c()
        self.h = ctypes.c_void_p()
        st = self.lib.diral_env_create(ctypes.byref(self.ccfg), B, 0, ctypes.byref(self.h))
        if st != 0:
            raise RuntimeError("diral_env_create returned %d" % st)

    def reset(self):
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        st = self.lib.diral_env_reset(self.h, None, None, None, SEED, s)
        if st != 0:
            raise RuntimeError("diral_env_reset returned %d" % st)

    def close(self):
        self.lib.diral_env_destroy(self.h)


def run(emit, name, rounds, warm, parent_lib):
    make, B = SHAPES[name]
    cfg = make()
    dev = torch.device("cuda:0")
    E, T = VecV2VEnv(cfg, batch=B, device=dev), VecV2VEnv(cfg, batch=B, device=dev)
    E.reset_topology(seed=1234)
    acts = E.sample(7)
    for t in range(10):
        E.step(acts, t)
    per_env = state_bytes_per_env(cfg.num_users)
    forms, written = [], {}
    for n in (1, B // 64, B // 8, B):
        idx = torch.randperm(B, device=dev)[:n].to(torch.int32).contiguous()
        mask = torch.zeros(B, dtype=torch.bool, device=dev)
        mask[idx.long()] = True
        forms.append(dict(form="index %d" % n, body=lambda idx=idx: E.reset_envs(idx, seed=SEED)))
        forms.append(dict(form="mask %d" % n, body=lambda mask=mask: E.reset_envs(mask=mask, seed=SEED)))
        forms.append(dict(form="workaround %d" % n,
                          body=lambda idx=idx: (T.reset_topology(seed=SEED), E.copy_envs_from(T, idx, idx))))
        for kind in ("index", "mask", "workaround"):
            written["%s %d" % (kind, n)] = n * per_env
    forms.append(dict(form="reset", body=lambda: E.reset_topology(seed=SEED)))
    written["reset"] = B * per_env
    own_raw = RawLib(_lib.load(), cfg, B)
    forms.append(dict(form="reset raw", body=own_raw.reset))
    written["reset raw"] = B * per_env
    parent = None
    if parent_lib:
        parent = RawLib(parent_lib, cfg, B)
        forms.append(dict(form="reset parent", body=parent.reset))
        written["reset parent"] = B * per_env
    clock = [10]

    def between(_):
        E.step(acts, clock[0])
        clock[0] += 1
    ab.timed_rounds(forms, ab.own_body, rounds, warm, between=between)
    # the subset call over every env leaves what the whole reset leaves
    E.reset_envs(count=B, seed=SEED)
    a = E.export_state()
    a["metrics"] = E.metrics()
    E.reset_topology(seed=SEED)
    b = E.export_state()
    b["metrics"] = E.metrics()
    equal = bool(all(torch.equal(a[k], b[k]) for k in a))
    for e in (E, T):
        e.check()
    us, rnd = ab.summary(forms, digits=1)
    tb = {k: round(written[k] / (us[k] * 1e-6) / 1e12, 3) for k in us if us[k] > 0}
    out = dict(config=name, B=B, N=cfg.num_users, A=cfg.num_channels, rounds=rounds, bytes_per_env=per_env, equal=equal, us=us,
               tb_written_per_s=tb, copy_kernel_tb_per_s=COPY_PEAK_TB_S,
               us_rounds=rnd,
               full_index_vs_reset=round(us["index %d" % B] / us["reset"], 3),
               full_mask_vs_reset=round(us["mask %d" % B] / us["reset"], 3))
    if parent:
        out["reset_raw_vs_parent"] = round(us["reset raw"] / us["reset parent"], 3)      # like for like: both raw ctypes
        out["full_index_vs_parent"] = round(us["index %d" % B] / us["reset parent"], 3)
        parent.close()
    own_raw.close()
    emit("%s B=%d (%d bytes per env), us: %s" % (name, B, per_env, "  ".join("%s %.1f" % kv for kv in us.items())), out)
    del forms, E, T
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--only", default="c2,toy")
    ap.add_argument("--parent-lib", default=None, help="libdiral_env.so built from the parent commit (the `reset parent` column)")
    args = ap.parse_args()
    print("device: %s" % torch.cuda.get_device_name(0), flush=True)
    if not args.parent_lib:
        print("no --parent-lib: the `reset parent` column is left out", flush=True)
    parent = ab.two_libraries(args.parent_lib, lacking=("diral_env_reset_envs",))[0] if args.parent_lib else None
    with ab.report() as emit:
        for name in ("c2", "toy"):
            if name in args.only.split(","):
                run(emit, name, args.rounds, args.warm, parent)


if __name__ == "__main__":
    main()
