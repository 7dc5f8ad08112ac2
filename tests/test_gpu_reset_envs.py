"""`diral_env_reset_envs` / `VecV2VEnv.reset_envs`: a chosen subset of a handle's envs back to a fresh topology, one launch.

Two independent statements of what the call must do:

(a) the whole reset, env by env, bit for bit.  Handle E has stepped; handle R (same config, batch, env offset) is freshly
    ``reset_topology(seed=s)``.  Behind ``E.reset_envs(idx, seed=s)`` everything a call can read of the listed envs equals
    R's, everything of the other envs equals what E's never-reset twin P holds, the mask form leaves the same handle as
    the index form, and all of them then step like P with the listed rows copied in from R (`copy_envs_from`).
(b) the CPU oracle.  One `Oracle` object per env follows E; the listed ones are made again from the positions and speeds
    E exports right behind the call; six further slots and the final tables and metrics are compared with the suite's
    bars (IEEE-square mode: everything bit for bit, exp() rewards within the bar of tests/oracle_compare.py).

What keeps (a) from being vacuous is asserted: before the call every listed env differs from R's in positions, speeds,
tables and metric sums.  P's exports stand for "E before the call", so that E itself is called in the table form its last
step left (an export would complete the planes)."""
import numpy as np
import pytest
import torch

from diral_amd.config import (ERR_BAD_ARG, ERR_CAPTURE, ERR_ENV_INDEX, KERNEL_FAST64, KERNEL_GENERAL, KERNEL_LARGE,
                              KERNEL_SUBWAVE, KERNEL_WIDE, STEP_MY_STEP, STEP_MY_STEP_CH, bench_config)
from diral_amd.vec_env import DiralError
from tests.call_programs import FAMILIES
from tests.gpu_util import dev, draw_acts, env_of, everything, exported, make_env, oracle_slot, same, slot, topo
from tests.oracle_compare import ALL, metrics_equal, slot_equal, tables_equal

pytestmark = pytest.mark.gpu

OFFSET = 37          # env offset of every handle here: the device draws are indexed globally
SEED = 20241         # of the reset under test


def toy(**kw):
    """configs/4ue_3r_toy's shape on a highway where some pairs are out of range."""
    return bench_config(4, 3, 300.0, communication_range=120.0, State=dict(num_bins=20), **kw)


def case(cfg, B, mode=STEP_MY_STEP, form=None, path="auto", pre=7, kernel=None, rollout=False, prep=None, sticky=False):
    return dict(cfg=cfg, B=B, mode=mode, form=form, path=path, pre=pre, kernel=kernel, rollout=rollout, prep=prep, sticky=sticky)


def age_the_old_entries(envs, t):
    """Entries the ring no longer reaches (more than 7 stamps behind their subject) get ages at the 8-bit ceiling's edge,
    through export -> import on every handle alike; three more slots bring the handles back onto the ring."""
    st = exported(envs[0])
    own = np.diagonal(st["seq"], axis1=1, axis2=2)[:, None, :]
    old = (st["seq"] > 0) & (own - st["seq"] > 7)
    assert old.any(axis=(1, 2)).sum() >= 2, "the sparse highway left no env with entries beyond the ring"
    age = np.where(old, 253, st["age"]).astype(np.int32)
    for e in envs:
        e.import_state(st["pos_x"], st["pos_y"], st["vel"], seq=st["seq"], age=age, x=st["x"])
    return drive(envs, 3, 5, t)


def general_steps_leave_the_ring_stale(envs, t):
    """Planes current, ring stale: two slots on the general kernel, then back to AUTO without a step."""
    for e in envs:
        e.force_general_kernel()
    t = drive(envs, 2, 6, t)
    for e in envs:
        assert (e.last_kernel() & 15) == KERNEL_GENERAL
        e.force_general_kernel(False)
    return t


def import_leaves_the_ring_rebuilt(envs, t):
    st = exported(envs[0])
    for e in envs:
        e.import_state(st["pos_x"], st["pos_y"], st["vel"], seq=st["seq"], age=st["age"], x=st["x"])
    return t


CASES = {
    # ring + packed table (N <= 64)
    "n8": case(lambda: bench_config(8, 4, 300.0), 7, kernel=KERNEL_FAST64),
    "n33_rich": case(FAMILIES["f64_rich"]["cfg"], 9, kernel=KERNEL_FAST64, pre=9),
    "n64": case(FAMILIES["f64_full"]["cfg"], 7, kernel=KERNEL_FAST64, pre=10),
    # keyed quads (told != 0), entries handed over to the planes, ages near saturation
    "sparse_old": case(FAMILIES["f64_sparse"]["cfg"], 8, kernel=KERNEL_FAST64, pre=30, prep=age_the_old_entries),
    # pos_x is 72 bytes per env, metrics 48: the 4-byte units
    "n9": case(lambda: bench_config(9, 5, 300.0), 7, kernel=KERNEL_FAST64),
    # 64 < N <= 128 in both table forms
    "w2_plane": case(FAMILIES["w2_packed"]["cfg"], 7, form="plane", kernel=KERNEL_WIDE, pre=6),
    "w2_packed": case(FAMILIES["w2_packed"]["cfg"], 7, form="packed", kernel=KERNEL_WIDE, pre=6),
    # the general kernel: pinned, and the only one that takes A > 64
    "general": case(FAMILIES["f64_full"]["cfg"], 7, path="general", kernel=KERNEL_GENERAL, pre=6),
    "a70": case(lambda: bench_config(20, 70, 600.0), 7, kernel=KERNEL_GENERAL, pre=6),
    "large": case(lambda: bench_config(24, 6, 500.0), 7, path="large", kernel=KERNEL_LARGE, pre=6),
    # the toy config
    "toy_auto": case(toy, 13, kernel=KERNEL_FAST64),
    "toy_subwave": case(toy, 13, path="subwave", kernel=KERNEL_SUBWAVE),
    "toy_subwave_slots": case(toy, 13, path="subwave_slots", kernel=KERNEL_SUBWAVE, rollout=True),
    # buffers only some configs own
    "arrival": case(lambda: bench_config(33, 9, 1200.0, reward_design=3, track_arrival=True), 7, mode=STEP_MY_STEP_CH,
                    kernel=KERNEL_FAST64, pre=8),
    "pf": case(lambda: bench_config(20, 4, 340.0, reward_design=1, proportional_fair=True), 7, kernel=KERNEL_FAST64, pre=14,
               sticky=True),
    "piggy": case(lambda: bench_config(20, 5, 300.0, communication_range=301.0, State=dict(piggybacking=True, add_channel_obs=True)),
                  7, kernel=KERNEL_FAST64, pre=8),
    # both validity states other than "ring current, planes stale" (which every ring case above is in)
    "ring_stale": case(FAMILIES["f64_full"]["cfg"], 7, kernel=KERNEL_FAST64, pre=6, prep=general_steps_leave_the_ring_stale),
    "after_import": case(FAMILIES["f64_sparse"]["cfg"], 7, kernel=KERNEL_FAST64, pre=9, prep=import_leaves_the_ring_rebuilt),
}


def handle(c, cfg, topo_seed=1):
    env = make_env(cfg, c["B"], mode=c["mode"], dtype=torch.float64)
    env.set_env_offset(OFFSET)
    if c["path"] == "general":
        env.force_general_kernel()
    elif c["path"] == "large":
        env.force_large_path()
    elif c["path"].startswith("subwave"):
        env.use_subwave_path(slots=c["path"] == "subwave_slots")
    if topo_seed is not None:
        x0, v0 = topo(cfg, c["B"], topo_seed)
        env.reset_topology(x0, None, v0)
    return env


def actions_of(cfg, B, n, seed, sticky=False):
    rng = np.random.default_rng([seed, 77])
    a = [draw_acts(rng, B, cfg) for _ in range(n)]
    return [a[0]] * n if sticky else a


def drive(envs, n, seed, t, sticky=False):
    for k, a in enumerate(actions_of(envs[0].cfg, envs[0].B, n, seed, sticky)):
        for e in envs:
            e.step(dev(a), t + k)
    return t + n


def stepped(name, monkeypatch, n_handles):
    """`n_handles` bitwise twins behind the case's slots (and its preparation), their slot number, and a fresh R."""
    c = CASES[name]
    if c["form"]:
        monkeypatch.setenv("DIRAL_TABLE_FORM", c["form"])
    cfg = c["cfg"]()
    envs = [handle(c, cfg) for _ in range(n_handles)]
    t = drive(envs, c["pre"], 11, 0, c["sticky"])
    if c["prep"]:
        t = c["prep"](envs, t)
    R = handle(c, cfg, topo_seed=None)
    R.reset_topology(seed=SEED)
    return c, cfg, envs, t, R


def pick(B, seed=3):
    """About half of the envs, unsorted, the last env among them and env 0 left out."""
    rng = np.random.default_rng([seed, B])
    rest = rng.permutation(np.arange(1, B - 1))[:B // 2 - 1]
    return np.concatenate([[B - 1], rest]).astype(np.int32)


def mask_of(B, idx):
    m = np.zeros(B, bool)
    m[np.asarray(idx)] = True
    return m


def rows_equal(got, want, rows, what):
    for k in want:
        same(got[k][rows], want[k][rows], "%s: %s" % (what, k), equal_nan=True)


def follow(c, envs, t, n, seed):
    """`n` more slots of the same actions on every handle: every output of every handle equals the first one's."""
    cfg, B = envs[0].cfg, envs[0].B
    acts = actions_of(cfg, B, n, seed)
    if c["rollout"]:
        outs = []
        for e in envs:
            o = e.rollout(dev(np.stack(acts)), t, states="all")
            outs.append({k: v.cpu().numpy().copy() for k, v in o.items() if v is not None})
        for o in outs[1:]:
            for k in outs[0]:
                same(o[k], outs[0][k], "rollout %s" % k, equal_nan=True)
    else:
        for k, a in enumerate(acts):
            outs = [slot(e, a, t + k) for e in envs]
            for o in outs[1:]:
                for key in outs[0]:
                    same(o[key], outs[0][key], "slot %d %s" % (t + k, key), equal_nan=True)
    for e in envs:
        if c["kernel"] is not None:
            assert (e.last_kernel() & 15) == c["kernel"], (e.last_kernel(), c["kernel"])
    return t + n


# ---- 1. equals the whole reset, env by env ---------------------------------------------------------------------------
# export_first: the exports are compared right behind the call (which completes the planes: the steps that follow find both
# forms current).  step_first, where a table form can be stale at the call: the specialised path steps on the form the
# call found, and the exports are compared behind those steps only.
ORDERS = [(n, "export_first") for n in CASES] + [(n, "step_first") for n in ("n64", "sparse_old", "w2_packed", "ring_stale",
                                                                             "after_import", "toy_subwave_slots")]


@pytest.mark.parametrize("name,order", ORDERS)
def test_listed_envs_equal_the_whole_reset_and_the_others_stay(name, order, monkeypatch):
    peek = order == "export_first"
    c, cfg, (E, M, P), t, R = stepped(name, monkeypatch, 3)
    B = c["B"]
    idx = pick(B)
    rest = np.setdiff1d(np.arange(B), idx)
    before, want = everything(P, t), everything(R, t)
    for k in ("pos_x", "vel", "seq", "metrics"):                      # every listed env has something to lose
        for b in idx:
            assert not np.array_equal(before[k][b], want[k][b]), (k, b)
    E.reset_envs(dev(idx) if B % 2 else idx.tolist(), seed=SEED)      # (device tensors pass through; lists are uploaded)
    M.reset_envs(mask=dev(mask_of(B, idx)), seed=SEED)
    assert E.t == M.t == P.t == t                                     # the slot counter is the handle's
    if peek:
        for tag, h in (("index", E), ("mask", M)):
            got = everything(h, t)
            rows_equal(got, want, idx, "%s form, listed envs" % tag)
            rows_equal(got, before, rest, "%s form, other envs" % tag)
    P.copy_envs_from(R, idx.tolist(), idx.tolist())                   # the workaround this call replaces
    t = follow(c, [P, E, M], t, 4, 21)
    ref = everything(P, t)
    for tag, h in (("index", E), ("mask", M)):
        rows_equal(everything(h, t), ref, np.arange(B), "%s form, 4 slots on" % tag)
    assert ref["metrics"][idx, 0].max() == 4 and ref["metrics"][rest, 0].min() == t
    for h in (E, M, P):
        h.check()


# ---- 2. against the CPU oracle ---------------------------------------------------------------------------------------
def oracles_behind(c, cfg, B, t_prep):
    """One oracle per env behind the case's slots; None where the preparation went through an import."""
    from oracle.oracle import SQ_IEEE, Oracle
    x0, v0 = topo(cfg, B, 1)
    out = []
    for b in range(B):
        o = Oracle(cfg, batch=1, sq_mode=SQ_IEEE)
        o.reset(x0[b:b + 1], np.zeros((1, cfg.num_users)), v0[b:b + 1])
        out.append(o)
    for k, a in enumerate(actions_of(cfg, B, c["pre"], 11, c["sticky"])):
        for b, o in enumerate(out):
            o.step(c["mode"], a[b:b + 1], k)
    return out


def oracle_from(cfg, st, b):
    """An oracle holding env b of the exported state `st`."""
    from oracle.oracle import SQ_IEEE, Oracle
    o = Oracle(cfg, batch=1, sq_mode=SQ_IEEE)
    o.reset(st["pos_x"][b:b + 1], st["pos_y"][b:b + 1], st["vel"][b:b + 1])
    return o


def compare_slots(c, cfg, env, orcs, t, n, seed):
    for k, a in enumerate(actions_of(cfg, env.B, n, seed)):
        got = slot(env, a, t + k)
        for b, o in enumerate(orcs):
            want = [x[0] for x in oracle_slot(o, c["mode"], a[b:b + 1], t + k)]
            slot_equal(cfg, c["mode"], (got["state"][b], got["reward"][b], got["chobs"][b]), want, "slot %d env %d" % (t + k, b))
    return t + n


def compare_tables(cfg, env, orcs, t, metrics_rows):
    st = everything(env, t)
    for b, o in enumerate(orcs):
        e = env_of(o.export(), 0)
        same(st["pos_y"][b], e["pos_y"], ("pos_y", b))
        tables_equal({k: st[k][b] for k in ALL if k in st}, e, b)
        if cfg.track_arrival:
            assert np.array_equal(st["info_age"][b], o.info_age(t)[0]), b
        if cfg.State.piggybacking:
            assert np.array_equal(st["prev_obs"][b], o.prev_obs()[0]), b
        if b in metrics_rows:
            metrics_equal(st["metrics"][b:b + 1], o.metrics(), b, prr=cfg.track_prr or env.step_mode == STEP_MY_STEP_CH)


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n]["prep"] is None and not CASES[n]["rollout"]] + ["sparse_old"])
def test_reset_envs_against_the_oracle(name, monkeypatch):
    c, cfg, (E,), t, _ = stepped(name, monkeypatch, 1)
    B = c["B"]
    idx = pick(B, seed=4)
    if c["prep"] is None:
        orcs = oracles_behind(c, cfg, B, t)
    else:                                                             # (aged through an import: the oracles start from E's tables)
        pre = exported(E)
        orcs = []
        for b in range(B):
            o = oracle_from(cfg, pre, b)
            o.import_state(seq=pre["seq"][b:b + 1], age=pre["age"][b:b + 1], x=pre["x"][b:b + 1], y=pre["y"][b:b + 1])
            orcs.append(o)
        t = drive([E], 2, 8, t)                                       # back onto the ring before the call
        for k, a in enumerate(actions_of(cfg, B, 2, 8)):
            for b, o in enumerate(orcs):
                o.step(c["mode"], a[b:b + 1], t - 2 + k)
    if B % 2:
        E.reset_envs(mask=dev(mask_of(B, idx)), seed=SEED)
    else:
        E.reset_envs(idx, seed=SEED)
    st = exported(E)
    L = cfg.highway_length
    assert (st["pos_x"][idx] == np.floor(st["pos_x"][idx])).all() and (st["pos_x"][idx] >= 0).all() and (st["pos_x"][idx] < L).all()
    assert not st["pos_y"][idx].any() and not st["seq"][idx].any() and not st["age"][idx].any() and not st["x"][idx].any()
    for b in idx:                                                     # the listed envs start again, on the oracle's side too
        orcs[b] = oracle_from(cfg, st, b)
    t = compare_slots(c, cfg, E, orcs, t, 6, 31)
    fresh_metrics = set(int(b) for b in idx) | (set(range(B)) if c["prep"] is None else set())
    compare_tables(cfg, E, orcs, t, fresh_metrics)
    E.check()


# ---- 5. explicit rows ------------------------------------------------------------------------------------------------
def test_given_rows_are_read_for_the_listed_envs_only():
    c = CASES["n9"]
    cfg = c["cfg"]()
    E, P = handle(c, cfg), handle(c, cfg)
    t = drive([E, P], 5, 11, 0)
    B, N = c["B"], cfg.num_users
    idx = pick(B)
    rest = np.setdiff1d(np.arange(B), idx)
    rng = np.random.default_rng(12)
    x0 = rng.uniform(0.0, cfg.highway_length, size=(B, N))
    v0 = rng.uniform(1.1, 2.7, size=(B, N))
    x0[rest], v0[rest] = np.nan, np.nan                               # rows of envs that are not listed are never read
    before = everything(P, t)
    E.reset_envs(idx, x0=x0, v0=v0, seed=SEED)
    got = everything(E, t)
    same(got["pos_x"][idx], x0[idx], "pos_x")
    same(got["vel"][idx], v0[idx], "vel")
    assert not got["pos_y"][idx].any() and not got["seq"][idx].any() and not got["metrics"][idx].any()
    rows_equal(got, before, rest, "other envs")
    # x0 alone: the speeds are the draws of the whole reset
    R = handle(c, cfg, topo_seed=None)
    R.reset_topology(seed=SEED)
    E.reset_envs(idx, x0=x0, seed=SEED)
    got = everything(E, t)
    same(got["pos_x"][idx], x0[idx], "pos_x")
    same(got["vel"][idx], everything(R, t)["vel"][idx], "drawn vel")
    assert np.isfinite(got["pos_x"]).all() and np.isfinite(got["vel"]).all()
    E.check()


def test_lanes_given_for_a_listed_env_take_the_handle_off_the_flat_path():
    c = CASES["n64"]
    cfg = c["cfg"]()
    E = handle(c, cfg)
    B, N = c["B"], cfg.num_users
    t = drive([E], 6, 11, 0)
    orcs = oracles_behind(dict(c, pre=6), cfg, B, t)
    idx = np.array([5, 2], np.int32)
    rng = np.random.default_rng(13)
    y0 = np.full((B, N), np.nan)
    y0[idx] = rng.choice(np.array([0.0, 1.0, 2.0]), size=(2, N))
    y0[5, 0], y0[2, 1] = 1.0, 2.0
    E.rollout(dev(np.stack(actions_of(cfg, B, 2, 14))), t)            # (the flat lane: K-slot launches are taken)
    for k, a in enumerate(actions_of(cfg, B, 2, 14)):
        for b, o in enumerate(orcs):
            o.step(c["mode"], a[b:b + 1], t + k)
    t += 2
    E.reset_envs(idx, y0=y0, seed=SEED)
    with pytest.raises(DiralError):                                   # ... and refused once a vehicle is off the lane
        E.rollout(dev(np.stack(actions_of(cfg, B, 2, 15))), t)
    st = exported(E)
    same(st["pos_y"][idx], y0[idx], "pos_y")
    assert not st["pos_y"][np.setdiff1d(np.arange(B), idx)].any()
    for b in idx:
        orcs[b] = oracle_from(cfg, st, b)
    t = compare_slots(c, cfg, E, orcs, t, 6, 32)
    assert (E.last_kernel() & 15) == KERNEL_FAST64
    compare_tables(cfg, E, orcs, t, set(range(B)))
    # back on the lane for every env: the flag is recomputed, K-slot launches are taken again
    E.reset_envs(idx, y0=np.zeros((B, N)), seed=SEED)
    E.rollout(dev(np.stack(actions_of(cfg, B, 2, 16))), t)
    E.check()


def status_of(call):
    with pytest.raises(DiralError) as ei:
        call()
    return ei.value.status


def test_lanes_inside_a_capture_are_refused_with_the_env_untouched():
    c = CASES["n64"]
    cfg = c["cfg"]()
    E, P = handle(c, cfg), handle(c, cfg)
    t = drive([E, P], 6, 11, 0)
    idx = dev(pick(c["B"]))
    y0 = E._f64(0.0, (c["B"], cfg.num_users))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            keep = idx + 0                                            # (the captured graph is not empty)
            assert status_of(lambda: E.reset_envs(idx, y0=y0, seed=SEED)) == ERR_CAPTURE
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    del keep
    t = follow(c, [P, E], t, 3, 22)                                   # nothing was reset, launched or recorded
    rows_equal(everything(E, t), everything(P, t), np.arange(c["B"]), "after the refused call")
    E.check()


# ---- 6. edges ----------------------------------------------------------------------------------------------------------
def test_an_all_zero_mask_is_a_no_op_and_a_full_count_is_the_whole_reset():
    c = CASES["n33_rich"]
    cfg = c["cfg"]()
    E, P = handle(c, cfg), handle(c, cfg)
    B = c["B"]
    t = drive([E, P], 6, 11, 0)
    E.reset_envs(mask=torch.zeros(B, dtype=torch.uint8, device="cuda:0"), seed=SEED)
    E.reset_envs(mask=torch.zeros(B, dtype=torch.bool, device="cuda:0"), x0=np.full((B, cfg.num_users), np.nan), seed=SEED)
    rows_equal(everything(E, t), everything(P, t), np.arange(B), "all-zero mask")
    # envs 0 ... count - 1
    R = handle(c, cfg, topo_seed=None)
    R.reset_topology(seed=SEED)
    want, before = everything(R, t), everything(P, t)
    E.reset_envs(count=3, seed=SEED)
    got = everything(E, t)
    rows_equal(got, want, np.arange(3), "count = 3")
    rows_equal(got, before, np.arange(3, B), "count = 3, other envs")
    E.reset_envs(seed=SEED)                                           # count = B, every pointer NULL
    rows_equal(everything(E, t), want, np.arange(B), "count = B")
    assert status_of(lambda: E.reset_envs(count=B + 1, seed=SEED)) == ERR_BAD_ARG      # a NULL index with count > B
    assert status_of(lambda: E.reset_envs(count=0, seed=SEED)) == ERR_BAD_ARG
    with pytest.raises(ValueError):
        E.reset_envs([1], mask=torch.ones(B, dtype=torch.bool, device="cuda:0"))
    # ... and the handle goes on like the freshly reset one
    t2 = follow(c, [R, E], 0, 3, 23)
    rows_equal(everything(E, t2), everything(R, t2), np.arange(B), "3 slots on")
    E.check()


def test_duplicates_and_indices_outside_the_handle():
    c = CASES["n8"]
    cfg = c["cfg"]()
    E, P = handle(c, cfg), handle(c, cfg)
    B = c["B"]
    t = drive([E, P], 6, 11, 0)
    R = handle(c, cfg, topo_seed=None)
    R.reset_topology(seed=SEED)
    want, before = everything(R, t), everything(P, t)
    E.reset_envs([4, 1, 4, 4, 1], seed=SEED)                          # duplicates: every writer stores the same values
    got = everything(E, t)
    rows_equal(got, want, [1, 4], "duplicates")
    rows_equal(got, before, [0, 2, 3, 5, 6], "duplicates, other envs")
    E.check()
    for bad in (-1, B):
        E.reset_envs([2, bad, 5], seed=SEED)
        assert status_of(E.check) == ERR_ENV_INDEX
        E.check()                                                     # reported once
    got = everything(E, t)
    rows_equal(got, want, [1, 2, 4, 5], "an index outside skips that env only")
    rows_equal(got, before, [0, 3, 6], "an index outside, other envs")
    P.copy_envs_from(R, [1, 2, 4, 5], [1, 2, 4, 5])
    follow(c, [P, E], t, 3, 24)
    E.check()


def test_more_listed_envs_than_one_grid_dimension_holds():
    """66 000 indices into 70 000 toy envs: the launch's y dimension (65 535 at most) is strided."""
    cfg = toy()
    B, n = 70000, 66000
    c = case(toy, B, kernel=KERNEL_FAST64)
    E = handle(c, cfg, topo_seed=None)                                # (one handle: what the whole reset leaves, read first)

    def read():
        out = E.export_state()
        out["metrics"] = E.metrics()
        return out
    E.reset_topology(seed=SEED)
    want = read()
    x0, v0 = topo(cfg, B, 1)
    E.reset_topology(x0, None, v0)
    a = dev(draw_acts(np.random.default_rng(5), B, cfg))
    for k in range(3):
        E.step(a, k)
    before = read()
    idx = np.random.default_rng(6).permutation(B)[:n].astype(np.int32)
    listed = torch.zeros(B, dtype=torch.bool, device="cuda:0")
    listed[dev(idx).long()] = True
    E.reset_envs(dev(idx), seed=SEED)
    got = read()
    for k in got:
        assert torch.equal(got[k][listed], want[k][listed]), k
        assert torch.equal(got[k][~listed], before[k][~listed]), k
    assert int(got["metrics"][listed][:, 0].max()) == 0 and int(got["metrics"][~listed][:, 0].min()) == 3
    assert int((~listed).sum()) == B - n
    E.check()


# ---- 7. captured: a device mask decides, replay by replay -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["n64", "toy_subwave"])
def test_a_captured_reset_and_step_follow_the_mask_of_each_replay(name, monkeypatch):
    from diral_amd.rollout import no_finalizers_during_capture
    c, cfg, (E, P), t, _ = stepped(name, monkeypatch, 2)
    B = c["B"]
    masks = [mask_of(B, pick(B, seed=s)) for s in (7, 8, 9)]
    assert not np.array_equal(masks[1], masks[2])
    m = dev(masks[0].astype(np.uint8))
    a = dev(draw_acts(np.random.default_rng(9), B, cfg))
    t_step = t + 1                                                    # (baked into the graph)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                        # warm-up, on both handles alike
        E.reset_envs(mask=m, seed=SEED)
        E.step(a, t_step)
    P.reset_envs(mask=m, seed=SEED)
    P.step(a, t_step)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with no_finalizers_during_capture():
        with torch.cuda.graph(g, stream=s):
            E.reset_envs(mask=m, seed=SEED)
            obs, rew, done = E.step(a, t_step)
    for r in (1, 2):
        m.copy_(dev(masks[r].astype(np.uint8)))
        g.replay()
        torch.cuda.synchronize()
        P.reset_envs(mask=dev(masks[r]), seed=SEED)
        w_obs, w_rew, w_done = P.step(a, t_step)
        same(obs.cpu().numpy(), w_obs.cpu().numpy(), "replay %d: state" % r)
        same(rew.cpu().numpy(), w_rew.cpu().numpy(), "replay %d: reward" % r)
        same(done.cpu().numpy(), w_done.cpu().numpy(), "replay %d: done" % r)
    # (only now: an export completes the planes and says so in the host flags, which a replay would not take back)
    x, y = everything(E, t_step + 1), everything(P, t_step + 1)
    rows_equal(x, y, np.arange(B), "after the replays")
    slots = x["metrics"][:, 0]
    assert (slots[masks[2]] == 1).all() and (slots[~masks[2] & masks[1]] == 2).all()
    E.check()
