"""Helpers the GPU test modules share: making a handle and stepping it against the oracle (`against_oracle`,
`three_handles`, `random_rollout`; the rules themselves are tests/oracle_compare.py's) and the reference fixtures, the
twin-handle helpers of the copy tests and the oracle-side helpers of the sequence-number horizon tests.  Test modules
import from here, never from each other."""
import contextlib

import numpy as np
import pytest
import torch

from diral_amd.config import (ERR_SEQ_OVERFLOW, KERNEL_FAST64, KERNEL_GENERAL, KERNEL_LARGE, KERNEL_OBSERVE, KERNEL_WIDE,
                              STEP_DESIGN, STEP_MY_STEP, STEP_MY_STEP_CH, bench_config)
from diral_amd.vec_env import DiralError
from tests import call_programs as P
from tests.golden_util import Golden, out_sha, ulp_diff
from tests.oracle_compare import exp_close, metrics_equal, same, slot_equal, tables_equal, uses_exp  # noqa: F401  (`same`: re-exported)

DIST_ULP = 1       # sqrt(x*x+y*y) vs sqrt(pow(x,2)+pow(y,2))


# ---- a handle against the oracle and the reference fixtures ---------------------------------------------------------------
def make_env(cfg, B, mode=STEP_MY_STEP, dtype=torch.float64):
    from diral_amd.vec_env import VecV2VEnv
    return VecV2VEnv(cfg, batch=B, device="cuda:0", out_dtype=dtype, step_mode=mode)


def gpu_step(env, mode, acts, t, ep=0.0, eps=1.0):
    a = env._actions(np.asarray(acts))
    obs, rew, done = env._step(mode, a, t, ep, eps, want_chobs=True)
    torch.cuda.synchronize()
    return obs.cpu().numpy().copy(), rew.cpu().numpy().copy(), env._chobs.cpu().numpy().copy(), \
        done.cpu().numpy().copy()


def host(t):
    return t.cpu().numpy().copy()


def exported(env):
    return {k: v.cpu().numpy() for k, v in env.export_state().items()}


def env_of(d, b):
    """Env `b` of a dict of batched arrays."""
    return {k: v[b] for k, v in d.items()}


def default_family(N):
    """What `plan_step` (csrc/diral_env.hip) serves a one-lane highway with at most 64 resources on."""
    return KERNEL_FAST64 if N <= 64 else KERNEL_WIDE


@contextlib.contextmanager
def general_kernel(env):
    """This env's steps run on the general step_kernel (DIRAL_OPT_KERNEL_PATH, include/diral_env.h)."""
    env.force_general_kernel(True)
    try:
        yield
    finally:
        env.force_general_kernel(False)


def xpos_of(seq, B, N):
    """Imported tables: an entry is the subject's stamp at that sequence number, so entries about one subject with
    equal seq carry equal xpos in every reachable state (DIRAL_ERR_TABLE_CONFLICT otherwise).  `seq` is [B, N, N] with
    the subject last."""
    kk, bb = np.arange(N)[None, None, :], np.arange(B)[:, None, None]
    return ((kk * 7919 + seq * 104729 + bb * 31) % 200000) / 100.0


def oracle_slot(orc, mode, acts, t, state=True):
    """The oracle's slot `t` as `slot_equal` wants it: (state, reward, chobs)."""
    rew, chobs = orc.step(mode, acts, t)
    return orc.obtain_state(acts, chobs, rew) if state else None, rew, chobs


def draw_velocities(rng, B, N, *handles):
    draws = rng.integers(1, 4, size=(B, N)).astype(np.uint8)
    for h in handles:
        h.update_velocity(draws)


def against_oracle(env, orc, cfg, mode, T, rng, *, compare_at=None, actions=None, vel_every=None, dtype=np.float64,
                   want_chobs=True, each_slot=None):
    """One handle and the oracle through the slots `T` (a count, or the slot numbers themselves): draw actions (or take
    `actions(t)`), step both, `slot_equal` at the slots `compare_at(t)` names (default: all), then `each_slot(t, acts)`,
    then `update_velocity` on both every `vel_every`.  `want_chobs`: the channel observation is asked for and compared
    (a RICH instantiation); without it the plain `step` runs.  Returns the last compared slot's (state, reward, chobs)."""
    B, N, A = env.B, cfg.num_users, cfg.num_channels
    out = None
    for t in (range(T) if isinstance(T, int) else T):
        acts = rng.integers(0, A, size=(B, N)).astype(np.int32) if actions is None else actions(t)
        obs, rew, _ = env._step(mode, env._actions(acts), t, want_chobs=want_chobs)
        compare = compare_at is None or compare_at(t)
        want = oracle_slot(orc, mode, acts, t, state=compare)
        if compare:
            out = host(obs), host(rew), host(env._chobs) if want_chobs else None
            slot_equal(cfg, mode, out, want, t, dtype)
        if each_slot is not None:
            each_slot(t, acts)
        if vel_every and t % vel_every == vel_every - 1:
            draw_velocities(rng, B, N, env, orc)
    return out


def three_handles(cfg, B, T, *, mode, seed, family, y0=None, actions=None, each_slot=None, f32=True):
    """A float32 handle (with `f32`), a float64 handle, a float64 handle forced to the general kernel and the oracle on
    one random topology (`y0(rng)`: lanes, drawn between positions and speeds) and `T` slots of random actions (or
    `actions(rng, t, previous)`).  Every slot: the float64 handle equals the general one bit for bit and passes
    `slot_equal` against the oracle, the float32 handle equals the cast, the specialised handles ran on `family` and the
    forced one on KERNEL_GENERAL; then `each_slot(t, handles, orc)`.  At the end every exported plane is equal between
    the handles and to the oracle's, the metrics agree and `check()` passes.  Returns ((f32 or None, f64, gen), orc)."""
    from oracle.oracle import Oracle, SQ_IEEE
    N, A, L = cfg.num_users, cfg.num_channels, cfg.highway_length
    name = {STEP_MY_STEP: "my_step", STEP_MY_STEP_CH: "my_step_ch", STEP_DESIGN: "my_step_design"}[mode]
    rng = np.random.default_rng(seed)
    x0 = rng.integers(0, int(L), size=(B, N)).astype(np.float64)
    lanes = None if y0 is None else y0(rng)
    v0 = rng.uniform(1.1, 2.7, size=(B, N))
    e32 = make_env(cfg, B, mode=name, dtype=torch.float32) if f32 else None
    e64, gen = make_env(cfg, B, mode=name, dtype=torch.float64), make_env(cfg, B, mode=name, dtype=torch.float64)
    special = [e for e in (e32, e64) if e is not None]
    orc = Oracle(cfg, batch=B, sq_mode=SQ_IEEE, threads=8)
    for e in special + [gen]:
        e.reset_topology(x0, lanes, v0)
    orc.reset(x0, np.zeros((B, N)) if lanes is None else lanes, v0)
    a = None
    for t in range(T):
        a = rng.integers(0, A, size=(B, N)).astype(np.int32) if actions is None else actions(rng, t, a)
        got = [[host(x) for x in e.step(a, t)] for e in special]
        with general_kernel(gen):
            want = [host(x) for x in gen.step(a, t)]
        oracle = oracle_slot(orc, mode, a, t)
        for e, (obs, rew, done), dt in zip(special, got, (np.float32, np.float64)[2 - len(special):]):
            ran_on(e, family)
            slot_equal(cfg, mode, (obs, rew, None), oracle, (t, dt.__name__), dt)
            same(done, want[2], (t, "done"))
        for g, w, what in zip(got[-1], want, ("state", "reward")):
            same(g, w, (t, what, "against the general kernel"))
        ran_on(gen, KERNEL_GENERAL)
        if each_slot is not None:
            each_slot(t, (e32, e64, gen), orc)
    sg, mg = exported(gen), host(gen.metrics())
    for e in special:
        st = exported(e)
        assert set(st) == set(sg)
        for k in sg:
            same(st[k], sg[k], (k, "against the general kernel"))
        metrics_equal(host(e.metrics()), mg, "against the general kernel", prr=mode == STEP_MY_STEP_CH or cfg.track_prr)
    tables_equal(exported(e64), orc.export(), "end")
    for e in special + [gen]:
        e.check()
    return (e32, e64, gen), orc


def assert_slot_matches_reference(g, i, mode, rew, chobs, obs):
    """One env's outputs of slot i against what the reference recorded (tests/golden/*.npz): rewards exact (exp()
    designs within the exp() bar), distances within DIST_ULP, the type-2 histogram bins exact.  A thinned fixture
    (gen_golden.py `record_every`) holds the arrays at some slots and a hash at every slot: the hash is compared
    wherever this bar is "exact", so a slot without arrays still pins its rewards."""
    cfg, name = g.cfg, g.name
    ref_rew, ref_chobs, ref_state = g.out("rews", i), g.out("chobs", i), g.out("state", i)
    if not uses_exp(cfg, mode) and g.kept is not None:
        assert out_sha(rew) == g.out_sha("rews", i), (name, i)
    if ref_rew is None:
        return
    assert exp_close(rew, ref_rew) if uses_exp(cfg, mode) else np.array_equal(rew, ref_rew), (name, i)
    assert ulp_diff(chobs, ref_chobs) <= DIST_ULP, (name, i)
    assert ulp_diff(obs, ref_state) <= DIST_ULP or (cfg.State.add_reward and exp_close(obs, ref_state)), (name, i)
    if cfg.State.add_positional_dist_piggy:
        K = cfg.State.num_bins
        off = (cfg.num_channels if cfg.State.action_index == "binary" else 1) if cfg.State.add_action else 0
        off += cfg.chobs_width if cfg.State.add_channel_obs else 0
        off += cfg.num_users - 1 if cfg.State.add_positional_dist else 0
        if cfg.State.add_positional_dist_type == 2:
            assert np.array_equal(obs[:, off:off + K], ref_state[:, off:off + K]), "histogram bins"


def assert_moves_match_reference(g, i, pos_x, vel, ia):
    """Positions, speeds and the information-age histogram after slot i: exact (by hash where a thinned fixture
    dropped the arrays)."""
    for key, got in (("pos_x", pos_x), ("vel", vel), ("ia", ia)):
        ref = g.out(key, i)
        if ref is None:
            assert out_sha(got) == g.out_sha(key, i), (g.name, key, i)
        else:
            assert np.array_equal(got, ref), (g.name, key, i)


def golden_replay_on_gpu(name):
    """Every reference fixture replayed through libdiral_env.so (B=3 replicas)."""
    from oracle.oracle import Oracle, SQ_IEEE
    g = Golden(name)
    B = 3
    env = make_env(g.cfg, B)
    env.reset_topology(g["x0"], g["y0"], g["v0"])
    orc = Oracle(g.cfg, batch=1, sq_mode=SQ_IEEE)
    orc.reset(g["x0"], g["y0"], g["v0"])
    ck = g.table_checkpoints()
    S = env.S
    cfg = g.cfg
    for i, mode, acts, t, (ep, eps) in g.steps():
        obs, rew, chobs, done = gpu_step(env, mode, acts, t, ep, eps)
        o_rew, o_chobs = orc.step(mode, acts, t)
        o_state = orc.obtain_state(acts, o_chobs, o_rew, ep, eps)
        for b in range(B):
            slot_equal(cfg, mode, (obs[b], rew[b], chobs[b]), (o_state[0], o_rew[0], o_chobs[0]), (name, i))
            assert_slot_matches_reference(g, i, mode, rew[b], chobs[b], obs[b])
            assert done[b] == ((t % cfg.episode_interval) == cfg.episode_interval - 1)
        if i in g.vel_updates:
            env.update_velocity(g.vel_updates[i])
            orc.update_velocity(g.vel_updates[i])
        if g.trace is not None and i == g.trace_after:
            env.load_saved_positions(g.trace)
            orc.set_trace(g.trace)
        ia = env.info_age(t).cpu().numpy()
        st, oe = exported(env), env_of(orc.export(), 0)
        for b in range(B):
            assert_moves_match_reference(g, i, st["pos_x"][b], st["vel"][b], ia[b])
            tables_equal(env_of(st, b), oe, (name, i))
            if i in ck:
                j = ck[i]
                assert np.array_equal(st["seq"][b], g["tab_seq"][j])
                assert np.array_equal(st["age"][b], np.minimum(g["tab_age"][j], 255))
                assert np.array_equal(st["x"][b], g["tab_x"][j])
                assert np.array_equal(st["y"][b], g["tab_y"][j])
                assert np.array_equal(st["la"][b], g["tab_la"][j])
    env.check()
    if cfg.State.piggybacking:
        # TestEnv.prev_obs after the last slot (test_env.py:260-261): distances, within 1 ulp of the reference's pow()
        po = env.prev_obs().cpu().numpy()
        for b in range(B):
            assert np.array_equal(po[b], orc.prev_obs()[0]) and ulp_diff(po[b], g["prev_obs"]) <= DIST_ULP
        if "keyerror_actions" in g.d.files:
            # the slot the reference left with KeyError (`self.prev_obs[None]`, test_env.py:243): the sticky device flag
            from diral_amd.config import ERR_PIGGY_NO_TX
            from diral_amd.vec_env import DiralError
            gpu_step(env, STEP_MY_STEP, g["keyerror_actions"], int(g["keyerror_t"]))
            with pytest.raises(DiralError) as ei:
                env.check()
            assert ei.value.status == ERR_PIGGY_NO_TX
            env.check()                                             # reported once, then cleared


def random_rollout(cfg, B, T, seed, mode=STEP_MY_STEP, sticky=0.0, vel_every=None, threads=8, track_prr=False,
                   expect_kernel=None, force_general=False, path=None, y0=None):
    """GPU vs oracle (IEEE squares) on B different random envs, T slots; returns
    the number of compared slots.  Everything must match bit for bit (exp()
    rewards within the exp() bar).  The specialised kernels serve every configuration they can
    (`expect_kernel`: assert which family ran); `force_general` pins the run to the general
    kernel (DIRAL_OPT_KERNEL_PATH), `path="large"` to the three launches of csrc/step_large.hpp (the only path beyond
    256 vehicles / 256 resources / 64 bins); track_prr: PRR metrics also in my_step (a build extension); `y0`: a
    function (rng, B, N) -> lanes (default: the one-lane highway the reference draws)."""
    from oracle.oracle import Oracle, SQ_IEEE
    rng = np.random.default_rng(seed)
    N, A, L = cfg.num_users, cfg.num_channels, cfg.highway_length
    cfg = cfg.replace(track_arrival=True, track_prr=track_prr)
    x0 = rng.integers(0, int(L), size=(B, N)).astype(np.float64)
    y0 = np.zeros((B, N)) if y0 is None else y0(rng, B, N)
    v0 = np.full((B, N), 1.7) if cfg.mobility_vary else rng.uniform(1.1, 2.7, size=(B, N))
    env = make_env(cfg, B)
    env.force_general_kernel(force_general)
    if path == "large":
        env.force_large_path()
    env.reset_topology(x0, y0, v0)
    orc = Oracle(cfg, batch=B, sq_mode=SQ_IEEE, threads=threads)
    orc.reset(x0, y0, v0)
    observe = KERNEL_LARGE if (path == "large" or expect_kernel == KERNEL_LARGE) else (KERNEL_GENERAL if force_general else KERNEL_OBSERVE)
    held = [rng.integers(0, A, size=(B, N))]

    def actions(t):
        new = rng.integers(0, A, size=(B, N))
        held[0] = np.where(rng.random((B, N)) < sticky, held[0], new).astype(np.int32)
        return held[0]

    def each_slot(t, acts):
        if expect_kernel is not None:
            ran_on(env, expect_kernel)
        if t % 6 == 4 and env.S > 0:
            # a stand-alone obtain_state with FOREIGN arguments (test_env.py:527-583 on the current tables):
            # diral_env_observe -> observe_kernel.hpp (the general kernel's observe mode when forced)
            fa = rng.integers(0, A, size=(B, N)).astype(np.int32)
            fc = rng.uniform(0.0, 300.0, size=(B, N, cfg.chobs_width))
            fr = rng.uniform(-3.0, 1.0, size=(B, N))
            s1 = env.obtain_state(fc, fa, fr, 3.0, 0.25).cpu().numpy()
            ran_on(env, observe)
            same(s1, orc.obtain_state(fa, fc, fr, 3.0, 0.25), (t, "foreign arguments"))

    against_oracle(env, orc, cfg, mode, T, rng, actions=actions, each_slot=each_slot, vel_every=vel_every)
    oe = orc.export()
    tables_equal(exported(env), oe, "end")
    same(host(env.info_age(T - 1)), orc.info_age(T - 1), "information age")
    if cfg.proportional_fair and mode == STEP_MY_STEP and sticky >= 0.9 and T >= 40:
        assert oe["pf"].max() > 10                    # the threshold was crossed: the penalty branch ran
    metrics_equal(host(env.metrics()), orc.metrics(), "end", prr=track_prr or mode == STEP_MY_STEP_CH)
    env.check()
    return T


# ---- twin handles (tests/test_gpu_copy_envs.py, tests/test_gpu_search.py) --------------------------------------------------
def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def topo(cfg, B, seed):
    rng = np.random.default_rng([seed, B, cfg.num_users])
    return P._positions(rng, B, cfg.num_users, cfg.highway_length), P._speeds(rng, B, cfg.num_users, cfg.mobility_vary)


def draw_acts(rng, B, cfg):
    return rng.integers(0, cfg.num_channels, size=(B, cfg.num_users)).astype(np.int32)


def new_env(f, cfg, B, seed, y0=None, f64=None):
    f64 = f["f64"] if f64 is None else f64
    env = make_env(cfg, B, mode=f["mode"], dtype=torch.float64 if f64 else torch.float32)
    x0, v0 = topo(cfg, B, seed)
    env.reset_topology(x0, y0, v0)
    return env


def run(envs, n, seed, t0=0, sticky=False):
    """`n` slots of the same random actions on every handle of `envs` (equal batches)."""
    cfg, B = envs[0].cfg, envs[0].B
    rng = np.random.default_rng([seed, 77])
    a = dev(draw_acts(rng, B, cfg))
    for k in range(n):
        if not sticky and k:
            a = dev(draw_acts(rng, B, cfg))
        for e in envs:
            e.step(a, t0 + k)
    return t0 + n


def slot(env, a, t):
    obs, rew, done = env._step(env.step_mode, dev(a), t, want_chobs=True)
    return dict(state=obs.cpu().numpy().copy(), reward=rew.cpu().numpy().copy(), done=done.cpu().numpy().copy(),
                chobs=env._chobs.cpu().numpy().copy())


def everything(env, t):
    out = {k: v.cpu().numpy() for k, v in env.export_state().items()}
    out["metrics"] = env.metrics().cpu().numpy()
    if env.cfg.track_arrival:
        out["info_age"] = env.info_age(t).cpu().numpy()
    if env.cfg.State.piggybacking:
        out["prev_obs"] = env.prev_obs().cpu().numpy()
    return out


# ---- which family ran --------------------------------------------------------------------------------------------------------
FAMILY = {KERNEL_FAST64: "FAST64", KERNEL_WIDE: "WIDE", KERNEL_GENERAL: "GENERAL", KERNEL_LARGE: "LARGE", KERNEL_OBSERVE: "OBSERVE"}


def ran_on(env, family):
    assert (env.last_kernel() & 15) == family, (FAMILY.get(env.last_kernel() & 15), FAMILY.get(family, family), env.last_kernel())


# ---- handles and oracles on given tables (tests/test_gpu_seq_horizon.py, tests/test_gpu_subwave.py) ------------------------
def make_oracle(cfg, tab, threads=8):
    from oracle.oracle import Oracle, SQ_IEEE
    B, N = tab["pos_x"].shape
    orc = Oracle(cfg, batch=B, sq_mode=SQ_IEEE, threads=threads)
    orc.reset(tab["pos_x"], np.zeros((B, N)), tab["vel"])
    orc.import_state(seq=tab["seq"], age=tab["age"], x=tab["x"], y=np.zeros((B, N, N)))
    return orc


def load(env, tab):
    env.reset_topology(tab["pos_x"], 0.0, tab["vel"])
    env.import_state(tab["pos_x"], np.zeros(tab["pos_x"].shape), tab["vel"], seq=tab["seq"], age=tab["age"], x=tab["x"])


def _expect_overflow(env):
    with pytest.raises(DiralError) as ei:
        env.check()
    assert ei.value.status == ERR_SEQ_OVERFLOW, ei.value
    env.check()                                                                  # reported once, then cleared


# ---- the random configurations of tests/test_gpu_fuzz.py --------------------------------------------------------------------
def draw_case(i):
    rng = np.random.default_rng(9000 + i)
    N = int(rng.choice([2, 3, 5, 17, 31, 64, 65, 90, 128, 150, 256]))
    A = int(rng.choice([1, 2, 3, 7, 16, 32, 40, 64]))
    K = int(rng.choice([1, 3, 10, 20, 21, 40, 64]))
    mode = int(rng.choice([STEP_MY_STEP, STEP_MY_STEP, STEP_MY_STEP_CH, STEP_DESIGN]))
    rd = int(rng.choice([2, 3, 4])) if mode == STEP_MY_STEP_CH else int(rng.integers(1, 6))
    L = float(rng.choice([8.0, 20.0, 40.0]) * N + rng.integers(20, 200))
    state = dict(type=int(rng.choice([1, 2])), add_reward=bool(rng.random() < 0.3), add_action=bool(rng.random() < 0.8),
                 add_index=bool(rng.random() < 0.3), add_velocity=bool(rng.random() < 0.3),
                 action_index=str(rng.choice(["binary", "real"])), add_position=bool(rng.random() < 0.3),
                 add_positional_dist=bool(rng.random() < 0.2), add_positional_dist_piggy=bool(rng.random() < 0.8),
                 add_positional_dist_type=int(rng.choice([1, 2, 2])), num_bins=K,
                 add_channel_obs=bool(rng.random() < 0.4))
    if state["type"] == 1 and state["add_positional_dist_piggy"]:
        state["type"] = 2          # the reference crashes on this pair when no tx is in range
    cfg = bench_config(N, A, L, reward_design=rd, State=state,
                       mobility=bool(rng.random() < 0.85), mobility_vary=bool(rng.random() < 0.4),
                       enable_fingerprint=bool(rng.random() < 0.3),
                       proportional_fair=bool(rng.random() < 0.2 and mode == STEP_MY_STEP),
                       congestion_test=bool(rng.random() < 0.2),
                       communication_range=float(rng.choice([30.0, 120.0, 250.0])),
                       bin_range=float(rng.choice([100.0, 500.0])))
    return cfg, mode, float(rng.choice([0.0, 0.5, 0.9])), int(rng.choice([0, 7]))
