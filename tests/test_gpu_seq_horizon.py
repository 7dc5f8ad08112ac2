"""Every step path at large sequence numbers and at the 24-bit horizon (include/diral_env.h: DIRAL_MAX_SLOTS).

The table words are (number << 8) | age and the keyed merges order (number << 8) | source lane: from number 2^23 on
bit 31 of those words is set, and at 2^24 - 1 the field is full (DIRAL_ERR_SEQ_OVERFLOW).  No run of the reference gets
there (8 million slots); `import_state` puts a handle anywhere in the range, and the oracle - plain int32 numbers, no
packing, translation-invariant in them (tests/test_seq_horizon.py) - states the operation.  Per path family and table
form (`last_kernel()` asserted on every slot), from tables that hold every representation boundary
(golden_util.horizon_tables):
  * ten slots from own number 1 300 000, from 2^23 - 4 (keys on both sides of bit 31 in one merge) and from
    2^24 - 2 - 10 (the run ends on the last legal number): rewards, channel observation, state and the exported tables
    bit for bit against the oracle after every slot, and the three runs against each other (numbers shifted by the
    constant, everything else identical - an error kernel and oracle could share would show here);
  * the horizon: three clean slots from DIRAL_MAX_SLOTS - 3, the fourth raises the sticky flag once, a reset clears it;
    with ONE vehicle at the horizon the per-column checks fire on that column;
  * K slots in one launch (step_policy, rollout, prefill) across 2^23 and up to the last legal number, and one past it;
  * a captured slot replayed across 2^23;
  * imports: a number outside [0, DIRAL_MAX_SLOTS] is reported, not truncated; DIRAL_MAX_SLOTS round-trips.
"""
import numpy as np
import pytest
import torch

import tests.gpu_util as gu
from diral_amd.config import (KERNEL_CH, KERNEL_FAST64, KERNEL_GENERAL, KERNEL_LARGE, KERNEL_PACKED,
                              KERNEL_POLICY, KERNEL_RING, KERNEL_WIDE, MAX_SLOTS, STEP_DESIGN, STEP_MY_STEP, STEP_MY_STEP_CH,
                              bench_config)
from diral_amd.vec_env import VecV2VEnv
from tests.golden_util import HORIZON_LAGS, horizon_tables
from tests.gpu_util import _expect_overflow, exported, load, make_oracle, oracle_slot
from tests.oracle_compare import metrics_equal, slot_equal, tables_equal
from tests.kslots_harness import VEL_SEED, as_rollout, assert_same, assert_same_envs, slot_loop

pytestmark = pytest.mark.gpu

T = 10
BASE = 1_300_000
STARTS = (BASE, (1 << 23) - 4, MAX_SLOTS - T)
RICH = dict(add_channel_obs=True, add_reward=True, add_index=True, add_velocity=True, add_position=True)
NO_ANCIENT = tuple(k for k in HORIZON_LAGS if k != "ancient")


class Case:
    """One path family at one shape: how to make its handle and what `last_kernel()` must say."""

    def __init__(self, name, N, A, L, family, path=None, form=None, mode=STEP_MY_STEP, rd=2, rich=False, B=2, rc=250.0):
        self.name, self.N, self.A, self.L, self.family, self.path, self.form = name, N, A, L, family, path, form
        self.mode, self.rd, self.rich, self.B, self.rc = mode, rd, rich, B, rc

    def cfg(self, **kw):
        kw.setdefault("track_arrival", True)
        kw.setdefault("track_prr", self.mode == STEP_MY_STEP)
        return bench_config(self.N, self.A, self.L, reward_design=self.rd, communication_range=self.rc,
                            State=RICH if self.rich else {}, **kw)

    def env(self, monkeypatch, cfg=None, dtype=torch.float64):
        if self.form:
            monkeypatch.setenv("DIRAL_TABLE_FORM", self.form)
        env = VecV2VEnv(cfg or self.cfg(), batch=self.B, device="cuda:0", out_dtype=dtype, step_mode=self.mode)
        if self.path == "general":
            env.force_general_kernel()
        elif self.path == "large":
            env.force_large_path()
        return env

    def assert_kernel(self, env):
        """The family and table form the case is about ran - a case that lands elsewhere fails.  `last_kernel()` names
        the family and, for N <= 256, the table form; the finer forms of the general kernel (values per lane) and of the
        three-launch path (codes + gated rank keys up to 512 vehicles, rank keys alone up to 1024, (number, source) keys
        beyond: k_large.hip) follow from N and A alone, so there the case's shape is what pins the form."""
        lk = env.last_kernel()
        assert (lk & 15) == self.family, (self.name, lk)
        if self.family == KERNEL_FAST64:
            assert lk & KERNEL_RING and lk & KERNEL_PACKED, (self.name, lk)
        elif self.family == KERNEL_WIDE:
            assert lk & KERNEL_RING and bool(lk & KERNEL_PACKED) == (self.form == "packed"), (self.name, lk)
        else:
            assert not lk & KERNEL_RING, (self.name, lk)

    def __repr__(self):
        return self.name


def _fast64_cases():
    out = []
    for N, A, L in ((40, 6, 1500.0), (64, 32, 2000.0)):
        for mode, tag, rd in ((STEP_MY_STEP, "step", 2), (STEP_MY_STEP_CH, "ch", 3), (STEP_DESIGN, "design", 5)):
            for rich in (False, True):
                out.append(Case("fast64-%d-%d-%s%s" % (N, A, tag, "-rich" if rich else ""), N, A, L, KERNEL_FAST64,
                                mode=mode, rd=rd, rich=rich, B=3))
    return out


def _wide_cases():
    out = []
    shapes = ((100, 16, 2500.0, STEP_MY_STEP, 2), (128, 64, 4000.0, STEP_MY_STEP_CH, 2),      # 2 values per lane
              (200, 33, 6000.0, STEP_DESIGN, 1), (256, 64, 4000.0, STEP_MY_STEP, 5))           # 4 values per lane
    for N, A, L, mode, rd in shapes:
        for form in ("packed", "plane"):
            out.append(Case("wide-%d-%d-%s" % (N, A, form), N, A, L, KERNEL_WIDE, form=form, mode=mode, rd=rd, rich=(N == 128)))
    return out


FAST64 = _fast64_cases()
WIDE = _wide_cases()
GENERAL = [Case("general-forced-40-6", 40, 6, 1500.0, KERNEL_GENERAL, path="general", rich=True, B=3),
           Case("general-forced-130-33", 130, 33, 4000.0, KERNEL_GENERAL, path="general", mode=STEP_MY_STEP_CH, rd=4),
           Case("general-by-size-40-100", 40, 100, 1500.0, KERNEL_GENERAL, mode=STEP_DESIGN, rd=1)]
LARGE = [Case("large-forced-40-6", 40, 6, 1500.0, KERNEL_LARGE, path="large", rich=True, B=3),
         Case("large-by-size-300-20", 300, 20, 6000.0, KERNEL_LARGE, mode=STEP_MY_STEP_CH, rd=2),
         Case("large-rank-keys-600-24", 600, 24, 12000.0, KERNEL_LARGE, B=1),       # 512 < N <= 1024: the rank keys alone
         Case("large-keys-only-1100-30", 1100, 30, 20000.0, KERNEL_LARGE, B=1)]
BY_NAME = {c.name: c for c in FAST64 + WIDE + GENERAL + LARGE}


def shifted(tab, delta):
    out = dict(tab)
    out["seq"] = np.where(tab["seq"] > 0, tab["seq"].astype(np.int64) + delta, 0).astype(np.int32)
    return out


def run_from(case, monkeypatch, tab, acts):
    """len(acts) slots of the case from the tables `tab`, each compared with the oracle; returns what the slots gave."""
    cfg = case.cfg()
    env = case.env(monkeypatch, cfg)
    load(env, tab)
    orc = make_oracle(cfg, tab)
    out = []
    for t in range(len(acts)):
        obs, rew, chobs, _ = gu.gpu_step(env, case.mode, acts[t], t)
        case.assert_kernel(env)
        slot_equal(cfg, case.mode, (obs, rew, chobs), oracle_slot(orc, case.mode, acts[t], t), (case.name, t))
        st = exported(env)
        tables_equal(st, orc.export(), (case.name, t))
        out.append(dict(st, obs=obs, rew=rew, chobs=chobs))
    n = len(acts) - 1
    assert np.array_equal(env.info_age(n).cpu().numpy(), orc.info_age(n))
    m, om = env.metrics().cpu().numpy(), orc.metrics()
    metrics_equal(m, om, case.name, prr=True)
    env.check()
    return out, m


@pytest.mark.parametrize("name", [c.name for c in FAST64 + WIDE + GENERAL + LARGE])
def test_ten_slots_from_three_points_of_the_range(name, monkeypatch):
    """The case's kernel from own numbers 1 300 000, 2^23 - 4 and DIRAL_MAX_SLOTS - 10: each run against the oracle slot by
    slot, and the three runs against each other - the numbers shifted by the constant, everything else identical."""
    case = BY_NAME[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    tab = horizon_tables(rng, case.B, case.N, case.L, BASE)
    lag = BASE - tab["seq"].astype(np.int64)
    heard = tab["seq"] > 0
    for lo, hi in ((1, 3), (6, 6), (7, 7), (8, 8), (9, 40), (253, 253), (254, 254), (255, 255), (1 << 20, 1 << 21)):
        assert (heard & (lag >= lo) & (lag <= hi)).any(), (lo, hi)              # the boundaries the case is about are there
    assert (~heard).any()
    acts = rng.integers(0, case.A, size=(T, case.B, case.N)).astype(np.int32)
    base, base_m = run_from(case, monkeypatch, tab, acts)
    for own in STARTS[1:]:
        delta = own - BASE
        run, m = run_from(case, monkeypatch, shifted(tab, delta), acts)
        for t in range(T):
            for k in base[t]:
                if k == "seq":
                    want = np.where(base[t]["seq"] > 0, base[t]["seq"].astype(np.int64) + delta, 0)
                    assert np.array_equal(run[t]["seq"], want), (name, own, t)
                else:
                    assert np.array_equal(run[t][k], base[t][k]), (name, own, t, k)
        assert np.array_equal(m, base_m), (name, own)
    assert run[-1]["seq"].max() == MAX_SLOTS                                     # the last run ended on the last legal number


HORIZON = ["fast64-64-32-step-rich", "wide-128-64-packed", "wide-200-33-plane", "wide-100-16-plane", "wide-256-64-packed",
           "general-forced-40-6", "general-forced-130-33", "large-by-size-300-20", "large-rank-keys-600-24",
           "large-keys-only-1100-30"]


def _fresh_slots(case, env, cfg, rng, n):
    """After a reset the handle steps like a new one."""
    x0 = rng.integers(0, int(case.L), size=(case.B, case.N)).astype(np.float64)
    v0 = rng.uniform(1.1, 2.7, size=(case.B, case.N))
    env.reset_topology(x0, 0.0, v0)
    from oracle.oracle import Oracle, SQ_IEEE
    orc = Oracle(cfg, batch=case.B, sq_mode=SQ_IEEE, threads=8)
    orc.reset(x0, np.zeros((case.B, case.N)), v0)
    for t in range(n):
        a = rng.integers(0, case.A, size=(case.B, case.N)).astype(np.int32)
        obs, rew, chobs, _ = gu.gpu_step(env, case.mode, a, t)
        case.assert_kernel(env)
        slot_equal(cfg, case.mode, (obs, rew, chobs), oracle_slot(orc, case.mode, a, t), (case.name, "after reset", t))
    tables_equal(exported(env), orc.export(), (case.name, "after reset"))
    env.check()


@pytest.mark.parametrize("name", HORIZON)
def test_the_slot_past_the_last_number_is_reported_once(name, monkeypatch):
    """From DIRAL_MAX_SLOTS - 3: three slots are clean and the oracle's, the fourth raises DIRAL_ERR_SEQ_OVERFLOW - a
    status, reported by one diral_env_check and cleared by it; what the handle holds then is undefined until a reset,
    after which it runs like a new one."""
    case = BY_NAME[name]
    cfg = case.cfg()
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    tab = horizon_tables(rng, case.B, case.N, case.L, MAX_SLOTS - 3)
    env = case.env(monkeypatch, cfg)
    load(env, tab)
    orc = make_oracle(cfg, tab)
    for t in range(3):
        a = rng.integers(0, case.A, size=(case.B, case.N)).astype(np.int32)
        obs, rew, chobs, _ = gu.gpu_step(env, case.mode, a, t)
        case.assert_kernel(env)
        slot_equal(cfg, case.mode, (obs, rew, chobs), oracle_slot(orc, case.mode, a, t), (name, t))
        env.check()
    st = exported(env)
    tables_equal(st, orc.export(), name)
    assert st["seq"].max() == MAX_SLOTS
    gu.gpu_step(env, case.mode, rng.integers(0, case.A, size=(case.B, case.N)).astype(np.int32), 3)
    case.assert_kernel(env)
    _expect_overflow(env)
    _fresh_slots(case, env, cfg, rng, 3)


@pytest.mark.parametrize("name", ["fast64-40-6-step", "wide-100-16-packed", "wide-256-64-plane", "general-forced-130-33",
                                  "large-by-size-300-20", "large-rank-keys-600-24", "large-keys-only-1100-30"])
def test_one_vehicle_at_the_horizon_among_young_ones(name, monkeypatch):
    """Only vehicle N - 3 of env 0 has run for DIRAL_MAX_SLOTS - 1 slots, the others for a few thousand: one more slot is
    clean (that column ends on the last legal number, keyed above bit 31 next to columns far below it), the next one
    raises the flag - from that one column's check."""
    case = BY_NAME[name]
    cfg = case.cfg()
    rng = np.random.default_rng(sum(map(ord, name)) + 2)
    own = rng.integers(3000, 9000, size=(case.B, case.N))
    own[0, case.N - 3] = MAX_SLOTS - 1
    tab = horizon_tables(rng, case.B, case.N, case.L, own)
    assert (tab["seq"][0, :, case.N - 3] > 0).sum() > 2 and np.delete(tab["seq"], case.N - 3, axis=2).max() < 9000
    env = case.env(monkeypatch, cfg)
    load(env, tab)
    orc = make_oracle(cfg, tab)
    a = rng.integers(0, case.A, size=(case.B, case.N)).astype(np.int32)
    obs, rew, chobs, _ = gu.gpu_step(env, case.mode, a, 0)
    case.assert_kernel(env)
    slot_equal(cfg, case.mode, (obs, rew, chobs), oracle_slot(orc, case.mode, a, 0), name)
    st = exported(env)
    tables_equal(st, orc.export(), name)
    assert st["seq"][0, case.N - 3, case.N - 3] == MAX_SLOTS
    env.check()
    gu.gpu_step(env, case.mode, a, 1)
    case.assert_kernel(env)
    _expect_overflow(env)


# ---- K slots in one launch --------------------------------------------------------------------------------------------

K = 5
KSTARTS = ((1 << 23) - 3, MAX_SLOTS - 5)


def _kcase(N, A, L, form=None, mode=STEP_MY_STEP, rd=2, B=3):
    fam = KERNEL_FAST64 if N <= 64 else KERNEL_WIDE
    c = Case("k-%d-%d-%s" % (N, A, form or "fast64"), N, A, L, fam, form=form, mode=mode, rd=rd, B=B)
    return c


def _twins(case, monkeypatch, own, seed, dtype=torch.float64):
    """Two handles of the case and an oracle, all three on the same horizon tables."""
    cfg = case.cfg(track_arrival=False, track_prr=False)
    rng = np.random.default_rng(seed)
    tab = horizon_tables(rng, case.B, case.N, case.L, own, lags=NO_ANCIENT if own < (1 << 21) else HORIZON_LAGS)
    envs = [case.env(monkeypatch, cfg, dtype) for _ in range(2)]
    for e in envs:
        load(e, tab)
    return cfg, tab, envs, make_oracle(cfg, tab)


def _policy_slots(case, env, pol, k_slots, launches):
    """`launches` step_policy calls of `k_slots` slots each; returns the per-slot shaped rewards / sums / collisions, the
    last slot's outputs and the actions every slot of a one-slot run was given."""
    B, N = case.B, case.N
    o = dict(dtype=env.out_dtype, device="cuda:0")
    a, nxt = pol.prev_action.clone(), torch.empty_like(pol.prev_action)
    sh, sr, co, given = [], [], [], []
    t = 0
    for _ in range(launches):
        lead = (k_slots,) if k_slots > 1 else ()
        s, r, c = torch.zeros(lead + (B, N), **o), torch.zeros(lead + (B,), **o), torch.zeros(lead + (B,), **o)
        given.append(a.clone())
        env.step_policy(a, t, pol, nxt, shaped_out=s, sum_r_out=r, collision_out=c, slots=k_slots, want_chobs=True,
                        mode=case.mode)
        lk = env.last_kernel()
        assert (lk & 15) == case.family, lk
        assert k_slots == 1 or lk & KERNEL_POLICY, lk
        if case.family == KERNEL_WIDE:
            assert bool(lk & KERNEL_PACKED) == (case.form == "packed"), lk
        a, nxt = nxt, a
        t += k_slots
        sh.append(s.reshape((-1, B, N))); sr.append(r.reshape((-1, B))); co.append(c.reshape((-1, B)))
    torch.cuda.synchronize()
    return dict(shaped=torch.cat(sh), sum_r=torch.cat(sr), coll=torch.cat(co), obs=env._obs.clone(), rew=env._rew.clone(),
                chobs=env._chobs.clone(), next=a.clone()), given


KPOLICY = [_kcase(40, 6, 1500.0), _kcase(64, 32, 2000.0, mode=STEP_MY_STEP_CH), _kcase(100, 16, 2500.0, "packed"),
           _kcase(200, 33, 6000.0, "plane")]


@pytest.mark.parametrize("own", KSTARTS)
@pytest.mark.parametrize("case", KPOLICY, ids=repr)
def test_k_policy_slots_in_one_launch_across_the_range(case, own, monkeypatch):
    """step_policy(slots=5) from 2^23 - 3 and from DIRAL_MAX_SLOTS - 5 (ending on the last legal number): clean, equal to
    five one-slot calls bit for bit, tables included (the twin carries the per-slot values: shaped rewards, sums,
    collisions); against the oracle, run on the actions the policy chose: the LAST slot's reward, channel observation
    and state, and the exported tables."""
    from diral_amd.sps import SpsPolicy
    cfg, tab, (e1, e2), orc = _twins(case, monkeypatch, own, 600 + case.N)
    p1, p2 = (SpsPolicy(case.B, case.N, case.A, device="cuda:0", seed=3) for _ in range(2))
    one, given = _policy_slots(case, e1, p1, 1, K)
    got, _ = _policy_slots(case, e2, p2, K, 1)
    for k in one:
        assert torch.equal(one[k], got[k]), (k, (one[k] != got[k]).nonzero()[:4])
    assert torch.equal(p1.prev_action, p2.prev_action) and torch.equal(p1.counter, p2.counter)
    s2 = assert_same_envs(e1, e2, entries=False)
    for t, a in enumerate(given):
        a = a.cpu().numpy()
        o_rew, o_chobs = orc.step(case.mode, a, t)
    assert np.array_equal(got["rew"].cpu().numpy(), o_rew) and np.array_equal(got["chobs"].cpu().numpy(), o_chobs)
    assert np.array_equal(got["obs"].cpu().numpy(), orc.obtain_state(a, o_chobs, o_rew))
    tables_equal(exported(e2), orc.export(), (case.name, own))
    assert s2["seq"].max().item() == own + K
    e1.check(); e2.check()


@pytest.mark.parametrize("case", KPOLICY, ids=repr)
def test_k_policy_slots_one_past_the_last_number_are_reported(case, monkeypatch):
    from diral_amd.sps import SpsPolicy
    cfg, tab, (e1, e2), orc = _twins(case, monkeypatch, MAX_SLOTS - 5, 700 + case.N)
    _policy_slots(case, e2, SpsPolicy(case.B, case.N, case.A, device="cuda:0", seed=3), K + 1, 1)
    _expect_overflow(e2)


KROLLOUT = [_kcase(40, 6, 1500.0, mode=STEP_MY_STEP_CH, rd=3), _kcase(64, 32, 2000.0), _kcase(128, 64, 4000.0, "packed"),
            _kcase(256, 64, 4000.0, "plane")]


@pytest.mark.parametrize("own", KSTARTS)
@pytest.mark.parametrize("case", KROLLOUT, ids=repr)
def test_rollout_in_one_launch_across_the_range(case, own, monkeypatch):
    """rollout (five slots of a given action sequence) against the loop of one-slot steps on a twin handle (every slot's
    shaped rewards, sums and collisions, the last slot's outputs, tables, metrics) and against the oracle (the LAST slot's
    reward and state, the exported tables); six slots from DIRAL_MAX_SLOTS - 5 raise the flag."""
    cfg, tab, (e1, e2), orc = _twins(case, monkeypatch, own, 800 + case.N)
    mode = "my_step_ch" if case.mode == STEP_MY_STEP_CH else "my_step"
    seq = torch.stack([e1.sample(7000 + k) for k in range(K + 1)])
    want = as_rollout(slot_loop(e1, seq[:K], 0, mode), "last")
    got = e2.rollout(seq[:K], 0, mode=mode, states="last", global_reward_avg=True, vel_seed=VEL_SEED)
    torch.cuda.synchronize()
    lk = e2.last_kernel()
    assert (lk & 15) == case.family and lk & KERNEL_POLICY, lk
    assert case.family != KERNEL_WIDE or bool(lk & KERNEL_PACKED) == (case.form == "packed"), lk
    assert_same(want, got, (case.name, own))
    assert_same_envs(e1, e2, entries=False)
    for t in range(K):
        want = oracle_slot(orc, case.mode, seq[t].cpu().numpy(), t, state=t == K - 1)
    slot_equal(cfg, case.mode, (gu.host(got["states"]), gu.host(got["reward"]), None), want, (case.name, own))
    tables_equal(exported(e2), orc.export(), (case.name, own))
    e1.check(); e2.check()
    if own == MAX_SLOTS - K:
        load(e2, tab)
        e2.rollout(seq, 0, mode=mode, states="last")
        _expect_overflow(e2)


@pytest.mark.parametrize("own", KSTARTS)
@pytest.mark.parametrize("mode,rd", [("my_step_design", 2), ("my_step_ch", 3)])
def test_prefill_in_one_launch_across_the_range(mode, rd, own, monkeypatch):
    """The prefill launch (five slots of device-drawn actions) against the loop of sample + step + obtain_state calls on a
    twin handle (every slot's state and actions, tables, metrics).  Of the oracle only the tables are compared: it is
    stepped with the loop's actions at t = 0 on every slot, as the prefill steps (main_test.py:99-114), and its per-slot
    outputs are the twin's business.  Six slots from DIRAL_MAX_SLOTS - 5 raise the flag."""
    from diral_amd.driver import DriverLoop
    step_mode = STEP_DESIGN if mode == "my_step_design" else STEP_MY_STEP_CH
    case = Case("prefill-" + mode, 64, 32, 2000.0, KERNEL_FAST64, mode=step_mode, rd=rd, rich=True, B=3)
    cfg = case.cfg(track_arrival=False, track_prr=False)
    rng = np.random.default_rng(900 + rd)
    tab = horizon_tables(rng, case.B, case.N, case.L, own)
    envs = [case.env(monkeypatch, cfg) for _ in range(2)]
    loops = [DriverLoop(e, enable_channel=(mode == "my_step_ch")) for e in envs]
    a0 = envs[0].sample(123)
    for e, lp in zip(envs, loops):
        e.reset_topology(tab["pos_x"], 0.0, tab["vel"])
        lp.bootstrap(a0)                                             # the stale reward column of the prefill's states
        e.import_state(tab["pos_x"], np.zeros(tab["pos_x"].shape), tab["vel"], seq=tab["seq"], age=tab["age"], x=tab["x"])
    e_loop, e_one = envs
    orc = make_oracle(cfg, tab)
    seed = 77001
    want_s, want_a = [], []
    for k in range(K):
        a = e_loop.sample(seed + k)
        want_a.append(a.clone())
        want_s.append(loops[0].prefill_step(a).clone())
        orc.step(step_mode, a.cpu().numpy(), 0)
    states, acts, nxt = e_one.prefill(e_one.sample(seed), K, seed, rew_in=loops[1]._rews0, mode=mode)
    torch.cuda.synchronize()
    lk = e_one.last_kernel()
    assert (lk & 15) == KERNEL_FAST64 and lk & KERNEL_POLICY and bool(lk & KERNEL_CH) == (mode == "my_step_ch"), lk
    assert torch.equal(acts, torch.stack(want_a))
    for k in range(K):
        assert torch.equal(states[k], want_s[k]), (k, (states[k] != want_s[k]).nonzero()[:5])
    assert_same_envs(e_loop, e_one, entries=False)
    tables_equal(exported(e_one), orc.export(), (mode, own))
    e_loop.check(); e_one.check()
    if own == MAX_SLOTS - K:
        e_one.import_state(tab["pos_x"], np.zeros(tab["pos_x"].shape), tab["vel"], seq=tab["seq"], age=tab["age"], x=tab["x"])
        e_one.prefill(e_one.sample(seed), K + 1, seed, rew_in=loops[1]._rews0, mode=mode)
        _expect_overflow(e_one)


# ---- graph replay ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["fast64-64-32-step", "wide-128-64-packed"])
def test_a_captured_slot_replayed_across_bit_31(name, monkeypatch):
    """One slot captured at own number 2^23 - 5 and replayed 12 times (the keys cross bit 31 inside the replays) equals
    eager stepping and the oracle."""
    case = BY_NAME[name]
    cfg = case.cfg(track_arrival=False)
    rng = np.random.default_rng(sum(map(ord, name)) + 3)
    tab = horizon_tables(rng, case.B, case.N, case.L, (1 << 23) - 6)
    eager, graphed = case.env(monkeypatch, cfg), case.env(monkeypatch, cfg)
    orc = make_oracle(cfg, tab)
    acts = rng.integers(0, case.A, size=(13, case.B, case.N)).astype(np.int32)
    a_dev = torch.as_tensor(acts[0], device="cuda:0").contiguous()
    for e in (eager, graphed):
        load(e, tab)
        e._step(case.mode, a_dev, 1, want_chobs=True)            # (the first step behind an import, outside the capture)
    orc.step(case.mode, acts[0], 1)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            obs_g, rew_g, _ = graphed._step(case.mode, a_dev, 1, want_chobs=True)
    chobs_g = graphed._chobs
    for i in range(1, 13):
        a_dev.copy_(torch.as_tensor(acts[i]))
        g.replay()
        torch.cuda.synchronize()
        case.assert_kernel(graphed)
        got = (obs_g.cpu().numpy(), rew_g.cpu().numpy(), chobs_g.cpu().numpy())
        obs_e, rew_e, chobs_e, _ = gu.gpu_step(eager, case.mode, acts[i], 1)
        assert all(np.array_equal(x, y) for x, y in zip(got, (obs_e, rew_e, chobs_e))), i
        slot_equal(cfg, case.mode, got, oracle_slot(orc, case.mode, acts[i], 1), (name, i))
    sg = exported(graphed)
    tables_equal(sg, orc.export(), name)
    tables_equal(exported(eager), orc.export(), name)
    assert sg["seq"].max() == (1 << 23) + 7
    graphed.check(); eager.check()


# ---- imports -----------------------------------------------------------------------------------------------------------

def _entries(tab):
    from diral_amd.vec_env import ENTRY_DTYPE
    rec = np.zeros(tab["seq"].shape, dtype=ENTRY_DTYPE)
    rec["pos_x"], rec["seq_num"], rec["last_update"] = tab["x"], tab["seq"], tab["age"]
    return rec


@pytest.mark.parametrize("N,A,L", [(40, 6, 1500.0), (130, 33, 4000.0)])
@pytest.mark.parametrize("where", ["own", "other"])
@pytest.mark.parametrize("bad", [(1 << 24) - 1, (1 << 24) + 5, -1])
def test_an_imported_number_outside_the_range_is_reported(bad, where, N, A, L):
    """One entry of an otherwise valid table carries a number the 24-bit field cannot hold (2^24 + 5 would arrive as 5, -1
    as 2^24 - 1), or the one no step may start from: the next diral_env_check returns DIRAL_ERR_SEQ_OVERFLOW, through
    import_state and through import_entries; the same table without it is clean."""
    B = 2
    cfg = bench_config(N, A, L)
    rng = np.random.default_rng(N + 5)
    tab = horizon_tables(rng, B, N, L, 5000, lags=NO_ANCIENT)
    u, k = (N - 2, N - 2) if where == "own" else (3, N - 2)
    env = gu.make_env(cfg, B)
    load(env, tab)
    env.check()
    env.import_entries(_entries(tab))
    env.check()
    wrong = dict(tab, seq=tab["seq"].copy())
    wrong["seq"][1, u, k] = bad
    env.import_state(seq=wrong["seq"])
    _expect_overflow(env)
    load(env, tab)
    env.check()
    env.import_entries(_entries(wrong))
    _expect_overflow(env)


@pytest.mark.parametrize("N,A,L", [(40, 6, 1500.0), (130, 33, 4000.0)])
def test_the_last_legal_number_round_trips_through_both_imports(N, A, L):
    B = 2
    cfg = bench_config(N, A, L)
    tab = horizon_tables(np.random.default_rng(N + 6), B, N, L, MAX_SLOTS)
    assert tab["seq"].max() == MAX_SLOTS == (1 << 24) - 2
    env = gu.make_env(cfg, B)
    load(env, tab)
    for again in range(2):
        st = exported(env)
        for k in ("seq", "age", "x"):
            assert np.array_equal(st[k], tab[k]), k
        from diral_amd.vec_env import ENTRY_DTYPE
        rec = env.export_entries().cpu().numpy().view(ENTRY_DTYPE)[..., 0]
        assert np.array_equal(rec["seq_num"], tab["seq"]) and np.array_equal(rec["last_update"], tab["age"])
        assert np.array_equal(rec["pos_x"], tab["x"].astype(np.float32))
        env.check()
        if not again:
            env.import_entries(_entries(tab))                        # (xpos are integers below 2^24: exact in float32)
