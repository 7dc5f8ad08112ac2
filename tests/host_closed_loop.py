"""TEST-ONLY host statement of the closed loop the device runs as one launch per slot or per K slots: the CPU oracle's
env step + the driver's reward shaping (diral_amd/driver.py's torch statement) + the SPS agent (the behaviour
include/diral_env.h and diral_amd/sps.py document) + the counter-based generator the device draws from.  Plain NumPy /
Python on top of tests/oracle_backend.OracleBackend; never imported by diral_amd/.

Three parts:
  * the generator mirror: `mix64`, `rng_u64`, `rng_unit` over uint64 and the draw rules of the nine streams;
  * `HostSps`: SemiPersistentScheduling.step + choose_new_resource for many agents, with Python's `sorted`, and a record
    of every re-selection (shortcut condition, threshold raises, decision margin);
  * `HostClosedLoop`: slots of [oracle step -> shaping -> HostSps -> update_velocity at an episode end] and the prefill.
"""
import math

import numpy as np
import torch

from diral_amd.config import STEP_DESIGN, STEP_MY_STEP, STEP_MY_STEP_CH
from diral_amd.driver import np_sum_lastdim
from oracle.oracle import SQ_IEEE
from tests.oracle_compare import exp_bounds as _exp_bounds, stored_age  # noqa: F401  (`_exp_bounds`: re-exported)
from tests.oracle_backend import OracleBackend

U64 = (1 << 64) - 1
MARGIN_DB = 1e-9        # a re-selection whose margin is below this is ambiguous: device log10 may round the other way

# ---- the generator -----------------------------------------------------------------------------------------------
# splitmix64's output function over seed / stream / index (the constants are the published ones)
_GAMMA = 0x9E3779B97F4A7C15
_M1 = 0xBF58476D1CE4E5B9
_M2 = 0x94D049BB133111EB
_STREAM = 0xD1342543DE82EF95

(STREAM_TOPO_X, STREAM_TOPO_V, STREAM_SAMPLE, STREAM_VELOCITY, STREAM_SPS_PREV, STREAM_SPS_COUNTER, STREAM_NEW_COUNTER,
 STREAM_KEEP, STREAM_CHOICE) = range(1, 10)


def mix64(z):
    """splitmix64: z += gamma, then the two xor-shift-multiply rounds; uint64 in, uint64 out (any shape)."""
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64)).copy()
    with np.errstate(over="ignore"):
        z += np.uint64(_GAMMA)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_M2)
        return z ^ (z >> np.uint64(31))


def rng_u64(seed, stream, idx):
    """The draw of (seed, stream, idx): mix64(mix64(seed ^ stream * c) + idx).  `idx` may be an array."""
    key = (int(seed) & U64) ^ ((int(stream) * _STREAM) & U64)
    with np.errstate(over="ignore"):
        return mix64(mix64(np.uint64(key)) + np.asarray(idx, dtype=np.uint64))


def rng_unit(r):
    """[0, 1) from the top 53 bits."""
    return (np.asarray(r, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def _global_idx(B, N, env_offset):
    return np.arange(B * N, dtype=np.uint64) + np.uint64(int(env_offset) * N)


def draw_topology(seed, B, N, highway_length, mobility_vary, env_offset=0):
    """reset_topology(seed): x integer-uniform in [0, L) (stream 1), v ~ U(1.1, 2.7) or 1.7 with mobility_vary
    (stream 2); indexed by the GLOBAL vehicle index."""
    idx = _global_idx(B, N, env_offset)
    Lf = math.floor(highway_length)
    x = np.floor(rng_unit(rng_u64(seed, STREAM_TOPO_X, idx)) * Lf)
    x = np.where(x >= Lf, Lf - 1.0, x)
    if mobility_vary:
        v = np.full(B * N, 1.7)
    else:
        v = 1.1 + rng_unit(rng_u64(seed, STREAM_TOPO_V, idx)) * (2.7 - 1.1)
    return x.reshape(B, N), v.reshape(B, N)


def draw_sample(seed, B, N, A, env_offset=0):
    """sample(seed): uniform actions (stream 3), global index."""
    return (rng_u64(seed, STREAM_SAMPLE, _global_idx(B, N, env_offset)) % np.uint64(A)).astype(np.int32).reshape(B, N)


def draw_velocity(seed, B, N, env_offset=0):
    """update_velocity(seed=...): random.randrange(1, 4) per vehicle (stream 4), global index."""
    return (1 + rng_u64(seed, STREAM_VELOCITY, _global_idx(B, N, env_offset)) % np.uint64(3)).astype(np.uint8).reshape(B, N)


def draw_sps_init(seed, agents, window):
    """SpsPolicy(...): prev_action = randint(0, window) (stream 5), counter = randint(5, 15) (stream 6); indexed per
    handle, i = b * N + lane."""
    i = np.arange(agents, dtype=np.uint64)
    prev = (rng_u64(seed, STREAM_SPS_PREV, i) % np.uint64(window + 1)).astype(np.int32)
    cnt = (5 + rng_u64(seed, STREAM_SPS_COUNTER, i) % np.uint64(11)).astype(np.int32)
    return prev, cnt


def draw_sps_step(seed, agents):
    """The three draws of one SPS step, per handle index: new counter randint(5, 16) (stream 7), keep random()
    (stream 8), choice (stream 9, the top 31 bits)."""
    i = np.arange(agents, dtype=np.uint64)
    cnt = (5 + rng_u64(seed, STREAM_NEW_COUNTER, i) % np.uint64(12)).astype(np.int32)
    keep = rng_unit(rng_u64(seed, STREAM_KEEP, i))
    choice = (rng_u64(seed, STREAM_CHOICE, i) >> np.uint64(33)).astype(np.int64)
    return cnt, keep, choice


# ---- the SPS agent -----------------------------------------------------------------------------------------------
def window_from_chobs(chobs, actions):
    """The documented map from the channel observation to the RSSI-like window: own -60, out of range -160, idle -200,
    heard -40 - 30 log10(max(d, 1)).  chobs [agents, A], actions [agents] -> (window, heard mask)."""
    d = np.asarray(chobs, dtype=np.float64)
    heard = (d > 0) & (d < 100000.0)
    w = np.full(d.shape, -200.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(heard, -40.0 - 30.0 * np.log10(np.maximum(d, 1.0)), w)
    w = np.where(d >= 100000.0, -160.0, w)
    own = np.arange(d.shape[-1])[None, :] == np.asarray(actions)[:, None]
    w = np.where(own, -60.0, w)
    return w, heard & ~own


def choose_new_resource(w, prev, threshold, inc_db, r):
    """choose_new_resource for one agent: raise the threshold in `inc_db` steps until len(sA) >= A / 5 (prev excluded),
    sort by (value, subframe) with Python's `sorted`, need = max(1, ceil(min(A / 5, len(sA)))), pick r % need.
    Returns (chosen, raises, thresholds tried)."""
    A = len(w)
    min_sA = A / 5
    thr, tried = threshold, []
    for _ in range(100000):
        tried.append(thr)
        sA = [s for s in range(A) if s != prev and w[s] < thr]
        if not len(sA) < min_sA:
            break
        thr = thr + inc_db
    if not sA:
        return prev, len(tried) - 1, tried
    order = sorted(sA, key=lambda s: (w[s], s))
    need = max(1, math.ceil(min(min_sA, len(sA))))
    return order[int(r) % need], len(tried) - 1, tried


class HostSps:
    """SemiPersistentScheduling for `agents` independent agents (counter, prev_action per agent)."""

    def __init__(self, agents, A, threshold=-110.0, inc_db=3.0, keep_prob=0.8, prev_action=None, counter=None):
        self.n, self.A = int(agents), int(A)
        self.threshold, self.inc_db, self.keep_prob = float(threshold), float(inc_db), float(keep_prob)
        self.prev_action = np.zeros(self.n, np.int32) if prev_action is None else np.array(prev_action, np.int32).reshape(-1)
        self.counter = np.zeros(self.n, np.int32) if counter is None else np.array(counter, np.int32).reshape(-1)
        self.log = []           # one dict per re-selection: agent, shortcut, raises, margin, far

    @classmethod
    def from_seed(cls, agents, A, seed, **kw):
        prev, cnt = draw_sps_init(seed, agents, A - 1)
        return cls(agents, A, prev_action=prev, counter=cnt, **kw)

    def step(self, window=None, draw_counter=None, draw_keep=None, draw_choice=None, seed=None, chobs=None, actions=None):
        """One step for every agent.  Either `window` [agents, A], or `chobs` + `actions` (the window is then built by
        `window_from_chobs`, and the shortcut condition / margin are recorded from the observation).  Draws: injected,
        or the mirror's from `seed`.  Returns actions [agents] int32."""
        if draw_counter is None or draw_keep is None or draw_choice is None:
            mc, mk, mch = draw_sps_step(seed, self.n)
            draw_counter = mc if draw_counter is None else draw_counter
            draw_keep = mk if draw_keep is None else draw_keep
            draw_choice = mch if draw_choice is None else draw_choice
        draw_counter, draw_keep, draw_choice = (np.asarray(a).reshape(-1) for a in (draw_counter, draw_keep, draw_choice))
        heard = None
        if window is None:
            chobs = np.asarray(chobs, dtype=np.float64).reshape(self.n, self.A)
            actions = np.asarray(actions).reshape(-1)
            window, heard = window_from_chobs(chobs, actions)
        window = np.asarray(window, dtype=np.float64).reshape(self.n, self.A)
        expired = self.counter == 0
        self.counter = np.where(expired, draw_counter, self.counter - 1).astype(np.int32)
        resel = expired & ~(draw_keep < self.keep_prob)
        for i in np.flatnonzero(resel):
            w = window[i].tolist()
            prev = int(self.prev_action[i])
            chosen, raises, tried = choose_new_resource(w, prev, self.threshold, self.inc_db, int(draw_choice[i]) & 0xFFFFFFFF)
            rec = dict(agent=int(i), raises=raises, shortcut=None, margin=math.inf, far=False)
            if heard is not None:
                rec.update(self._judge(chobs[i], w, heard[i], prev, int(actions[i]), tried))
            self.log.append(rec)
            self.prev_action[i] = chosen
        return self.prev_action.copy()

    def _judge(self, d, w, heard, prev, own, tried):
        """What the host knows about one re-selection from the observation: whether the unheard subframes alone decide
        it (enough idle / out-of-range candidates below the threshold and no heard transmitter beyond 5 km - then no
        log10 value matters), and how close a heard value came to anything it was compared with."""
        A = self.A
        need = max(1, math.ceil(A / 5))
        unheard = sum(1 for s in range(A) if s != prev and s != own and not heard[s]
                      and ((d[s] >= 100000.0 and -160.0 < self.threshold) or (d[s] == 0.0 and -200.0 < self.threshold)))
        far = any(heard[s] and not d[s] <= 5000.0 for s in range(A))
        margin = math.inf
        for s in range(A):
            if not heard[s] or s == prev:
                continue
            for thr in tried:
                margin = min(margin, abs(w[s] - thr))
            for s2 in range(A):
                # (equal arguments of log10 - equal distances, or two below the 1 m clamp - give equal values on any
                # log10: that order is the subframes', not a rounding's)
                if s2 != s and s2 != prev and max(d[s2], 1.0) != max(d[s], 1.0):
                    margin = min(margin, abs(w[s] - w[s2]))
        return dict(shortcut=unheard >= need and not far, margin=margin, far=far)


# ---- the closed loop ---------------------------------------------------------------------------------------------
_STEP = {STEP_MY_STEP: "my_step", STEP_MY_STEP_CH: "my_step_ch", STEP_DESIGN: "my_step_design",
         "my_step": "my_step", "my_step_ch": "my_step_ch", "my_step_design": "my_step_design"}


class HostClosedLoop:
    """B envs of the CPU oracle (IEEE squares) driven by HostSps, with the driver's reward shaping in `dtype`.

    `policy_seed`, `sps`: as SpsPolicy(seed=policy_seed); the slot of the policy's step counter `_t` draws with
    policy_seed * 1000003 + _t + 1 (VecV2VEnv.step_policy), the clocked form with policy_seed * 1000003 + offset + clock.
    `stuck_penalty` = (threshold, value) or None.  Envs one of whose re-selections was ambiguous (margin below MARGIN_DB)
    are marked in `left_out` from that slot on."""

    def __init__(self, cfg, B, x0, v0, sps, policy_seed, mode="my_step", dtype=np.float64, global_reward_avg=True,
                 stuck_penalty=None, vel_seed=0, env_offset=0):
        self.cfg, self.B, self.N, self.A = cfg, int(B), cfg.num_users, cfg.num_channels
        self.ob = OracleBackend(cfg, batch=B, sq_mode=SQ_IEEE)
        self.ob.reset_topology(np.asarray(x0, np.float64), np.zeros((B, self.N)), np.asarray(v0, np.float64))
        self.step_fn = getattr(self.ob, _STEP[mode])
        self.sps, self.policy_seed, self._t = sps, int(policy_seed), 0
        self.dtype = np.dtype(dtype)
        self.tdtype = torch.float32 if self.dtype == np.float32 else torch.float64
        self.global_reward_avg = bool(global_reward_avg)
        self.stuck_penalty = stuck_penalty
        self.pen_counter = np.zeros((B, self.N), np.int32)
        self.pen_prev = np.full((B, self.N), -1, np.int32)
        self.vel_seed, self.env_offset = int(vel_seed), int(env_offset)
        self.left_out = np.zeros(B, bool)
        self.vel_updates = 0

    # the driver's reward post-processing (diral_amd/driver.py DriverLoop.slot, the torch statement) in `dtype`
    def shape(self, rew, actions):
        reward = torch.from_numpy(np.ascontiguousarray(rew.astype(self.dtype)))
        sum_r = np_sum_lastdim(reward)
        coll = self.A - sum_r
        if self.stuck_penalty is not None:
            thr, val = self.stuck_penalty
            a = torch.from_numpy(np.ascontiguousarray(actions, dtype=np.int32))
            cnt, prev = torch.from_numpy(self.pen_counter), torch.from_numpy(self.pen_prev)
            stuck = (reward < 1) & (a == prev)
            cnt = torch.where(stuck, cnt + 1, torch.zeros_like(cnt))
            reward = torch.where(cnt > int(thr), torch.as_tensor(float(val), dtype=reward.dtype), reward)
            self.pen_counter, self.pen_prev = cnt.numpy().copy(), a.numpy().copy()
        if self.global_reward_avg:
            n_t = torch.as_tensor(float(self.N), dtype=reward.dtype)
            reward = reward + (sum_r / n_t).unsqueeze(-1)
        return reward.numpy(), sum_r.numpy(), coll.numpy()

    def slot(self, actions, t, sps_seed, want_state=True):
        """One slot: oracle step, shaping, the agents' decisions for the next slot, the velocity update when the slot
        ends an episode of a mobility_vary config.  Everything in the handle's output dtype."""
        a = np.ascontiguousarray(actions, dtype=np.int32)
        chobs, rew = self.step_fn(a, int(t))
        state = self.ob.obtain_state(chobs, a, rew).astype(self.dtype) if (want_state and self.cfg.state_space > 0) else None
        shaped, sum_r, coll = self.shape(rew, a)
        chobs_out = chobs.astype(self.dtype)        # what the handle hands the policy: a float32 handle stages float32
        n0 = len(self.sps.log)
        nxt = self.sps.step(chobs=chobs_out.reshape(self.B * self.N, self.A), actions=a.reshape(-1), seed=sps_seed)
        for rec in self.sps.log[n0:]:
            rec["slot"] = int(t)
            if rec["margin"] < MARGIN_DB:
                self.left_out[rec["agent"] // self.N] = True
        EI = self.cfg.episode_interval
        done = (int(t) % EI) == EI - 1
        if self.cfg.mobility_vary and done:
            before = self.ob.export_state()["vel"].copy()
            self.ob.update_velocity(draw_velocity(self.vel_seed + int(t) // EI, self.B, self.N, self.env_offset))
            self.vel_updates += int((self.ob.export_state()["vel"] != before).sum())
        return dict(shaped=shaped, sum_r=sum_r, coll=coll, rew=rew.astype(self.dtype), chobs=chobs_out, state=state,
                    done=np.full(self.B, done, np.uint8), actions=nxt.reshape(self.B, self.N))

    def run(self, actions, t, K=1, clock=None, offset=0):
        """K slots from `actions` at slot number t (clocked form: slot number clock + t, seeds from the clock).  Returns
        the per-slot shaped / sum_r / coll stacked [K, ...], the last slot's outputs, and the next actions."""
        outs, a = [], np.asarray(actions, np.int32)
        for ks in range(int(K)):
            if clock is None:
                seed = self.policy_seed * 1000003 + self._t + 1 + ks
                tt = int(t) + ks
            else:
                seed = self.policy_seed * 1000003 + int(offset) + int(clock) + ks
                tt = int(clock) + int(t) + ks
            o = self.slot(a, tt, seed, want_state=ks == K - 1)
            outs.append(o)
            a = o["actions"]
        if clock is None:
            self._t += int(K)
        last = dict(outs[-1])
        for k in ("shaped", "sum_r", "coll"):
            last[k] = np.stack([o[k] for o in outs])
        return last

    def prefill(self, actions, K, seed, rew_in=None, mode="my_step_design", actions_all=None, t=0):
        """The driver's random prefill: slot 0 acts on `actions`, slot ks + 1 on sample(seed + ks + 1) (or on
        `actions_all[ks + 1]` when given); every slot is my_step_design / my_step_ch at t = 0 followed by obtain_state
        with `rew_in` as the reward column (None: the slot's own reward).  Returns (states [K, B, N, S],
        actions_all [K, B, N], next actions [B, N])."""
        step = getattr(self.ob, _STEP[mode])
        states, acts = [], []
        a = np.ascontiguousarray(actions, dtype=np.int32)
        for ks in range(int(K)):
            chobs, rew = step(a, int(t))
            col = rew if rew_in is None else np.asarray(rew_in, np.float64)
            states.append(self.ob.obtain_state(chobs, a, col).astype(self.dtype))
            acts.append(a.copy())
            if actions_all is not None and ks + 1 < len(actions_all):
                a = np.ascontiguousarray(actions_all[ks + 1], dtype=np.int32)
            else:
                a = draw_sample(int(seed) + ks + 1, self.B, self.N, self.A, self.env_offset)
        return np.stack(states), np.stack(acts), a

    # ---- what the tests read ---------------------------------------------------------------------------------
    def export_state(self):
        e = self.ob.export_state()
        e["age"] = stored_age(e["age"])                 # as the suite compares them
        return e

    def metrics(self):
        return self.ob.o.metrics()

    def record(self):
        """The host's own account of the re-selections so far, for the tests' non-vacuity assertions."""
        log = self.sps.log
        return dict(reselections=len(log), shortcut=sum(1 for r in log if r["shortcut"]),
                    general=sum(1 for r in log if r["shortcut"] is False), raises=sum(r["raises"] for r in log),
                    far=sum(1 for r in log if r["far"]), min_margin=min([r["margin"] for r in log], default=math.inf),
                    left_out=int(self.left_out.sum()), vel_changed=self.vel_updates)


# ---- a closed-loop case and its run on the host (tests/test_gpu_closed_loop_host.py, tests/test_gpu_rollout_host.py) ------
RICH = dict(add_channel_obs=True, add_reward=True, add_index=True, add_velocity=True, add_position=True)


MODE_NAME = {STEP_MY_STEP: "my_step", STEP_MY_STEP_CH: "my_step_ch"}


def uses_exp(cfg, mode):
    return cfg.reward_design == 3 or (cfg.reward_design == 4 and mode == STEP_MY_STEP_CH)


class Case:
    def __init__(self, cfg, B, dt, plan, *, mode=STEP_MY_STEP, thr=-110.0, keep=0.8, pen=False, vel_seed=0, want_obs=True,
                 want_chobs=True, clock=False, x0=None, form=None, topo_seed=21, pol_seed=3, env_offset=0, counter_mod=None,
                 kernel=None, expect=()):
        self.cfg, self.B, self.dt, self.plan, self.mode = cfg, B, dt, list(plan), mode
        self.thr, self.keep, self.pen, self.vel_seed = thr, keep, pen, vel_seed
        self.want_obs, self.want_chobs, self.clock, self.x0, self.form = want_obs, want_chobs, clock, x0, form
        self.topo_seed, self.pol_seed, self.env_offset, self.counter_mod = topo_seed, pol_seed, env_offset, counter_mod
        self.kernel, self.expect = kernel, set(expect)
        self.N, self.A = cfg.num_users, cfg.num_channels
        self.npdt = np.float32 if dt == torch.float32 else np.float64


def host_run(c):
    """The whole plan of a case on the host: returns (HostClosedLoop, the outputs of every launch)."""
    B, N, A = c.B, c.N, c.A
    if c.x0 is not None:
        x0, v0 = c.x0, np.full(c.x0.shape, 1.7)
    else:
        x0, v0 = draw_topology(c.topo_seed, B, N, c.cfg.highway_length, c.cfg.mobility_vary, c.env_offset)
    sps = HostSps.from_seed(B * N, A, c.pol_seed, threshold=c.thr, keep_prob=c.keep)
    if c.counter_mod:
        sps.counter %= c.counter_mod
    host = HostClosedLoop(c.cfg, B, x0, v0, sps, c.pol_seed, mode=MODE_NAME[c.mode], dtype=c.npdt,
                            stuck_penalty=(2, -10.0) if c.pen else None, vel_seed=c.vel_seed, env_offset=c.env_offset)
    a, t, outs = sps.prev_action.reshape(B, N).copy(), 0, []
    for K in c.plan:
        o = host.run(a, 0, K, clock=t, offset=0) if c.clock else host.run(a, t, K)
        o["left_out"] = host.left_out.copy()
        o["pen"] = (host.pen_counter.copy(), host.pen_prev.copy())
        o["sps"] = (sps.prev_action.reshape(B, N).copy(), sps.counter.reshape(B, N).copy())
        outs.append(o)
        a, t = o["actions"], t + K
    return host, (x0, v0), outs


def _eq(name, dev, want, keep, baxis=0, atol=None):
    dev = dev.cpu().numpy() if isinstance(dev, torch.Tensor) else np.asarray(dev)
    dev, want = np.compress(keep, dev, axis=baxis), np.compress(keep, np.asarray(want), axis=baxis)
    assert dev.shape == want.shape, (name, dev.shape, want.shape)
    if atol is None:
        assert np.array_equal(dev, want), (name, np.argwhere(dev != want)[:4], dev[dev != want][:4], want[dev != want][:4])
    else:
        assert np.all(np.abs(dev - want) <= atol), (name, float(np.abs(dev - want).max()), atol)
