"""The env-facing half of the reference driver, vectorised.

``main_test.marl_test`` (main_test.py:86-236) interleaves the TF agent with a
fixed sequence of env calls and some reward post-processing.  This module keeps
that sequence - bootstrap, prefill, slot loop, information age, reward shaping,
episode boundary - for B envs at once on top of :class:`VecV2VEnv` (or any
object with its method names), so a PyTorch agent can be dropped where the
reference's ``mainDRQN`` sat.  The agent itself is out of scope.

    loop = DriverLoop(env, global_reward_avg=True, episode_interval=25)
    state = loop.bootstrap()                         # main_test.py:89-94
    for _ in range(prefill): state = loop.prefill_step(env.sample())     # :99-114
    for t in range(time_slots):
        out = loop.slot(policy(state), t)            # :119-236, one fused launch + small torch ops
        state = out["next_state"]
"""
from __future__ import annotations

from typing import Any, Dict, Optional

import torch

from .config import ERR_UNSUPPORTED, STEP_MY_STEP, STEP_MY_STEP_CH
from .vec_env import DiralError, driver_shape


def calculate_ia_penalty(ia: torch.Tensor) -> torch.Tensor:
    """utils/misc.py:1-12: sum over bins of (i+1)*ia[i] (bins with ia > 0);
    ia [..., 100] integer -> [...] int64."""
    ia = torch.as_tensor(ia).to(torch.int64)
    w = torch.arange(1, ia.shape[-1] + 1, dtype=torch.int64, device=ia.device)
    return (torch.clamp(ia, min=0) * w).sum(-1)


def np_sum_lastdim(a: torch.Tensor) -> torch.Tensor:
    """Sum over the last axis in NumPy's order (`np.sum(reward)`, main_test.py:171):
    numpy/_core/src/umath/loops_utils.h pairwise_sum - fewer than 8 elements
    sequentially, otherwise eight running accumulators combined as
    ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) plus a sequential tail, blocks above 128
    elements split recursively.  Float addition is not associative; keeping the
    order keeps the driver's shaped rewards bit-identical."""
    n = a.shape[-1]
    if n < 8:
        res = torch.zeros_like(a[..., 0])
        for i in range(n):
            res = res + a[..., i]
        return res
    if n <= 128:
        r = [a[..., j] for j in range(8)]
        i = 8
        while i < n - (n % 8):
            for j in range(8):
                r[j] = r[j] + a[..., i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res = res + a[..., i]
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return np_sum_lastdim(a[..., :n2]) + np_sum_lastdim(a[..., n2:])


class DriverLoop:
    """Call-sequence and reward post-processing of main_test.py:86-236."""

    def __init__(self, env: Any, enable_channel: bool = False, global_reward_avg: bool = False,
                 ia_averaging: bool = False, ia_penalty_enable: bool = False, ia_penalty_threshold: int = 5,
                 ia_penalty_value: float = -10, episode_interval: int = 25,
                 eps_init: float = 0.99, eps_decay: float = 0.9992, eps_min: float = 0.001,
                 fused: bool = False, device_shaping: Optional[bool] = None):
        self.env = env
        self.enable_channel = enable_channel                  # main_test.py:40
        self.global_reward_avg = global_reward_avg            # :38
        self.ia_averaging = ia_averaging                      # :43
        self.ia_penalty_enable = ia_penalty_enable            # :42
        self.ia_penalty_threshold = ia_penalty_threshold      # :50
        self.ia_penalty_value = ia_penalty_value              # :51
        self.episode_interval = episode_interval              # :31
        self.eps, self.eps_decay, self.eps_min = eps_init, eps_decay, eps_min   # algorithms/policies.py:38-77
        # fused=True: my_step + obtain_state in ONE launch (VecV2VEnv.step semantics; same
        # values, but the channel observation `obs` is not materialised)
        self.fused = fused
        # device_shaping: the reward post-processing of a slot as ONE launch of `diral_driver_shape`
        # (include/diral_env.h) instead of ~70 small torch ops; None = whenever the env is the HIP one.
        # The torch statement below stays: it is what runs on the CPU (oracle-backed tests) and what the
        # kernel is tested against.
        self.device_shaping = (hasattr(env, "lib") and hasattr(env, "_stream")) if device_shaping is None else device_shaping
        # the env rotates >= 2 output-buffer sets (VecV2VEnv(io_ring=2)): what a slot returns stays intact
        # during the next slot, no defensive copies
        self._own_outputs = getattr(env, "io_ring", 1) < 2
        self.episode = 0
        self.N = env.get_total_users()
        self.A = env.get_action_space()
        self._rews0: Optional[torch.Tensor] = None
        self._sum_ia_prev: Optional[torch.Tensor] = None
        self._pen_counter: Optional[torch.Tensor] = None
        self._prev_actions: Optional[torch.Tensor] = None
        self._keep: tuple = ()                # what the last `diral_driver_shape` launch's raw pointers refer to

    @staticmethod
    def _t(x) -> torch.Tensor:
        return x if isinstance(x, torch.Tensor) else torch.as_tensor(x)

    def _actions(self, a) -> torch.Tensor:
        a = self._t(a)
        return a if a.dim() == 2 else a.unsqueeze(0)

    # main_test.py:89-94
    def bootstrap(self, action=None) -> torch.Tensor:
        action = self.env.sample() if action is None else action
        obs, rews = self.env.my_step(action, 0)
        state = self._t(self.env.obtain_state(obs, action, rews)).clone()
        self._rews0 = self._t(rews).clone()
        return state

    # main_test.py:99-114 (the stored reward is the stale bootstrap `rews`, :110-112)
    def prefill_step(self, action) -> torch.Tensor:
        if self.enable_channel:
            obs, _ = self.env.my_step_ch(action, 0)
        else:
            obs, _ = self.env.my_step_design(action, 0)
        return self._t(self.env.obtain_state(obs, action, self._rews0)).clone()

    # main_test.py:99-114 as a whole: K random slots, every state kept (what the loop hands to memory.add)
    def prefill(self, slots: int, seed: int, memory=None):
        """``for k in range(slots): a = env.sample(seed + k); states[k] = prefill_step(a)``: returns
        ``(states [K, B, N, S], actions [K, B, N])``.  On the HIP env this is ONE launch (`VecV2VEnv.prefill` ->
        `diral_env_prefill_mode`, my_step_design or - `enable_channel` - my_step_ch: the env stays on the chip for the K
        slots); configurations that launch does not take - and any other env - run the loop.

        `memory` (a :class:`diral_amd.ReplayMemory`): the K transitions are stored in it with the bootstrap's stale
        rewards (main_test.py:110-112) - by the launch itself where the env takes that (`VecV2VEnv.prefill(memory=)`),
        otherwise by this call's usual form followed by ``memory.add_prefill``: the same rings either way.  Returns
        ``(None, None)`` then."""
        env = self.env
        if memory is not None:
            if hasattr(env, "prefill") and hasattr(env, "lib"):
                try:
                    env.prefill(env.sample(seed), slots, seed, rew_in=self._rews0, memory=memory,
                                mode="my_step_ch" if self.enable_channel else "my_step_design")
                    return None, None
                except DiralError as exc:
                    if exc.status != ERR_UNSUPPORTED:
                        raise
            states, acts = self.prefill(slots, seed)
            dev = memory.device
            memory.add_prefill(self._t(states).to(dev).contiguous(), self._t(acts).to(device=dev, dtype=torch.int32).contiguous(),
                               self._t(self._rews0).to(dev).contiguous())
            return None, None
        if hasattr(env, "prefill"):
            try:
                if self.enable_channel:
                    states, acts, _ = env.prefill(env.sample(seed), slots, seed, rew_in=self._rews0, mode="my_step_ch")
                else:
                    states, acts, _ = env.prefill(env.sample(seed), slots, seed, rew_in=self._rews0)
                return states, acts
            except DiralError as exc:
                if exc.status != ERR_UNSUPPORTED:
                    raise
        states, acts = [], []
        for k in range(int(slots)):
            a = env.sample(seed + k)
            acts.append(self._t(a).clone())
            states.append(self.prefill_step(a))
        return torch.stack(states), torch.stack(acts)

    # main_test.py:127-136: where a slot's actions come from
    def act(self, q, time_step: int, episode: int, policy: Any, explore_step: int, greedy_step: int) -> torch.Tensor:
        """The three-way choice of the reference's slot loop: uniform draws (``policy="explore"``, `env.sample`) while
        `time_step` < `explore_step`, the exploration policy over the Q-values `q` [B, N, A] (`policy.act`, a
        :class:`QPolicy`) while `time_step` < `greedy_step`, ``np.argmax`` (``policy="greedy"``) behind it."""
        if time_step < explore_step:
            return self.env.sample()
        if time_step < greedy_step:
            return policy.act(q, episode=episode, time_slot=time_step)
        return policy.greedy(q)

    # main_test.py:119-236, everything between the agent's action and memory.add
    def slot(self, action, time_step: int, want_ia: Optional[bool] = None) -> Dict[str, Any]:
        env = self.env
        fused_state = None
        if self.fused:
            mode = STEP_MY_STEP_CH if self.enable_channel else STEP_MY_STEP
            fused_state, reward, _ = env._step(mode, env._actions(action), time_step, self.episode, self.eps)
            obs = None
        elif self.enable_channel:
            obs, reward = env.my_step_ch(action, time_step)                  # :144
        else:
            obs, reward = env.my_step(action, time_step)                     # :146
        reward_ret = reward                      # as returned: what main_test.py:164 hands to obtain_state
        reward = self._t(reward)
        if self._own_outputs:
            reward = reward.clone()
        raw = reward.clone() if self._own_outputs else reward    # (nothing below writes `reward` in place)
        out: Dict[str, Any] = {}
        need_ia = self.ia_averaging if want_ia is None else want_ia
        ia_penalty = None
        if need_ia:
            ia = self._t(env.info_age(time_step))                            # :150
            out["ia"] = ia
        if need_ia and not self.device_shaping:
            ia_sum = calculate_ia_penalty(ia)                                # :151
            out["ia_sum"] = ia_sum
            if self.ia_averaging:                                            # :153-160
                prev = self._sum_ia_prev if self._sum_ia_prev is not None else torch.zeros_like(ia_sum)
                ia_penalty = torch.where(ia_sum > prev, -1, torch.where(ia_sum < prev, 1, 0)).to(reward.dtype)
                self._sum_ia_prev = ia_sum
                out["ia_penalty"] = ia_penalty
        if fused_state is not None:
            next_state = fused_state.clone() if self._own_outputs else fused_state
        else:
            # (the returned tensors, unmodified: VecV2VEnv then serves the state its fused launch
            # already built instead of a second launch)
            next_state = self._t(env.obtain_state(obs, action, reward_ret, self.episode, self.eps))   # :164
            if self._own_outputs:
                next_state = next_state.clone()
        a = self._actions(action).to(reward.device)
        if self.device_shaping:
            reward, sum_r, collision, pen, ia_sum = self._shape_on_device(reward, a, out.get("ia"))
            if ia_sum is not None:
                out["ia_sum"] = ia_sum
            if pen is not None:
                out["ia_penalty"] = pen
        else:
            sum_r = np_sum_lastdim(reward)                                       # :171 (NumPy's summation order)
            collision = self.A - sum_r                                           # :178
            if ia_penalty is not None:
                reward = reward + ia_penalty.unsqueeze(-1)                       # :190-192
            if self.ia_penalty_enable:                                           # :194-203
                if self._pen_counter is None:
                    self._pen_counter = torch.zeros_like(a, dtype=torch.int64)
                    self._prev_actions = torch.full_like(a, -1)
                stuck = (reward < 1) & (a == self._prev_actions)
                self._pen_counter = torch.where(stuck, self._pen_counter + 1, torch.zeros_like(self._pen_counter))
                reward = torch.where(self._pen_counter > self.ia_penalty_threshold,
                                     torch.as_tensor(float(self.ia_penalty_value), dtype=reward.dtype, device=reward.device),
                                     reward)
                self._prev_actions = a.clone()
            if self.global_reward_avg:
                # (tensor / tensor: a true IEEE division like Python's `sum_r / len(reward)`; tensor / Python scalar
                # is computed on the GPU as a multiplication by the rounded reciprocal - one ulp off unless N is a
                # power of two)
                n_t = torch.as_tensor(float(self.N), dtype=reward.dtype, device=reward.device)
                reward = reward + (sum_r / n_t).unsqueeze(-1)                    # :205-206
        episode_end = (time_step % self.episode_interval) == self.episode_interval - 1   # :226
        out.update(next_state=next_state, reward=reward, raw_reward=raw, sum_r=sum_r, collision=collision,
                   episode_end=episode_end, episode=self.episode, eps=self.eps)
        return out

    # K slots of main_test.py:119-236 with the actions given in advance (a replayed log, a fixed schedule)
    def rollout(self, actions_seq, t: int, states: Optional[str] = "last", vel_seed: int = 0,
                positions=None, memory=None) -> Dict[str, Any]:
        """``for k in range(K): out = slot(actions_seq[k], t + k)`` and, behind a slot that ends an episode,
        ``env.update_velocity(seed=vel_seed + (t + k) // episode_interval)``: returns ``states`` (the last slot's
        [B, N, S]; `states` = ``"all"``: every slot's [K, B, N, S]; None: none), ``reward`` [B, N] (as the env returned it)
        and ``done`` [B] of the last slot, ``shaped`` [K, B, N], ``sum_r`` / ``collision`` [K, B].  On the HIP env this is
        ONE launch (`VecV2VEnv.rollout` -> `diral_env_rollout`); configurations that launch does not take, the
        information-age terms of a my_step driver - and any other env - run the loop.  The loop's episode counter and
        epsilon stay where they are (`end_episode` is the caller's): every slot's fingerprint columns carry the current ones.

        `enable_channel` on a HIP env with `track_arrival` (the driver reads the information age behind every slot,
        main_test.py:150): the launch carries the information-age block (`diral_env_rollout_ia`) - `ia_averaging` included -
        and the result gains ``ia`` [K, B, 100], ``ia_sum`` [K, B] and, with `ia_averaging`, ``ia_penalty`` [K, B]; the loop
        behind a refused launch stacks what ``slot(want_ia=True)`` returns.

        `positions` ([T, N] or [B, T, N] float64): recorded mobility for these K slots, main_test.py:118's
        `load_saved_positions` - inside the launch where it is taken (`diral_env_rollout_replay`); behind a refused launch
        the sequence is set on the handle (`load_saved_positions`), the slots are looped and the trace is removed again.
        ValueError if the handle already carries a trace: one source of positions per call.

        `memory` (a :class:`diral_amd.ReplayMemory`): the K transitions - every slot's state, actions and shaped reward -
        are stored in it, by the launch itself where the env takes that (`VecV2VEnv.rollout(memory=)`: no [K]-major
        scratch, no second launch); where it does not (N > 64, an unpinned toy handle, fingerprint columns, any other
        env) this call runs with ``states="all"`` and ``memory.add_rollout`` follows: the same rings either way.
        `states` is not read; ``shaped`` is None in the result and ``states`` the memory's last state row (None when
        it counts on the device)."""
        env = self.env
        seq = self._t(actions_seq)
        K = int(seq.shape[0])
        hip = hasattr(env, "lib") and hasattr(env, "_stream")
        direct = memory is not None and hip and not env.cfg.enable_fingerprint
        if memory is not None and not direct:
            return self._rollout_then_add(seq, t, vel_seed, positions, memory)
        if positions is not None:
            if not hip:
                raise ValueError("DriverLoop.rollout: positions needs the HIP env")
            if env.has_trace:
                raise ValueError("DriverLoop.rollout: the env already replays a trace of its own (load_saved_positions)")
            positions = env._positions("DriverLoop.rollout", positions)
        with_ia = bool(self.enable_channel and getattr(getattr(env, "cfg", None), "track_arrival", False))
        if hasattr(env, "rollout") and ((with_ia and hip) or not self.ia_averaging):
            pen = None
            if self.ia_penalty_enable:
                if self._pen_counter is None:
                    self._pen_counter = torch.zeros((env.B, env.N), dtype=torch.int32, device=env.device)
                    self._prev_actions = torch.full((env.B, env.N), -1, dtype=torch.int32, device=env.device)
                pen = (int(self.ia_penalty_threshold), float(self.ia_penalty_value), self._pen_counter, self._prev_actions)
            ia_kw = {}
            if with_ia and hip:
                if self.ia_averaging and self._sum_ia_prev is None:
                    self._sum_ia_prev = torch.zeros((env.B,), dtype=torch.int64, device=env.device)
                ia_kw = dict(info_age=True, sum_ia_prev=self._sum_ia_prev if self.ia_averaging else None)
            if positions is not None:
                ia_kw["positions"] = positions
            if direct:
                ia_kw["memory"] = memory
            try:
                out = env.rollout(seq, t, mode="my_step_ch" if self.enable_channel else "my_step", states=states,
                                  global_reward_avg=self.global_reward_avg, stuck_penalty=pen, vel_seed=vel_seed, **ia_kw)
                if "ia_penalty" in out:                                          # (as slot() reports it)
                    out["ia_penalty"] = out["ia_penalty"].to(out["sum_r"].dtype)
                if out["states"] is not None and env.cfg.enable_fingerprint:     # test_env.py:577-579
                    out["states"][..., env._fp_offset] = self.episode
                    out["states"][..., env._fp_offset + 1] = self.eps
                return out
            except DiralError as exc:
                if exc.status != ERR_UNSUPPORTED:
                    raise
        if memory is not None:                   # (the launch was refused, or this driver's terms keep it from being tried)
            return self._rollout_then_add(seq, t, vel_seed, positions, memory)
        if positions is None:
            return self._rollout_loop(seq, t, states, vel_seed, with_ia)
        env.load_saved_positions(positions)
        try:
            return self._rollout_loop(seq, t, states, vel_seed, with_ia)
        finally:
            env.load_saved_positions(None)

    def _rollout_then_add(self, seq, t: int, vel_seed: int, positions, memory) -> Dict[str, Any]:
        """`rollout(memory=)` in two calls: every slot's state kept, then ``memory.add_rollout``."""
        out = self.rollout(seq, t, states="all", vel_seed=vel_seed, positions=positions)
        dev = memory.device
        if seq.dim() == 2:                                               # ([K, N]: every env alike)
            seq = seq.unsqueeze(1).expand(seq.shape[0], memory.B, memory.N)
        memory.add_rollout(seq.to(device=dev, dtype=torch.int32).contiguous(),
                           dict(states=self._t(out["states"]).to(dev).contiguous(), shaped=self._t(out["shaped"]).to(dev).contiguous()))
        last = None if memory.count_dev is not None else memory.states[memory.count % (memory.C + 1)]
        return dict(out, states=last, shaped=None)

    def _rollout_loop(self, seq, t: int, states: Optional[str], vel_seed: int, with_ia: bool) -> Dict[str, Any]:
        """`rollout` slot by slot: what its launch is equal to."""
        env = self.env
        K = int(seq.shape[0])
        kept, shaped, sum_r, coll = [], [], [], []
        ia_keys = ("ia", "ia_sum", "ia_penalty")
        ia_kept: Dict[str, list] = {k: [] for k in ia_keys}
        out: Dict[str, Any] = {}
        for k in range(K):
            out = self.slot(seq[k], t + k, want_ia=True if with_ia else None)
            if with_ia:
                for key in ia_keys:
                    if key in out:
                        ia_kept[key].append(self._t(out[key]).clone())
            if states == "all":
                kept.append(self._t(out["next_state"]).clone())
            shaped.append(self._t(out["reward"]).clone())
            sum_r.append(self._t(out["sum_r"]).clone())
            coll.append(self._t(out["collision"]).clone())
            if out["episode_end"]:
                env.update_velocity(seed=vel_seed + (t + k) // self.episode_interval)
        raw = self._t(out["raw_reward"])
        done = torch.full((raw.shape[0],), 1 if out["episode_end"] else 0, dtype=torch.uint8, device=raw.device)
        st = None if states is None else (torch.stack(kept) if states == "all" else self._t(out["next_state"]))
        return dict(states=st, reward=raw, done=done, shaped=torch.stack(shaped), sum_r=torch.stack(sum_r),
                    collision=torch.stack(coll), **{key: torch.stack(v) for key, v in ia_kept.items() if v})

    def _shape_on_device(self, reward: torch.Tensor, a: torch.Tensor, ia: Optional[torch.Tensor]):
        """main_test.py:171-206 through `diral_driver_shape` (one launch)."""
        B, N = reward.shape
        dev = reward.device
        reward = reward.contiguous()
        a32 = a.to(torch.int32).contiguous()
        if self.ia_averaging and self._sum_ia_prev is None:
            self._sum_ia_prev = torch.zeros((B,), dtype=torch.int64, device=dev)
        if self.ia_penalty_enable and self._pen_counter is None:
            self._pen_counter = torch.zeros((B, N), dtype=torch.int32, device=dev)
            self._prev_actions = torch.full((B, N), -1, dtype=torch.int32, device=dev)
        shaped = torch.empty_like(reward)
        sum_r = torch.empty((B,), dtype=reward.dtype, device=dev)
        coll = torch.empty((B,), dtype=reward.dtype, device=dev)
        pen = torch.zeros((B,), dtype=torch.int32, device=dev) if (self.ia_averaging and ia is not None) else None
        ia32 = None if ia is None else ia.to(torch.int32).contiguous()
        ia_sum = None if ia is None else torch.empty((B,), dtype=torch.int64, device=dev)
        # (the information-age term only when this slot fetched the histogram: slot(..., want_ia=False) with
        # ia_averaging skips it, exactly like the torch statement in slot())
        use_ia = self.ia_averaging and ia is not None
        pen_on = self.ia_penalty_enable
        driver_shape(self.env, reward, a32, shaped=shaped, sum_r=sum_r, collision=coll, global_reward_avg=self.global_reward_avg,
                     ia=ia32, sum_ia_prev=self._sum_ia_prev if use_ia else None, ia_sum=ia_sum, ia_penalty=pen,
                     pen_counter=self._pen_counter if pen_on else None, prev_actions=self._prev_actions if pen_on else None,
                     pen_threshold=self.ia_penalty_threshold, pen_value=self.ia_penalty_value)
        self._keep = (reward, a32, ia32)
        return shaped, sum_r, coll, (pen.to(reward.dtype) if pen is not None else None), ia_sum

    # main_test.py:226-233: call when out["episode_end"]; `draws` are the
    # random.randrange(1,4) values of Network.update_velocity (None = device RNG)
    def end_episode(self, draws=None) -> None:
        self.episode += 1
        self.eps = max(self.eps * self.eps_decay, self.eps_min)
        if draws is None:
            self.env.update_velocity()
        else:
            self.env.update_velocity(draws)
