"""Candidate search on top of the env copies (`VecV2VEnv.copy_envs_from` -> `diral_env_copy_envs`).

A search over action sequences does three things: put C envs on the state of one, run the C candidates, keep the winner or
throw everything away.  `CandidateSearch` owns a work handle of B * C envs - work env ``b * C + c`` is candidate c of env
b - and does each of the three as one launch: a gather of `env` into `work`, one K-slot rollout of `work`
(`VecV2VEnv.rollout`; the loop of step + `diral_driver_shape` where that launch does not take the configuration), a gather
of the chosen candidates back.  Nothing synchronises with the host, and `env` is untouched until `commit`.

Configs with mobility_vary: device random draws are a function of the GLOBAL env index (include/diral_env.h,
DIRAL_OPT_ENV_OFFSET), so a rollout that crosses an episode end draws each candidate's velocity changes by its own
position in `work` - the candidates of one env then differ in more than their actions, and the committed winner carries
the draw of work env ``b * C + c``, not the one env b itself would have made.

The stuck-action penalty state of a driver (`stuck_penalty` tensors) is the caller's and is not forked here.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .config import ERR_UNSUPPORTED
from .vec_env import _MODES, DiralError, VecV2VEnv, driver_shape


def candidate_index(B: int, C: int, device=None) -> torch.Tensor:
    """[B * C] int32: the env of `env` that work env ``b * C + c`` starts from, i.e. b."""
    return torch.arange(int(B), dtype=torch.int32, device=device).repeat_interleave(int(C))


def winner_index(choice: torch.Tensor, C: int) -> torch.Tensor:
    """[B] int32: the work env that holds candidate ``choice[b]`` of env b, ``b * C + choice[b]``; computed where `choice`
    lives, without synchronising."""
    b = torch.arange(choice.shape[0], dtype=torch.int64, device=choice.device)
    return (b * int(C) + choice.to(torch.int64)).to(torch.int32)


class CandidateSearch:
    def __init__(self, env: VecV2VEnv, candidates: int):
        C = int(candidates)
        if C < 1:
            raise ValueError("CandidateSearch: candidates must be >= 1")
        self.env, self.C = env, C
        self.work = env.twin(env.B * C)
        self._gather = candidate_index(env.B, C, env.device)        # built once, on the device
        self._K = 0

    def evaluate(self, seqs, t: Optional[int] = None, mode="my_step", global_reward_avg: bool = False, vel_seed: int = 0,
                 info_age: bool = False, positions=None) -> Dict[str, torch.Tensor]:
        """Run every candidate: `seqs` [K, B, C, N] int32, ``seqs[k, b, c]`` the actions of env b's candidate c in slot
        ``t + k`` (`t` defaults to ``env.t``).  Returns ``returns`` [B, C] (the sum of `sum_r` over the K slots, float64),
        ``sum_r`` and ``collision`` [K, B, C] (main_test.py:171, 178) - and leaves `env` as it was.  `info_age` (`mode` =
        ``"my_step_ch"`` on a `track_arrival` handle): the rollout of `work` keeps the arrival stamps (`copy_envs_from`
        carries them) and ``ia_sum`` [K, B, C] int64 - utils/misc.calculate_ia_penalty of every candidate's information-age
        histogram behind every slot - is returned beside ``returns``: candidates can be scored by information age.
        `positions`: recorded mobility for the K slots (`VecV2VEnv.rollout`'s `positions`) - [T, N] for every env and
        candidate alike, or [B, T, N], env b's sequence for each of its C candidates (expanded to `work`'s env order here)."""
        env, work, C = self.env, self.work, self.C
        seq = torch.as_tensor(seqs, device=env.device)
        if seq.dim() != 4 or tuple(seq.shape[1:]) != (env.B, C, env.N) or seq.shape[0] < 1:
            raise ValueError("evaluate: seqs must have shape [K >= 1, B=%d, C=%d, N=%d], got %s" % (env.B, C, env.N, tuple(seq.shape)))
        K = int(seq.shape[0])
        seq = seq.to(torch.int32).reshape(K, env.B * C, env.N).contiguous()
        if t is None:
            t = env.t
        pos_kw = {}
        if positions is not None:
            pos = env._positions("evaluate", positions)
            if pos.dim() == 3:                                      # work env b * C + c replays env b's sequence
                pos = pos.repeat_interleave(C, dim=0)
            pos_kw = dict(positions=pos)
        work.copy_envs_from(env, src_index=self._gather)
        try:
            out = work.rollout(seq, t, mode=mode, states=None, global_reward_avg=global_reward_avg, vel_seed=vel_seed,
                               info_age=True if info_age else None, **pos_kw)
            sum_r, coll, ia_sum = out["sum_r"], out["collision"], out.get("ia_sum")
        except DiralError as exc:
            if exc.status != ERR_UNSUPPORTED:                       # (refused: nothing launched, `work` untouched)
                raise
            if positions is None:
                sum_r, coll, ia_sum = self._loop(seq, int(t), _MODES[mode], global_reward_avg, vel_seed, info_age)
            else:                                                   # (the loop replays the sequence from the handle)
                work.load_saved_positions(pos_kw["positions"])
                try:
                    sum_r, coll, ia_sum = self._loop(seq, int(t), _MODES[mode], global_reward_avg, vel_seed, info_age)
                finally:
                    work.load_saved_positions(None)
        self._K = K
        res = dict(returns=sum_r.to(torch.float64).sum(0).view(env.B, C), sum_r=sum_r.view(K, env.B, C),
                   collision=coll.view(K, env.B, C))
        if info_age:
            res["ia_sum"] = ia_sum.view(K, env.B, C)
        return res

    def _loop(self, seq: torch.Tensor, t: int, step_mode: int, global_reward_avg: bool, vel_seed: int, info_age: bool = False):
        """What `rollout` is equal to, slot by slot (as diral_amd.driver.DriverLoop.rollout loops)."""
        work = self.work
        K, EI = int(seq.shape[0]), work.cfg.episode_interval
        o = dict(dtype=work.out_dtype, device=work.device)
        shaped = torch.empty((work.B, work.N), **o)
        sum_r, coll = torch.empty((K, work.B), **o), torch.empty((K, work.B), **o)
        ia_sum = torch.empty((K, work.B), dtype=torch.int64, device=work.device) if info_age else None
        for k in range(K):
            _, rew, _ = work._step(step_mode, seq[k], t + k, want_obs=False)
            ia = work.info_age(t + k) if info_age else None
            driver_shape(work, rew, seq[k], shaped=shaped, sum_r=sum_r[k], collision=coll[k], global_reward_avg=global_reward_avg,
                         ia=ia, ia_sum=None if ia is None else ia_sum[k])
            if (t + k) % EI == EI - 1:
                work.update_velocity(seed=vel_seed + (t + k) // EI)
        work.t = t + K
        return sum_r, coll, ia_sum

    def commit(self, choice) -> None:
        """Keep candidate ``choice[b]`` of every env b ([B] integer tensor, e.g. ``returns.argmax(1)``): `env` becomes
        what `work` holds for it after the K slots of the last `evaluate`, and its slot counter moves on by K."""
        env = self.env
        choice = torch.as_tensor(choice, device=env.device)
        if tuple(choice.shape) != (env.B,):
            raise ValueError("commit: choice must have shape [B=%d], got %s" % (env.B, tuple(choice.shape)))
        env.copy_envs_from(self.work, src_index=winner_index(choice, self.C))
        env.t += self._K
