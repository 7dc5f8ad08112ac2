"""Actions from Q-values on the device: the exploration policies of the reference's agent.

The reference's driver takes a slot's actions from ``env.sample`` (``policy="explore"``), from the agent's exploration
policy over its Q-values, or from ``np.argmax`` (``policy="greedy"``) - main_test.py:127-136.  :class:`QPolicy` is the
second and the third for ``Q[B, N, A]`` out of a PyTorch network: ``GreedyPolicy``, ``EpsilonGreedy``, ``SoftmaxPolicy``
and ``BoltzmanPolicy`` of algorithms/policies.py as ONE launch of ``diral_policy_select`` (include/diral_env.h), with
their host-side schedules kept here.  The draws are a function of (seed, draw counter, global agent index): they do not
touch torch's generator, shards of a batch draw what the whole batch draws (`env_offset`), and the clocked form draws
afresh at every replay of a captured graph.  No network, no training, no replay memory.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._tensors import MSG_OUT, _ptr, check_tensor, policy_seed
from .config import (DT_BF16, DT_F16, DT_F32, DT_F64, SELECT_BOLTZMANN, SELECT_EPS_GREEDY, SELECT_GREEDY, SELECT_SOFTMAX,
                     DiralSelect)
from .vec_env import check_status

KINDS = {"greedy": SELECT_GREEDY, "eps_greedy": SELECT_EPS_GREEDY, "softmax": SELECT_SOFTMAX, "boltzmann": SELECT_BOLTZMANN}
Q_DTYPES = {torch.float64: DT_F64, torch.float32: DT_F32, torch.float16: DT_F16, torch.bfloat16: DT_BF16}


class QPolicy:
    """``kind``: "greedy", "eps_greedy" (`eps_init`, `eps_decay`), "softmax" (`temperature`, `episodes`) or "boltzmann"
    (`beta`, `explore_start`, `explore_stop`, `decay_rate`, `alpha`); the defaults are the reference's."""

    def __init__(self, batch: int, num_users: int, num_channels: int, kind: str = "eps_greedy", *, seed: int = 0,
                 env_offset: int = 0, device="cuda:0", eps_init: float = 0.99, eps_decay: float = 0.999,
                 temperature: float = 0.05, episodes: int = 1000, beta: float = 1.0, explore_start: float = 0.02,
                 explore_stop: float = 0.01, decay_rate: float = 0.0001, alpha: float = 0.0):
        if kind not in KINDS:
            raise ValueError("kind must be one of %s" % sorted(KINDS))
        self.lib = _lib.load()
        self.B, self.N, self.A = int(batch), int(num_users), int(num_channels)
        self.kind, self.seed, self.env_offset = kind, int(seed), int(env_offset)
        self.device = torch.device(device)
        self.eps, self.eps_decay, self.episode = float(eps_init), float(eps_decay), 0          # policies.py:39-43
        self.temperature, self.tmp = float(temperature), None                                  # :80-90
        n_geo = int(episodes * 2.0 / 3)
        self.temperature_list = np.concatenate((np.geomspace(1.0, temperature, n_geo), np.repeat(temperature, episodes - n_geo)))
        self.beta, self.alpha = float(beta), float(alpha)                                      # :136-142
        self.explore_start, self.explore_stop, self.decay_rate = float(explore_start), float(explore_stop), float(decay_rate)
        self.explore_p: Optional[float] = None
        self.bad_rows = torch.zeros((1,), dtype=torch.int32, device=self.device)   # SOFTMAX rows answered by the greedy rule
        self._t = 0                                   # draw counter: the call number `k` draws with policy_seed(seed, k)
        self._keep: tuple = ()                        # what the last launch's raw pointers refer to

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def get_epsilon(self):
        """policies.py:65-69, 114-118: eps, or the softmax's current temperature."""
        return self.tmp if self.kind == "softmax" else self.eps

    def set_epsilon(self, eps: float) -> None:
        self.eps = float(eps)                         # policies.py:71-77

    # ---- the reference's host-side schedules: what one call would set, committed once the launch is in ----
    def _schedule(self, episode, time_slot) -> dict:
        if self.kind == "eps_greedy" and episode is not None and episode > self.episode:       # policies.py:46-48, 56-63
            return dict(eps=max(self.eps * self.eps_decay, 0.001), episode=episode)
        if self.kind == "softmax":                                                             # :93-96
            try:
                return dict(tmp=self.temperature if episode is None else float(self.temperature_list[episode]))
            except IndexError:
                return dict(tmp=self.temperature)
        if self.kind == "boltzmann":                                                           # :153-159
            if time_slot is None:
                raise ValueError("QPolicy(kind='boltzmann').act needs time_slot")
            new = {}
            if time_slot % 50 == 0 and time_slot < 5000:
                new["beta"] = self.beta - 0.001
            new["explore_p"] = float(self.explore_stop + (self.explore_start - self.explore_stop)
                                     * np.exp(-self.decay_rate * time_slot))
            return new
        return {}

    def _launch(self, where: str, q: torch.Tensor, out, explored, *, kind=None, draw_u=None, draw_a=None, seed=0, clock=None,
                offset=0, param=None, **sched) -> torch.Tensor:
        if not isinstance(q, torch.Tensor) or q.dtype not in Q_DTYPES:
            raise ValueError("q must be a float64 / float32 / float16 / bfloat16 tensor [B, N, A]")
        check_tensor("q", q, q.dtype, (self.B, self.N, self.A), self.device, MSG_OUT)
        if out is None:
            out = torch.empty((self.B, self.N), dtype=torch.int32, device=self.device)
        check_tensor("out", out, torch.int32, (self.B, self.N), self.device, MSG_OUT)
        if explored is not None:
            check_tensor("explored", explored, torch.uint8, (self.B, self.N), self.device, MSG_OUT)
        if draw_u is not None:
            draw_u = torch.as_tensor(draw_u, dtype=torch.float64, device=self.device).reshape(self.B, self.N).contiguous()
        if draw_a is not None:
            draw_a = torch.as_tensor(draw_a, dtype=torch.int32, device=self.device).reshape(self.B, self.N).contiguous()
        if param is not None:
            if param.dtype != torch.float64 or param.device != self.device or not param.is_contiguous() \
                    or param.numel() not in (1, self.B):
                raise ValueError("param must be a contiguous float64 tensor of 1 or B values on %s" % self.device)
        s = DiralSelect()
        s.struct_bytes = ctypes.sizeof(DiralSelect)
        s.kind = KINDS[self.kind] if kind is None else kind
        s.agents, s.num_users, s.num_channels = self.B * self.N, self.N, self.A
        s.q, s.q_dtype = _ptr(q), Q_DTYPES[q.dtype]
        s.eps = sched.get("eps", self.eps)
        s.tmp = sched.get("tmp", self.temperature if self.tmp is None else self.tmp)
        s.beta, s.alpha = sched.get("beta", self.beta), self.alpha
        s.explore_p = sched.get("explore_p", self.explore_stop if self.explore_p is None else self.explore_p)
        s.param_dev, s.param_per_env = _ptr(param), int(param is not None and param.numel() == self.B and self.B > 1)
        s.draw_u, s.draw_a = _ptr(draw_u), _ptr(draw_a)
        s.seed, s.idx0 = seed, self.env_offset * self.N
        s.clock, s.clock_offset = _ptr(clock), int(offset)
        s.actions_out, s.explored_out, s.bad_rows = _ptr(out), _ptr(explored), _ptr(self.bad_rows)
        check_status(self.lib.diral_policy_select(ctypes.byref(s), self._stream()), where)
        self._keep = (q, out, explored, draw_u, draw_a, param, clock)
        return out

    def act(self, q: torch.Tensor, episode=None, time_slot=None, out: Optional[torch.Tensor] = None,
            explored: Optional[torch.Tensor] = None, draw_u=None, draw_a=None) -> torch.Tensor:
        """``Qs`` [B, N, A] -> actions [B, N] int32: ``policy.action(Qs, episode)`` / ``take_action(Qs, time_slot)`` of
        every agent, the schedule advanced once as one call of the reference advances it.  `draw_u` / `draw_a` [B, N]:
        the draws (np.random.random() and randint(A)) given instead of generated; `explored` (uint8 [B, N]): 1 where the
        exploring branch chose.  `episode` None: the schedule stays where it is."""
        sched = self._schedule(episode, time_slot)
        out = self._launch("diral_policy_select", q, out, explored, draw_u=draw_u, draw_a=draw_a,
                           seed=policy_seed(self.seed, self._t + 1), **sched)
        self._t += 1                  # only once the call is in: a refused call leaves the draw counter and the schedule alone
        for k, v in sched.items():
            setattr(self, k, v)
        return out

    def greedy(self, q: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``np.argmax(Qs, axis=1)`` whatever the policy's kind (main_test.py:136, policy="greedy"): no draw is taken."""
        return self._launch("diral_policy_select", q, out, None, kind=SELECT_GREEDY)

    def act_clocked(self, q: torch.Tensor, clock, offset: int = 0, param: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None, explored: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`act` for captured graphs: device draws seeded by policy_seed(seed, offset + *clock) - the call `act` number
        offset + *clock draws alike -, the kind's parameter (eps / temperature / explore_p) as it stands or read from
        `param` (float64, 1 value or [B]: one per env) at every replay.  No host schedule and no counter moves.
        `clock`: a rollout.SlotClock or an int64 device tensor."""
        ct = clock if isinstance(clock, torch.Tensor) else clock.t
        check_tensor("clock", ct, torch.int64, (1,), self.device, MSG_OUT)
        return self._launch("diral_policy_select", q, out, explored, seed=policy_seed(self.seed, 0), clock=ct, offset=offset,
                            param=param)
