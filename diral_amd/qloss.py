"""TD targets, the hysteretic loss and its gradient on the device: the learning side's glue around a torch Q-network.

The reference's training step runs the target and the eval net on ``next_states``, builds the target in NumPy
(``DRQN._calc_target``, algorithms/drl_drqn.py:267-292: the arg-max, the gather, ``r + gamma * next`` in mixed
float32 / float64) and feeds it to the loss head (:76-80: the one-hot gather of ``Q(s, a)``, the TD error, the hysteretic
``where(h < 0, h / 10, h)``, the mean of squares).  :class:`QLoss` is both as ONE launch of ``diral_td_head``
(include/diral_env.h, where the arithmetic is pinned rule by rule) that also leaves dL/dQ, so that autograd has one node
between the loss and the network's output.  The next-state Q-values are constants, as a fed NumPy target is in the
reference.  No network, no optimiser, no replay memory.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch

from . import _lib
from ._tensors import MSG_OUT, _ptr, check_tensor, dtype_code
from .config import DT_BF16, DT_F16, DT_F32
from .vec_env import check_status

Q_DTYPES = {torch.float32: DT_F32, torch.float16: DT_F16, torch.bfloat16: DT_BF16}
R_DTYPES = (torch.float32, torch.float64)


class _TdLoss(torch.autograd.Function):
    """loss = mean(hl^2) with d loss / d q kept from the forward launch; every other input is a constant."""

    @staticmethod
    def forward(ctx, q, head, actions, rewards, q_next_target, q_next_eval):
        loss, grad_q = head._launch(q.detach(), actions, rewards, q_next_target, q_next_eval)
        ctx.save_for_backward(grad_q)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        (grad_q,) = ctx.saved_tensors
        return grad_q * grad_output.to(grad_q.dtype), None, None, None, None, None


class QLoss:
    """``gamma``, ``double`` (``use_double``: the arg-max comes from the eval net's next Q-values) and ``hysteretic`` are
    the reference agent's.  `last_td` (``hl`` [rows]), `last_targets` [rows], `last_next_actions` [rows] hold the last
    call's; `bad_rows` counts the rows whose action was outside ``[0, A)`` (Q = 0 and no gradient there, as tf.one_hot)."""

    def __init__(self, gamma: float = 0.99, double: bool = True, hysteretic: bool = False, device="cuda:0"):
        if not math.isfinite(float(gamma)):
            raise ValueError("gamma must be finite")
        self.lib = _lib.load()
        self.gamma, self.double, self.hysteretic = float(gamma), bool(double), bool(hysteretic)
        self.device = torch.device(device)
        self.bad_rows = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self.last_td: Optional[torch.Tensor] = None
        self.last_targets: Optional[torch.Tensor] = None
        self.last_next_actions: Optional[torch.Tensor] = None
        self._keep: tuple = ()                        # what the last launch's raw pointers refer to

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _next(self, q_next_target, rewards, q_next_eval):
        """Checks of what both calls take -> (rows, A)."""
        if not isinstance(q_next_target, torch.Tensor) or q_next_target.dim() != 2 or q_next_target.dtype not in Q_DTYPES:
            raise ValueError("q_next_target must be a float32 / float16 / bfloat16 tensor [rows, A]")
        rows, A = (int(v) for v in q_next_target.shape)
        if rows < 1 or A < 1:
            raise ValueError("q_next_target must be a float32 / float16 / bfloat16 tensor [rows, A]")
        check_tensor("q_next_target", q_next_target, q_next_target.dtype, (rows, A), self.device, MSG_OUT)
        if self.double:
            if q_next_eval is None:
                raise ValueError("QLoss(double=True) needs q_next_eval, the eval net's Q-values of next_states")
            check_tensor("q_next_eval", q_next_eval, q_next_target.dtype, (rows, A), self.device, MSG_OUT)
        if not isinstance(rewards, torch.Tensor) or rewards.dtype not in R_DTYPES:
            raise ValueError("rewards must be a float32 or float64 tensor [rows]")
        check_tensor("rewards", rewards, rewards.dtype, (rows,), self.device, MSG_OUT)
        return rows, A

    def _call(self, rows, A, q, q_next_target, q_next_eval, actions, rewards, td, grad_q, loss):
        targets = torch.empty((rows,), dtype=torch.float32, device=self.device)
        nxt = torch.empty((rows,), dtype=torch.int32, device=self.device)
        qe = q_next_eval if self.double else None     # (double=False: the plain target, whatever was handed over)
        acts = nxt if actions is None else actions    # without q the launch does not read them
        check_status(self.lib.diral_td_head(rows, A, _ptr(q), _ptr(q_next_target), _ptr(qe), Q_DTYPES[q_next_target.dtype],
                                            _ptr(acts), _ptr(rewards), dtype_code(rewards), self.gamma, int(self.hysteretic),
                                            _ptr(targets), _ptr(td), _ptr(nxt), _ptr(grad_q), _ptr(loss),
                                            _ptr(self.bad_rows), self._stream()), "diral_td_head")
        self._keep = (q, q_next_target, qe, actions, rewards, td, grad_q, loss)
        self.last_targets, self.last_next_actions = targets, nxt
        return targets

    def targets(self, q_next_target: torch.Tensor, rewards: torch.Tensor,
                q_next_eval: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``_calc_target(rewards, next_states)`` from the two nets' Q-values of ``next_states`` ``[rows, A]`` and the
        last step's rewards ``[rows]`` (``sample(last_only=True)``'s): ``[rows]`` float32, what the float32 placeholder
        holds."""
        rows, A = self._next(q_next_target, rewards, q_next_eval)
        return self._call(rows, A, None, q_next_target, q_next_eval, None, rewards, None, None, None)

    def _launch(self, q, actions, rewards, q_next_target, q_next_eval):
        rows, A = self._next(q_next_target, rewards, q_next_eval)
        check_tensor("q", q, q_next_target.dtype, (rows, A), self.device, MSG_OUT)
        check_tensor("actions", actions, torch.int32, (rows,), self.device)
        td = torch.empty((rows,), dtype=torch.float32, device=self.device)
        grad_q = torch.empty((rows, A), dtype=q.dtype, device=self.device)
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        self._call(rows, A, q, q_next_target, q_next_eval, actions, rewards, td, grad_q, loss)
        self.last_td = td
        return loss, grad_q

    def loss(self, q: torch.Tensor, actions: torch.Tensor, rewards: torch.Tensor, q_next_target: torch.Tensor,
             q_next_eval: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``self.loss`` of the reference's graph (drl_drqn.py:76-80) on targets built as `targets` builds them: a 0-d
        float32 tensor with a ``grad_fn``.  ``q`` ``[rows, A]`` is the eval net on ``states``, ``actions`` ``[rows]``
        int32; ``backward`` hands ``q`` the gradient the forward launch left (times the incoming one) and nothing to the
        next-state Q-values."""
        return _TdLoss.apply(q, self, actions, rewards, q_next_target, q_next_eval)
