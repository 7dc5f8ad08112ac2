"""The reference's dense Q-network chain on the device: ``DRQN._create_network`` (algorithms/drl_drqn.py:109-155),
``[matmul + bias -> relu -> layer_norm] x L``, then ``matmul + bias``.

With ``use_lstm_input: false`` (the DQN branch, ``state_vector[-1:, user]``, drl_drqn.py:174) the chain is the whole
Q-network; with ``use_lstm_input: true`` it is the head behind ``lstm_out[:, -1, :]``.  :class:`QNet` keeps every
parameter in ONE flat float32 device tensor (`params`, the blob of ``diral_qnet_forward``, include/diral_env.h, where the
arithmetic is pinned rule by rule) and has two ways through it:

* `forward`: ONE launch of ``diral_qnet_forward``, no ``grad_fn`` - the three evaluations of a training iteration that
  never see a gradient (the acting pass, ``target(next_states)`` and ``net(next_states)`` in ``_calc_target``);
* `torch_module`: an ``nn.Module`` whose parameters are views of the same blob and whose forward is the same chain in
  torch ops - the gradient path, ``net(states)``.  An optimiser step through it updates the blob in place, and the next
  `forward` launch reads the new weights: no copy in either direction.

No launch of the LSTM cell (its parameters and gradient path are diral_amd/lstm.py), no backward kernel, no optimiser.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence

import torch

from . import _lib
from ._tensors import MSG_OUT, _ptr, check_tensor
from .config import DT_BF16, DT_F16, DT_F32
from .vec_env import check_status

X_DTYPES = {torch.float32: DT_F32, torch.float16: DT_F16, torch.bfloat16: DT_BF16}
MAX_HIDDEN, MAX_IN, MAX_WIDTH = 3, 1024, 256


def layout(widths: Sequence[int]) -> Dict[str, tuple]:
    """{name: (offset, shape)} of the blob of a chain ``[D, h_1 .. h_L, A]``: per hidden layer ``W [in, out]``, ``b``,
    ``gamma``, ``beta``, then ``W_out``, ``b_out`` - the order ``diral_qnet_forward`` reads."""
    views, off, L = {}, 0, len(widths) - 2
    for l in range(L + 1):
        i, o = int(widths[l]), int(widths[l + 1])
        names = ("W%d" % (l + 1), "b%d" % (l + 1), "gamma%d" % (l + 1), "beta%d" % (l + 1)) if l < L else ("W_out", "b_out")
        for k, name in enumerate(names):
            shape = (i, o) if k == 0 else (o,)
            views[name] = (off, shape)
            off += i * o if k == 0 else o
    return views


def blob_len(widths: Sequence[int]) -> int:
    off, shape = list(layout(widths).values())[-1]
    return off + shape[0]


class _Chain(torch.nn.Module):
    """The chain in torch ops over parameters that are views of a QNet's blob."""

    def __init__(self, net: "QNet"):
        super().__init__()
        self.L, self.norm, self.eps = net.L, net.norm, net.ln_eps
        for name, view in net.views().items():
            param = torch.nn.Parameter(view)                 # shares the blob's storage
            assert param.data_ptr() == view.data_ptr()
            self.register_parameter(name, param)

    def forward(self, x):
        h = x.to(torch.float32)
        for l in range(1, self.L + 1):
            h = torch.relu(h @ getattr(self, "W%d" % l) + getattr(self, "b%d" % l))
            if self.norm:
                h = torch.nn.functional.layer_norm(h, h.shape[-1:], getattr(self, "gamma%d" % l),
                                                   getattr(self, "beta%d" % l), eps=self.eps)
        return h @ self.W_out + self.b_out


class QNet:
    """``QNet(in_dim, hidden, num_actions)``: the chain ``in_dim -> hidden[0] -> .. -> num_actions`` with at most three
    hidden layers, ``in_dim <= 1024``, every other width ``<= 256``.  ``norm=False`` leaves the layer norm out (relu
    only); ``ln_eps`` defaults to 1e-12, the ``variance_epsilon`` of TF 1.14's ``tf.contrib.layers.layer_norm`` as far as
    its source is remembered (TensorFlow was not at hand to check).  ``init="reference"``: ``W ~ U[0, 1)``, hidden biases
    0.1, output bias 0, gamma 1, beta 0 (drl_drqn.py:124-152) from a ``torch.Generator`` seeded with `seed`;
    ``init="zeros"``: a zero blob (to be filled by `copy_from` / `load_sequential`)."""

    def __init__(self, in_dim: int, hidden: Sequence[int], num_actions: int, device="cuda:0", norm: bool = True,
                 ln_eps: float = 1e-12, init: str = "reference", seed: int = 0):
        self.widths = [int(in_dim)] + [int(h) for h in hidden] + [int(num_actions)]
        self.L = len(self.widths) - 2
        if self.L > MAX_HIDDEN:
            raise ValueError("QNet takes at most %d hidden layers" % MAX_HIDDEN)
        if not 1 <= self.widths[0] <= MAX_IN or any(not 1 <= w <= MAX_WIDTH for w in self.widths[1:]):
            raise ValueError("QNet needs 1 <= in_dim <= %d and hidden widths and num_actions in [1, %d]" % (MAX_IN, MAX_WIDTH))
        if not float(ln_eps) >= 0.0 or float(ln_eps) == float("inf"):
            raise ValueError("ln_eps must be finite and >= 0")
        if init not in ("reference", "zeros"):
            raise ValueError("init must be 'reference' or 'zeros'")
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.norm, self.ln_eps = bool(norm), float(ln_eps)
        self.in_dim, self.num_actions = self.widths[0], self.widths[-1]
        self._layout = layout(self.widths)
        self._widths_c = (ctypes.c_int32 * len(self.widths))(*self.widths)
        self.params = torch.zeros((blob_len(self.widths),), dtype=torch.float32, device=self.device)
        self._keep: tuple = ()                               # what the last launch's raw pointers refer to
        if init == "reference":
            gen = torch.Generator(device="cpu").manual_seed(int(seed))
            with torch.no_grad():
                for name, view in self.views().items():
                    if name.startswith("W"):
                        view.copy_(torch.rand(view.shape, generator=gen, dtype=torch.float32))
                    elif name.startswith("gamma"):
                        view.fill_(1.0)
                    elif name.startswith("b") and name != "b_out" and not name.startswith("beta"):
                        view.fill_(0.1)

    def views(self) -> Dict[str, torch.Tensor]:
        """Named views into `params`: ``W1, b1, gamma1, beta1, .., W_out, b_out`` (``W`` is ``[in, out]``)."""
        out = {}
        for name, (off, shape) in self._layout.items():
            n = shape[0] * shape[1] if len(shape) == 2 else shape[0]
            out[name] = self.params[off:off + n].view(shape)
        return out

    def forward(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``q [rows, A]`` float32 of ``x [rows, in_dim]`` (float32 / float16 / bfloat16): one launch on the current
        stream, no ``grad_fn``.  ``x`` may be a view with a row stride (``window[:, -1]`` of a ``[rows, step, S]``
        window, ``lstm_out[:, -1]``) as long as its last dimension has unit stride; `out` a contiguous ``[rows, A]``
        float32 tensor, for instance a slice of a larger buffer."""
        D, A = self.in_dim, self.num_actions
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype not in X_DTYPES or x.device != self.device \
                or int(x.shape[1]) != D or int(x.shape[0]) < 1:
            raise ValueError("x must be a float32 / float16 / bfloat16 tensor [rows, %d] on %s" % (D, self.device))
        rows = int(x.shape[0])
        stride = int(x.stride(0)) if rows > 1 else D
        if (D > 1 and x.stride(1) != 1) or stride < D:
            raise ValueError("x must have unit stride along its last dimension and a row stride >= %d" % D)
        if out is None:
            out = torch.empty((rows, A), dtype=torch.float32, device=self.device)
        check_tensor("out", out, torch.float32, (rows, A), self.device, MSG_OUT)
        x = x.detach()
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        check_status(self.lib.diral_qnet_forward(rows, self.L, self._widths_c, _ptr(x), X_DTYPES[x.dtype], stride,
                                                 _ptr(self.params), int(self.params.numel()), int(self.norm), self.ln_eps,
                                                 _ptr(out), stream), "diral_qnet_forward")
        self._keep = (x, out)
        return out

    __call__ = forward

    def torch_module(self) -> torch.nn.Module:
        """The gradient path: an ``nn.Module`` whose ``nn.Parameter``s share storage with `params` and whose forward is
        the same chain in torch ops.  What an optimiser does to them, the next `forward` launch sees."""
        return _Chain(self)

    def copy_from(self, other: "QNet") -> None:
        """The reference's ``update_target_op``: one ``copy_`` of the blob."""
        if other.widths != self.widths:
            raise ValueError("copy_from needs a QNet of the same widths")
        with torch.no_grad():
            self.params.copy_(other.params)

    def load_sequential(self, seq) -> None:
        """Packs a ``Sequential(Linear, ReLU, LayerNorm, .., Linear)`` (without the LayerNorms when ``norm=False``):
        ``Linear.weight`` is ``[out, in]`` and goes in transposed."""
        mods = list(seq)
        per = 3 if self.norm else 2
        if len(mods) != per * self.L + 1:
            raise ValueError("load_sequential needs %d modules for this chain" % (per * self.L + 1))
        v = self.views()
        with torch.no_grad():
            for l in range(self.L + 1):
                lin = mods[per * l]
                W = v["W%d" % (l + 1)] if l < self.L else v["W_out"]
                b = v["b%d" % (l + 1)] if l < self.L else v["b_out"]
                if not isinstance(lin, torch.nn.Linear) or tuple(lin.weight.shape) != (W.shape[1], W.shape[0]) or lin.bias is None:
                    raise ValueError("module %d must be a Linear(%d, %d) with a bias" % (per * l, W.shape[0], W.shape[1]))
                W.copy_(lin.weight.t())
                b.copy_(lin.bias)
                if l == self.L:
                    break
                if not isinstance(mods[per * l + 1], torch.nn.ReLU):
                    raise ValueError("module %d must be a ReLU" % (per * l + 1))
                if self.norm:
                    ln = mods[per * l + 2]
                    if not isinstance(ln, torch.nn.LayerNorm) or tuple(ln.normalized_shape) != (W.shape[1],) or ln.weight is None:
                        raise ValueError("module %d must be a LayerNorm(%d) with weight and bias" % (per * l + 2, W.shape[1]))
                    v["gamma%d" % (l + 1)].copy_(ln.weight)
                    v["beta%d" % (l + 1)].copy_(ln.bias)
