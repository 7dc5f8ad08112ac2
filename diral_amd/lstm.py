"""The parameters and the gradient path of the reference's recurrent layer: TF 1.x ``BasicLSTMCell(layers[0])`` under
``dynamic_rnn`` with ``lstm_out[:, -1, :]`` taken (algorithms/drl_drqn.py:116-121), in front of the dense head
(:class:`diral_amd.QNet`) when ``use_lstm_input: true``.

Per row, for t = 0 .. T-1 from ``(h, c) = (h0, c0)`` or zeros: ``z = [x_t, h] @ kernel + bias``; ``i, j, f, o = split(z, 4)``;
``c = c * sigmoid(f + forget_bias) + sigmoid(i) * tanh(j)``; ``h = tanh(c) * sigmoid(o)``.  :class:`LSTM` keeps ``kernel
[S + H, 4H]`` (rows in the concat order ``[x, h]``, gate blocks ``i | j | f | o``) and ``bias [4H]`` in ONE flat float32 tensor,
`params`, laid out as :class:`QNet` lays out its chain, and `torch_module` is the cell unrolled in torch ops over views of it:
``net(states)``, the one evaluation of a training iteration that sees a gradient.  :class:`DRQNet` is the cell and the head
together.  tests/lstm_cases.py states the cell in float64 NumPy; tests/test_lstm_module.py holds this module against it.

There is NO device launch of the cell here and so no ``forward`` on either class: the three evaluations without a gradient
go through the module under ``torch.no_grad()`` and then ``DRQNet.head.forward``, which is a launch.
No TensorFlow run exists to compare with: the cell and its default initializer are TensorFlow's as far as its source is
remembered (TensorFlow was not at hand to check).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from .qnet import QNet

MAX_IN, MAX_HIDDEN_UNITS = 1024, 256


def layout(in_dim: int, hidden: int) -> Dict[str, tuple]:
    """{name: (offset, shape)} of the blob: ``kernel [S + H, 4H]`` row-major, then ``bias [4H]``."""
    S, H = int(in_dim), int(hidden)
    return {"kernel": (0, (S + H, 4 * H)), "bias": ((S + H) * 4 * H, (4 * H,))}


def blob_len(in_dim: int, hidden: int) -> int:
    return (int(in_dim) + int(hidden) + 1) * 4 * int(hidden)


class _Cell(torch.nn.Module):
    """The unrolled cell in torch ops over parameters that are views of an LSTM's blob."""

    def __init__(self, net: "LSTM"):
        super().__init__()
        self.in_dim, self.hidden, self.forget_bias = net.in_dim, net.hidden, net.forget_bias
        for name, view in net.views().items():
            param = torch.nn.Parameter(view)                 # shares the blob's storage
            assert param.data_ptr() == view.data_ptr()
            self.register_parameter(name, param)

    def forward(self, x, state: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, return_state: bool = False):
        """``h_T [rows, H]`` of ``x [rows, T, S]`` (``lstm_out[:, -1, :]``), ``(h_T, c_T)`` with `return_state`."""
        if x.dim() != 3 or int(x.shape[2]) != self.in_dim or int(x.shape[1]) < 1:
            raise ValueError("x must be [rows, T >= 1, %d]" % self.in_dim)
        x = x.to(torch.float32)
        H = self.hidden
        if state is None:
            h = c = torch.zeros((x.shape[0], H), dtype=torch.float32, device=x.device)
        else:
            h, c = state
        for t in range(x.shape[1]):
            z = torch.cat([x[:, t], h], dim=1) @ self.kernel + self.bias
            i, j, f, o = torch.split(z, H, dim=1)
            c = c * torch.sigmoid(f + self.forget_bias) + torch.sigmoid(i) * torch.tanh(j)
            h = torch.tanh(c) * torch.sigmoid(o)
        return (h, c) if return_state else h


class LSTM:
    """``LSTM(in_dim, hidden)``: the cell's parameters for ``1 <= in_dim <= 1024`` and ``1 <= hidden <= 256``.
    ``init="reference"`` is what ``BasicLSTMCell`` gets from ``tf.get_variable`` with no initializer, as far as its source
    is remembered: the kernel Glorot-uniform, ``U(-l, l)`` with ``l = sqrt(6 / ((S + H) + 4H))``, from a ``torch.Generator``
    seeded with `seed`, the bias zeros; ``init="zeros"``: a zero blob (to be filled by `copy_from` / `load_torch`).
    ``forget_bias`` (1.0 in TF) is added to the f pre-activation inside the sigmoid and is no parameter."""

    def __init__(self, in_dim: int, hidden: int, device="cuda:0", forget_bias: float = 1.0, init: str = "reference",
                 seed: int = 0):
        self.in_dim, self.hidden = int(in_dim), int(hidden)
        if not 1 <= self.in_dim <= MAX_IN or not 1 <= self.hidden <= MAX_HIDDEN_UNITS:
            raise ValueError("LSTM needs 1 <= in_dim <= %d and 1 <= hidden <= %d" % (MAX_IN, MAX_HIDDEN_UNITS))
        if not math.isfinite(float(forget_bias)):
            raise ValueError("forget_bias must be finite")
        if init not in ("reference", "zeros"):
            raise ValueError("init must be 'reference' or 'zeros'")
        self.device = torch.device(device)
        self.forget_bias = float(forget_bias)
        self._layout = layout(self.in_dim, self.hidden)
        self.params = torch.zeros((blob_len(self.in_dim, self.hidden),), dtype=torch.float32, device=self.device)
        if init == "reference":
            gen = torch.Generator(device="cpu").manual_seed(int(seed))
            kernel = self.views()["kernel"]
            limit = math.sqrt(6.0 / ((self.in_dim + self.hidden) + 4 * self.hidden))
            with torch.no_grad():
                kernel.copy_((torch.rand(kernel.shape, generator=gen, dtype=torch.float64) * 2.0 - 1.0) * limit)

    def views(self) -> Dict[str, torch.Tensor]:
        """Named views into `params`: ``kernel [S + H, 4H]`` and ``bias [4H]``."""
        out = {}
        for name, (off, shape) in self._layout.items():
            out[name] = self.params[off:off + math.prod(shape)].view(shape)
        return out

    def torch_module(self) -> torch.nn.Module:
        """The gradient path: an ``nn.Module`` whose ``nn.Parameter``s share storage with `params` and whose forward
        ``module(x [rows, T, S], state=None, return_state=False)`` is the unrolled cell in torch ops.  What an optimiser
        does to them is in `params` at once."""
        return _Cell(self)

    def copy_from(self, other: "LSTM") -> None:
        """The reference's ``update_target_op``: one ``copy_`` of the blob."""
        if (other.in_dim, other.hidden) != (self.in_dim, self.hidden):
            raise ValueError("copy_from needs an LSTM of the same in_dim and hidden")
        with torch.no_grad():
            self.params.copy_(other.params)

    def load_torch(self, lstm: torch.nn.LSTM) -> None:
        """Packs a one-layer, unidirectional, ``batch_first`` ``torch.nn.LSTM``: gate blocks ``i, f, g, o -> i, j, f, o``
        (torch's g is TF's j), the weights transposed and stacked as ``[W_ih; W_hh]``, ``bias = b_ih + b_hh`` with
        `forget_bias` subtracted on the f block (torch adds none), summed in float64 and rounded to float32 once."""
        S, H = self.in_dim, self.hidden
        if not isinstance(lstm, torch.nn.LSTM) or lstm.num_layers != 1 or lstm.bidirectional or not lstm.batch_first \
                or not lstm.bias or lstm.proj_size != 0 or (lstm.input_size, lstm.hidden_size) != (S, H):
            raise ValueError("load_torch needs a one-layer, unidirectional, batch_first LSTM(%d, %d) with biases" % (S, H))
        w = torch.cat([lstm.weight_ih_l0.detach(), lstm.weight_hh_l0.detach()], dim=1).double()      # [4H, S + H]
        b = lstm.bias_ih_l0.detach().double() + lstm.bias_hh_l0.detach().double()
        v = self.views()
        with torch.no_grad():
            for n, g in enumerate((0, 2, 1, 3)):             # TF block n is torch block g
                v["kernel"][:, n * H:(n + 1) * H].copy_(w[g * H:(g + 1) * H].t())
                v["bias"][n * H:(n + 1) * H].copy_(b[g * H:(g + 1) * H] - (self.forget_bias if n == 2 else 0.0))


class _Drqn(torch.nn.Module):
    def __init__(self, net: "DRQNet"):
        super().__init__()
        self.lstm, self.head = net.lstm.torch_module(), net.head.torch_module()

    def forward(self, window):
        return self.head(self.lstm(window))


class DRQNet:
    """The reference's default agent (``use_lstm_input: true``, drl_drqn.py:117, 130-153):
    ``LSTM(state_size, layers[0])`` as `lstm`, then ``QNet(layers[0], layers[1:], num_actions)`` as `head`, two blobs.
    `norm`, `ln_eps` go to the head, `forget_bias` to the cell; `seed` seeds the cell, ``seed + 1`` the head."""

    def __init__(self, state_size: int, layers: Sequence[int], num_actions: int, device="cuda:0", norm: bool = True,
                 ln_eps: float = 1e-12, forget_bias: float = 1.0, init: str = "reference", seed: int = 0):
        layers = [int(w) for w in layers]
        if not layers:
            raise ValueError("DRQNet needs layers[0], the width of the LSTM cell")
        self.lstm = LSTM(state_size, layers[0], device=device, forget_bias=forget_bias, init=init, seed=seed)
        self.head = QNet(layers[0], layers[1:], num_actions, device=device, norm=norm, ln_eps=ln_eps, init=init,
                         seed=int(seed) + 1)

    def torch_module(self) -> torch.nn.Module:
        """``module(window [rows, T, S]) -> q [rows, A]`` in torch ops over views of both blobs, with submodules `lstm`
        and `head`."""
        return _Drqn(self)

    def copy_from(self, other: "DRQNet") -> None:
        self.lstm.copy_from(other.lstm)
        self.head.copy_from(other.head)
