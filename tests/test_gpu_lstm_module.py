"""diral_amd.LSTM and diral_amd.DRQNet on the device: the gradient path `torch_module()` over the device blob against the
float64 statement of tests/lstm_cases.py, an optimiser step landing in the blobs, and the cell's output going into the
head's launch without a copy.  Torch ops only in front of the head: the cell has no launch of its own.

The tolerance is `lstm_cases.TOL_ABS`, 4 x what two float32 host evaluations are off by; rocBLAS may sum a row's products
in another order than either, which that factor is for."""
import numpy as np
import pytest
import torch

from diral_amd import DRQNet, LSTM
from tests import lstm_cases as H
from tests import qnet_cases as Q

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SOME = [(193, 6, 52, 256), (65, 2, 515, 40), (31, 2, 3, 3), (1, 6, 257, 1)]


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.mark.parametrize("case", SOME, ids=[H.case_id(c) for c in SOME])
def test_torch_module_on_the_device_against_the_statement(case):
    rows, T, S, Hh = case
    x, blob = H.real_case(*case, seed=1)
    h0, c0 = H.real_state(rows, Hh, seed=1)
    net = LSTM(S, Hh, device=DEV, init="zeros")
    net.params.copy_(dev(blob))
    mod = net.torch_module()
    assert mod.kernel.is_cuda and mod.kernel.data_ptr() == net.params.data_ptr()
    for state in (None, (h0, c0)):
        want_h, want_c = H.lstm_f64(x, blob, S, Hh, H.FORGET_BIAS, *(state or (None, None)))
        with torch.no_grad():
            h, c = mod(dev(x), state=None if state is None else (dev(h0), dev(c0)), return_state=True)
        err = max(np.abs(h.cpu().numpy() - want_h).max(), np.abs(c.cpu().numpy() - want_c).max())
        print("%s state %s: %.3e" % (H.case_id(case), state is not None, err))
        assert h.dtype == torch.float32 and tuple(h.shape) == (rows, Hh) and err <= H.TOL_ABS


def test_a_step_lands_in_both_blobs_and_the_head_launch_takes_the_cells_output():
    rows, T, S, Hh, A = 65, 6, 23, 40, 3
    net, target = DRQNet(S, (Hh,), A, device=DEV, seed=2), DRQNet(S, (Hh,), A, device=DEV, init="zeros")
    mod = net.torch_module()
    w = dev(np.random.default_rng(1).normal(0, 1, (rows, T, S)).astype(np.float32))
    before = (net.lstm.params.clone(), net.head.params.clone())
    opt = torch.optim.Adam(mod.parameters(), lr=1e-2)
    (mod(w) ** 2).mean().backward()
    opt.step()
    assert (net.lstm.params != before[0]).float().mean() > 0.9 and (net.head.params != before[1]).float().mean() > 0.9
    target.copy_from(net)
    # the evaluations without a gradient: the cell in torch ops, its h_T straight into the head's launch
    with torch.no_grad():
        h = target.torch_module().lstm(w)
    q = target.head.forward(h)
    assert q.grad_fn is None and tuple(q.shape) == (rows, A)
    torch.cuda.synchronize()
    h_np, blob, widths = h.cpu().numpy(), target.head.params.cpu().numpy(), [Hh, A]
    err = np.abs(q.cpu().numpy().astype(np.float64) - Q.qnet_f64(h_np, blob, widths))
    assert (err <= Q.dense_bound(h_np, blob, widths)).all()
    # and h_T is the statement's on the stepped weights
    want_h, _ = H.lstm_f64(w.cpu().numpy(), target.lstm.params.cpu().numpy(), S, Hh)
    assert np.abs(h_np - want_h).max() <= H.TOL_ABS
