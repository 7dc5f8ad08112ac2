"""diral_amd.LSTM and diral_amd.DRQNet on the CPU: the parameter blob of the reference's recurrent layer and its gradient
path, `torch_module()`, held against the float64 statement of tests/lstm_cases.py.

The blob's layout is written out here again (`H.unpack` / `H.pack`), not imported from the package; the tolerance on `h_T`
and `c_T` is `H.TOL_ABS`, measured on two float32 host evaluations.  No kernel is tested here: the cell has no device launch
(DESIGN.md section 3.4)."""
import types

import numpy as np
import pytest
import torch

import diral_amd
from diral_amd import DRQNet, LSTM, QNet
from tests import lstm_cases as H

IDS = [H.case_id(c) for c in H.CASES]


def net_of(blob, S, Hh, forget_bias=H.FORGET_BIAS):
    net = LSTM(S, Hh, device="cpu", forget_bias=forget_bias, init="zeros")
    net.params.copy_(torch.from_numpy(blob))
    return net


def test_exported_and_laid_out_as_the_statement_reads_it():
    assert diral_amd.LSTM is LSTM and diral_amd.DRQNet is DRQNet and {"LSTM", "DRQNet"} <= set(diral_amd.__all__)
    S, Hh = 5, 3
    net = LSTM(S, Hh, device="cpu", init="zeros")
    assert net.params.dtype == torch.float32 and tuple(net.params.shape) == (H.blob_len(S, Hh),) and not net.params.any()
    v = net.views()
    assert list(v) == ["kernel", "bias"] and tuple(v["kernel"].shape) == (S + Hh, 4 * Hh) and tuple(v["bias"].shape) == (4 * Hh,)
    net.params.copy_(torch.arange(net.params.numel(), dtype=torch.float32))
    kernel, bias = H.unpack(net.params.numpy(), S, Hh)
    assert np.array_equal(v["kernel"].numpy(), kernel) and np.array_equal(v["bias"].numpy(), bias)
    assert v["kernel"].data_ptr() == net.params.data_ptr()
    assert not hasattr(net, "forward")                               # no launch of the cell: nothing that looks like one


def test_reference_init_is_glorot_uniform_with_a_zero_bias():
    S, Hh = 52, 256
    net = LSTM(S, Hh, device="cpu", seed=11)
    v = net.views()
    limit = np.sqrt(6.0 / ((S + Hh) + 4 * Hh))
    k = v["kernel"].numpy().astype(np.float64)
    assert not v["bias"].any() and np.abs(k).max() <= np.float32(limit)
    # U(-l, l) over 315 392 draws: mean 0 +- l / sqrt(3 n), variance l^2 / 3, the extremes within l / 1000 of +-l
    assert abs(k.mean()) < 5 * limit / np.sqrt(3 * k.size) and abs(k.var() / (limit ** 2 / 3) - 1) < 0.01
    assert k.max() > 0.999 * limit and k.min() < -0.999 * limit
    assert torch.equal(LSTM(S, Hh, device="cpu", seed=11).params, net.params)
    assert not torch.equal(LSTM(S, Hh, device="cpu", seed=12).params, net.params)
    for bad in (dict(in_dim=0, hidden=3), dict(in_dim=1025, hidden=3), dict(in_dim=3, hidden=0), dict(in_dim=3, hidden=257),
                dict(in_dim=3, hidden=3, forget_bias=float("inf")), dict(in_dim=3, hidden=3, forget_bias=float("nan")),
                dict(in_dim=3, hidden=3, init="glorot")):
        with pytest.raises(ValueError):
            LSTM(device="cpu", **bad)
    LSTM(1024, 256, device="cpu", init="zeros")


@pytest.mark.parametrize("case", H.CASES, ids=IDS)
def test_torch_module_against_the_statement(case):
    rows, T, S, Hh = case
    x, blob = H.real_case(*case, seed=1)
    h0, c0 = H.real_state(rows, Hh, seed=1)
    for fb in (H.FORGET_BIAS, 0.0):
        mod = net_of(blob, S, Hh, fb).torch_module()
        for state in (None, (h0, c0)):
            want_h, want_c = H.lstm_f64(x, blob, S, Hh, fb, *(state or (None, None)))
            with torch.no_grad():
                st = None if state is None else tuple(torch.from_numpy(v) for v in state)
                h, c = mod(torch.from_numpy(x), state=st, return_state=True)
                assert torch.equal(mod(torch.from_numpy(x), state=st), h)
            assert h.dtype == c.dtype == torch.float32 and tuple(h.shape) == tuple(c.shape) == (rows, Hh)
            err = max(np.abs(h.numpy() - want_h).max(), np.abs(c.numpy() - want_c).max())
            print("%s fb %.1f state %s: %.3e" % (H.case_id(case), fb, state is not None, err))
            assert err <= H.TOL_ABS
    # and every wrong restatement is further from the module than the tolerance, where the case has the feature
    with torch.no_grad():
        h, c = net_of(blob, S, Hh).torch_module()(torch.from_numpy(x), return_state=True)
    for w in H.WRONG:
        wrong = H.lstm_f64(x, blob, S, Hh, wrong=w)
        moved = max(np.abs(h.numpy() - wrong[0]).max(), np.abs(c.numpy() - wrong[1]).max())
        assert (moved > H.TOL_ABS) == H.has_feature(w, case), (w, moved)


def test_torch_module_takes_views_and_narrow_inputs_and_splits_like_the_recurrence():
    rows, T, S, Hh = 31, 6, 23, 40
    x, blob = H.real_case(rows, T, S, Hh, seed=2)
    mod = net_of(blob, S, Hh).torch_module()
    parent = torch.zeros((rows, T + 2, S + 3))
    parent[:, 1:T + 1, 2:S + 2] = torch.from_numpy(x)
    with torch.no_grad():
        h, c = mod(torch.from_numpy(x), return_state=True)
        assert torch.equal(mod(parent[:, 1:T + 1, 2:S + 2]), h)
        for k in range(1, T):                                        # the same ops in the same order: bit for bit
            h2, c2 = mod(torch.from_numpy(x[:, k:]), state=mod(torch.from_numpy(x[:, :k]), return_state=True), return_state=True)
            assert torch.equal(h2, h) and torch.equal(c2, c)
        for dtype in (torch.float16, torch.bfloat16):                # converted exactly, then float32
            narrow = torch.from_numpy(x).to(dtype)
            assert torch.equal(mod(narrow), mod(narrow.float())) and mod(narrow).dtype == torch.float32
    for bad in (torch.zeros((rows, S)), torch.zeros((rows, T, S + 1)), torch.zeros((rows, 0, S))):
        with pytest.raises(ValueError):
            mod(bad)


def test_load_torch_is_the_statements_mapping_bit_for_bit():
    S, Hh = 23, 40
    torch.manual_seed(4)
    lstm = torch.nn.LSTM(S, Hh, batch_first=True)
    for fb in (1.0, 0.0, 0.5):
        net = LSTM(S, Hh, device="cpu", forget_bias=fb, init="zeros")
        net.load_torch(lstm)
        assert H.same_bits(net.params.numpy(), H.pack_torch_lstm(lstm, fb))
        # round trip: the blob unpacked by the statement's inverse is the LSTM again (the two biases as their sum)
        back = H.torch_lstm_of(net.params.numpy(), S, Hh, fb, torch.float32)
        assert torch.equal(back.weight_ih_l0, lstm.weight_ih_l0) and torch.equal(back.weight_hh_l0, lstm.weight_hh_l0)
        assert torch.allclose(back.bias_ih_l0, lstm.bias_ih_l0 + lstm.bias_hh_l0, rtol=0, atol=2 ** -23)   # -fb, +fb: two roundings below 2
        # and the two compute the same: torch's float32 LSTM against the module, both within the host tolerance of float64
        x = torch.from_numpy(np.random.default_rng(6).normal(0, 1, (31, 6, S)).astype(np.float32))
        with torch.no_grad():
            out, (h, c) = lstm(x)
            got_h, got_c = net.torch_module()(x, return_state=True)
        assert (got_h - h[0]).abs().max() <= 2 * H.TOL_ABS and (got_c - c[0]).abs().max() <= 2 * H.TOL_ABS
    net = LSTM(S, Hh, device="cpu", init="zeros")
    for bad in (torch.nn.LSTM(S, Hh, num_layers=2, batch_first=True), torch.nn.LSTM(S, Hh, bidirectional=True, batch_first=True),
                torch.nn.LSTM(S, Hh), torch.nn.LSTM(S, Hh, bias=False, batch_first=True), torch.nn.LSTM(S + 1, Hh, batch_first=True),
                torch.nn.LSTM(S, Hh + 1, batch_first=True), torch.nn.LSTM(S, Hh, proj_size=8, batch_first=True),
                torch.nn.GRU(S, Hh, batch_first=True)):
        with pytest.raises(ValueError):
            net.load_torch(bad)
    assert not net.params.any()


def test_gradients_are_torch_lstms_and_an_optimiser_step_lands_in_the_blob():
    """The module's gradients against ``torch.nn.LSTM``'s for the same float32 loss, mapped as the weights are (a linear
    map, so `pack_torch_lstm` with no forget bias packs gradients too; ``b_ih`` and ``b_hh`` each get the bias's gradient,
    one of them is packed).  Both are float32 backward passes over 6 steps of sums up to 92 terms long: a relative 1e-4 of
    the largest gradient is a hundred times float32's 6e-8 x 92 x 6 and far below any wrong wiring."""
    rows, T, S, Hh = 31, 6, 52, 40
    torch.manual_seed(9)
    lstm = torch.nn.LSTM(S, Hh, batch_first=True)
    net = LSTM(S, Hh, device="cpu", init="zeros")
    net.load_torch(lstm)
    mod = net.torch_module()
    assert [n for n, _ in mod.named_parameters()] == ["kernel", "bias"]
    assert mod.kernel.data_ptr() == net.params.data_ptr() and mod.bias.data_ptr() == net.views()["bias"].data_ptr()
    x = torch.from_numpy(np.random.default_rng(7).normal(0, 1, (rows, T, S)).astype(np.float32))
    g = torch.from_numpy(np.random.default_rng(8).normal(0, 1, (rows, Hh)).astype(np.float32))
    (mod(x) * g).sum().backward()
    (lstm(x)[0][:, -1] * g).sum().backward()
    grads = types.SimpleNamespace(hidden_size=Hh, weight_ih_l0=lstm.weight_ih_l0.grad, weight_hh_l0=lstm.weight_hh_l0.grad,
                                  bias_ih_l0=lstm.bias_ih_l0.grad, bias_hh_l0=torch.zeros(4 * Hh))
    assert torch.equal(lstm.bias_ih_l0.grad, lstm.bias_hh_l0.grad)
    want_k, want_b = H.unpack(H.pack_torch_lstm(grads, 0.0), S, Hh)
    for got, want in ((mod.kernel.grad.numpy(), want_k), (mod.bias.grad.numpy(), want_b)):
        assert np.abs(want).max() > 0.1 and np.abs(got - want).max() <= 1e-4 * np.abs(want).max()
    before = net.params.clone()
    torch.optim.SGD(mod.parameters(), lr=0.5).step()
    want = before - 0.5 * torch.from_numpy(H.pack(mod.kernel.grad.numpy(), mod.bias.grad.numpy()))
    assert torch.equal(net.params, want) and not torch.equal(net.params, before)


def test_copy_from():
    net, target = LSTM(23, 40, device="cpu", seed=1), LSTM(23, 40, device="cpu", init="zeros")
    mod = target.torch_module()
    target.copy_from(net)
    assert torch.equal(target.params, net.params) and target.params.data_ptr() != net.params.data_ptr()
    assert torch.equal(mod.kernel, net.views()["kernel"])            # the module made before the copy sees it
    for other in (LSTM(23, 41, device="cpu"), LSTM(24, 40, device="cpu")):
        with pytest.raises(ValueError):
            target.copy_from(other)


def test_drqnet_is_the_cell_and_the_head():
    S, layers, A = 23, (40, 64), 3
    net = DRQNet(S, layers, A, device="cpu", seed=5)
    assert isinstance(net.lstm, LSTM) and isinstance(net.head, QNet) and not hasattr(net, "forward")
    assert (net.lstm.in_dim, net.lstm.hidden) == (S, 40) and net.head.widths == [40, 64, A]
    assert torch.equal(net.lstm.params, LSTM(S, 40, device="cpu", seed=5).params)
    assert torch.equal(net.head.params, QNet(40, (64,), A, device="cpu", seed=6).params)
    mod = net.torch_module()
    w = torch.from_numpy(np.random.default_rng(3).normal(0, 1, (31, 6, S)).astype(np.float32))
    with torch.no_grad():
        assert torch.equal(mod(w), net.head.torch_module()(net.lstm.torch_module()(w))) and tuple(mod(w).shape) == (31, A)
    ptrs = {p.data_ptr() for p in mod.parameters()}
    assert {v.data_ptr() for v in net.lstm.views().values()} | {v.data_ptr() for v in net.head.views().values()} == ptrs
    mod(w).sum().backward()
    assert all(p.grad is not None and p.grad.abs().max() > 0 for n, p in mod.named_parameters() if n != "head.b_out") \
        and mod.head.b_out.grad is not None
    target = DRQNet(S, layers, A, device="cpu", init="zeros")
    target.copy_from(net)
    assert torch.equal(target.lstm.params, net.lstm.params) and torch.equal(target.head.params, net.head.params)
    assert DRQNet(S, (40,), A, device="cpu").head.L == 0             # layers = [H]: the head is the output layer alone
    with pytest.raises(ValueError):
        DRQNet(S, (), A, device="cpu")
