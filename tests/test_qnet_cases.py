"""`diral_qnet_forward` / `QNet` without a device: the host statement the GPU tests compare against (tests/qnet_cases.py)
equals an independent torch-CPU float64 evaluation of the reference's graph, restatements with one rule wrong are each told
apart by some generated case, the C-ABI of the entry point is what include/diral_env.h declares and every refusal comes
back before a device is touched, and `QNet` packs, views and copies its blob as documented.

What nobody has measured: TensorFlow is not installed here, so the chain has never been compared with a TensorFlow run of
``_create_network``; ``eps = 1e-12`` is ``tf.contrib.layers.layer_norm``'s as far as its source is remembered."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from diral_amd import QNet, _lib
from diral_amd.config import DT_BF16, DT_F16, DT_F32, DT_F64, ERR_BAD_ARG, ERR_UNSUPPORTED, bench_config
from tests import abi_header
from tests import qnet_cases as H

IDS = [H.shape_id(s) for s in H.SHAPES]


def torch_f64(x, blob, widths, norm, eps, dtype=torch.float64):
    """The reference's graph in torch ops on the CPU, written here without the package and without tests/qnet_cases.py's
    arithmetic: x @ W + b, F.relu, F.layer_norm."""
    t = torch.from_numpy(np.asarray(blob)).to(dtype)
    h, off, L = torch.from_numpy(np.asarray(x)).to(dtype), 0, len(widths) - 2

    def take(n, shape):
        nonlocal off
        v = t[off:off + n].view(shape)
        off += n
        return v
    for l in range(L):
        i, o = widths[l], widths[l + 1]
        W, b, gamma, beta = take(i * o, (i, o)), take(o, (o,)), take(o, (o,)), take(o, (o,))
        h = F.relu(h @ W + b)
        if norm:
            h = F.layer_norm(h, (o,), gamma, beta, eps=eps)
    i, o = widths[L], widths[L + 1]
    W, b = take(i * o, (i, o)), take(o, (o,))
    assert off == t.numel()
    return (h @ W + b).numpy()


def net_of(blob, widths, norm=True, eps=H.EPS):
    net = QNet(widths[0], widths[1:-1], widths[-1], device="cpu", norm=norm, ln_eps=eps, init="zeros")
    net.params.copy_(torch.from_numpy(blob))
    return net


# ---- the statement ----
@pytest.mark.parametrize("shape", H.SHAPES, ids=IDS)
def test_statement_equals_the_torch_graph(shape):
    for norm in (True, False):
        x, blob, widths = H.real_case(*shape, seed=1)
        want = torch_f64(x, blob, widths, norm, H.EPS)
        got = H.qnet_f64(x, blob, widths, norm, H.EPS)
        assert np.allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
        mod = net_of(blob, widths, norm).torch_module()
        with torch.no_grad():
            f32 = mod(torch.from_numpy(x)).numpy()
        assert f32.dtype == np.float32 and np.abs(f32 - want).max() <= 1e-4 * np.abs(want).max()


@pytest.mark.parametrize("shape", H.SHAPES, ids=IDS)
def test_integer_cases_have_one_value(shape):
    x, blob, widths, q = H.integer_case(*shape, seed=2)
    assert np.array_equal(H.qnet_f64(x, blob, widths, False), q.astype(np.float64))
    assert H.same_bits(H.qnet_serial_f32(x, blob, widths, False), q)
    assert H.same_bits(x.astype(np.float16).astype(np.float32), x)              # exact in the 16-bit kinds too
    assert H.same_bits(torch.from_numpy(x).to(torch.bfloat16).float().numpy(), x)


def test_wrong_restatements_are_each_told_apart():
    """'Told apart': on some generated case the wrong form moves a Q-value by more than 1e-9 of the case's largest, four
    orders above what float64 rounding moves (rtol 1e-12 above)."""
    told = {w: [] for w in H.WRONG}
    for shape in H.SHAPES:
        x, blob, widths = H.real_case(*shape, seed=1)
        right = H.qnet_f64(x, blob, widths, True, H.EPS)
        for w in H.WRONG:
            if np.abs(H.qnet_f64(x, blob, widths, True, H.EPS, wrong=w) - right).max() > 1e-9 * np.abs(right).max():
                told[w].append(H.shape_id(shape))
    assert all(told.values()), told
    assert set(told["padded_stats"]) == {H.shape_id(s) for s in H.SHAPES if any(h % 32 for h in s[2])}
    assert set(told["w_transposed"]) >= {H.shape_id(s) for s in H.SHAPES if len(s[2]) >= 2 and s[2][0] == s[2][1]}


def test_the_tolerance_is_what_the_host_evaluations_give():
    """tests/qnet_cases.py TOL_REL is 4 x the larger error, relative to max |q|, of two float32 host evaluations against
    the float64 statement: `torch_module()` on the CPU and the serial k-ordered restatement.  The NumPy one is the same on
    every machine and is held here; torch's CPU matmul may sum in another order elsewhere, so its figure is only bounded."""
    worst_serial = worst_torch = 0.0
    for shape in H.SHAPES:
        if not shape[2]:
            continue                                                 # L = 0 is held to the derived bound
        x, blob, widths = H.real_case(*shape, seed=1)
        want = H.qnet_f64(x, blob, widths, True, H.EPS)
        scale = np.abs(want).max()
        worst_serial = max(worst_serial, np.abs(H.qnet_serial_f32(x, blob, widths, True, H.EPS) - want).max() / scale)
        with torch.no_grad():
            f32 = net_of(blob, widths).torch_module()(torch.from_numpy(x)).numpy()
        worst_torch = max(worst_torch, np.abs(f32 - want).max() / scale)
    print("serial %.3e torch %.3e" % (worst_serial, worst_torch))
    assert H.MEASURED_SERIAL == pytest.approx(worst_serial, rel=1e-3)
    assert worst_torch <= 2 * H.MEASURED_TORCH
    assert H.TOL_REL == 4 * max(H.MEASURED_SERIAL, H.MEASURED_TORCH)


def test_dense_bound_holds_for_the_host_evaluations():
    for shape in [s for s in H.SHAPES if not s[2]]:
        x, blob, widths = H.real_case(*shape, seed=1)
        err = np.abs(H.qnet_serial_f32(x, blob, widths) - H.qnet_f64(x, blob, widths))
        assert (err <= H.dense_bound(x, blob, widths)).all()


# ---- C-ABI ----
def test_the_header_declares_the_entry_point_and_the_table_has_its_row():
    protos = abi_header.prototypes()
    P, I32, I64, F64 = abi_header.PTR, abi_header.I32, abi_header.I64, abi_header.F64
    assert protos["diral_qnet_forward"].params == [I32, I32, P, P, I32, I64, P, I64, I32, F64, P, P]
    assert protos["diral_qnet_forward"].ret == I32
    restype, argtypes = _lib.SIGNATURES["diral_qnet_forward"]
    assert restype is ctypes.c_int and argtypes == [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                     ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
                                                     ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    assert hasattr(_lib.load(), "diral_qnet_forward")
    assert not [s for s in abi_header.structs() if "qnet" in s.lower()]          # flat arguments: ABI 8 keeps its structs


def _buf():
    return ctypes.cast((ctypes.c_char * 64)(), ctypes.c_void_p).value           # never dereferenced by a refused call


def _qnet(**kw):
    a = dict(rows=4, widths=[52, 256, 256, 32], x=_buf(), x_dtype=DT_F32, stride=None, params=_buf(), params_len=None,
             norm=1, eps=1e-12, q=_buf())
    a.update(kw)
    w = a["widths"]
    L = a.get("L", None if w is None else len(w) - 2)
    arr = None if w is None else (ctypes.c_int32 * max(len(w), 6))(*w)
    stride = w[0] if a["stride"] is None else a["stride"]
    plen = H.blob_len(w) if a["params_len"] is None else a["params_len"]
    return _lib.load().diral_qnet_forward(a["rows"], L, arr, a["x"], a["x_dtype"], stride, a["params"], plen, a["norm"], a["eps"],
                                          a["q"], None)


QNET_REFUSALS = [(dict(widths=[52, 64, 64, 64, 64, 32], params_len=1), ERR_UNSUPPORTED),              # L = 4
                 (dict(widths=[52, 256, 0, 32], params_len=1), ERR_BAD_ARG), (dict(widths=[0, 32], params_len=1), ERR_BAD_ARG),
                 (dict(widths=[52, 32, 0], params_len=1), ERR_BAD_ARG),
                 (dict(widths=[52, 257, 32]), ERR_UNSUPPORTED), (dict(widths=[52, 256, 257]), ERR_UNSUPPORTED),
                 (dict(widths=[1025, 256, 32]), ERR_UNSUPPORTED),
                 (dict(rows=0), ERR_BAD_ARG), (dict(rows=-1), ERR_BAD_ARG), (dict(widths=[52, 32], L=-1), ERR_BAD_ARG),
                 (dict(params_len=52 * 256), ERR_BAD_ARG), (dict(params_len=H.blob_len([52, 256, 256, 32]) + 1), ERR_BAD_ARG),
                 (dict(stride=51), ERR_BAD_ARG), (dict(stride=0), ERR_BAD_ARG), (dict(stride=-52), ERR_BAD_ARG),
                 (dict(x_dtype=4), ERR_BAD_ARG), (dict(x_dtype=-1), ERR_BAD_ARG), (dict(x_dtype=DT_F64), ERR_UNSUPPORTED),
                 (dict(eps=-1.0), ERR_BAD_ARG), (dict(eps=float("nan")), ERR_BAD_ARG),
                 (dict(x=None), ERR_BAD_ARG), (dict(params=None), ERR_BAD_ARG), (dict(q=None), ERR_BAD_ARG)]


def test_qnet_forward_refuses_without_a_device():
    for kw, status in QNET_REFUSALS:
        assert _qnet(**kw) == status, kw
    assert _lib.load().diral_qnet_forward(4, 2, None, _buf(), DT_F32, 52, _buf(), 1, 1, 1e-12, _buf(), None) == ERR_BAD_ARG
    assert (DT_F32, DT_F64, DT_F16, DT_BF16) == (0, 1, 2, 3)          # (x_dtype 4 and -1 above are unknown kinds)


# ---- packing ----
def test_views_tile_the_blob_once():
    for shape in H.SHAPES:
        widths = H.widths_of(*shape[1:])
        net = QNet(widths[0], widths[1:-1], widths[-1], device="cpu", seed=3)
        views, at = net.views(), 0
        L = len(widths) - 2
        want = [n + str(l) for l in range(1, L + 1) for n in ("W", "b", "gamma", "beta")] + ["W_out", "b_out"]
        assert list(views) == want and net.params.dtype == torch.float32 and net.params.dim() == 1
        for (name, v), (hname, (off, hshape)) in zip(views.items(), H.layout(widths).items()):
            assert name == hname and tuple(v.shape) == hshape and v.is_contiguous()
            assert v.data_ptr() == net.params.data_ptr() + 4 * at and off == at       # no gap, no overlap, in order
            at += v.numel()
        assert at == net.params.numel() == H.blob_len(widths)


def test_reference_init():
    net = QNet(23, (256, 256), 3, device="cpu", seed=11)
    v = net.views()
    for name, t in v.items():
        if name.startswith("W"):
            assert 0 <= float(t.min()) and float(t.max()) < 1 and 0.45 < float(t.mean()) < 0.55
        elif name.startswith("gamma"):
            assert (t == 1).all()
        elif name.startswith("beta") or name == "b_out":
            assert (t == 0).all()
        else:
            assert (t == np.float32(0.1)).all()
    assert torch.equal(QNet(23, (256, 256), 3, device="cpu", seed=11).params, net.params)
    assert not torch.equal(QNet(23, (256, 256), 3, device="cpu", seed=12).params, net.params)
    with pytest.raises(ValueError):
        QNet(23, (256, 256, 256, 256), 3, device="cpu")
    with pytest.raises(ValueError):
        QNet(1025, (256,), 3, device="cpu")
    with pytest.raises(ValueError):
        QNet(23, (257,), 3, device="cpu")


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "relu-only"])
def test_load_sequential_round_trips(norm):
    torch.manual_seed(5)
    dims, mods = [23, 96, 40, 3], []
    for i, o in zip(dims[:-2], dims[1:-1]):
        mods += [torch.nn.Linear(i, o), torch.nn.ReLU()] + ([torch.nn.LayerNorm(o, eps=1e-12)] if norm else [])
    seq = torch.nn.Sequential(*mods, torch.nn.Linear(dims[-2], dims[-1])).double()
    with torch.no_grad():
        for m in seq:
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.5, 0.5)
    net = QNet(23, (96, 40), 3, device="cpu", norm=norm, init="zeros")
    net.load_sequential(seq)
    v = net.views()
    assert torch.equal(v["W1"], seq[0].weight.t().float()) and torch.equal(v["b_out"], seq[-1].bias.float())
    x = torch.rand((17, 23), dtype=torch.float64) * 2 - 0.5
    with torch.no_grad():
        want = seq(x).numpy()
    got = H.qnet_f64(x.numpy(), net.params.numpy(), net.widths, norm, 1e-12)
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()                 # the blob is the float32 rounding of seq
    with pytest.raises(ValueError):
        net.load_sequential(torch.nn.Sequential(*list(seq)[:-1]))


def test_copy_from_and_the_shared_storage():
    net, target = QNet(23, (64,), 3, device="cpu", seed=1), QNet(23, (64,), 3, device="cpu", seed=2)
    assert not torch.equal(net.params, target.params)
    ptr = target.params.data_ptr()
    target.copy_from(net)
    assert torch.equal(net.params, target.params) and target.params.data_ptr() == ptr != net.params.data_ptr()
    with pytest.raises(ValueError):
        target.copy_from(QNet(23, (96,), 3, device="cpu"))
    mod = net.torch_module()
    params = dict(mod.named_parameters())
    assert list(params) == list(net.views()) and all(isinstance(p, torch.nn.Parameter) for p in params.values())
    assert all(p.data_ptr() == v.data_ptr() for p, v in zip(params.values(), net.views().values()))
    before = net.params.clone()
    opt = torch.optim.SGD(mod.parameters(), lr=0.1)
    mod(torch.rand((5, 23))).square().mean().backward()
    opt.step()
    assert not torch.equal(net.params, before)                                   # the step moved the blob itself


# ---- the wiring case's cap, checked where there is no device ----
def test_wiring_case_leaves_out_at_most_a_tenth():
    S = bench_config(4, 3, 300.0, communication_range=120.0, State=dict(num_bins=20)).state_space
    states, blob, widths = H.wiring_case(S)
    q = H.qnet_f64(states.reshape(-1, S), blob, widths, True, H.EPS)
    keep = H.decided(q, H.TOL_REL * np.abs(q).max())
    assert (~keep).sum() * 10 <= keep.size and len(set(np.argmax(q, axis=1))) > 1
