"""`diral_qnet_forward` / `QNet.forward` on the device against the host statement of tests/qnet_cases.py, which
tests/test_qnet_cases.py holds against torch's CPU float64 graph.

* Exact integer data, no layer norm: bit for bit (every partial sum is an integer below 2^24) - the fragment-layout test.
* The chain with layer norm: within ``TOL_REL * max |q|`` of the float64 statement.  TOL_REL = 1.4765e-04 was measured on
  the host, never on the kernel (tests/qnet_cases.py): the largest error against the statement, relative to max |q| of the
  case, is 3.183e-05 for the serial k-ordered float32 restatement and 3.691e-05 for ``torch_module()`` on the CPU; the
  tolerance is the larger times 4, the kernel's layer-norm sums having an order of their own.  (The kernel's own largest
  error on these cases, as the test prints it: 1.518e-05, at 193 x 256 -> 256 -> 256 -> 256 -> 32.)  A single dense layer
  (L = 0) is held to ``gamma_{D+1} (|b| + sum |x| |w|)`` instead.
* Row independence, tails, strides, live parameters and capture: bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from diral_amd import QNet, QPolicy, ReplayMemory
from diral_amd.config import bench_config
from diral_amd.rollout import no_finalizers_during_capture
from tests import qnet_cases as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [H.shape_id(s) for s in H.SHAPES]
TORCH = (torch.float32, torch.float16, torch.bfloat16)


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def net_of(blob, widths, norm=True):
    net = QNet(widths[0], widths[1:-1], widths[-1], device=DEV, norm=norm, ln_eps=H.EPS, init="zeros")
    net.params.copy_(dev(blob))
    return net


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


_REAL = {}


def real(shape):
    """(x, blob, widths, the float64 statement) of a shape, computed once."""
    if shape not in _REAL:
        x, blob, widths = H.real_case(*shape, seed=1)
        _REAL[shape] = (x, blob, widths, H.qnet_f64(x, blob, widths, True, H.EPS))
    return _REAL[shape]


# ---- 1. the fragment layout ----
@pytest.mark.parametrize("n, shape", list(enumerate(H.SHAPES)), ids=IDS)
def test_integer_chain_is_bit_equal(n, shape):
    x, blob, widths, want = H.integer_case(*shape, seed=2)
    net = net_of(blob, widths, norm=False)
    for dtype in TORCH if shape[2] in ((256, 256), (96, 40)) else (TORCH[n % 3],):
        q = net.forward(dev(x, dtype))
        assert q.dtype == torch.float32 and tuple(q.shape) == want.shape and q.grad_fn is None and not q.requires_grad
        got = host(q)
        assert H.same_bits(got, want), (dtype, np.argwhere(got != want)[:4], got[got != want][:4], want[got != want][:4])


# ---- 2. the chain with layer norm ----
@pytest.mark.parametrize("shape", H.SHAPES, ids=IDS)
def test_chain_with_layer_norm_against_the_statement(shape):
    x, blob, widths, want = real(shape)
    got = host(net_of(blob, widths).forward(dev(x))).astype(np.float64)
    err = np.abs(got - want)
    print("%s: max err %.3e = %.3e of max |q|" % (H.shape_id(shape), err.max(), err.max() / np.abs(want).max()))
    if shape[2]:
        assert err.max() <= H.TOL_REL * np.abs(want).max()
    else:
        assert (err <= H.dense_bound(x, blob, widths)).all()


def test_rows_behind_a_dead_relu_row_are_constant_and_stay_exact():
    """A row whose first layer is all negative leaves zeros, the next layer the same b in every column: var == 0, where
    1 / sqrt(var + 1e-12) = 1e6 would turn an ulp of the mean into 0.06 per column.  The statement gives y == beta there."""
    rows, D, hidden, A = 65, 23, (256, 256), 3
    x, blob, widths = H.real_case(rows, D, hidden, A, seed=5)
    x[::4] = -np.abs(x[::4]) - np.float32(0.5)                       # W >= 0 and b = 0.1: every fourth row is dead
    p = H.unpack(blob, widths)
    p["beta1"][:] = 0                                                # (a view of the blob) as the reference starts: y1 == 0 there
    want = H.qnet_f64(x, blob, widths, True, H.EPS)
    assert np.allclose(want[::4], p["beta2"].astype(np.float64) @ p["W_out"].astype(np.float64), rtol=1e-9)
    got = host(net_of(blob, widths).forward(dev(x))).astype(np.float64)
    assert np.abs(got - want).max() <= H.TOL_REL * np.abs(want).max()


# ---- 3. row independence and tails ----
def test_rows_are_independent_bit_for_bit():
    shape = (193, 52, (256, 256), 32)
    x, blob, widths = H.real_case(*shape, seed=3)
    net, xd = net_of(blob, widths), dev(x)
    full = host(net.forward(xd))
    assert H.same_bits(host(net.forward(xd)), full)                              # two calls, equal bits
    for r in (0, 63, 64, 192):
        assert H.same_bits(host(net.forward(xd[r:r + 1])), full[r:r + 1]), r
    assert H.same_bits(host(net.forward(xd[64:129])), full[64:129])              # another place in the tile, another `rows`
    poisoned = xd.clone()
    poisoned[70, 5] = float("nan")
    got = host(net.forward(poisoned))
    assert np.isnan(got[70]).all() and H.same_bits(np.delete(got, 70, axis=0), np.delete(full, 70, axis=0))


def test_out_is_a_slice_and_the_sentinels_stay():
    shape = (65, 23, (96, 40), 3)
    x, blob, widths = H.real_case(*shape, seed=3)
    net, rows, A, guard = net_of(blob, widths), shape[0], shape[3], 64
    want = host(net.forward(dev(x)))
    buf = torch.full((rows * A + 2 * guard,), 77.0, device=DEV)
    out = buf[guard:guard + rows * A].view(rows, A)
    assert net.forward(dev(x), out=out) is out
    assert H.same_bits(host(out), want)
    assert bool((buf[:guard] == 77).all() and (buf[guard + rows * A:] == 77).all())
    with pytest.raises(ValueError):
        net.forward(dev(x), out=torch.empty((rows, A + 1), device=DEV)[:, :A])
    with pytest.raises(ValueError):
        net.forward(dev(x)[:, :-1])


# ---- 4. strided input ----
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_the_last_step_of_a_window_goes_in_without_a_copy(dtype):
    shape = (65, 52, (256, 256), 32)
    x, blob, widths = H.real_case(*shape, seed=4)
    net = net_of(blob, widths)
    xd = dev(x, dtype)
    window = torch.full((shape[0], 6, shape[1]), float("nan"), dtype=dtype, device=DEV)
    window[:, -1] = xd
    view = window[:, -1]
    assert not view.is_contiguous() and view.data_ptr() != xd.data_ptr()
    assert H.same_bits(host(net.forward(view)), host(net.forward(xd)))
    with pytest.raises(ValueError):
        net.forward(xd.t().contiguous().t())                        # no unit stride along D


# ---- 5. live parameters and capture ----
def nodes_of(graph):
    """The number of nodes of a captured graph kept with keep_graph=True, from the HIP runtime torch runs on."""
    with open("/proc/self/maps") as fh:
        path = next(line.split()[-1] for line in fh if "libamdhip64" in line)
    hip = ctypes.CDLL(path)                                         # (already loaded: the same runtime)
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(ctypes.c_void_p(graph.raw_cuda_graph()), None, ctypes.byref(n)) == 0
    return n.value


def within(net, x, q):
    want = H.qnet_f64(x, host(net.params), net.widths, True, H.EPS)
    return np.abs(host(q).astype(np.float64) - want).max() <= H.TOL_REL * np.abs(want).max()


def test_live_parameters_capture_and_the_target_copy():
    shape = (65, 23, (96, 40), 64)
    x, blob, widths, _ = real(shape)
    net, xd = net_of(blob, widths), dev(x)
    first = host(net.forward(xd)).copy()
    with torch.no_grad():                                           # an in-place update of the blob
        net.views()["W2"].mul_(0.5)
        net.views()["beta1"].add_(0.25)
    second = host(net.forward(xd)).copy()
    assert not H.same_bits(first, second) and within(net, x, net.forward(xd))
    mod = net.torch_module()                                        # an optimiser step through the gradient path
    opt = torch.optim.Adam(mod.parameters(), lr=1e-2)
    before = net.params.clone()
    mod(xd).square().mean().backward()
    opt.step()
    assert not torch.equal(before, net.params)
    third = host(net.forward(xd)).copy()
    assert not H.same_bits(second, third) and within(net, x, net.forward(xd))
    with torch.no_grad():
        assert np.abs(host(mod(xd)) - third).max() <= 2 * H.TOL_REL * np.abs(third).max()       # both paths, one blob

    out = torch.zeros((shape[0], shape[3]), device=DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        net.forward(xd, out=out)                                    # eagerly first
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with no_finalizers_during_capture():
        with torch.cuda.graph(graph, stream=stream):
            net.forward(xd, out=out)
    torch.cuda.synchronize()
    assert nodes_of(graph) == 1
    with torch.no_grad():
        net.views()["b_out"].add_(1.0)
        net.views()["gamma2"].mul_(1.5)
    out.zero_()
    graph.replay()
    replayed = host(out).copy()
    assert not H.same_bits(replayed, third) and H.same_bits(replayed, host(net.forward(xd)))

    target = QNet(widths[0], widths[1:-1], widths[-1], device=DEV, ln_eps=H.EPS, seed=9)
    assert not H.same_bits(host(target.forward(xd)), replayed)
    target.copy_from(net)
    assert H.same_bits(host(target.forward(xd)), replayed)


# ---- 6. the wiring ----
def test_window_to_actions():
    w = H.WIRING
    B, N, A = w["B"], w["N"], w["A"]
    S = bench_config(N, A, 300.0, communication_range=120.0, State=dict(num_bins=20)).state_space
    states, blob, widths = H.wiring_case(S)
    memory = ReplayMemory(4, B, N, S, dtype=torch.float32, device=DEV)
    memory.begin(dev(states))
    net, policy = net_of(blob, widths), QPolicy(B, N, A, "greedy", device=DEV)
    window = memory.history(1)
    assert tuple(window.shape) == (B * N, 1, S)
    q = net.forward(window.view(B * N, S))
    actions = host(policy.greedy(q.view(B, N, A))).reshape(-1)
    want = H.qnet_f64(states.reshape(-1, S), blob, widths, True, H.EPS)
    keep = H.decided(want, H.TOL_REL * np.abs(want).max())
    assert (~keep).sum() * 10 <= keep.size
    assert np.array_equal(actions[keep], np.argmax(want, axis=1)[keep])
