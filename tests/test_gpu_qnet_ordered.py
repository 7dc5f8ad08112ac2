"""`diral_qnet_forward` on the device against the ORDERED float32 statement of tests/qnet_ordered.py - rules 1-5 of
csrc/qnet_kernel.hpp in NumPy float32, which tests/test_qnet_ordered.py holds on the host -, bit for bit, no tolerance: the
k-ordered `fmaf` chain from zero, the four strided partial sums added as ((p0 + p1) + p2) + p3, the mean summed twice, y
never fused, division and square root correctly rounded.  The header's order is what this file asserts; tests/test_gpu_qnet.py
keeps the tolerance around the float64 statement and the order-blind integer cases.

The cases are the lattice `ORDERED_SHAPES` (rows, D, hidden, A), each the smallest shape that reaches its branch of the
kernel, with and without layer norm and the dtype of x rotating (the statement is computed on x after the exact conversion):

    (1, 1, (1,), 1)                  every width minimal, only the odd tail runs, a layer norm of width 1
    (33, 7, (7, 9), 65)              in < 8 at l = 0 and l = 1, in = 9; three output tiles, one live column in the last
    (130, 8, (16,), 33)              in = 8 (one block, loads itself again), in = 16 (a block prefetched); 2 tail rows
    (65, 257, (33,), 129)            a second chunk of one column; odd in = 33 at l > 0 (the pad column of act is read);
                                     five output tiles: only wave 0 owns a second one
    (64, 2, (255, 32), 200)          in = 2; eight tiles, the last partial; odd in = 255 at l > 0; a hidden layer of one
                                     tile; seven output tiles
    (32, 512, (256,), 64)            exactly two chunks, exactly one row tile
    (127, 513, (200, 33, 129), 256)  three different hidden widths (off[]), a third chunk of one column, full-width output
    (129, 1024, (65,), 96)           the maximum D, four full chunks; 1 tail row in the third workgroup
    (65, 511, (), 255)               L = 0 with eight output tiles

and, on top: every `SHAPES` entry on its real_case data, eps = 1e-5, a float16 window view with a row stride over three
chunks, row slices and single rows of the 129-row shape, and one case with infinities (`padding_case`), where each of the
two zeros of the kernel's k padding has to be there by itself.  Every launch writes into an `out` full of NaNs, so a tile
that no wave wrote shows.  A mismatch names the first differing (row, column), both values, and the count of differing
elements per column tile and per row tile (`first_difference`)."""
import numpy as np
import pytest
import torch

from diral_amd import QNet
from tests import qnet_cases as H
from tests import qnet_ordered as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = (torch.float32, torch.float16, torch.bfloat16)
LATTICE = list(enumerate(O.ORDERED_SHAPES))
LATTICE_IDS = [H.shape_id(s) for s in O.ORDERED_SHAPES]
SHAPE_257, SHAPE_513, SHAPE_129_ROWS = O.ORDERED_SHAPES[3], O.ORDERED_SHAPES[6], O.ORDERED_SHAPES[7]


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def net_of(blob, widths, norm=True, eps=H.EPS):
    net = QNet(widths[0], widths[1:-1], widths[-1], device=DEV, norm=norm, ln_eps=eps, init="zeros")
    net.params.copy_(dev(blob))
    return net


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def run(net, xd):
    """One launch into an `out` full of NaNs: an element no wave wrote shows, whatever the allocator held there."""
    out = torch.full((int(xd.shape[0]), net.num_actions), float("nan"), dtype=torch.float32, device=DEV)
    assert net.forward(xd, out=out) is out
    return host(out)


def assert_same_bits(got, want, what=""):
    diff = O.first_difference(got, want)
    assert diff is None, "%s: %s" % (what, diff)


_CASES = {}


def case(shape, dtype):
    """(x on the device in `dtype`, x as float32 after that conversion, blob, widths, memo) of a lattice shape, drawn once;
    the memo carries the first layer's sums from one statement to the next."""
    if (shape, dtype) not in _CASES:
        x, blob, widths = O.ordered_case(shape, 1)
        xd = dev(x, dtype)
        _CASES[shape, dtype] = (xd, O.exact_f32(xd), blob, widths, {})
    return _CASES[shape, dtype]


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "relu-only"])
@pytest.mark.parametrize("n, shape", LATTICE, ids=LATTICE_IDS)
def test_lattice_equals_the_ordered_statement(n, shape, norm):
    dtype = TORCH[n % 3]
    xd, xs, blob, widths, memo = case(shape, dtype)
    want = O.qnet_ordered_f32(xs, blob, widths, norm, H.EPS, memo=memo)
    assert_same_bits(run(net_of(blob, widths, norm), xd), want, "%s %s norm=%d" % (H.shape_id(shape), dtype, norm))


@pytest.mark.parametrize("shape", H.SHAPES, ids=[H.shape_id(s) for s in H.SHAPES])
def test_real_cases_equal_the_ordered_statement(shape):
    x, blob, widths = H.real_case(*shape, seed=1)
    want = O.qnet_ordered_f32(x, blob, widths, True, H.EPS)
    assert_same_bits(run(net_of(blob, widths), dev(x)), want, H.shape_id(shape))


def test_another_eps_is_the_callers():
    xd, xs, blob, widths, memo = case(SHAPE_257, torch.float32)
    want = O.qnet_ordered_f32(xs, blob, widths, True, 1e-5, memo=memo)
    assert not H.same_bits(want, O.qnet_ordered_f32(xs, blob, widths, True, H.EPS, memo=memo))
    assert_same_bits(run(net_of(blob, widths, eps=1e-5), xd), want, "eps 1e-5")


@pytest.mark.parametrize("norm", [True, False], ids=["norm", "relu-only"])
def test_what_the_padding_multiplies_is_zero_on_both_sides(norm):
    """`padding_case`: an infinity where the LDS tile's pad column would keep it and one where a row k = in of W would be
    read.  On finite data either zero of the padding covers for the other; here each has to be there."""
    x, blob, widths = O.padding_case(2)
    want = O.qnet_ordered_f32(x, blob, widths, norm, H.EPS)
    assert np.isfinite(want).all()
    assert_same_bits(run(net_of(blob, widths, norm), dev(x)), want, "padding case norm=%d" % norm)


def test_float16_window_view_with_a_row_stride_over_three_chunks():
    xd, xs, blob, widths, memo = case(SHAPE_513, torch.float16)
    rows, D = xs.shape
    window = torch.full((rows, 3, D), float("nan"), dtype=torch.float16, device=DEV)
    window[:, -1] = xd
    view = window[:, -1]
    assert not view.is_contiguous() and view.stride(0) == 3 * D and view.data_ptr() != xd.data_ptr()
    want = O.qnet_ordered_f32(xs, blob, widths, True, H.EPS, memo=memo)
    assert_same_bits(run(net_of(blob, widths), view), want, "window[:, -1] float16")


def test_row_slices_and_single_rows_equal_the_same_rows_of_the_statement():
    xd, xs, blob, widths, memo = case(SHAPE_129_ROWS, TORCH[7 % 3])
    assert xs.shape[0] == 129
    want = O.qnet_ordered_f32(xs, blob, widths, True, H.EPS, memo=memo)
    net = net_of(blob, widths)
    assert_same_bits(run(net, xd[64:129]), want[64:129], "rows 64..128")
    for r in (0, 63, 64, 128):
        assert_same_bits(run(net, xd[r:r + 1]), want[r:r + 1], "row %d alone" % r)
