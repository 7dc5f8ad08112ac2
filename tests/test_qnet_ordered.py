"""The ordered float32 statement of `diral_qnet_forward` (tests/qnet_ordered.py) without a device.  Since
tests/test_gpu_qnet_ordered.py holds the kernel to that statement bit for bit, the order csrc/qnet_kernel.hpp documents is
what the suite asserts - so the statement itself is held here:

* its fused multiply-add is correctly rounded: equal to exact rational arithmetic on random triples over several exponent
  gaps, on triples next to a float32 tie, and on a constructed triple that the detour through float64 gets wrong;
* without layer norm it gives the integer cases' one value, bit for bit;
* it lies within TOL_REL of the float64 statement on the real cases (the anchor: its worst error is a recorded constant);
* rows behind a dead relu row come out as y == beta exactly, as the header says, and not with the mean summed once;
* a layer norm of width 1 gives y == beta; the case with infinities (`padding_case`) has a finite statement;
* every lattice case stays in normal numbers (the header says nothing about subnormals);
* each of the nine `wrong=` forms - one rule off - differs IN BITS from the right one on every lattice case with a hidden
  layer of more than one column, so a kernel that kept any of those orders instead would fail the GPU comparison; the
  layer-norm forms cannot show on L = 0, and do not.

The lattice (rows, D, hidden, A), each the smallest shape that reaches its branch of the kernel: see
`tests.qnet_ordered.LATTICE`."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import qnet_cases as H
from tests import qnet_ordered as O

IDS = [H.shape_id(s) for s in H.SHAPES]
F32 = np.float32


def round_fraction_to_f32(v):
    """A rational number to the nearest float32, ties to even, in integer arithmetic (normal range only)."""
    if v == 0:
        return F32(0)
    sign, v = (-1 if v < 0 else 1), abs(v)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    assert Fraction(2) ** e <= v < Fraction(2) ** (e + 1) and -126 <= e < 127
    scaled = v / Fraction(2) ** (e - 23)                             # in [2^23, 2^24)
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return F32(sign * math.ldexp(n, e - 23))


def exact_fma(a, b, c):
    return round_fraction_to_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


# ---- the fused multiply-add ----
def test_fmaf32_is_correctly_rounded():
    rng = np.random.default_rng(11)
    a, b, c = [], [], []
    for gap in (-60, -30, -25, -24, -23, -12, -1, 0, 1, 12, 23, 24, 25, 30, 60):    # exponent of c over that of a * b
        n = 200
        ai = ((1 + rng.random(n)) * rng.choice([-1, 1], n) * 2.0 ** rng.integers(-20, 20, n)).astype(F32)
        bi = ((1 + rng.random(n)) * rng.choice([-1, 1], n) * 2.0 ** rng.integers(-20, 20, n)).astype(F32)
        ci = ((1 + rng.random(n)) * rng.choice([-1, 1], n) * np.abs(ai.astype(np.float64) * bi) * 2.0 ** gap).astype(F32)
        a, b, c = a + [ai], b + [bi], c + [ci]
    # next to a tie: c = 1 + m 2^-23 and a * b = 2^-24 -+ j^2 2^-70 / 2^-24 + j 2^-46 + .., a hair under or over half an ulp
    j = np.arange(1, 41, dtype=np.float64)
    m = rng.integers(0, 64, j.size)
    for sa, sb in ((1, -1), (1, 1), (-1, -1)):
        a.append((2.0 ** -12 + sa * j * 2.0 ** -35).astype(F32))
        b.append((2.0 ** -12 + sb * j * 2.0 ** -35).astype(F32))
        c.append((1 + m * 2.0 ** -23).astype(F32))
    a, b, c = np.concatenate(a), np.concatenate(b), np.concatenate(c)
    assert np.isfinite(c).all() and (np.abs(c) >= np.finfo(F32).tiny).all()
    got, detour = O.fmaf32(a, b, c), O.fmaf32_through_float64(a, b, c)
    want = np.array([exact_fma(*t) for t in zip(a, b, c)], dtype=F32)
    assert got.dtype == F32 and H.same_bits(got, want), np.argwhere(got != want)[:4]
    assert not H.same_bits(detour, want)                            # the near-tie family catches the detour too


def test_the_float64_detour_double_rounds_where_fmaf32_does_not():
    a, b, c = O.DOUBLE_ROUNDING
    assert Fraction(float(a)) * Fraction(float(b)) == Fraction(1, 2 ** 24) - Fraction(1, 2 ** 70)
    right = exact_fma(a, b, c)
    assert right == F32(1 + 2.0 ** -23)
    assert O.fmaf32(a, b, c) == right
    assert O.fmaf32_through_float64(a, b, c) == F32(1 + 2.0 ** -22) != right
    x, W = np.array([[a]], dtype=F32), np.array([[b]], dtype=F32)   # and as the dense layers use it: acc = c, one more k
    x2, W2 = np.array([[c, a]], dtype=F32), np.array([[F32(1)], [b]], dtype=F32)
    assert O.dense_ordered_f32(x2, W2)[0, 0] == right and H.dense_serial_f32(x2, W2)[0, 0] != right
    assert O.dense_ordered_f32(x, W)[0, 0] == F32(float(a) * float(b))


def test_fmaf32_keeps_infinities_and_nans():
    inf, nan, one = F32(np.inf), F32(np.nan), F32(1)
    assert O.fmaf32(inf, one, one) == inf and O.fmaf32(one, one, -inf) == -inf
    assert np.isnan(O.fmaf32(nan, one, one)) and np.isnan(O.fmaf32(one, one, nan)) and np.isnan(O.fmaf32(inf, one, -inf))
    assert O.fmaf32(F32(3e38), F32(2), F32(0)) == inf               # the float32 overflow is the last rounding's


# ---- the statement against what the suite already has ----
@pytest.mark.parametrize("shape", H.SHAPES, ids=IDS)
def test_without_layer_norm_the_integer_cases_have_their_one_value(shape):
    x, blob, widths, q = H.integer_case(*shape, seed=2)
    assert H.same_bits(O.qnet_ordered_f32(x, blob, widths, norm=False), q)
    assert H.same_bits(O.qnet_ordered_f32(x.astype(np.float16), blob, widths, norm=False), q)


def test_the_ordered_statement_lies_within_the_tolerance_of_the_float64_statement():
    """The anchor: the statement the kernel is held to in bits is itself a float32 evaluation of the chain, inside the
    tolerance the kernel has been held to so far - and its worst error is a recorded figure, not a bound on anything."""
    worst = 0.0
    for shape in H.SHAPES:
        if not shape[2]:
            continue
        x, blob, widths = H.real_case(*shape, seed=1)
        want = H.qnet_f64(x, blob, widths, True, H.EPS)
        err = np.abs(O.qnet_ordered_f32(x, blob, widths, True, H.EPS) - want).max() / np.abs(want).max()
        print("%s: %.6e of max |q|" % (H.shape_id(shape), err))
        assert err <= H.TOL_REL
        worst = max(worst, err)
    assert H.MEASURED_ORDERED == pytest.approx(worst, rel=1e-3)


def test_dense_bound_holds_for_the_ordered_statement():
    for shape in [s for s in H.SHAPES if not s[2]] + [O.ORDERED_SHAPES[-1]]:
        x, blob, widths = H.real_case(*shape, seed=1)
        err = np.abs(O.qnet_ordered_f32(x, blob, widths) - H.qnet_f64(x, blob, widths))
        assert (err <= H.dense_bound(x, blob, widths)).all()


def test_rows_behind_a_dead_relu_row_give_beta_exactly_and_not_with_the_mean_summed_once():
    """The case of test_gpu_qnet.py's test_rows_behind_a_dead_relu_row_are_constant_and_stay_exact: every fourth row dies
    in the first layer, the second layer holds b2 = 0.1 in all 256 columns of it.  The header: mean == 0.1, var == 0,
    y == beta exactly - so q of those rows is the output layer of beta2 -, where m0 alone is an ulp off."""
    rows, D, hidden, A = 65, 23, (256, 256), 3
    x, blob, widths = H.real_case(rows, D, hidden, A, seed=5)
    x[::4] = -np.abs(x[::4]) - F32(0.5)
    p = H.unpack(blob, widths)
    p["beta1"][:] = 0
    memo = {}
    q = O.qnet_ordered_f32(x, blob, widths, True, H.EPS, memo=memo)
    beta_only = O.dense_ordered_f32(p["beta2"][None, :], p["W_out"]) + p["b_out"]
    assert H.same_bits(q[::4], np.repeat(beta_only, q[::4].shape[0], axis=0))
    assert not H.same_bits(q[1], beta_only[0])                       # (a live row is something else)
    once = O.qnet_ordered_f32(x, blob, widths, True, H.EPS, wrong="mean_once", memo=memo)
    assert np.abs(once[::4] - beta_only).max() > 1e-3 * np.abs(beta_only).max()
    c = np.full((3, 256), 0.1, dtype=F32)                            # the layer norm alone, on the constant row
    assert H.same_bits(O.layer_norm_ordered_f32(c, p["gamma2"], p["beta2"], H.EPS), np.repeat(p["beta2"][None, :], 3, axis=0))
    assert O.sum4(c)[0, 0] / F32(256) != F32(0.1)                    # m0 IS off here: the second sum is what mends it


def test_a_layer_norm_of_width_one_gives_beta():
    shape = O.ORDERED_SHAPES[0]
    assert shape == (1, 1, (1,), 1)
    for seed in range(8):                                            # a live relu in some draws, a dead one in others
        x, blob, widths = O.ordered_case(shape, seed)
        p = H.unpack(blob, widths)
        want = O.fmaf32(p["beta1"][0], p["W_out"][0, 0], F32(0)) + p["b_out"][0]
        assert H.same_bits(O.qnet_ordered_f32(x, blob, widths), np.array([[want]], dtype=F32))


def test_the_padding_case_has_a_finite_statement():
    x, blob, widths = O.padding_case(2)
    p = H.unpack(blob, widths)
    assert np.isinf(x[::5, 33]).all() and np.isfinite(np.delete(x, 33, axis=1)).all() and np.isinf(blob).sum() == 1
    z1 = O.dense_ordered_f32(x, p["W1"]) + p["b1"]
    assert (z1[::5] == -np.inf).all() and (z1[:, 5] == -np.inf).all() and np.isfinite(np.delete(z1[1:5], 5, axis=1)).all()
    beta_only = O.dense_ordered_f32(p["beta1"][None, :], p["W_out"]) + p["b_out"]
    for norm in (True, False):
        q = O.qnet_ordered_f32(x, blob, widths, norm)
        assert np.isfinite(q).all()
        assert H.same_bits(q[::5], np.repeat(beta_only if norm else p["b_out"][None, :], q[::5].shape[0], axis=0))


# ---- the lattice ----
_LATTICE = {}


def lattice(shape):
    """(x, blob, widths, memo, the statement with layer norm) of a lattice shape at seed 1, computed once."""
    if shape not in _LATTICE:
        x, blob, widths = O.ordered_case(shape, 1)
        memo = {}
        _LATTICE[shape] = (x, blob, widths, memo, O.qnet_ordered_f32(x, blob, widths, memo=memo))
    return _LATTICE[shape]


def test_the_lattice_is_the_documented_one_and_within_the_limits():
    assert O.ORDERED_SHAPES == [(1, 1, (1,), 1), (33, 7, (7, 9), 65), (130, 8, (16,), 33), (65, 257, (33,), 129),
                                (64, 2, (255, 32), 200), (32, 512, (256,), 64), (127, 513, (200, 33, 129), 256),
                                (129, 1024, (65,), 96), (65, 511, (), 255)]
    for rows, D, hidden, A in O.ORDERED_SHAPES:
        assert 1 <= D <= 1024 and len(hidden) <= 3 and all(1 <= h <= 256 for h in hidden + (A,)) and rows >= 1


def test_ordered_cases_stay_in_normal_numbers_and_relus_die():
    smallest = np.finfo(F32).tiny
    for shape in O.ORDERED_SHAPES:
        x, blob, widths = O.ordered_case(shape, 1)
        for v in (x, blob):
            assert np.isfinite(v).all() and (np.abs(v[v != 0]) >= smallest).all()
        assert x.min() < 0 < x.max() or shape[0] * shape[1] == 1
        tiny = []
        q = O.qnet_ordered_f32(x, blob, widths, tiny=tiny)
        assert H.same_bits(q, lattice(shape)[4])                     # (neither `tiny` nor `memo` changes a bit)
        assert np.isfinite(q).all() and min(tiny) >= smallest, (shape, min(tiny))
        if shape[2] and shape[2][0] > 1:
            p = H.unpack(blob, widths)
            z = O.dense_ordered_f32(x, p["W1"]) + p["b1"]
            assert (z <= 0).any() and (z > 0).any()                  # mixed signs: some relus die, some live
        x16 = x.astype(np.float16)                                   # and so with the 16-bit roundings of x
        assert (np.abs(x16) >= 2.0 ** -14).all()
        for xs in (O.exact_f32(x16), O.exact_f32(torch.from_numpy(x).to(torch.bfloat16))):
            tiny = []
            assert np.isfinite(O.qnet_ordered_f32(xs, blob, widths, tiny=tiny)).all() and min(tiny) >= smallest


def test_every_wrong_form_differs_in_bits_on_the_lattice():
    told = {w: [] for w in O.WRONG}
    for shape in O.ORDERED_SHAPES:
        x, blob, widths, memo, right = lattice(shape)
        n = min(16, shape[0])                                        # rows are independent: the first 16 tell as much
        for w in O.WRONG:
            if w in O.WRONG_NORM:                                    # (the first layer's sums are the memo's)
                got = O.qnet_ordered_f32(x, blob, widths, wrong=w, memo=memo)[:n]
            else:
                got = O.qnet_ordered_f32(x[:n], blob, widths, wrong=w)
            if not H.same_bits(got, right[:n]):
                told[w].append(shape)
    assert all(told.values()), told
    wide = [s for s in O.ORDERED_SHAPES if s[2] and s[2][0] > 1]
    assert len(wide) == 7
    for w in O.WRONG:
        assert set(wide) <= set(told[w]), (w, told[w])
    L0 = O.ORDERED_SHAPES[-1]
    assert L0[2] == ()
    for w in O.WRONG_NORM:
        assert L0 not in told[w]                                     # nothing of the layer norm runs at L = 0
    for w in O.WRONG_DENSE:
        assert L0 in told[w]
    assert not any(O.ORDERED_SHAPES[0] in t for t in told.values())  # one term, one column: nothing has an order


def test_first_difference_names_the_place_and_the_tiles():
    want = np.arange(70 * 40, dtype=F32).reshape(70, 40) + 1
    assert O.first_difference(want.copy(), want) is None
    nan = want.copy()
    nan[3, 3] = np.nan
    assert O.first_difference(nan.copy(), nan) is None
    got = want.copy()
    got[33, 35] = np.nextafter(got[33, 35], F32(np.inf))
    got[65, 2] = 0
    msg = O.first_difference(got, want)
    assert "2 of 2800 differ" in msg and "(row 33, col 35)" in msg
    assert "per column tile [1, 1]" in msg and "per row tile [0, 1, 1]" in msg
    assert "shape" in O.first_difference(want[:, :3], want)
