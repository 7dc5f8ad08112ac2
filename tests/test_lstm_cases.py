"""The host statement of the reference's recurrent layer (tests/lstm_cases.py) without a device: it equals
``torch.nn.LSTM`` on the CPU in float64 through the gate mapping written both ways, restatements with one rule wrong are
each told apart on every case that has the feature, the float32 tolerance is what two host evaluations give, the dyadic
cases are exact in any order of summation, and the sweep's rounding procedure agrees with mpmath.

No kernel is tested here: the LSTM cell is still outside the device forward, and this is what one
will be held against.  What nobody has measured: TensorFlow is not installed here, so the cell has never been compared with
a TensorFlow run of ``BasicLSTMCell``; its gate order ``i | j | f | o``, the concat order ``[x, h]``, ``forget_bias`` added
inside the sigmoid and the Glorot-uniform default initializer are TensorFlow's as far as its source is remembered."""
import numpy as np
import pytest
import torch

from tests import lstm_cases as H

IDS = [H.case_id(c) for c in H.CASES]


def dyadic_lstm(S, Hh, seed):
    """A float64 ``torch.nn.LSTM`` whose weights are float32 values and whose biases are multiples of 2^-10: what
    `pack_torch_lstm` puts into the float32 blob is then exact, the forget bias taken off included."""
    torch.manual_seed(seed)
    lstm = torch.nn.LSTM(S, Hh, batch_first=True).double()
    with torch.no_grad():
        for name, p in lstm.named_parameters():
            p.copy_(torch.round(p * 1024) / 1024 if "bias" in name else p.float().double())
    return lstm


# ---- the statement ----
@pytest.mark.parametrize("case", H.CASES, ids=IDS)
def test_statement_equals_torch_lstm_through_the_gate_mapping(case):
    rows, T, S, Hh = case
    lstm = dyadic_lstm(S, Hh, seed=3)
    rng = np.random.default_rng(5)
    x = rng.normal(0.0, 1.0, (rows, T, S)).astype(np.float32)
    h0, c0 = H.real_state(rows, Hh, seed=5)
    for fb in (1.0, 0.0, 0.5):
        blob = H.pack_torch_lstm(lstm, fb)
        assert blob.dtype == np.float32 and blob.shape == (H.blob_len(S, Hh),)
        for state in (None, (h0, c0)):
            with torch.no_grad():
                st = None if state is None else tuple(torch.from_numpy(v).double()[None] for v in state)
                out, (h, c) = lstm(torch.from_numpy(x).double(), st)
            got_h, got_c = H.lstm_f64(x, blob, S, Hh, fb, *(state or (None, None)))
            assert np.allclose(got_h, h[0].numpy(), rtol=1e-12, atol=1e-15) and np.allclose(got_c, c[0].numpy(), rtol=1e-12, atol=1e-15)
            assert np.array_equal(out[:, -1].numpy(), h[0].numpy())
    # and the mapping written the other way round
    back = H.torch_lstm_of(blob, S, Hh, 0.5, torch.float64)
    assert torch.equal(back.weight_ih_l0, lstm.weight_ih_l0) and torch.equal(back.weight_hh_l0, lstm.weight_hh_l0)
    assert torch.equal(back.bias_ih_l0 + back.bias_hh_l0, lstm.bias_ih_l0 + lstm.bias_hh_l0)
    back_h, back_c = H.torch_lstm_eval(x, blob, S, Hh, 0.5, torch.float64)
    want_h, want_c = H.lstm_f64(x, blob, S, Hh, 0.5)
    assert np.allclose(back_h, want_h, rtol=1e-12, atol=1e-15) and np.allclose(back_c, want_c, rtol=1e-12, atol=1e-15)


def test_the_gate_mapping_block_by_block():
    S, Hh = 23, 40
    lstm = dyadic_lstm(S, Hh, seed=8)
    kernel, bias = H.unpack(H.pack_torch_lstm(lstm, 1.0), S, Hh)
    w_ih, w_hh = lstm.weight_ih_l0.detach().numpy(), lstm.weight_hh_l0.detach().numpy()
    b = (lstm.bias_ih_l0 + lstm.bias_hh_l0).detach().numpy()
    assert np.array_equal(kernel[:S, Hh:2 * Hh], w_ih[2 * Hh:3 * Hh].T)            # TF's j is torch's g
    assert np.array_equal(kernel[S:, 2 * Hh:3 * Hh], w_hh[Hh:2 * Hh].T)            # TF's f is torch's second block
    assert np.array_equal(kernel[:S, :Hh], w_ih[:Hh].T) and np.array_equal(kernel[S:, 3 * Hh:], w_hh[3 * Hh:].T)
    assert np.array_equal(bias[2 * Hh:3 * Hh], b[Hh:2 * Hh] - 1.0) and np.array_equal(bias[Hh:2 * Hh], b[2 * Hh:3 * Hh])


def test_wrong_restatements_are_each_told_apart():
    """'Told apart': the wrong form moves h_T or c_T by more than 1e-6, nine orders above what float64 rounding moves
    (rtol 1e-12 above), on EVERY case that has the feature."""
    for case in H.CASES:
        rows, T, S, Hh = case
        x, blob = H.real_case(*case, seed=1)
        right = H.lstm_f64(x, blob, S, Hh)
        for w in H.WRONG:
            wrong = H.lstm_f64(x, blob, S, Hh, wrong=w)
            moved = max(np.abs(wrong[0] - right[0]).max(), np.abs(wrong[1] - right[1]).max())
            assert (moved > 1e-6) == H.has_feature(w, case), (w, case, moved)
    assert len(set(H.WRONG)) == len(H.WRONG) >= 8
    assert [H.has_feature("c_not_carried", c) for c in H.CASES].count(True) >= 5


def test_the_cases_cover_the_lists():
    rows, T, S, Hh = (sorted(set(v)) for v in zip(*H.CASES))
    assert rows == [1, 31, 64, 65, 193] and T == [1, 2, 6] and S == [1, 3, 23, 52, 257, 515] and Hh == [1, 3, 40, 96, 256]
    assert (193, 6, 52, 256) in H.CASES and (65, 2, 515, 40) in H.CASES and len(H.CASES) <= 12


def test_the_tolerance_is_what_the_host_evaluations_give():
    """tests/lstm_cases.py TOL_ABS is 4 x the larger absolute error on h_T and c_T of two float32 host evaluations against
    the float64 statement: the serial k-ordered restatement and ``torch.nn.LSTM`` on the CPU.  NumPy's float32 exp / tanh
    and torch's CPU LSTM may round or sum differently elsewhere, so the figures are bounded, not pinned."""
    worst = {"serial": 0.0, "torch": 0.0}
    for case in H.CASES:
        rows, T, S, Hh = case
        x, blob = H.real_case(*case, seed=1)
        want = H.lstm_f64(x, blob, S, Hh)
        for which, got in (("serial", H.lstm_serial_f32(x, blob, S, Hh)),
                           ("torch", H.torch_lstm_eval(x, blob, S, Hh, H.FORGET_BIAS, torch.float32))):
            assert got[0].dtype == got[1].dtype == np.float32
            worst[which] = max(worst[which], np.abs(got[0] - want[0]).max(), np.abs(got[1] - want[1]).max())
    print("serial %.6e torch %.6e" % (worst["serial"], worst["torch"]))
    assert worst["serial"] <= 2 * H.MEASURED_SERIAL and H.MEASURED_SERIAL <= 2 * worst["serial"]
    assert worst["torch"] <= 2 * H.MEASURED_TORCH
    assert H.TOL_ABS == 4 * max(H.MEASURED_SERIAL, H.MEASURED_TORCH)


# ---- the dyadic cases ----
def test_dyadic_cases_are_exact_in_any_order():
    one = np.float32(1)
    args = H.table_arguments()
    sig, tanh = one / (one + np.exp(-args)), np.tanh(args)            # a stand-in for a device's values: NumPy's float32
    for through_h in (False, True):
        for case in H.CASES:
            rows, _, S, Hh = case
            x, blob, h0, c0, z = H.dyadic_case(rows, S, Hh, seed=7, through_h=through_h)
            kernel, bias = H.unpack(blob, S, Hh)
            a = np.concatenate([x[:, 0], np.zeros((rows, Hh), np.float32) if h0 is None else h0], axis=1)
            assert np.array_equal(H.dense_serial_f32(a, kernel) + bias, z.astype(np.float32))            # k order
            assert np.array_equal(H.dense_serial_f32(a[:, ::-1], kernel[::-1]) + bias, z.astype(np.float32))   # and reversed
            assert H.same_bits(x.astype(np.float16).astype(np.float32), x)                               # exact in the 16-bit kinds
            assert H.same_bits(torch.from_numpy(x).to(torch.bfloat16).float().numpy(), x)
            assert args[0] <= z.min() and z.max() + H.FORGET_BIAS <= args[-1]
            # the table arithmetic against the same cell written directly on z
            z32 = z.astype(np.float32)
            i, j, f, o = (z32[:, g * Hh:(g + 1) * Hh] for g in range(4))
            old = np.zeros(i.shape, np.float32) if c0 is None else c0
            want_c = old * (one / (one + np.exp(-(f + one)))) + (one / (one + np.exp(-i))) * np.tanh(j)
            want_h = np.tanh(want_c) * (one / (one + np.exp(-o)))
            got_h, got_c = H.dyadic_expected(z, Hh, c0, sig, tanh, np.tanh)
            assert H.same_bits(got_c, want_c) and H.same_bits(got_h, want_h)


# ---- the rounding procedure of the sweep ----
def test_sweep_rounding_procedure_against_mpmath():
    z = H.sweep_arguments()
    assert (np.abs(z) >= 2.0 ** -100).all() and np.abs(z).max() < 128 and np.array_equal(z, -z[::-1]) and len(np.unique(z)) == len(z)
    assert abs(float(H.saturation_threshold(H.sigmoid64)) - 17.33) < 0.01 and abs(float(H.saturation_threshold(np.tanh)) - 9.01) < 0.01
    rng = np.random.default_rng(11)
    for kind in ("sigmoid", "tanh"):
        rn, rel = H.correctly_rounded(kind, z)
        close = np.flatnonzero(rel < H.MIDPOINT_REL)
        sample = np.unique(np.concatenate([rng.choice(len(z), 1500, replace=False), close[:200], [0, len(z) - 1]]))
        for n in sample:
            want, mp_rel = H.mp_round(kind, z[n])
            assert rn[n].view(np.uint32) == want.view(np.uint32), (kind, float(z[n]))
            assert mp_rel >= H.MIDPOINT_REL / 2 or rel[n] == mp_rel, (kind, float(z[n]), mp_rel, rel[n])
        if kind == "tanh":
            assert np.array_equal(rn, -rn[::-1])
        else:
            assert (rn >= 0).all() and (rn <= 1).all()
            assert close.size > 0                                    # 0.5 + z / 4 at z = 2^-23: a midpoint but for z^3 / 48
