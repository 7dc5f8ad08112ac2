"""Host statement of the reference's recurrent layer in NumPy float64: what a device LSTM forward (DESIGN.md section 3.4,
out of scope so far: "the launch of the LSTM cell") is to be held against, with the cases, the wrong restatements, the host-measured
tolerance and the correctly rounded sigmoid / tanh values such a kernel's tests need.  tests/test_lstm_cases.py holds all
of it on the CPU: the statement against ``torch.nn.LSTM`` in float64, the rounding procedure against mpmath.

The layer is TF 1.x ``BasicLSTMCell`` under ``dynamic_rnn`` (algorithms/drl_drqn.py:116-121): per step
``z = [x_t, h] @ kernel + bias``, ``i, j, f, o = split(z, 4)``, ``c = c * sigmoid(f + forget_bias) + sigmoid(i) * tanh(j)``,
``h = tanh(c) * sigmoid(o)``; a blob is ``kernel [S + H, 4H]`` (rows in the concat order ``[x, h]``) followed by ``bias [4H]``.
No TensorFlow run exists to compare with: TensorFlow is not installed here, and the cell is written from its source as far as
it is remembered."""
import numpy as np

# rows x T x S x H: rows 1, 31, 64, 65, 193 (one row, a tail, a 64-row tile, a tile plus one, several tiles with a tail);
# S 1, 3, 23, 52 (the config sizes), 257, 515 (beyond one 256-column chunk, with an odd tail); H 1, 3, 40, 96, 256; T 1, 2, 6
CASES = [(1, 1, 1, 1), (31, 2, 3, 3), (64, 6, 23, 96), (65, 1, 257, 256), (193, 6, 52, 256), (65, 2, 515, 40),
         (31, 6, 52, 40), (193, 2, 23, 3), (64, 1, 3, 96), (1, 6, 257, 1)]
WRONG = ("gate_order_ifjo", "no_forget_bias", "forget_bias_on_i", "h_before_x", "kernel_transposed", "c_not_carried",
         "h_from_old_c", "tanh_sigmoid_swapped_on_j")
FORGET_BIAS = 1.0
# The tolerance on h_T and c_T, absolute (h lies in (-1, 1)).  Measured on the host, never on the kernel: the largest
# error against lstm_f64 over real_case(*case, seed=1) for the CASES, of
#   lstm_serial_f32 (dense sums as serial k-ordered float32 chains, NumPy float32 exp / tanh)     8.649e-07
#   torch.nn.LSTM in float32 on the CPU, packed from the same blob                                 8.751e-07
# (both at 65 x 2 x 515 -> 40: the longest sums)
# times 4: the device's sigmoid / tanh may sit at their ulp bound where the host's are close to correctly rounded, and T
# steps pass errors on.  tests/test_lstm_cases.py recomputes both.
MEASURED_SERIAL = 8.648911e-07
MEASURED_TORCH = 8.750742e-07
TOL_ABS = 4 * max(MEASURED_SERIAL, MEASURED_TORCH)


def case_id(case):
    return "r%d-T%d-S%d-H%d" % tuple(case)


def has_feature(wrong, case):
    """Whether the wrong form `wrong` can show on `case` (zero initial state): c_not_carried and no_forget_bias need a second
    step - the first one's c is zero whatever the forget gate says -, the rest show everywhere."""
    return case[1] > 1 if wrong in ("c_not_carried", "no_forget_bias") else True


def blob_len(S, H):
    return (S + H + 1) * 4 * H


def unpack(blob, S, H):
    n = (S + H) * 4 * H
    return np.asarray(blob[:n]).reshape(S + H, 4 * H), np.asarray(blob[n:n + 4 * H])


def pack(kernel, bias):
    return np.concatenate([np.asarray(kernel, dtype=np.float32).reshape(-1), np.asarray(bias, dtype=np.float32).reshape(-1)])


def sigmoid64(z):
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-z))


def lstm_f64(x, blob, S, H, forget_bias=FORGET_BIAS, h0=None, c0=None, wrong=None):
    """(h_T, c_T) in float64 on float32 (or narrower) data.  `wrong`: one of WRONG, a restatement with that one rule wrong."""
    x = np.asarray(x, dtype=np.float64)
    rows, T = x.shape[0], x.shape[1]
    kernel, bias = (v.astype(np.float64) for v in unpack(blob, S, H))
    if wrong == "kernel_transposed":                                 # torch's [4H, S + H] orientation read as TF's
        kernel = np.asarray(blob[:(S + H) * 4 * H], dtype=np.float64).reshape(4 * H, S + H).T
    h = np.zeros((rows, H)) if h0 is None else np.asarray(h0, dtype=np.float64)
    c = np.zeros((rows, H)) if c0 is None else np.asarray(c0, dtype=np.float64)
    start = c
    for t in range(T):
        a = np.concatenate([h, x[:, t]] if wrong == "h_before_x" else [x[:, t], h], axis=1)
        z = a @ kernel + bias
        if wrong == "gate_order_ifjo":
            i, f, j, o = (z[:, g * H:(g + 1) * H] for g in range(4))
        else:
            i, j, f, o = (z[:, g * H:(g + 1) * H] for g in range(4))
        fb = 0.0 if wrong == "no_forget_bias" else forget_bias
        old = start if wrong == "c_not_carried" else c
        if wrong == "forget_bias_on_i":
            c = old * sigmoid64(f) + sigmoid64(i + fb) * np.tanh(j)
        elif wrong == "tanh_sigmoid_swapped_on_j":
            c = old * sigmoid64(f + fb) + np.tanh(i) * sigmoid64(j)
        else:
            c = old * sigmoid64(f + fb) + sigmoid64(i) * np.tanh(j)
        h = np.tanh(old if wrong == "h_from_old_c" else c) * sigmoid64(o)
    return h, c


def dense_serial_f32(a, W):
    """``a @ W`` as a serial k-ordered float32 chain: every product exact in float64 (24 x 24 bits), every sum rounded to
    float32 - the documented result of the f32-input MFMA, one rounding per term."""
    acc = np.zeros((a.shape[0], W.shape[1]), dtype=np.float32)
    a64, W64 = a.astype(np.float64), W.astype(np.float64)
    for k in range(W.shape[0]):
        acc = (acc.astype(np.float64) + a64[:, k:k + 1] * W64[k:k + 1, :]).astype(np.float32)
    return acc


def lstm_serial_f32(x, blob, S, H, forget_bias=FORGET_BIAS, h0=None, c0=None):
    """A float32 host evaluation: dense sums as `dense_serial_f32`, NumPy float32 exp / tanh, the cell left to right."""
    x = np.asarray(x).astype(np.float32)
    rows, T = x.shape[0], x.shape[1]
    kernel, bias = (v.astype(np.float32) for v in unpack(blob, S, H))
    one, fb = np.float32(1), np.float32(forget_bias)
    h = np.zeros((rows, H), dtype=np.float32) if h0 is None else np.asarray(h0, dtype=np.float32)
    c = np.zeros((rows, H), dtype=np.float32) if c0 is None else np.asarray(c0, dtype=np.float32)

    def sig(z):
        return one / (one + np.exp(-z))
    for t in range(T):
        z = dense_serial_f32(np.concatenate([x[:, t], h], axis=1), kernel) + bias
        i, j, f, o = (z[:, g * H:(g + 1) * H] for g in range(4))
        c = c * sig(f + fb) + sig(i) * np.tanh(j)
        h = np.tanh(c) * sig(o)
        assert h.dtype == c.dtype == np.float32
    return h, c


def torch_lstm_of(blob, S, H, forget_bias, dtype):
    """A CPU ``torch.nn.LSTM`` holding the blob's cell, the inverse of `pack_torch_lstm`: torch's blocks i, f, g, o are TF's
    i, f, j, o; ``b_ih`` takes the bias with `forget_bias` added on f, ``b_hh`` zeros."""
    import torch
    kernel, bias = (torch.from_numpy(v.astype(np.float64)) for v in unpack(blob, S, H))
    lstm = torch.nn.LSTM(S, H, batch_first=True).to(dtype)
    tf_block = {0: 0, 1: 2, 2: 1, 3: 3}                              # torch block -> TF block
    with torch.no_grad():
        for g, n in tf_block.items():
            w = kernel[:, n * H:(n + 1) * H].t()                     # [H, S + H]
            lstm.weight_ih_l0[g * H:(g + 1) * H] = w[:, :S].to(dtype)
            lstm.weight_hh_l0[g * H:(g + 1) * H] = w[:, S:].to(dtype)
            lstm.bias_ih_l0[g * H:(g + 1) * H] = (bias[n * H:(n + 1) * H] + (forget_bias if n == 2 else 0.0)).to(dtype)
        lstm.bias_hh_l0.zero_()
    return lstm


def pack_torch_lstm(lstm, forget_bias):
    """The blob of a one-layer, unidirectional ``torch.nn.LSTM``: gate blocks i, f, g, o -> i, j, f, o (torch's g is TF's
    j), the weights transposed and stacked as ``[W_ih; W_hh]``, ``bias = b_ih + b_hh`` with `forget_bias` subtracted on the
    f block (torch adds none).  Float32, as a device blob is."""
    H = lstm.hidden_size
    w = np.concatenate([lstm.weight_ih_l0.detach().double().numpy(), lstm.weight_hh_l0.detach().double().numpy()], axis=1)
    b = lstm.bias_ih_l0.detach().double().numpy() + lstm.bias_hh_l0.detach().double().numpy()
    order = (0, 2, 1, 3)                                             # TF block n is torch block order[n]
    kernel = np.concatenate([w[g * H:(g + 1) * H].T for g in order], axis=1)
    bias = np.concatenate([b[g * H:(g + 1) * H] - (forget_bias if n == 2 else 0.0) for n, g in enumerate(order)])
    return pack(kernel, bias)


def torch_lstm_eval(x, blob, S, H, forget_bias, dtype):
    import torch
    lstm = torch_lstm_of(blob, S, H, forget_bias, dtype)
    with torch.no_grad():
        out, (h, c) = lstm(torch.from_numpy(np.asarray(x)).to(dtype))
    assert torch.equal(out[:, -1], h[0])
    return h[0].numpy(), c[0].numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ---- the real-valued cases ----
def real_case(rows, T, S, H, seed):
    """Glorot-uniform kernel (what ``BasicLSTMCell`` gets from ``tf.get_variable`` with no initializer, as far as that is
    remembered: ``U(-l, l)``, ``l = sqrt(6 / ((S + H) + 4H))``), bias ~ N(0, 0.1), x ~ N(0, 1) in float32.  -> (x, blob)."""
    rng = np.random.default_rng(2000 + seed)
    limit = np.sqrt(6.0 / ((S + H) + 4 * H))
    kernel = rng.uniform(-limit, limit, (S + H, 4 * H))
    bias = rng.normal(0.0, 0.1, (4 * H,))
    return rng.normal(0.0, 1.0, (rows, T, S)).astype(np.float32), pack(kernel, bias)


def real_state(rows, H, seed):
    rng = np.random.default_rng(3000 + seed)
    return rng.uniform(-0.9, 0.9, (rows, H)).astype(np.float32), rng.normal(0.0, 1.0, (rows, H)).astype(np.float32)


# ---- the dyadic cases: every pre-activation an exact multiple of 1/64 in [-4, 4] ----
GRID = 64
ZMAX = 4


def dyadic_case(rows, S, H, seed, through_h):
    """One step whose pre-activations are exact in any order of summation: at most six non-zero small integers per row of
    ``a = [x, h0]`` (in x with `through_h` false, in h0 otherwise: x is then zero and c0 a multiple of 1/8), an
    asymmetric kernel of multiples of 1/64 and a bias that moves with unit and gate.  Asserts that every z is a multiple of
    1/64 within [-4, 4] and that z differs between rows, units and gates.  -> (x [rows, 1, S], blob, h0, c0, z [rows, 4H]
    float64), h0 and c0 None without `through_h`."""
    rng = np.random.default_rng(4000 + seed)
    n = H if through_h else S
    a = np.zeros((rows, n))
    for r in range(rows):
        cols = rng.choice(n, size=min(n, 6), replace=False)
        a[r, cols] = rng.integers(1, 3, cols.size) * rng.choice([-1, 1], cols.size)
    a[:, 0] = (np.arange(rows) % 5) - 2                              # the row shows in every z
    part = rng.integers(-5, 6, (n, 4 * H)) / GRID
    part[0, :] = (1 + (np.arange(4 * H) % 3)) / GRID
    kernel = rng.integers(-3, 4, (S + H, 4 * H)) / GRID              # the other block: whatever, it meets zeros
    if through_h:
        kernel[S:] = part
    else:
        kernel[:S] = part
    bias = (((np.arange(4 * H) * 37) % 129) - 64) / GRID
    full = np.zeros((rows, S + H))
    full[:, S:] = a if through_h else 0
    full[:, :S] = 0 if through_h else a
    z = full @ kernel + bias
    assert np.array_equal(z * GRID, np.round(z * GRID)) and np.abs(z).max() <= ZMAX
    assert len(np.unique(z)) > min(60, rows * H) and (np.ptp(z, axis=0) > 0).all() == (rows > 1)
    x = full[:, None, :S].astype(np.float32)
    if not through_h:
        return x, pack(kernel, bias), None, None, z
    c0 = (rng.integers(-16, 17, (rows, H)) / 8).astype(np.float32)
    return x, pack(kernel, bias), full[:, S:].astype(np.float32), c0, z


def table_arguments():
    """Every value a dyadic case's sigmoid or tanh can meet: m / 64 for -4 <= m / 64 <= 4 + FORGET_BIAS."""
    return (np.arange(-ZMAX * GRID, (ZMAX + 1) * GRID + 1) / GRID).astype(np.float32)


def dyadic_expected(z, H, c0, table_sigmoid, table_tanh, tanh_of):
    """(h_T, c_T) of a dyadic case in float32 from given sigmoid / tanh values - a device's own, read out of its kernel -,
    one float32 rounding per operation: `table_sigmoid` / `table_tanh` map the index of `table_arguments` to values,
    `tanh_of(values)` evaluates the same tanh at other points."""
    args = table_arguments()
    idx = lambda v: np.round((np.asarray(v, dtype=np.float64) - float(args[0])) * GRID).astype(np.int64)
    i, j, f, o = (z[:, g * H:(g + 1) * H] for g in range(4))
    old = np.zeros(i.shape, dtype=np.float32) if c0 is None else c0
    c = old * table_sigmoid[idx(f + FORGET_BIAS)] + table_sigmoid[idx(i)] * table_tanh[idx(j)]
    assert c.dtype == np.float32
    h = tanh_of(c.reshape(-1)).reshape(c.shape) * table_sigmoid[idx(o)]
    return h.astype(np.float32), c


# ---- the transcendental sweep ----
def f32_neighbours(v, n=64):
    """The float32 values from n below to n above `v` (positive, normal)."""
    bits = np.float32(v).view(np.uint32).astype(np.int64)
    return np.arange(bits - n, bits + n + 1).astype(np.uint32).view(np.float32)


def saturation_threshold(fn64):
    """The smallest float32 z in [1, 64] with RN_float32(fn64(z)) == 1."""
    lo, hi = int(np.float32(1).view(np.uint32)), int(np.float32(64).view(np.uint32))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        z = np.array([mid], dtype=np.uint32).view(np.float32)
        if np.float32(fn64(z.astype(np.float64))[0]) == np.float32(1):
            hi = mid
        else:
            lo = mid
    return np.array([hi], dtype=np.uint32).view(np.float32)[0]


def sweep_arguments():
    """Both signs of: every binade from 2^-100 to 2^6 with 4096 evenly spaced mantissas each, and the 64 float32
    neighbours on each side of 2^-12, 0.5, 1, the two saturation thresholds and 87.  All normal floats."""
    mant = 1.0 + np.arange(4096) / 4096.0
    pos = [np.ldexp(mant, e).astype(np.float32) for e in range(-100, 7)]
    for v in (2.0 ** -12, 0.5, 1.0, saturation_threshold(sigmoid64), saturation_threshold(np.tanh), 87.0):
        pos.append(f32_neighbours(v))
    pos = np.unique(np.concatenate(pos))
    return np.concatenate([-pos[::-1], pos])


MIDPOINT_REL = 2.0 ** -45      # closer than this (relative) to a float32 rounding midpoint: float64 does not decide, mpmath does


def _mp_value(kind, z):
    import mpmath
    mpmath.mp.prec = 200
    z = mpmath.mpf(float(z))
    return 1 / (1 + mpmath.exp(-z)) if kind == "sigmoid" else mpmath.tanh(z)


def mp_round(kind, z):
    """(RN_float32 of the true value, its relative distance from the nearest float32 rounding midpoint), all in mpmath."""
    import mpmath
    v = _mp_value(kind, z)
    near = np.float32(float(v))
    cands = sorted({float(np.nextafter(near, np.float32(-np.inf))), float(near), float(np.nextafter(near, np.float32(np.inf)))})
    best = min(cands, key=lambda c: abs(v - mpmath.mpf(c)))
    mids = [(mpmath.mpf(a) + mpmath.mpf(b)) / 2 for a, b in zip(cands[:-1], cands[1:])]
    rel = min(abs(v - m) for m in mids) / abs(v) if v != 0 else mpmath.mpf(1)
    return np.float32(best), float(rel)


def correctly_rounded(kind, z):
    """RN_float32 of sigmoid / tanh at the float32 arguments `z` (finite, non-zero), and per argument the relative distance
    of the true value from the nearest rounding midpoint (as far as it matters: exact below MIDPOINT_REL, else the float64
    figure).  The true value is the float64 evaluation's; where that lies within MIDPOINT_REL of a midpoint mpmath decides."""
    z = np.asarray(z, dtype=np.float32)
    v = sigmoid64(z) if kind == "sigmoid" else np.tanh(z.astype(np.float64))
    rn = v.astype(np.float32)
    below, above = np.nextafter(rn, np.float32(-np.inf)).astype(np.float64), np.nextafter(rn, np.float32(np.inf)).astype(np.float64)
    r64 = rn.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.minimum(np.abs(v - (r64 + below) / 2), np.abs(v - (r64 + above) / 2)) / np.abs(v)
    rel = np.where(np.isfinite(rel), rel, 1.0)
    for n in np.flatnonzero(rel < MIDPOINT_REL):
        rn[n], rel[n] = mp_round(kind, z[n])
    return rn, rel
