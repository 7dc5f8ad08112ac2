"""Host statement of `diral_qnet_forward` (include/diral_env.h) in NumPy float64, shared by tests/test_qnet_cases.py (no
device: the statement against torch's CPU graph, wrong restatements told apart) and tests/test_gpu_qnet.py (the kernel
against the statement), with the case generators both use.  tests/qnet_ordered.py is the same chain in float32 in the
kernel's documented order, which tests/test_gpu_qnet_ordered.py holds the kernel to bit for bit.

The chain is the reference's ``DRQN._create_network`` (algorithms/drl_drqn.py:109-155):
``[matmul + bias -> relu -> layer_norm] x L``, then ``matmul + bias``; the blob holds per hidden layer ``W [in, out]``,
``b``, ``gamma``, ``beta`` and then ``W_out``, ``b_out``."""
import numpy as np

# rows x D x hidden x A: every value of the issue's lists at least once, (96, 40) with 65 rows; and a first layer of more
# than 256 columns (two LDS chunks and an odd tail), the one other path the kernel has
SHAPES = [(1, 3, (), 3), (31, 23, (64,), 3), (64, 52, (256, 256), 32), (65, 23, (96, 40), 64),
          (193, 256, (256, 256, 256), 32), (193, 52, (), 64), (65, 256, (64,), 32), (31, 52, (96, 40), 3),
          (65, 515, (64,), 3)]
WRONG = ("norm_before_relu", "unbiased", "eps_1e-5", "w_transposed", "gamma_beta_swapped", "padded_stats", "relu_on_output")
EPS = 1e-12
MIN_VAR = 1e-2          # real_case: the smallest variance a row may have in front of a layer norm
# The tolerance of the chain with layer norm, relative to max |q| of a case.  Measured on the host, never on the kernel:
# the largest error against qnet_f64 over real_case(*shape, seed=1) for the SHAPES with a hidden layer, of
#   qnet_serial_f32 (dense layers as serial k-ordered float32 chains)          3.183e-05
#   QNet.torch_module() in float32 on the CPU                                   3.691e-05
# (both at 193 x 256 -> 256 -> 256 -> 256 -> 32: W >= 0 makes a row's columns alike, so the layer norm divides by a small
# deviation three times over), times 4 because the kernel's layer-norm sums run in an order of their own.
# tests/test_qnet_cases.py recomputes both.
MEASURED_SERIAL = 3.183133e-05
MEASURED_TORCH = 3.691303e-05
TOL_REL = 4 * max(MEASURED_SERIAL, MEASURED_TORCH)
# The same figure for tests/qnet_ordered.py's qnet_ordered_f32, the header's rules in the header's order (at the same shape;
# tests/test_qnet_ordered.py recomputes it).  No tolerance comes from it: the kernel is held to that statement in bits.
MEASURED_ORDERED = 1.517816e-05


def shape_id(shape):
    rows, D, hidden, A = shape
    return "r%d-D%d-h%s-A%d" % (rows, D, "x".join(str(h) for h in hidden) or "0", A)


def widths_of(D, hidden, A):
    return [int(D)] + [int(h) for h in hidden] + [int(A)]


def layout(widths):
    """{name: (offset, shape)} in blob order - written out here on its own, not imported from the package."""
    out, off, L = {}, 0, len(widths) - 2
    for l in range(L + 1):
        i, o = widths[l], widths[l + 1]
        tag = str(l + 1) if l < L else "_out"
        out["W" + tag] = (off, (i, o))
        off += i * o
        for name in ("b", "gamma", "beta") if l < L else ("b",):
            out[name + tag] = (off, (o,))
            off += o
    return out


def blob_len(widths):
    off, shape = list(layout(widths).values())[-1]
    return off + shape[0]


def unpack(blob, widths):
    return {k: np.asarray(blob[off:off + int(np.prod(shape))]).reshape(shape) for k, (off, shape) in layout(widths).items()}


def pack(named, widths):
    blob = np.zeros((blob_len(widths),), dtype=np.float32)
    for k, (off, shape) in layout(widths).items():
        blob[off:off + int(np.prod(shape))] = np.asarray(named[k], dtype=np.float32).reshape(-1)
    return blob


def qnet_f64(x, blob, widths, norm=True, eps=EPS, wrong=None, variances=None):
    """The chain in float64 on float32 (or narrower) data.  `wrong`: one of WRONG, a restatement with that one rule wrong;
    `variances`: a list that gets every hidden layer's per-row variance appended."""
    p = {k: v.astype(np.float64) for k, v in unpack(blob, widths).items()}
    h, L = np.asarray(x, dtype=np.float64), len(widths) - 2

    def moments_norm(r, gamma, beta):
        n = r.shape[1]
        if wrong == "padded_stats":                                  # the statistics over the MFMA tile's zero padding too
            n = -(-n // 32) * 32
            mean = r.sum(axis=1, keepdims=True) / n
            var = (((r - mean) ** 2).sum(axis=1, keepdims=True) + (n - r.shape[1]) * mean ** 2) / n
        else:
            mean = r.sum(axis=1, keepdims=True) / n
            var = ((r - mean) ** 2).sum(axis=1, keepdims=True) / (n - 1 if wrong == "unbiased" else n)
        if variances is not None:
            variances.append(var[:, 0])
        e = 1e-5 if wrong == "eps_1e-5" else eps
        if wrong == "gamma_beta_swapped":
            gamma, beta = beta, gamma
        return (r - mean) * (1.0 / np.sqrt(var + e)) * gamma + beta

    for l in range(1, L + 1):
        W, b, gamma, beta = (p["%s%d" % (k, l)] for k in ("W", "b", "gamma", "beta"))
        if wrong == "w_transposed" and W.shape[0] == W.shape[1]:
            W = W.T
        z = h @ W + b
        if wrong == "norm_before_relu" and norm:
            h = np.maximum(moments_norm(z, gamma, beta), 0.0)
        else:
            h = np.maximum(z, 0.0)
            if norm:
                h = moments_norm(h, gamma, beta)
    W = p["W_out"]
    if wrong == "w_transposed" and W.shape[0] == W.shape[1]:
        W = W.T
    q = h @ W + p["b_out"]
    return np.maximum(q, 0.0) if wrong == "relu_on_output" else q


def dense_serial_f32(h, W):
    """A dense layer as a serial k-ordered float32 chain: every product exact in float64 (24 x 24 bits), every sum rounded
    to float32 - the documented result of the f32-input MFMA, one rounding per term."""
    acc = np.zeros((h.shape[0], W.shape[1]), dtype=np.float32)
    h64, W64 = h.astype(np.float64), W.astype(np.float64)
    for k in range(W.shape[0]):
        acc = (acc.astype(np.float64) + h64[:, k:k + 1] * W64[k:k + 1, :]).astype(np.float32)
    return acc


def qnet_serial_f32(x, blob, widths, norm=True, eps=EPS):
    """A float32 host evaluation whose dense layers are `dense_serial_f32`; everything else plain NumPy float32 (its
    sums in NumPy's own order)."""
    p, L = unpack(blob, widths), len(widths) - 2
    h = np.asarray(x).astype(np.float32)
    for l in range(1, L + 1):
        h = np.maximum(dense_serial_f32(h, p["W%d" % l]) + p["b%d" % l], np.float32(0))
        if norm:
            n = np.float32(h.shape[1])
            mean = h.sum(axis=1, keepdims=True, dtype=np.float32) / n
            d = h - mean
            var = (d * d).sum(axis=1, keepdims=True, dtype=np.float32) / n
            h = d * (np.float32(1) / np.sqrt(var + np.float32(eps))) * p["gamma%d" % l] + p["beta%d" % l]
    return dense_serial_f32(h, p["W_out"]) + p["b_out"]


# ---- the exact-integer cases ----
def integer_case(rows, D, hidden, A, seed):
    """x in [0, 3], weights in {-1, 0, 1} (thinned for three hidden layers), biases in [-2, 2], for the chain WITHOUT layer
    norm.  Asserts |b| + sum |a| |w| < 2^24 at every layer: every partial sum is then an integer below 2^24 in magnitude,
    exact in float32 in any order, and the chain has one float32 value, bit for bit.  -> (x, blob, widths, q) with q the
    integer statement as float32.  The weights are asymmetric, so a transposed fragment shows."""
    rng = np.random.default_rng(seed)
    widths = widths_of(D, hidden, A)
    keep = 0.12 if len(hidden) == 3 else 0.6
    x = rng.integers(0, 4, (rows, D)).astype(np.int64)
    named, h = {}, x
    for l in range(len(widths) - 1):
        i, o = widths[l], widths[l + 1]
        tag = str(l + 1) if l < len(hidden) else "_out"
        W = rng.integers(-1, 2, (i, o)) * (rng.random((i, o)) < keep)
        W[0, :] = 1                                                  # no all-zero column
        W[:, 0] = -1 if i > 1 else W[:, 0]
        W[0, 0] = 1
        b = rng.integers(-2, 3, (o,))
        if i == o and i > 1:
            assert (W != W.T).any()
        bound = np.abs(h) @ np.abs(W) + np.abs(b)
        assert bound.max() < 2 ** 24, (l, int(bound.max()))
        named["W" + tag], named["b" + tag] = W, b
        z = h @ W + b
        if l < len(hidden):
            named["gamma" + tag], named["beta" + tag] = np.full((o,), 7), np.full((o,), -3)      # never read with norm = 0
            h = np.maximum(z, 0)
            assert (h > 0).any(axis=0).sum() > o // 4                # the relu leaves something to multiply
        else:
            q = z
    return x.astype(np.float32), pack(named, widths), widths, q.astype(np.float32)


# ---- the real-valued cases ----
def real_case(rows, D, hidden, A, seed):
    """Parameters as ``QNet(init="reference")`` draws them - W ~ U[0, 1), hidden biases 0.1, output bias 0 - with a random
    gamma in [0.5, 1.5) and beta in [-0.5, 0.5); x ~ U[-0.5, 1) in float32.  Asserts that every row's variance in front
    of every layer norm is above MIN_VAR, where the values themselves are of the order 1 and more (a row of equal values
    would make 1 / sqrt(var + eps) of the order 1e6 and the comparison meaningless).  -> (x, blob, widths)."""
    widths = widths_of(D, hidden, A)
    for attempt in range(50):                                        # a draw with a nearly dead row is drawn again
        rng = np.random.default_rng(1000 + seed + 7919 * attempt)
        named = {}
        for k, (off, shape) in layout(widths).items():
            if k.startswith("W"):
                named[k] = rng.random(shape)
            elif k.startswith("gamma"):
                named[k] = 0.5 + rng.random(shape)
            elif k.startswith("beta"):
                named[k] = rng.random(shape) - 0.5
            else:
                named[k] = np.full(shape, 0.0 if k == "b_out" else 0.1)
        blob = pack(named, widths)
        x = (rng.random((rows, D)) * 1.5 - 0.5).astype(np.float32)
        if D <= 3:
            x = np.abs(x) + np.float32(0.05)                         # (three inputs could all be negative: a zero row)
        variances = []
        qnet_f64(x, blob, widths, True, EPS, variances=variances)
        if all(var.min() > MIN_VAR for var in variances):
            break
    for l, var in enumerate(variances):
        assert var.min() > MIN_VAR, (l, float(var.min()))
    return x, blob, widths


def dense_bound(x, blob, widths):
    """L = 0: |err| <= gamma_{D + 1} (|b| + sum |x| |w|) with gamma_n = n u / (1 - n u), u = 2^-24 - D products-and-sums
    and the bias addition, each rounded once."""
    p = unpack(blob, widths)
    n = widths[0] + 1
    g = n * 2.0 ** -24 / (1 - n * 2.0 ** -24)
    return g * (np.abs(np.asarray(x, dtype=np.float64)) @ np.abs(p["W_out"].astype(np.float64)) + np.abs(p["b_out"].astype(np.float64)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ---- the wiring case: a toy-size env's shapes, B = 8 ----
WIRING = dict(B=8, N=4, A=3, hidden=(64,), seed=4)


def wiring_case(S):
    """States of B x N agents in [0, 1) (a CPU draw, so that the cap below can be checked without a device) and a
    reference-initialised chain S -> 64 -> A with random gamma and beta.  -> (states [B, N, S] float32, blob, widths)."""
    w = WIRING
    _, blob, widths = real_case(1, S, w["hidden"], w["A"], seed=w["seed"])
    rng = np.random.default_rng(w["seed"])
    return rng.random((w["B"], w["N"], S)).astype(np.float32), blob, widths


def decided(q64, tol):
    """Rows whose two largest Q-values differ by more than `tol` (absolute): their arg-max is not the rounding's to move."""
    top = np.sort(q64, axis=1)
    return (top[:, -1] - top[:, -2]) > tol
