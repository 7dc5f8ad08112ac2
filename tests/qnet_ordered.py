"""The ORDERED float32 statement of `diral_qnet_forward`: rules 1-5 of csrc/qnet_kernel.hpp (the same text as
include/diral_env.h) in NumPy float32, one rounding where the header has one, in the header's order - so that the kernel can
be held to its header bit for bit (tests/test_gpu_qnet_ordered.py) and not only to a tolerance around the float64 statement
of tests/qnet_cases.py.  tests/test_qnet_ordered.py holds this module without a device: the fused multiply-add against exact
rational arithmetic, the statement against the integer cases and the float64 statement, and every `wrong=` form - the
statement with ONE rule off - against the right one, in bits.

The rules, as they are evaluated here (vectorised over rows and columns, serial over k):

1. dense: ``acc = fmaf(x[k], W[k][j], acc)`` from +0 over k = 0 .. in - 1, a correctly rounded fused multiply-add
   (`fmaf32`), then one float32 ``+ b[j]``;
2. relu: a NaN stays, everything else ``<= 0`` becomes +0;
3. layer norm: `sum4` is four partial sums, partial s over the columns s, s + 4, .. in turn from +0, added as
   ``((p0 + p1) + p2) + p3``; ``m0 = sum4(r) / h``, ``mean = m0 + sum4(r - m0) / h``, ``var = sum4((r - mean)^2) / h``;
4. ``rstd = 1 / sqrt(var + float32(eps))``, ``y = ((r - mean) * rstd) * gamma + beta``, every operation rounded to float32;
5. the output layer is rule 1 alone.

`ORDERED_SHAPES` is the lattice of smallest shapes that reach each branch of the kernel (the table in `LATTICE`), and
`ordered_case` draws their data: mixed-sign weights so that relus die, no variance floor - the comparison is bitwise, so
conditioning does not matter -, every magnitude a normal number or zero (the header says nothing about subnormals;
`qnet_ordered_f32(.., tiny=[])` reports the smallest non-zero magnitude it rounded to, and the CPU test holds it normal).
`padding_case` is the one case with infinities, for the zeros of the kernel's k padding; `first_difference` words a
mismatch by row, column and 32 x 32 tile."""
import numpy as np

from tests import qnet_cases as H

F32 = np.float32

# ---- the lattice: (rows, D, hidden, A), each the smallest shape that reaches its branch ----
LATTICE = [
    ((1, 1, (1,), 1), "every width minimal; only the odd tail runs; a layer norm of width 1 (var = 0, y = beta)"),
    ((33, 7, (7, 9), 65), "in < 8 at l = 0 and l = 1; in = 9; three output tiles with one live column in the last"),
    ((130, 8, (16,), 33), "in = 8 (one block, which loads itself again); in = 16 (a second block prefetched); 2 tail rows "
                          "in the third workgroup"),
    ((65, 257, (33,), 129), "a second chunk of one column; odd in = 33 at l > 0 (the pad column of act is read); five "
                            "output tiles, so only wave 0 owns a second tile"),
    ((64, 2, (255, 32), 200), "in = 2; eight tiles with the last partial; odd in = 255 at l > 0; a hidden layer of one "
                              "tile; seven output tiles"),
    ((32, 512, (256,), 64), "exactly two chunks; exactly one row tile"),
    ((127, 513, (200, 33, 129), 256), "three different hidden widths (off[]); a third chunk of one column; a full-width "
                                      "output layer"),
    ((129, 1024, (65,), 96), "the maximum D, four full chunks; 1 tail row in the third workgroup"),
    ((65, 511, (), 255), "L = 0 with eight output tiles"),
]
ORDERED_SHAPES = [shape for shape, _ in LATTICE]

# one rule off, each: the dense sum (rule 1), then the layer norm (rules 3 and 4)
WRONG_DENSE = ("product_rounded", "k_reversed", "pair_first")
WRONG_NORM = ("sum_sequential", "partials_pairwise", "mean_once", "rstd_f64", "rstd_gamma_first", "y_fused")
WRONG = WRONG_DENSE + WRONG_NORM


# ---- the fused multiply-add ----
def fmaf32(a, b, c):
    """``round_to_float32(a * b + c)`` with ONE rounding, for float32 arrays.  The product of two float32 values is exact
    in float64 (24 + 24 bits); its sum with c is rounded to float64 TO ODD - TwoSum gives the rounding error exactly, and
    where it is not zero and the sum's last mantissa bit is even the sum moves one float64 towards the error -, and a
    value rounded to odd at 53 >= 2 * 24 + 2 bits rounds on to float32 as the exact value would.  The repair is skipped
    where it cannot matter: the second rounding differs from that of the exact value only if the float64 sum lies exactly
    half way between two float32 values (every such point is a float64 value, and rounding is monotonic), which for a
    normal float32 result reads 0x10000000 in the 29 mantissa bits that float32 drops."""
    p = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.asarray(p + c)
        bits = s.view(np.uint64)
        risky = ((bits & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) | ((s != 0) & (np.abs(s) < 2.0 ** -126))
        if risky.any():
            t = s - p
            e = (p - (s - t)) + (c - t)                              # TwoSum: p + c == s + e exactly
            fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((bits & np.uint64(1)) == 0)
            s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def fmaf32_through_float64(a, b, c):
    """What `qnet_cases.dense_serial_f32` does: the sum rounded to float64 (to nearest) and then to float32 - two
    roundings, wrong where the first lands on a float32 tie."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F32)


# acc = 1 + 2^-23, a * b = 2^-24 - 2^-70: just BELOW the tie between 1 + 2^-23 and 1 + 2^-22, so the answer is 1 + 2^-23;
# float64 rounds the sum onto the tie, and the tie goes to even, 1 + 2^-22
DOUBLE_ROUNDING = (F32(2.0 ** -12 + 2.0 ** -35), F32(2.0 ** -12 - 2.0 ** -35), F32(1 + 2.0 ** -23))


class _Tiny:
    """The smallest non-zero magnitude among the values a statement rounded to."""

    def __init__(self, sink):
        self.sink = sink

    def __call__(self, v):
        if self.sink is not None:
            m = np.abs(v[np.isfinite(v) & (v != 0)])
            if m.size:
                self.sink.append(float(m.min()))
        return v


def dense_ordered_f32(h, W, wrong=None, seen=lambda v: v):
    """Rule 1 without the bias: [rows, in] x [in, out] as a k-ordered `fmaf32` chain from +0."""
    n = W.shape[0]
    acc = np.zeros((h.shape[0], W.shape[1]), dtype=F32)
    if wrong == "pair_first":                                        # a chain per k pair from zero, the pairs then added
        for k in range(0, n, 2):
            pair = fmaf32(h[:, k:k + 1], W[k:k + 1, :], np.zeros_like(acc))
            if k + 1 < n:
                pair = fmaf32(h[:, k + 1:k + 2], W[k + 1:k + 2, :], pair)
            acc = seen(acc + pair)
        return acc
    for k in (range(n - 1, -1, -1) if wrong == "k_reversed" else range(n)):
        if wrong == "product_rounded":                               # the product rounded in front of the addition
            acc = seen(acc + h[:, k:k + 1] * W[k:k + 1, :])
        else:
            acc = seen(fmaf32(h[:, k:k + 1], W[k:k + 1, :], acc))
    return acc


def sum4(v, wrong=None):
    """Rule 3's sum over the columns of v [rows, h] -> [rows, 1]."""
    n = v.shape[1]
    if wrong == "sum_sequential":
        s = np.zeros((v.shape[0],), dtype=F32)
        for c in range(n):
            s = s + v[:, c]
        return s[:, None]
    p = []
    for s in range(4):
        acc = np.zeros((v.shape[0],), dtype=F32)
        for c in range(s, n, 4):
            acc = acc + v[:, c]
        p.append(acc)
    if wrong == "partials_pairwise":
        return ((p[0] + p[1]) + (p[2] + p[3]))[:, None]
    return (((p[0] + p[1]) + p[2]) + p[3])[:, None]


def layer_norm_ordered_f32(r, gamma, beta, eps, wrong=None, seen=lambda v: v):
    """Rules 3 and 4 on r [rows, h] float32."""
    n = F32(r.shape[1])
    m0 = sum4(r, wrong) / n
    mean = m0 if wrong == "mean_once" else m0 + sum4(seen(r - m0), wrong) / n
    d = seen(r - mean)
    var = sum4(seen(d * d), wrong) / n
    if wrong == "rstd_f64":                                          # in float64 and rounded once, as a wider unit would
        rstd = (1.0 / np.sqrt(var.astype(np.float64) + np.float64(F32(eps)))).astype(F32)
    else:
        rstd = F32(1) / np.sqrt(var + F32(eps))
    assert m0.dtype == mean.dtype == var.dtype == rstd.dtype == F32
    if wrong == "rstd_gamma_first":
        return seen(d * (rstd * gamma) + beta)
    if wrong == "y_fused":
        return seen(fmaf32(d * rstd, gamma, beta))
    return seen(seen(seen(d * rstd) * gamma) + beta)


def exact_f32(x):
    """x (NumPy float32 / float16, or a torch tensor of float32 / float16 / bfloat16) as float32, exactly."""
    if isinstance(x, np.ndarray):
        assert x.dtype in (np.float32, np.float16), x.dtype
        return x.astype(F32)
    return x.detach().cpu().float().numpy()                          # (widening conversions are exact)


def qnet_ordered_f32(x, blob, widths, norm=True, eps=H.EPS, wrong=None, tiny=None, memo=None):
    """The header's rules 1-5 in float32, in the header's order.  `wrong`: one of WRONG, the statement with that one rule
    off; `tiny`: a list that gets the smallest non-zero magnitude of every rounded intermediate appended; `memo`: a dict
    of the caller's, one per (x, blob), that keeps the first layer's sums - the long chain over D, the same with and
    without layer norm and under every WRONG_NORM form - for the next call."""
    assert wrong is None or wrong in WRONG, wrong
    p, L, seen = H.unpack(np.asarray(blob, dtype=F32), widths), len(widths) - 2, _Tiny(tiny)
    h = exact_f32(x)
    assert h.ndim == 2 and h.shape[1] == widths[0]

    def dense(l, h, W):
        if l > 0 or memo is None or wrong in WRONG_DENSE or tiny is not None:
            return dense_ordered_f32(h, W, wrong, seen)
        if "first" not in memo:
            memo["first"] = dense_ordered_f32(h, W)
        return memo["first"]

    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(1, L + 1):
            z = seen(dense(l - 1, h, p["W%d" % l]) + p["b%d" % l])
            h = np.where(z > 0, z, np.where(np.isnan(z), z, F32(0)))
            if norm:
                h = layer_norm_ordered_f32(h, p["gamma%d" % l], p["beta%d" % l], eps, wrong, seen)
            assert h.dtype == F32
        q = seen(dense(L, h, p["W_out"]) + p["b_out"])
    assert q.dtype == F32
    return q


# ---- the lattice's data ----
def ordered_case(shape, seed):
    """x ~ U[-0.5, 1) (the one value in 800 below 2^-10 in magnitude moved out to it, so that x is a normal number in
    float16 as well), weights U[-1, 1) (mixed sign: relus die), biases U[-0.5, 0.5), gamma in [0.5, 1.5), beta in
    [-0.5, 0.5), all float32.  No variance floor.  -> (x, blob, widths)."""
    rows, D, hidden, A = shape
    widths = H.widths_of(D, hidden, A)
    rng = np.random.default_rng(7000 + seed)
    named = {}
    for k, (off, shp) in H.layout(widths).items():
        if k.startswith("W"):
            named[k] = rng.random(shp) * 2 - 1
        elif k.startswith("gamma"):
            named[k] = 0.5 + rng.random(shp)
        else:                                                        # b, beta
            named[k] = rng.random(shp) - 0.5
    x = (rng.random((rows, D)) * 1.5 - 0.5).astype(F32)
    x = np.where(np.abs(x) < F32(2.0 ** -10), np.copysign(F32(2.0 ** -10), x), x)    # (normal as float16 too: >= 2^-14)
    return x, H.pack(named, widths), widths


PAD_SHAPE = ORDERED_SHAPES[3]


def padding_case(seed):
    """The one case with infinities, on (65, 257, (33,), 129): what the kernel's zero padding multiplies must BE zero, not
    merely meet a zero.  Both widths in front of a dense layer are odd, so both layers end in a k pair whose second half
    is padding - the kernel zeroes it on both sides (the B value under a guard, the pad column of the LDS tile written as
    a zero) and on finite data either side alone would do: the other factor only ever meets an exact zero.
    * Every fifth row has x[33] = +inf and W1[33] is negative in every column: z1 = -inf and r1 = 0 throughout that row,
      q is the output layer of zeros.  x[33] is also what column 33 of the LDS tile held in front of the first layer's
      write - the pad column that the second layer's odd tail (in = 33) reads: left unwritten, inf * 0 is a NaN.
    * b1[5] = -inf: column 5 of the hidden layer is dead in every row.  b1 lies right behind W1 in the blob, where a row
      k = 257 of W1 would be: loaded without its guard in the first layer's odd tail, -inf * 0 is a NaN.
    -> (x, blob, widths); the statement of it is finite everywhere."""
    x, blob, widths = ordered_case(PAD_SHAPE, seed)
    p = H.unpack(blob, widths)                                       # views of the blob
    assert widths == [257, 33, 129] and np.abs(p["W1"][33]).min() > 0
    x[::5, 33] = np.inf
    p["W1"][33] = -np.abs(p["W1"][33])
    p["b1"][5] = -np.inf
    return x, blob, widths


# ---- where two results differ ----
def first_difference(got, want):
    """None where got and want are equal in bits (NaN equal to NaN); else one line: the first differing (row, column), the
    two values, and the number of differing elements per column tile (column // 32) and per row tile (row // 32) - which
    wave's 32 x 32 tile of which layer is off can be read from it without a second run."""
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    if got.shape != want.shape:
        return "shape %s against %s" % (got.shape, want.shape)
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    if not bad.any():
        return None
    r, c = (int(i) for i in np.argwhere(bad)[0])
    per_ct = np.bincount(np.nonzero(bad)[1] // 32, minlength=-(-got.shape[1] // 32))
    per_rt = np.bincount(np.nonzero(bad)[0] // 32, minlength=-(-got.shape[0] // 32))
    return ("%d of %d differ; first at (row %d, col %d): got %r (0x%08x) want %r (0x%08x); per column tile %s; per row tile %s"
            % (int(bad.sum()), bad.size, r, c, float(got[r, c]), int(got.view(np.uint32)[r, c]), float(want[r, c]),
               int(want.view(np.uint32)[r, c]), per_ct.tolist(), per_rt.tolist()))
