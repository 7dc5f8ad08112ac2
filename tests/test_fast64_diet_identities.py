"""What DESIGN.md 3.2 item 23 changed in the 64-vehicle step kernel, as far as it can be checked without a GPU.

* `column32` with the margin m in the fma's addend: s = trunc(y + m) where it was trunc(y) + m, y the fixed-point bin
  position (16 fraction bits).  Swept in NumPy for m = 1 ... 64, 1024, 16384 and y on a grid of eighths over
  [-2 m - 4, K 2^16 + 2 m + 4), K = 1, 20, 64: both forms count the same entries into the same bins, and every entry on
  which the two sums differ is in range and inside the band in BOTH - the float64 body decides it either way.
* `fast_lds_layout` (csrc/step_fast64.hpp), through a small host program compiled with the project's compiler and flags:
  for every K and A up to 64 and every flag set the kernels are instantiated with, the arrays are disjoint, aligned
  for their element types (the staging array to 16 bytes, and the histogram of the one-slot kernels, which zero it with
  16-byte stores), inside the total; in the one-slot kernels the arrays sized by neither K nor A sit at offsets that
  depend on the flags alone and the ones sized by A do not depend on K (the slot loops keep the earlier order); and the
  plain RICH workgroup of A <= 32, K <= 20 still fits eight times into a CU's 160 KiB."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "diral_amd", "csrc")


def _sums(i, m):
    """(old, new) sums of the grid points y = i / 8 (int64): trunc(y) + m and trunc(y + m), truncation towards zero."""
    t_old = np.where(i >= 0, i >> 3, -((-i) >> 3))
    j = i + 8 * m
    return t_old + m, np.where(j >= 0, j >> 3, -((-j) >> 3))


def _classify(s, K, m):
    """(counted, left for float64, bin) as column32 decides them from the sum, compared as unsigned 32-bit words."""
    u = s & 0xffffffff
    in_range = u < (K << 16) + 2 * m
    band = (u & 0xffff) < 2 * m
    return in_range & ~band, in_range & band, u >> 16


def test_margin_in_the_addend_counts_the_same_entries_into_the_same_bins():
    ms = list(range(1, 65)) + [1024, 16384]
    # y >= 0: the two sums are EQUAL, whatever K - one sweep over the longest range, in place
    top = 64 * 65536 + 2 * 16384 + 4
    i = np.arange(0, 8 * top, dtype=np.int32)
    t = i >> 3
    a, b = np.empty_like(i), np.empty_like(i)
    for m in ms:
        np.add(t, np.int32(m), out=a)
        np.add(i, np.int32(8 * m), out=b)
        np.right_shift(b, 3, out=b)
        assert np.array_equal(a, b), m
    # y < 0, and the windows around 0 and around K 2^16 where the range test and the band decide: everything, per K
    for K in (1, 20, 64):
        for m in ms:
            lo, hi = -2 * m - 4, K * 65536 + 2 * m + 4
            parts = [np.arange(8 * lo, 8 * min(2 * m + 4, hi), dtype=np.int64), np.arange(8 * max(lo, K * 65536 - 2 * m - 4), 8 * hi, dtype=np.int64)]
            i64 = np.unique(np.concatenate(parts))
            s_old, s_new = _sums(i64, m)
            c0, r0, b0 = _classify(s_old, K, m)
            c1, r1, b1 = _classify(s_new, K, m)
            assert np.array_equal(c0, c1), (K, m)
            assert np.array_equal(b0[c0], b1[c1]), (K, m)
            differ = s_old != s_new
            assert differ.any() and (i64[differ] < 0).all(), (K, m)          # (-m - 1, 0) only, and the sweep reaches it
            assert (r0[differ] & r1[differ]).all(), (K, m)
            # ... and what one form leaves for float64 the other does not count
            assert not (r0 & c1).any() and not (r1 & c0).any(), (K, m)


PROGRAM = r"""
#include <cstdio>
#include "step_fast64.hpp"
int main() {
  using namespace diral;
  // (rich, out64, flat, ratios, pol, ia): the one-slot instantiations, then the slot loops
  for (int f = 0; f < 16 + 8; ++f) {
    const bool pol = f >= 16;
    const bool rich = pol ? true : (f & 1), out64 = pol ? (f & 1) : (f & 2), flat = pol ? true : (f & 4);
    const bool ratios = pol ? (f & 2) : (f & 8), ia = pol && (f & 2) && (f & 4);
    if (pol && (f & 4) && !(f & 2)) continue;
    for (int K = 1; K <= 64; ++K)
      for (int A = 1; A <= 64; ++A) {
        const FastLds l = fast_lds_layout(K, A, rich, out64, flat, ratios, pol, ia);
        std::printf("%d %d %d %d %d %d %d %d  %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u\n", (int)rich, (int)out64, (int)flat,
                    (int)ratios, (int)pol, (int)ia, K, A, l.rv, l.edges, l.mask, l.act, l.hist, l.cnt, l.slow, l.inv, l.mtab, l.rtx, l.inr,
                    l.px, l.py, l.npx, l.rew, l.stage, l.nact, l.kvel, l.ia, l.total);
      }
  }
  return 0;
}
"""
FIELDS = "rv edges mask act hist cnt slow inv mtab rtx inr px py npx rew stage nact kvel ia total".split()


def test_lds_layout_of_the_step_kernel_through_a_host_program(tmp_path):
    from diral_amd import build
    src, exe = tmp_path / "layout.hip", tmp_path / "layout"
    src.write_text(PROGRAM)
    subprocess.check_call([build.hipcc_path()] + build.HIPCC_FLAGS + ["--cuda-host-only", "-I", CSRC, str(src), "-o", str(exe)])
    rows = np.array([[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)]).decode().splitlines()], dtype=np.int64)
    assert len(rows) == (16 + 6) * 64 * 64
    for row in rows:
        rich, out64, flat, ratios, pol, ia, K, A = (int(x) for x in row[:8])
        off = dict(zip(FIELDS, (int(x) for x in row[8:])))
        a32 = 32 if A <= 32 else 64
        es = 8 if out64 else 4
        # name -> (size in bytes, alignment); only the arrays this flag set has
        # (the slot loops, `pol`, keep the earlier order and zero the histogram word by word)
        size = dict(rv=(8 * a32, 8), edges=(8 * (K + 2), 8), mask=(8 * a32, 8), act=(256, 4), hist=(4 * ((K + 1) | 1) * 64, 4 if pol else 16),
                    cnt=(256, 4), slow=(16, 4), mtab=(64 * (a32 + 4), 4), px=(512, 8))
        if not out64:
            size["inv"] = (512, 8)
        if ratios:
            size["rtx"], size["inr"] = (512, 8), (256, 4)
        if rich:
            size["npx"], size["rew"], size["stage"] = (512, 8), (512, 8), (es * 64 * (a32 + 4), 16)
            if not flat:
                size["py"] = (512, 8)
        if pol:
            size["nact"], size["kvel"] = (256, 4), (512, 8)
        if ia:
            size["ia"] = (408, 8)
        spans = sorted((off[n], off[n] + s, n) for n, (s, _) in size.items())
        for (b0, e0, n0), (b1, e1, n1) in zip(spans, spans[1:]):
            assert e0 <= b1, (row[:8], n0, n1)
        assert spans[-1][1] <= off["total"] and off["total"] % 16 == 0 and off["total"] <= 65536, row[:8]
        for n, (_, al) in size.items():
            assert off[n] % al == 0, (row[:8], n)
        if rich and not out64 and flat and not ratios and not pol and A <= 32 and K <= 20:
            assert 8 * off["total"] <= 160 * 1024, row[:8]
    # what the offsets depend on
    key = rows[:, :6]
    for flags in np.unique(key, axis=0):
        if flags[4]:                                         # the slot loops: the earlier order
            continue
        sel = rows[(key == flags).all(axis=1)]
        fixed = [8 + FIELDS.index(n) for n in ("act", "cnt", "slow", "inv", "rtx", "inr", "px", "py", "npx", "rew", "nact", "kvel", "ia")]
        assert (sel[:, fixed] == sel[0, fixed]).all(), flags
        by_a = [8 + FIELDS.index(n) for n in ("mask", "rv", "mtab", "stage", "edges")]
        for wide in (False, True):
            s2 = sel[(sel[:, 7] > 32) == wide]
            assert (s2[:, by_a] == s2[0, by_a]).all(), (flags, wide)
