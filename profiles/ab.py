"""The one harness of the timing scripts in this directory: a second libdiral_env.so next to the tree's own, the interleaved
timing loop, the scripts' median, the parent-against-branch criterion of profiles/slot_request/bench_guard.txt, the equality
of two handles and the writer of a script's lines.  Plain Python: importing it needs no GPU, and the device timer is the
default of a parameter (tests/test_profiles_ab.py drives the arithmetic with a scripted one).
"""
import contextlib
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from diral_amd import _lib  # noqa: E402


def two_libraries(parent_path, lacking=()):
    """(parent, branch): the library built from the parent commit at `parent_path` - it predates the symbols in `lacking` -
    and the tree's own.  Handles built under `_lib.use(parent)` run on the parent's code."""
    parent, branch = _lib.bind(os.path.abspath(parent_path), lacking), _lib.load()
    assert ctypes.cast(parent.diral_env_step, ctypes.c_void_p).value != ctypes.cast(branch.diral_env_step, ctypes.c_void_p).value, \
        "the parent's library must be a second library"
    return parent, branch


def device_timer(body):
    """Milliseconds of body() between two device events, the device idle in front and behind."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    body()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def own_body(form):
    """The `run` of forms that carry a body of their own."""
    form["body"]()


def timed_rounds(forms, run, rounds, warm, reps=1, between=None, timer=device_timer):
    """Interleaved: every round times every form once (`reps` back-to-back run(form) calls inside one bracket), so that the
    box's drift meets all forms alike.  between(form) runs untimed in front of the bracket.  The first `warm` rounds are
    dropped; the milliseconds of the others are appended to form["ms"]."""
    for f in forms:
        f.setdefault("ms", [])
    for r in range(warm + rounds):
        for f in forms:
            if between is not None:
                between(f)

            def body():
                for _ in range(reps):
                    run(f)
            ms = timer(body)
            if r >= warm:
                f["ms"].append(ms)


def median(values):
    """The scripts' median: the upper middle one of an even count (the committed figures are these)."""
    return sorted(values)[len(values) // 2]


def per_unit(ms, units):
    """Milliseconds of `units` slots or calls -> microseconds of one."""
    return ms * 1e3 / units


def summary(forms, units=1, digits=2):
    """({form: median us per unit}, {form: every round's}) of timed forms, rounded as the records hold them."""
    us = {f["form"]: round(per_unit(median(f["ms"]), units), digits) for f in forms}
    return us, {f["form"]: [round(per_unit(m, units), digits) for m in f["ms"]] for f in forms}


def spread(values, mid=median):
    """(min, max, max - min in per cent of the median)."""
    lo, hi = min(values), max(values)
    return lo, hi, 100.0 * (hi - lo) / mid(values)


def verdict(parent_rounds, branch_rounds):
    """The criterion of profiles/slot_request/bench_guard.txt as that file words it: `within` where the branch's median lies
    inside min ... max of the parent's rounds, BELOW / ABOVE the spread by the distance otherwise.  That file's medians are
    the mean of the two middle rounds of its six (statistics.median), so this line's are too."""
    pm, bm = statistics.median(parent_rounds), statistics.median(branch_rounds)
    lo, hi, pct = spread(parent_rounds, statistics.median)
    word = "within"
    if bm < lo:
        word = "BELOW the spread by %.3f us (faster)" % (lo - bm)
    elif bm > hi:
        word = "ABOVE the spread by %.3f us (slower)" % (bm - hi)
    return "  parent median %.3f  spread %.3f ... %.3f (%.2f %% of the median)   branch median %.3f (%+.2f %% vs parent)   %s" % (
        pm, lo, hi, pct, bm, 100.0 * (bm / pm - 1.0), word)


def same_env(x, y):
    """Two handles hold the same envs: the exported state key by key, and the metrics."""
    import torch
    sa, sb = x.export_state(), y.export_state()
    return bool(all(torch.equal(sa[k], sb[k]) for k in sa) and torch.equal(x.metrics(), y.metrics()))


@contextlib.contextmanager
def report(out=None):
    """emit(line, record): the human line and the JSON record to stdout and, where a script has --out, to that file."""
    fh = None
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        fh = open(out, "w")

    def emit(line, record):
        for text in (line, json.dumps(record)):
            print(text, flush=True)
            if fh:
                fh.write(text + "\n")
                fh.flush()
    try:
        yield emit
    finally:
        if fh:
            fh.close()
