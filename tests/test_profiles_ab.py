"""profiles/ab.py, the harness of the timing scripts, with a scripted timer in place of the device's, and the loader's
`bind` / `use` that it stands on.  No GPU needed."""
import importlib.util
import os
import re

import pytest

from diral_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("profiles_ab", os.path.join(ROOT, "profiles", "ab.py"))
ab = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ab)

# the six line pairs of profiles/slot_request/bench_guard.txt: (parent rounds, branch rounds, the file's verdict line)
GUARD = (
    ((44.205, 43.833, 43.792, 43.574, 44.094, 44.001), (43.912, 44.026, 43.827, 43.812, 43.899, 43.972),
     "  parent median 43.917  spread 43.574 ... 44.205 (1.44 % of the median)   branch median 43.905 (-0.03 % vs parent)   within"),
    ((54.114, 53.128, 54.328, 54.205, 54.040, 53.104), (54.127, 53.295, 53.343, 53.851, 53.159, 53.699),
     "  parent median 54.077  spread 53.104 ... 54.328 (2.26 % of the median)   branch median 53.521 (-1.03 % vs parent)   within"),
    ((55.408, 55.189, 54.442, 55.001, 54.647, 54.994), (55.584, 54.986, 54.799, 55.634, 54.990, 55.361),
     "  parent median 54.997  spread 54.442 ... 55.408 (1.76 % of the median)   branch median 55.175 (+0.32 % vs parent)   within"),
    ((51.111, 50.911, 50.420, 50.993, 50.531, 50.994), (50.904, 50.929, 50.568, 50.356, 50.613, 50.844),
     "  parent median 50.952  spread 50.420 ... 51.111 (1.36 % of the median)   branch median 50.728 (-0.44 % vs parent)   within"),
    ((24.128, 24.137, 24.498, 24.229, 24.388, 24.271), (24.418, 24.329, 24.187, 24.371, 24.144, 24.215),
     "  parent median 24.250  spread 24.128 ... 24.498 (1.53 % of the median)   branch median 24.272 (+0.09 % vs parent)   within"),
    ((57.191, 57.331, 57.108, 56.774, 57.219, 57.571), (56.634, 56.541, 56.886, 56.662, 55.722, 56.122),
     "  parent median 57.205  spread 56.774 ... 57.571 (1.39 % of the median)   branch median 56.588 (-1.08 % vs parent)   "
     "BELOW the spread by 0.187 us (faster)"),
)


def scripted(log, ms):
    """A timer that runs the body, logs the bracket and returns the next scripted milliseconds."""
    it = iter(ms)

    def timer(body):
        log.append("start")
        body()
        log.append("stop")
        return next(it)
    return timer


def test_timed_rounds_order_warm_rounds_and_values():
    log = []
    forms = [dict(form="a"), dict(form="b")]
    ms = [float(i) for i in range(1, 9)]                            # (1 warm + 3 timed rounds) x 2 forms
    ab.timed_rounds(forms, lambda f: log.append("run " + f["form"]), rounds=3, warm=1, reps=2,
                    between=lambda f: log.append("between " + f["form"]), timer=scripted(log, ms))
    one = ["between %s", "start", "run %s", "run %s", "stop"]
    assert log == [x % f if "%" in x else x for _ in range(4) for f in "ab" for x in one]     # forms inner, rounds outer
    assert forms[0]["ms"] == [3.0, 5.0, 7.0] and forms[1]["ms"] == [4.0, 6.0, 8.0]            # the first round is dropped
    us, rnd = ab.summary(forms, units=2)
    assert us == {"a": 2500.0, "b": 3000.0} and rnd == {"a": [1500.0, 2500.0, 3500.0], "b": [2000.0, 3000.0, 4000.0]}


def test_timed_rounds_without_between_and_reps():
    log = []
    forms = [dict(form="a", body=lambda: log.append("body"))]
    ab.timed_rounds(forms, ab.own_body, rounds=2, warm=0, timer=scripted(log, [0.5, 0.25]))
    assert log == ["start", "body", "stop"] * 2 and forms[0]["ms"] == [0.5, 0.25]


@pytest.mark.parametrize("values", [[3.0, 1.0, 2.0], [4.0, 1.0, 3.0, 2.0], [5.0], [2.0, 1.0],
                                    [44.205, 43.833, 43.792, 43.574, 44.094, 44.001]])
def test_median_is_the_scripts(values):
    assert ab.median(values) == sorted(values)[len(values) // 2]


def test_median_of_an_even_count_is_the_upper_middle_one():
    assert ab.median([4.0, 1.0, 3.0, 2.0]) == 3.0
    assert ab.per_unit(2.5, 25) == 100.0
    assert ab.spread([4.0, 1.0, 3.0, 2.0]) == (1.0, 4.0, 100.0)


NUMBER = re.compile(r"[-+]?\d+\.\d+")


@pytest.mark.parametrize("parent, branch, line", GUARD)
def test_verdict_reproduces_the_committed_guard(parent, branch, line):
    """The file's words exactly; its figures to one unit of their last printed digit: the file's medians come from the
    unrounded rounds, the literals here are its rounds as printed (three decimals, so the mean of two is off by at most
    0.0005 in front of the rounding of the print)."""
    got = ab.verdict(parent, branch)
    assert NUMBER.sub("#", got) == NUMBER.sub("#", line)
    assert got.split("   ")[-1] == line.split("   ")[-1]            # within / BELOW the spread by 0.187 us (faster)
    for a, b in zip(NUMBER.findall(got), NUMBER.findall(line)):
        assert len(a.split(".")[1]) == len(b.split(".")[1]) and abs(float(a) - float(b)) <= 1.01 * 10.0 ** -len(b.split(".")[1]), (a, b)


def test_verdict_words():
    lines = [ab.verdict(p, b) for p, b, _ in GUARD]
    assert [x.endswith("   within") for x in lines] == [True] * 5 + [False]
    assert "BELOW the spread by 0.187 us" in lines[5]
    assert ab.verdict([1.0, 2.0, 3.0], [3.5, 3.5, 3.5]).endswith("ABOVE the spread by 0.500 us (slower)")
    with open(os.path.join(ROOT, "profiles", "slot_request", "bench_guard.txt")) as fh:
        text = fh.read()
    assert all(line in text for _, _, line in GUARD)                # the literals above are that file's
    for p, b, _ in GUARD:
        assert all("  %s rounds: %s\n" % (n, " ".join("%.3f" % x for x in v)) in text for n, v in (("parent", p), ("branch", b)))


def test_bind_names_the_first_missing_symbol():
    """A real shared object that lacks every product symbol."""
    with pytest.raises(_lib.DiralLibraryError) as exc:
        _lib.bind(os.path.join(ROOT, "oracle", "libdiral_oracle.so"))
    assert str(exc.value) == "libdiral_env.so lacks symbol %s" % next(iter(_lib.SIGNATURES))
    with pytest.raises(_lib.DiralLibraryError, match="is missing"):
        _lib.bind(os.path.join(ROOT, "oracle", "no_such_library.so"))


def test_bind_touches_no_module_state_and_honours_lacking():
    product = _lib.load()
    first = next(iter(_lib.SIGNATURES))
    other = _lib.bind(_lib.LIB_PATH, lacking=(first,))
    assert _lib.load() is product and other is not product
    assert getattr(other, first).argtypes is None and getattr(product, first).argtypes is not None
    assert other.diral_env_step.argtypes == _lib.SIGNATURES["diral_env_step"][1]


def test_use_swaps_the_library_and_puts_it_back():
    product, x, y = _lib.load(), object(), object()
    with _lib.use(x) as got:
        assert got is x and _lib.load() is x
        with _lib.use(y):
            assert _lib.load() is y
        assert _lib.load() is x
    assert _lib.load() is product
    with pytest.raises(KeyError):
        with _lib.use(x):
            assert _lib.load() is x
            raise KeyError("inside")
    assert _lib.load() is product
