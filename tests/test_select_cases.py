"""`diral_policy_select` without a device: the host statement the GPU test compares against (tests/select_cases.py) equals
the actions the reference's policies returned (fixtures q1 ... q4, recorded by tests/golden/gen_policy_golden.py from
algorithms/policies.py under the recorded draws), restatements with one rule wrong are each told apart from it, the rows
the GPU test compares hold no ambiguous one, and the C-ABI of the entry point is what include/diral_env.h declares."""
import ctypes

import numpy as np
import pytest

from diral_amd import _lib
from diral_amd.config import (DT_BF16, DT_F32, ERR_BAD_ARG, ERR_UNSUPPORTED, SELECT_BOLTZMANN, SELECT_EPS_GREEDY,
                              SELECT_GREEDY, SELECT_SOFTMAX, DiralSelect)
from tests import select_cases as H


# ---- the statement against the reference's recorded actions ----
@pytest.mark.parametrize("A", [3, 32])
def test_statement_equals_the_reference_on_every_fixture_row(A):
    g = H.load_fixture("q1_greedy")[A]
    assert np.array_equal(H.greedy(g["Qs"]), g["actions"])
    assert np.isnan(g["Qs"]).any() and np.isinf(g["Qs"]).any() and np.signbit(g["Qs"][g["Qs"] == 0]).any()
    g = H.load_fixture("q2_eps_greedy")[A]
    act, explored = H.eps_greedy(g["Qs"], g["param"], g["draw_u"], g["draw_a"])
    assert np.array_equal(act, g["actions"]) and 0.1 < explored.mean() < 0.9
    g = H.load_fixture("q3_softmax")[A]
    act, bad = H.softmax(g["Qs"], g["param"], g["draw_u"])
    assert np.array_equal(act, g["actions"]) and not bad.any() and len(np.unique(g["param"])) > 10
    g = H.load_fixture("q4_boltzmann")[A]
    act, explored = H.boltzmann(g["Qs"], g["beta"], g["alpha"], g["param"], g["draw_u"], g["draw_a"])
    assert np.array_equal(act, g["actions"]) and 0.1 < explored.mean() < 0.9
    with np.errstate(all="ignore"):
        assert any(np.isnan(H.boltzmann_prob(q, b, a)).any() for q, b, a in zip(g["Qs"][:8], g["beta"][:8], g["alpha"][:8]))


def test_np_sum_order_is_the_one_the_kernel_walks():
    rng = np.random.default_rng(5)
    for n in sorted({A for _, _, A in H.SHAPES} | {7, 8, 9, 127, 128, 129, 135, 249, 1031, 2055, 4095}):
        for _ in range(3):
            a = np.exp(rng.standard_normal(n) * 3.0)
            assert H.pairwise_sum(a) == np.sum(a), n
    # the lane walk of np_wave_sum_lds covers six levels of splits: enough for every row length the entry point takes
    assert max(H.pairwise_depth(n) for n in range(1, 4097)) <= 6
    assert H.pairwise_depth(4095) == 6


# ---- wrong restatements ----
def test_wrong_restatements_are_each_told_apart():
    # last index on ties; a NaN ignored
    Q = np.array([[1.0, 3.0, 3.0, 0.0], [0.0, -0.0, 0.0, -0.0], [1.0, np.nan, 5.0, 2.0]])
    assert list(H.greedy(Q)) == [1, 0, 1]
    assert list(H.wrong_greedy_last_tie(Q)[:2]) == [2, 3]
    assert H.wrong_greedy_nan_ignored(Q)[2] == 2
    # >= instead of >: a draw equal to eps explores
    Q = np.array([[0.0, 1.0, 0.0]])
    u, a = np.array([0.25]), np.array([2 + 3 * 1000])
    act, explored = H.eps_greedy(Q, 0.25, u, a)
    assert (act[0], explored[0]) == (2, True) and H.wrong_eps_greedy_ge(Q, 0.25, u, a)[0] == 1
    # side="left": all-equal rows, A a power of two, u = j / A lies exactly on cdf[j - 1]
    for A in (4, 32):
        Q = np.zeros((A, A))
        u = np.arange(A) / A
        assert np.array_equal(H.softmax(Q, 1.0, u)[0], np.arange(A))
        assert np.array_equal(H.wrong_softmax(Q, 1.0, u, "left")[1:], np.arange(A)[1:] - 1)
    # max subtracted before the division / a re-associating scan: the cdf differs in its last bits somewhere, and a draw
    # on the smaller of the two entries separates the actions
    rng = np.random.default_rng(11)
    for rule in ("max_first", "tree_cumsum"):
        found = 0
        for _ in range(200):
            q = rng.standard_normal(32)
            ok, _ = H.softmax_cdf(q, 0.3)
            Q = q[None, :]
            for j in range(31):
                for uu in (ok[j], np.nextafter(ok[j], 0.0)):
                    u = np.array([uu])
                    if H.softmax(Q, 0.3, u)[0][0] != H.wrong_softmax(Q, 0.3, u, rule)[0]:
                        found += 1
            if found:
                break
        assert found, rule


# ---- the rows the GPU test compares ----
def test_no_row_of_the_gpu_comparisons_is_ambiguous():
    for i, dtype in H.GPU_CASES:
        B, N, A, _, exact = H.random_case(i, dtype)
        u, _ = H.case_draws(i)
        assert not H.softmax_ambiguous(exact, H.SOFTMAX_TMP, u).any(), (i, dtype)
        assert not H.boltzmann_ambiguous(exact, H.BOLTZ["beta"], H.BOLTZ["alpha"]).any(), (i, dtype)
    for name in ("q3_softmax", "q4_boltzmann"):
        for A, g in H.load_fixture(name).items():
            if name == "q3_softmax":
                assert not H.softmax_ambiguous(g["Qs"], g["param"], g["draw_u"]).any()
            else:
                assert not H.boltzmann_ambiguous(g["Qs"], g["beta"], g["alpha"]).any()
    # the census does find what it looks for
    q = np.array([[0.0, 0.0, 0.0, 0.0]])
    assert H.softmax_ambiguous(q, 1.0, np.array([0.5])).all()
    assert H.boltzmann_ambiguous(np.array([[1.0, 1.0 + 2.0 ** -52, 0.0]]), 1.0, 0.0).all()
    assert not H.boltzmann_ambiguous(np.array([[1.0, 1.0, 0.0]]), 1.0, 0.0).any()


def test_generator_restatement():
    # splitmix64's published first outputs for state 0 are mix64 of 0, of the increment, ...
    assert H.mix64(0) == 0xE220A8397B1DCDAF and H.mix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    u, a = H.device_draws(H.policy_seed(3, 1), 64, 5, idx0=10)
    u2, a2 = H.device_draws(H.policy_seed(3, 1), 74, 5)
    assert np.array_equal(u, u2[10:]) and np.array_equal(a, a2[10:]) and 0 <= u.min() and u.max() < 1 and a.max() == 4


# ---- C-ABI ----
def _select(**kw):
    s = DiralSelect()
    s.struct_bytes = ctypes.sizeof(DiralSelect)
    buf = ctypes.cast((ctypes.c_char * 64)(), ctypes.c_void_p).value        # never dereferenced by a refused call
    s.kind, s.agents, s.num_users, s.num_channels, s.q, s.q_dtype = SELECT_GREEDY, 8, 4, 3, buf, DT_F32
    s.tmp, s.actions_out = 1.0, buf
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_entry_point_refuses_bad_arguments_without_a_device():
    fn = _lib.load().diral_policy_select
    assert fn(None, None) == ERR_BAD_ARG
    assert DT_BF16 == 3                                          # q_dtype 4 below is the first unknown one
    nan, inf = float("nan"), float("inf")
    bad = [dict(q=None), dict(actions_out=None), dict(struct_bytes=164), dict(struct_bytes=0), dict(agents=0), dict(agents=-4),
           dict(num_channels=0), dict(agents=7), dict(num_users=0), dict(kind=4), dict(kind=-1), dict(q_dtype=4), dict(q_dtype=-1),
           dict(kind=SELECT_SOFTMAX, tmp=0.0), dict(kind=SELECT_SOFTMAX, tmp=-1.0), dict(kind=SELECT_SOFTMAX, tmp=nan),
           dict(kind=SELECT_SOFTMAX, tmp=inf), dict(param_per_env=1),
           dict(kind=SELECT_EPS_GREEDY, param_per_env=1), dict(kind=SELECT_BOLTZMANN, num_channels=5000, param_per_env=1)]
    for kw in bad:
        assert fn(ctypes.byref(_select(**kw)), None) == ERR_BAD_ARG, kw
    for kind in (SELECT_GREEDY, SELECT_EPS_GREEDY, SELECT_SOFTMAX, SELECT_BOLTZMANN):
        assert fn(ctypes.byref(_select(kind=kind, num_channels=4097)), None) == ERR_UNSUPPORTED
