"""`diral_td_head` / `diral_memory_history` without a device: the host statements the GPU tests compare against
(tests/td_cases.py) equal what the reference's ``DRQN._calc_target`` returned and what ``DRQN.infer_action`` fed (fixtures
td1 ... td4 and h1, recorded by tests/golden/gen_td_golden.py), restatements with one rule wrong are each told apart by
some generated case, the loss head and its gradient agree with torch's CPU autograd of the reference's expression, and the
C-ABI of the two entry points is what include/diral_env.h declares.

What nobody has measured: TensorFlow is not installed where the fixtures were recorded, so the loss and the gradient have
never been compared with a TensorFlow run; the targets and the window are compared with the reference itself."""
import ctypes

import numpy as np
import pytest

from diral_amd import _lib
from diral_amd.config import DT_BF16, DT_F16, DT_F32, DT_F64, ERR_BAD_ARG, ERR_UNSUPPORTED, DiralMemory
from tests import abi_header
from tests import td_cases as H

TD_KEYS = ("td1", "td2", "td3", "td4")
GAMMA = 0.99


def _fixture_inputs(fx):
    rows, A, step, double = (int(v) for v in fx["meta"])
    last = fx["rewards"][:, -1] if step else fx["rewards"]          # drl_drqn.py:288 / :290
    return last, float(fx["gamma"]), bool(double)


def _fixture_targets(fx, wrong=None):
    last, gamma, double = _fixture_inputs(fx)
    return H.calc_target(fx["qn_target"], fx["qn_eval"], last, gamma, double, wrong)[0]


# ---- the statements against the reference's recorded results ----
@pytest.mark.parametrize("key", TD_KEYS)
def test_targets_equal_the_reference_bit_for_bit(key):
    fx = H.load_fixture(key)
    assert fx["targets"].dtype == np.float64 and fx["rewards"].dtype == np.float64 and fx["qn_target"].dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        fed = fx["targets"].astype(np.float32)                      # the float32 placeholder
    assert H.same_bits(_fixture_targets(fx), fed)


def test_fixtures_cover_what_they_are_for():
    metas = [tuple(int(v) for v in H.load_fixture(k)["meta"]) for k in TD_KEYS]
    assert [(m[2] > 0, m[3]) for m in metas] == [(True, 1), (False, 1), (True, 0), (False, 0)]      # lstm x double
    for k in TD_KEYS:
        fx = H.load_fixture(k)
        r, q = fx["rewards"], fx["qn_target"]
        assert np.any(r.astype(np.float32).astype(np.float64) != r) and np.any(r == 0.1)
        assert np.isnan(q).any() and np.isneginf(q).all(axis=1).any() and np.isposinf(q).any()
        assert any(len(np.unique(row)) < len(row) and (row == row.max()).sum() > 1 for row in q[~np.isnan(q).any(axis=1)])


def test_window_equals_the_reference_s_feeds():
    fx = H.load_fixture("h1")
    T, N, S, step = (int(v) for v in fx["meta"])
    window = H.deque_window([s[None] for s in fx["states"]], step)  # one env
    feeds = H.agent_feeds(window)
    assert feeds.shape == (N, step, S) and np.array_equal(feeds, fx["feeds_lstm"])
    assert np.array_equal(feeds[:, -1], fx["feeds_dqn"])            # state_vector[-1:, user]: the window's last row
    ring = np.zeros((T + 1, 1, N, S))                               # a ring that has not wrapped: state j in row j
    ring[1:, 0] = fx["states"]
    assert np.array_equal(H.ring_window(ring, T, T, step), fx["feeds_lstm"])
    assert not np.array_equal(H.ring_window(ring, T, T, step, wrong="ends_before_newest"), fx["feeds_lstm"])


def test_ring_window_equals_the_deque_across_the_wrap():
    rng = np.random.default_rng(4)
    B, N, S, C = 3, 5, 7, 5
    ring = np.zeros((C + 1, B, N, S))
    states = [rng.standard_normal((B, N, S))]
    ring[0] = states[0]
    for count in range(1, 13):                                      # adds 1 ... 12: before, at and across the wrap
        states.append(rng.standard_normal((B, N, S)))
        ring[count % (C + 1)] = states[-1]
        for step in sorted({1, min(3, count + 1), min(count, C) + 1}):            # step <= len + 1: the live states
            want = H.agent_feeds(H.deque_window(states, step))
            assert np.array_equal(H.ring_window(ring, count, C, step), want), (count, step)
            assert not np.array_equal(H.ring_window(ring, count, C, step, wrong="ends_before_newest"), want)


# ---- wrong restatements ----
def _random_targets(double, wrong=None):
    """Targets and next actions as one float32 array."""
    c = H.random_case(257, 3, seed=3)
    t, j = H.calc_target(c["qn_target"], c["qn_eval"], c["rewards"], GAMMA, double, wrong)
    return np.concatenate([t, j.astype(np.float32)])


@pytest.mark.parametrize("wrong, double", [("add_f32", False), ("fma", False), ("gamma_f64", False), ("last_tie", True),
                                           ("last_tie", False), ("double_from_eval", True), ("plain_index_eval", False)])
def test_wrong_target_restatements_are_each_told_apart(wrong, double):
    assert not H.same_bits(_random_targets(double, wrong), _random_targets(double)), wrong      # (plain ties: the action only)
    # ... and by the reference's own results, where the fixtures can (the plain ones never ran the eval net's arg-max)
    told = [k for k in TD_KEYS if not H.same_bits(_fixture_targets(H.load_fixture(k), wrong), _fixture_targets(H.load_fixture(k)))]
    assert told, wrong


def test_the_rounding_cases_are_what_they_say():
    c = H.rounding_cases()
    right = H.calc_target(c["qn_target"], None, c["rewards"], GAMMA, False)[0]
    assert np.all(right != H.calc_target(c["qn_target"], None, c["rewards"], GAMMA, False, wrong="add_f32")[0])
    assert len(right) == 64 and c["qn_target"].shape == (64, 3)


def test_a_multiply_by_a_tenth_is_told_apart():
    c = H.random_case(1000, 32, seed=5)
    args = (c["q"], c["actions"], c["rewards"], c["qn_target"], c["qn_eval"], GAMMA, True, True)
    right, wrong = H.td_head(*args), H.td_head(*args, wrong="mul_tenth")
    assert not H.same_bits(right["td"], wrong["td"]) and not H.same_bits(right["grad"], wrong["grad"])
    plain = H.td_head(*args[:-1], False)                            # without the switch there is no division at all
    assert H.same_bits(plain["td"], H.td_head(*args[:-1], False, wrong="mul_tenth")["td"])
    assert (plain["td"] < 0).any() and np.all(np.abs(right["td"]) <= np.abs(plain["td"]))


# ---- the loss head against torch's CPU autograd of the reference's expression ----
@pytest.mark.parametrize("hysteretic", [False, True])
@pytest.mark.parametrize("rows, A", [(17, 3), (257, 32), (1000, 5)])
def test_loss_and_gradient_agree_with_torch_autograd(rows, A, hysteretic):
    """Both sides are at most three float32 roundings from the exact value: they differ by at most about 6 * 2^-24 = 3.6e-7
    relative, asserted as rtol = 1e-6, on inputs with |h| in [1e-3, 1e3]."""
    import torch
    c = H.random_case(rows, A, seed=7)
    st = H.td_head(c["q"], c["actions"], c["rewards"], c["qn_target"], c["qn_eval"], GAMMA, True, hysteretic)
    h = c["q"][np.arange(rows), c["actions"]] - st["targets"]
    keep = (np.abs(h) >= 1e-3) & (np.abs(h) <= 1e3)
    assert keep.sum() >= 0.9 * rows
    q = torch.tensor(c["q"], requires_grad=True)
    loss = H.torch_loss(torch, q, torch.tensor(c["actions"]), torch.tensor(st["targets"]), hysteretic)
    loss.backward()
    np.testing.assert_allclose(st["loss"], loss.item(), rtol=1e-6)
    np.testing.assert_allclose(st["grad"][keep], q.grad.numpy()[keep], rtol=1e-6, atol=0.0)
    assert H.fsum_loss(st["td"]) in (st["loss"], np.nextafter(st["loss"], np.float32(np.inf)), np.nextafter(st["loss"], np.float32(-np.inf)))


def test_special_rows_follow_the_pinned_rules():
    c = H.special_case(32)
    n, v = len(c["q"]) - 16, len(c["q"]) - 8                        # the plain head's special rows, the value rows
    st = H.td_head(c["q"], c["actions"], c["rewards"], c["qn_target"], c["qn_eval"], GAMMA, True, True)
    a = c["actions"]
    assert st["bad"] == 2 and not st["grad"][0].any() and not st["grad"][v + 7].any()
    assert st["td"][v] == 0 and st["grad"][v, a[v]] == 0                                   # h == 0
    assert st["td"][v + 1] < 0 and st["td"][v + 2] > 0 and abs(st["td"][v + 2]) < 1e-5
    assert st["td"][v + 3] == -np.float32(1.4e-45)                                         # the tenth of a subnormal h
    assert np.signbit(st["td"][v + 4]) and np.signbit(st["grad"][v + 4, a[v + 4]])         # the chosen -0.0 stays
    assert np.isfinite(st["td"][v + 5]) and np.isfinite(st["td"][v + 6])                   # inf / NaN in another column
    assert list(st["next_actions"][:5]) == [0] * 5 and np.isfinite(st["targets"][4])       # all equal, ..., all NaN: the first
    plain = H.td_head(c["q"], c["actions"], c["rewards"], c["qn_target"], None, GAMMA, False, True)
    assert np.isnan(plain["targets"][n + 4]) and np.isneginf(plain["targets"][n + 2]) and np.isposinf(plain["targets"][n + 3])


# ---- C-ABI ----
def test_the_header_declares_both_entry_points_and_the_table_has_their_rows():
    protos = abi_header.prototypes()
    P, I32, F64 = abi_header.PTR, abi_header.I32, abi_header.F64
    assert protos["diral_memory_history"].params == [P, I32, I32, P, P, P] and protos["diral_memory_history"].ret == I32
    assert protos["diral_td_head"].params == [I32, I32, P, P, P, I32, P, P, I32, F64, I32, P, P, P, P, P, P, P]
    for name in ("diral_memory_history", "diral_td_head"):
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(protos[name].params)
        assert hasattr(_lib.load(), name)
    assert "DiralTdHead" not in abi_header.structs()                # flat arguments: ABI 8 keeps its set of structs


def _buf():
    return ctypes.cast((ctypes.c_char * 64)(), ctypes.c_void_p).value           # never dereferenced by a refused call


def _td(**kw):
    a = dict(rows=4, A=3, q=_buf(), qn_target=_buf(), qn_eval=_buf(), q_dtype=DT_F32, actions=_buf(), rewards=_buf(),
             r_dtype=DT_F64, gamma=0.99, hysteretic=1, targets=_buf(), td=_buf(), nxt=_buf(), grad=_buf(), loss=_buf(),
             bad=_buf())
    a.update(kw)
    return _lib.load().diral_td_head(a["rows"], a["A"], a["q"], a["qn_target"], a["qn_eval"], a["q_dtype"], a["actions"],
                                     a["rewards"], a["r_dtype"], a["gamma"], a["hysteretic"], a["targets"], a["td"], a["nxt"],
                                     a["grad"], a["loss"], a["bad"], None)


TD_REFUSALS = [(dict(qn_target=None), ERR_BAD_ARG), (dict(actions=None), ERR_BAD_ARG), (dict(rewards=None), ERR_BAD_ARG),
               (dict(rows=0), ERR_BAD_ARG), (dict(rows=-3), ERR_BAD_ARG), (dict(A=0), ERR_BAD_ARG), (dict(q_dtype=4), ERR_BAD_ARG),
               (dict(q_dtype=-1), ERR_BAD_ARG), (dict(r_dtype=DT_F16), ERR_BAD_ARG), (dict(r_dtype=9), ERR_BAD_ARG),
               (dict(gamma=float("nan")), ERR_BAD_ARG), (dict(gamma=float("inf")), ERR_BAD_ARG),
               (dict(q=None, grad=None, loss=None), ERR_BAD_ARG), (dict(q=None, td=None, loss=None), ERR_BAD_ARG),
               (dict(q=None, td=None, grad=None), ERR_BAD_ARG), (dict(td=None), ERR_BAD_ARG),
               (dict(A=4097), ERR_UNSUPPORTED), (dict(rows=2 ** 24 + 1), ERR_UNSUPPORTED), (dict(q_dtype=DT_F64), ERR_UNSUPPORTED)]


def test_td_head_refuses_without_a_device():
    for kw, status in TD_REFUSALS:
        assert _td(**kw) == status, kw
    assert DT_BF16 == 3 and DT_F16 == 2                             # (q_dtype 4 and -1 above are unknown kinds)


def _memory(**kw):
    m = DiralMemory()
    m.struct_bytes = ctypes.sizeof(DiralMemory)
    m.capacity, m.batch, m.num_users, m.state_space, m.dtype = 16, 2, 4, 5, DT_F32
    m.states, m.actions, m.rewards, m.count = _buf(), _buf(), _buf(), 10
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def test_history_refuses_without_a_device():
    history = _lib.load().diral_memory_history
    assert history(None, 3, DT_F32, _buf(), None, None) == ERR_BAD_ARG
    for kw in (dict(struct_bytes=60), dict(states=None), dict(capacity=0), dict(batch=0), dict(dtype=DT_F16), dict(count=-1)):
        assert history(ctypes.byref(_memory(**kw)), 3, DT_F32, _buf(), None, None) == ERR_BAD_ARG, kw
    m = _memory()                                                   # len = 10: the live states are [0, 10]
    for step, out in ((0, _buf()), (-1, _buf()), (3, None), (12, _buf())):
        assert history(ctypes.byref(m), step, DT_F32, out, None, None) == ERR_BAD_ARG, step
    assert history(ctypes.byref(_memory(count=0)), 2, DT_F32, _buf(), None, None) == ERR_BAD_ARG      # right after begin
    assert history(ctypes.byref(_memory(count=40)), 18, DT_F32, _buf(), None, None) == ERR_BAD_ARG    # len = capacity
    for ring, out in ((DT_F32, DT_F64), (DT_F64, DT_F16), (DT_F64, DT_BF16), (DT_F32, 7)):
        assert history(ctypes.byref(_memory(dtype=ring)), 3, out, _buf(), None, None) == ERR_UNSUPPORTED
