"""`diral_td_head` / `QLoss` on the device against the host statement of tests/td_cases.py, which tests/test_td_cases.py
holds against the reference's recorded targets and against torch's CPU autograd.  Everything is compared bit for bit (any
NaN equals any NaN) unless said otherwise; the 16-bit gradients are compared with the statement's float32 gradient rounded
once to the dtype."""
import ctypes
import math

import numpy as np
import pytest
import torch

from diral_amd import _lib
from diral_amd.config import DT_F32, DT_F64, ERR_BAD_ARG, ERR_UNSUPPORTED
from diral_amd.qloss import QLoss
from diral_amd.rollout import no_finalizers_during_capture
from tests import td_cases as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMMA = 0.99
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.detach().float().cpu().numpy()


def run(case, dtype, double, hysteretic, f32_rewards=False):
    """-> (QLoss, dict of what one `loss` call left on the device, the loss tensor)."""
    head = QLoss(GAMMA, double=double, hysteretic=hysteretic, device=DEV)
    q = dev(case["q"], TORCH[dtype]).requires_grad_(True)
    r = dev(case["rewards"].astype(np.float32) if f32_rewards else case["rewards"])
    loss = head.loss(q, dev(case["actions"]), r, dev(case["qn_target"], TORCH[dtype]),
                     dev(case["qn_eval"], TORCH[dtype]) if double else None)
    loss.backward()
    got = dict(targets=host(head.last_targets), next_actions=head.last_next_actions.cpu().numpy(), td=host(head.last_td),
               grad=host(q.grad), loss=host(loss), bad=int(head.bad_rows.item()))
    assert q.grad.dtype == TORCH[dtype] and loss.dtype == torch.float32 and loss.dim() == 0 and loss.grad_fn is not None
    return head, got


def statement(case, dtype, double, hysteretic, f32_rewards=False):
    r = case["rewards"].astype(np.float32) if f32_rewards else case["rewards"]
    st = H.td_head(case["q"], case["actions"], r, case["qn_target"], case["qn_eval"] if double else None, GAMMA, double, hysteretic)
    st["grad"] = H.quantize(st["grad"], dtype)
    return st


def assert_equal(got, want, what):
    for k in ("targets", "td", "grad"):
        assert H.same_bits(got[k], want[k]), (what, k)
    assert np.array_equal(got["next_actions"], want["next_actions"]), what
    assert H.same_bits(got["loss"], want["loss"]) and got["bad"] == want["bad"], (what, got["loss"], want["loss"], got["bad"])


def within_one_ulp(x, y):
    x, y = np.float32(x), np.float32(y)
    return x == y or x == np.nextafter(y, np.float32(np.inf)) or x == np.nextafter(y, np.float32(-np.inf))


# every A of both layouts; the dtypes taken in turn, and all three at the flagship A = 32 and at a strided A = 200
SHAPE_CASES = [(A, H.DTYPES[i % 3]) for i, A in enumerate(H.SMALL_A + H.WIDE_A)] + \
              [(A, d) for A in (32, 200) for d in H.DTYPES if (A, d) not in ((32, "f16"), (200, "bf16"))]


@pytest.mark.parametrize("A, dtype", SHAPE_CASES, ids=["A%d-%s" % c for c in SHAPE_CASES])
def test_head_equals_the_statement(A, dtype):
    for n, rows in enumerate(H.ROWS):
        case = H.random_case(rows, A, dtype, seed=n)
        double, hysteretic, f32r = bool((n + A) % 2), bool((n // 2 + A) % 2), n % 3 == 1
        _, got = run(case, dtype, double, hysteretic, f32r)
        want = statement(case, dtype, double, hysteretic, f32r)
        assert_equal(got, want, (rows, double, hysteretic))
        assert within_one_ulp(got["loss"], H.fsum_loss(want["td"])), rows      # the sum's order moves the rounding one step at most
        _, again = run(case, dtype, double, hysteretic, f32r)
        assert_equal(again, got, "two calls")


@pytest.mark.parametrize("double", [True, False], ids=["double", "plain"])
@pytest.mark.parametrize("A", [3, 32, 64, 65, 200])
def test_special_values(A, double):
    """Ties, -0.0 against +0.0, NaN rows, rows of -inf, +inf, h == 0, the tiniest h of either sign, a subnormal h / 10, a
    chosen -0.0, a non-finite value in a column that was not chosen, actions of -1 and A."""
    for dtype in ("f32", "bf16") if A in (32, 65) else ("f32",):
        case = H.special_case(A, dtype, double)
        head, got = run(case, dtype, double, True)
        want = statement(case, dtype, double, True)
        assert_equal(got, want, (A, dtype))
        rows = len(case["q"])
        assert got["bad"] == 2 and not got["grad"][0].any() and not got["grad"][rows - 1].any()
        t0 = got["targets"][0]                                      # Q = 0 for the action A: h = -target
        assert np.isnan(t0) or got["td"][0] == (-t0 / np.float32(10.0) if -t0 < 0 else -t0)
        if dtype == "f32":
            v, a = rows - 8, case["actions"]
            assert got["td"][v] == 0 and got["grad"][v, a[v]] == 0
            assert got["td"][v + 3] == -np.float32(1.4e-45) and np.signbit(got["grad"][v + 4, a[v + 4]])


def test_the_float64_sum_is_not_the_float32_sum():
    case = H.rounding_cases()
    for double in (False, True):
        _, got = run(case, "f32", double, False)
        assert_equal(got, statement(case, "f32", double, False), double)
    wrong = H.calc_target(case["qn_target"], None, case["rewards"], GAMMA, False, wrong="add_f32")[0]
    _, got = run(case, "f32", False, False)
    assert np.all(got["targets"] != wrong)


def test_targets_alone():
    case = H.random_case(257, 32, "f16", seed=9)
    for double in (True, False):
        head = QLoss(GAMMA, double=double, device=DEV)
        qe = dev(case["qn_eval"], torch.float16)
        t = head.targets(dev(case["qn_target"], torch.float16), dev(case["rewards"]), qe if double else None)
        want, j = H.calc_target(case["qn_target"], case["qn_eval"], case["rewards"], GAMMA, double)
        assert t.dtype == torch.float32 and H.same_bits(host(t), want) and np.array_equal(head.last_next_actions.cpu().numpy(), j)
        assert head.last_td is None and int(head.bad_rows.item()) == 0
    for key in ("td1", "td2", "td3", "td4"):                        # the reference's recorded targets
        fx = H.load_fixture(key)
        rows, A, step, double = (int(v) for v in fx["meta"])
        head = QLoss(float(fx["gamma"]), double=bool(double), device=DEV)
        last = np.ascontiguousarray(fx["rewards"][:, -1] if step else fx["rewards"])
        t = head.targets(dev(fx["qn_target"]), dev(last), dev(fx["qn_eval"]) if double else None)
        with np.errstate(invalid="ignore", over="ignore"):
            assert H.same_bits(host(t), fx["targets"].astype(np.float32)), key


# ---- autograd ----
def test_backward_scales_the_kept_gradient_and_touches_nothing_else():
    case = H.random_case(17, 33, "f32", seed=11)
    head = QLoss(GAMMA, double=True, hysteretic=True, device=DEV)
    q = dev(case["q"]).requires_grad_(True)
    qt, qe = dev(case["qn_target"]).requires_grad_(True), dev(case["qn_eval"]).requires_grad_(True)
    loss = head.loss(q, dev(case["actions"]), dev(case["rewards"]), qt, qe)
    (loss * 2.0).backward()
    want = statement(case, "f32", True, True)
    assert H.same_bits(host(q.grad), want["grad"] * np.float32(2.0)) and qt.grad is None and qe.grad is None
    with torch.no_grad():                                           # no graph asked for: the same numbers, no grad_fn
        plain = head.loss(q, dev(case["actions"]), dev(case["rewards"]), qt, qe)
    assert plain.grad_fn is None and H.same_bits(host(plain), want["loss"])


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["h-positive", "h-negative-damped"])
def test_parameter_gradients_through_an_mlp_agree_with_the_torch_composition(sign):
    """A 2-layer MLP in front of the head against the same MLP in front of torch's expression of the loss head.  Every
    weight, input and activation is positive and every h has one sign (the rewards sit 50 below or above the Q-values),
    so no sum in the backward pass cancels: a parameter gradient is a sum of like-signed terms, each within three float32
    roundings of the other side's (tests/test_td_cases.py), and the 24-term float32 sums add a rounding step of their own
    on either side - inside rtol = 1e-6."""
    rows, n_in, hidden, A = 24, 5, 8, 4
    g = torch.Generator(DEV).manual_seed(3)
    x = torch.rand((rows, n_in), device=DEV, generator=g) + 0.1
    params = [torch.rand(s, device=DEV, generator=g) + 0.1 for s in ((n_in, hidden), (hidden,), (hidden, A), (A,))]
    actions = torch.randint(0, A, (rows,), dtype=torch.int32, device=DEV, generator=g)
    rewards = torch.rand((rows,), dtype=torch.float64, device=DEV, generator=g) - sign * 50.0
    qn_t, qn_e = torch.rand((rows, A), device=DEV, generator=g), torch.rand((rows, A), device=DEV, generator=g)
    head = QLoss(GAMMA, double=True, hysteretic=True, device=DEV)

    def grads(loss_of):
        ps = [p.clone().requires_grad_(True) for p in params]
        q = torch.relu(x @ ps[0] + ps[1]) @ ps[2] + ps[3]
        loss = loss_of(q)
        loss.backward()
        return [host(p.grad) for p in ps], host(loss)

    ours, loss = grads(lambda q: head.loss(q, actions, rewards, qn_t, qn_e))
    targets = head.last_targets.clone()
    assert bool((sign * head.last_td > 0).all())
    theirs, tloss = grads(lambda q: H.torch_loss(torch, q, actions, targets, True))
    np.testing.assert_allclose(loss, tloss, rtol=1e-6)
    for o, t in zip(ours, theirs):
        print("max relative difference", float(np.max(np.abs(o - t) / np.abs(t))))
        np.testing.assert_allclose(o, t, rtol=1e-6, atol=0.0)


# ---- captured ----
def nodes_and_edges(graph):
    """(number of nodes, [(from, to)]) of a captured graph kept with keep_graph=True, from the HIP runtime torch runs on."""
    with open("/proc/self/maps") as fh:
        path = next(line.split()[-1] for line in fh if "libamdhip64" in line)
    hip = ctypes.CDLL(path)                                         # (already loaded: the same runtime)
    g, n, e = ctypes.c_void_p(graph.raw_cuda_graph()), ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, ctypes.byref(n)) == 0 and hip.hipGraphGetEdges(g, None, None, ctypes.byref(e)) == 0
    src, dst = (ctypes.c_void_p * max(e.value, 1))(), (ctypes.c_void_p * max(e.value, 1))()
    assert hip.hipGraphGetEdges(g, src, dst, ctypes.byref(e)) == 0
    return n.value, [(src[i], dst[i]) for i in range(e.value)]


def test_a_captured_head_is_one_chain_and_replays_on_new_contents():
    rows, A = 257, 32
    first = H.random_case(rows, A, "bf16", seed=20)
    head = QLoss(GAMMA, double=True, hysteretic=True, device=DEV)
    q, qt, qe = (dev(first[k], torch.bfloat16) for k in ("q", "qn_target", "qn_eval"))
    a, r = dev(first["actions"]), dev(first["rewards"])
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        head._launch(q, a, r, qt, qe)                               # eagerly first
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with no_finalizers_during_capture():
        with torch.cuda.graph(graph, stream=stream):
            loss, grad = head._launch(q, a, r, qt, qe)
    torch.cuda.synchronize()
    td, targets = head.last_td, head.last_targets
    nodes, edges = nodes_and_edges(graph)
    assert nodes == 2 and len(edges) == 1 and edges[0][0] != edges[0][1], (nodes, edges)   # the head, the loss behind it: no branches
    for n in (21, 22):
        case = H.random_case(rows, A, "bf16", seed=n)
        for t, k in ((q, "q"), (qt, "qn_target"), (qe, "qn_eval")):
            t.copy_(dev(case[k], torch.bfloat16))
        a.copy_(dev(case["actions"]))
        r.copy_(dev(case["rewards"]))
        graph.replay()
        torch.cuda.synchronize()
        got = dict(targets=host(targets), next_actions=head.last_next_actions.cpu().numpy(), td=host(td), grad=host(grad),
                   loss=host(loss), bad=0)
        assert_equal(got, statement(case, "bf16", True, True), n)
    assert int(head.bad_rows.item()) == 0


# ---- refusals ----
def test_refusals_leave_the_outputs_untouched():
    rows, A = 8, 3
    lib = _lib.load()
    q = torch.zeros((rows, A), device=DEV)
    acts, rew = torch.zeros((rows,), dtype=torch.int32, device=DEV), torch.zeros((rows,), dtype=torch.float64, device=DEV)
    outs = dict(targets=torch.full((rows,), 7.0, device=DEV), td=torch.full((rows,), 7.0, device=DEV),
                nxt=torch.full((rows,), 7, dtype=torch.int32, device=DEV), grad=torch.full((rows, A), 7.0, device=DEV),
                loss=torch.full((1,), 7.0, device=DEV), bad=torch.full((1,), 7, dtype=torch.int32, device=DEV))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(**kw):
        a = dict(rows=rows, A=A, q=q.data_ptr(), qn_target=q.data_ptr(), qn_eval=q.data_ptr(), q_dtype=DT_F32,
                 actions=acts.data_ptr(), rewards=rew.data_ptr(), r_dtype=DT_F64, gamma=GAMMA, hysteretic=1,
                 **{k: v.data_ptr() for k, v in outs.items()})
        a.update(kw)
        return lib.diral_td_head(a["rows"], a["A"], a["q"], a["qn_target"], a["qn_eval"], a["q_dtype"], a["actions"], a["rewards"],
                                 a["r_dtype"], a["gamma"], a["hysteretic"], a["targets"], a["td"], a["nxt"], a["grad"], a["loss"],
                                 a["bad"], stream)

    refused = [(dict(qn_target=None), ERR_BAD_ARG), (dict(actions=None), ERR_BAD_ARG), (dict(rewards=None), ERR_BAD_ARG),
               (dict(rows=0), ERR_BAD_ARG), (dict(A=0), ERR_BAD_ARG), (dict(q_dtype=4), ERR_BAD_ARG), (dict(r_dtype=2), ERR_BAD_ARG),
               (dict(gamma=math.nan), ERR_BAD_ARG), (dict(gamma=math.inf), ERR_BAD_ARG), (dict(q=None), ERR_BAD_ARG),
               (dict(q=None, td=None, grad=None), ERR_BAD_ARG), (dict(td=None), ERR_BAD_ARG),
               (dict(A=4097), ERR_UNSUPPORTED), (dict(rows=2 ** 24 + 1), ERR_UNSUPPORTED), (dict(q_dtype=DT_F64), ERR_UNSUPPORTED)]
    for kw, status in refused:
        assert call(**kw) == status, kw
    torch.cuda.synchronize()
    assert all(bool((v == 7).all()) for v in outs.values())
    assert call() == 0 and call(q=None, td=None, grad=None, loss=None) == 0      # ... and the same arguments are taken
    torch.cuda.synchronize()
    assert float(outs["loss"].item()) == 0.0 and int(outs["bad"].item()) == 7
    head = QLoss(GAMMA, double=True, device=DEV)
    with pytest.raises(ValueError):
        head.loss(q, acts, rew, q, None)                            # double=True without the eval net's next Q-values
    with pytest.raises(ValueError):
        head.loss(q.double(), acts, rew, q.double(), q.double())
    with pytest.raises(ValueError):
        head.loss(q, acts.long(), rew, q, q)
    with pytest.raises(ValueError):
        head.targets(q, rew[:-1], q)
