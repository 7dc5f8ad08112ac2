"""The comparators of tests/kslots_harness.py can fail: what they must reject, on CPU tensors."""
import pytest
import torch

from tests.kslots_harness import as_rollout, assert_same


def _result():
    return dict(states=torch.arange(24.0).reshape(2, 3, 4), reward=torch.ones(2, 3), done=torch.zeros(2, dtype=torch.int32),
                shaped=torch.full((5, 2, 3), 0.5))


def test_assert_same_passes_on_equal_dicts():
    assert_same(_result(), _result(), "equal")
    assert_same(dict(_result(), states=None), dict(_result(), states=None), "both without states")


@pytest.mark.parametrize("what", ["element", "dtype", "shape", "missing_key", "extra_key", "none_for_tensor", "tensor_for_none"])
def test_assert_same_raises_on_a_difference(what):
    want, got = _result(), _result()
    if what == "element":
        got["shaped"][4, 1, 2] += 1.0
    elif what == "dtype":
        got["reward"] = got["reward"].double()
    elif what == "shape":
        got["reward"] = got["reward"][:1]
    elif what == "missing_key":
        del got["done"]
    elif what == "extra_key":
        got["xpos"] = torch.zeros(5, 2, 3)
    elif what == "none_for_tensor":
        got["states"] = None
    else:
        want["states"] = None
    with pytest.raises(AssertionError):
        assert_same(want, got, what)


def test_as_rollout_selects_the_last_slot_and_the_states_asked_for():
    K = 5
    stacked = dict(states=torch.arange(K * 24.0).reshape(K, 2, 3, 4), reward=torch.arange(K * 6.0).reshape(K, 2, 3),
                   done=torch.arange(K * 2).reshape(K, 2), shaped=torch.ones(K, 2, 3), sum_r=torch.ones(K, 2),
                   collision=torch.zeros(K, 2), xpos=torch.ones(K, 2, 3), ia=torch.ones(K, 2, 100))
    last = as_rollout(stacked, "last")
    assert set(last) == {"states", "reward", "done", "shaped", "sum_r", "collision", "ia"}          # no xpos unless logged
    assert torch.equal(last["states"], stacked["states"][-1]) and torch.equal(last["reward"], stacked["reward"][-1])
    assert torch.equal(last["done"], stacked["done"][-1]) and last["shaped"] is stacked["shaped"]
    assert torch.equal(as_rollout(stacked, "all")["states"], stacked["states"])
    assert as_rollout(stacked, None)["states"] is None
    assert as_rollout(dict(stacked, states=None), "all")["states"] is None                         # a config without a state vector
    assert as_rollout(stacked, "last", log=True)["xpos"] is stacked["xpos"]
