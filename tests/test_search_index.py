"""The index arithmetic of diral_amd.search: work env b * C + c is candidate c of env b.  No GPU."""
import numpy as np
import pytest
import torch

from diral_amd.search import candidate_index, winner_index


@pytest.mark.parametrize("B,C", [(1, 1), (5, 3), (6, 8)])
def test_candidate_and_winner_index_match_their_numpy_statement(B, C):
    gather = candidate_index(B, C)
    assert gather.dtype == torch.int32 and tuple(gather.shape) == (B * C,)
    assert np.array_equal(gather.numpy(), np.arange(B * C) // C)
    # every work env is some candidate of some env exactly once
    hit = np.zeros(B * C, dtype=np.int64)
    for c in range(C):
        w = winner_index(torch.full((B,), c, dtype=torch.int64), C)
        assert w.dtype == torch.int32
        assert np.array_equal(w.numpy(), np.arange(B) * C + c)
        assert np.array_equal(gather.numpy()[w.numpy()], np.arange(B))   # ... and came from the env it is committed to
        hit[w.numpy()] += 1
    assert np.array_equal(hit, np.ones(B * C, dtype=np.int64))
    choice = np.random.default_rng(B * 31 + C).integers(0, C, size=B)
    for dt in (torch.int64, torch.int32):
        assert np.array_equal(winner_index(torch.as_tensor(choice).to(dt), C).numpy(), np.arange(B) * C + choice)
