"""diral_amd.search.CandidateSearch: fork every env into C candidates, run them, keep the winner.

`evaluate` must leave the env exactly as it was; `commit(choice)` must leave it bit-equal to a twin that ran the chosen
sequences directly (K = 4 slots, no episode end inside, so no device velocity draw separates the two); `returns` is the sum
of that twin's `sum_r`.  Configurations: step_fast64 (my_step and my_step_ch), step_wide's packed form, and A = 70, which
`rollout` refuses - there the loop of step + diral_driver_shape runs."""
import numpy as np
import pytest
import torch

from diral_amd.config import ERR_UNSUPPORTED, KERNEL_POLICY, STEP_MY_STEP, bench_config
from diral_amd.search import CandidateSearch
from diral_amd.vec_env import DiralError, driver_shape
from tests.call_programs import FAMILIES, MODE_NAME
from tests.gpu_util import dev, everything, new_env, run, slot

pytestmark = pytest.mark.gpu

CASES = dict({k: FAMILIES[k] for k in ("f64_full", "f64_ch", "w2_packed")},
             a70=dict(cfg=lambda: bench_config(24, 70, 800.0), B=4, f64=True, mode=STEP_MY_STEP, form=None))
C, K, T0 = 3, 4, 5


def setup(name, monkeypatch):
    f = CASES[name]
    if f["form"]:
        monkeypatch.setenv("DIRAL_TABLE_FORM", f["form"])
    cfg, B = f["cfg"](), f["B"]
    env, twin = new_env(f, cfg, B, 1), new_env(f, cfg, B, 1)
    assert run([env, twin], T0, 11) == T0 and T0 + K < cfg.episode_interval
    env.t = twin.t = T0
    seqs = np.random.default_rng(7).integers(0, cfg.num_channels, size=(K, B, C, cfg.num_users)).astype(np.int32)
    return f, cfg, env, twin, seqs


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def direct_rollout(env, seq, t, mode):
    """K slots of `seq` [K, B, N] on `env` itself: the launch, or slot by slot where the launch refuses."""
    try:
        return env.rollout(seq, t, mode=mode, states=None)["sum_r"]
    except DiralError as exc:
        assert exc.status == ERR_UNSUPPORTED
    o = dict(dtype=env.out_dtype, device=env.device)
    sum_r, coll, shaped = torch.empty((K, env.B), **o), torch.empty((K, env.B), **o), torch.empty((env.B, env.N), **o)
    for k in range(K):
        _, rew, _ = env.step(seq[k], t + k)
        driver_shape(env, rew, seq[k], shaped=shaped, sum_r=sum_r[k], collision=coll[k])
    return sum_r


@pytest.mark.parametrize("name", list(CASES))
def test_evaluate_leaves_the_env_untouched(name, monkeypatch):
    f, cfg, env, twin, seqs = setup(name, monkeypatch)
    mode = MODE_NAME[f["mode"]]
    before = everything(twin, T0)
    search = CandidateSearch(env, C)
    assert search.work.B == env.B * C
    out = search.evaluate(dev(seqs), mode=mode)
    assert tuple(out["returns"].shape) == (env.B, C) and tuple(out["sum_r"].shape) == (K, env.B, C) == tuple(out["collision"].shape)
    sr = out["sum_r"].cpu().numpy()
    assert np.array_equal(out["collision"].cpu().numpy(), (cfg.num_channels - sr).astype(sr.dtype))   # main_test.py:178
    # the K-slot launch where the handle takes it, the loop where it refuses
    assert bool(search.work.last_kernel() & KERNEL_POLICY) == (name != "a70")
    if name == "a70":
        with pytest.raises(DiralError) as ei:
            search.work.rollout(dev(seqs.reshape(K, -1, cfg.num_users)), T0, mode=mode, states=None)
        assert ei.value.status == ERR_UNSUPPORTED
    assert env.t == T0 and search.work.t == T0 + K
    same(everything(env, T0), before)
    a = np.random.default_rng(8).integers(0, cfg.num_channels, size=(env.B, cfg.num_users)).astype(np.int32)
    same(slot(env, a, T0), slot(twin, a, T0))
    same(everything(env, T0 + 1), everything(twin, T0 + 1))
    search.evaluate(dev(seqs), t=T0 + 1, mode=mode)                  # a second look-ahead from the new state: again no trace
    same(everything(env, T0 + 1), everything(twin, T0 + 1))
    env.check()
    search.work.check()


@pytest.mark.parametrize("name", list(CASES))
def test_commit_equals_a_twin_that_ran_the_chosen_sequences(name, monkeypatch):
    f, cfg, env, twin, seqs = setup(name, monkeypatch)
    mode = MODE_NAME[f["mode"]]
    B = env.B
    search = CandidateSearch(env, C)
    out = search.evaluate(dev(seqs), mode=mode, global_reward_avg=True)
    choice = np.random.default_rng(9).integers(0, C, size=B)
    assert len(set(choice.tolist())) > 1
    search.commit(dev(choice))
    chosen = np.ascontiguousarray(seqs[:, np.arange(B), choice])     # [K, B, N]
    sum_r = direct_rollout(twin, dev(chosen), T0, mode).cpu().numpy()
    twin.t = T0 + K
    assert env.t == T0 + K
    same(everything(env, T0 + K), everything(twin, T0 + K))
    # every candidate's numbers are its own rollout's ...
    got = out["sum_r"].cpu().numpy()[:, np.arange(B), choice]
    assert np.array_equal(got, sum_r)
    # ... and `returns` their sum over the slots (float64; K - 1 additions in whatever order: 3 roundings of the sum)
    want = sum_r.astype(np.float64).sum(0)
    ret = out["returns"].cpu().numpy()
    assert ret.dtype == np.float64
    assert np.all(np.abs(ret[np.arange(B), choice] - want) <= 3 * 2.0 ** -53 * np.abs(sum_r).astype(np.float64).sum(0))
    a = np.random.default_rng(10).integers(0, cfg.num_channels, size=(B, cfg.num_users)).astype(np.int32)
    for k in range(3):
        same(slot(env, a, T0 + K + k), slot(twin, a, T0 + K + k))
    env.check()
