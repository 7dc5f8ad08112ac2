"""Long mixed-schedule runs of the HIP path against the oracle (bit-exact): sticky and
iid actions, velocity updates every 25 slots, dense / sparse highways, both step kinds,
N <= 64 (step_fast64) and N > 64 (step_wide incl. ragged N).  `python tests/test_gpu_soak.py 10`
runs the same schedules ten times longer."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pytest
import torch

from diral_amd.config import bench_config, STEP_MY_STEP, STEP_MY_STEP_CH
from tests.oracle_compare import metrics_equal, slot_equal, tables_equal

pytestmark = pytest.mark.gpu


def soak(N, A, L, B, T, mode, vary, rc=250.0, every=250, rich=False):
    """rich: the reference's two-call pattern (`obs, rews = env.my_step*(a, t)`; `env.obtain_state(obs, a,
    rews)`) on the RICH instantiations, channel observation compared as well."""
    from diral_amd.vec_env import VecV2VEnv
    from oracle.oracle import Oracle, SQ_IEEE
    cfg = bench_config(N, A, L, mobility_vary=vary, communication_range=rc)
    rng = np.random.default_rng(N + T)
    x0 = rng.integers(0, int(L), size=(B, N)).astype(np.float64); v0 = rng.uniform(1.1, 2.7, size=(B, N))
    env = VecV2VEnv(cfg, batch=B, device="cuda:0", out_dtype=torch.float64, step_mode="my_step_ch" if mode == STEP_MY_STEP_CH else "my_step")
    orc = Oracle(cfg, batch=B, sq_mode=SQ_IEEE, threads=16)
    env.reset_topology(x0, None, v0); orc.reset(x0, np.zeros((B, N)), v0)
    t0 = time.time(); prev = None
    for t in range(T):
        a = rng.integers(0, A, size=(B, N)).astype(np.int32)
        if prev is not None and t % 2: a = np.where(rng.random((B, N)) < 0.8, prev, a)
        prev = a
        if rich:
            a_dev = env._actions(a)
            chobs, rew = (env.my_step_ch if mode == STEP_MY_STEP_CH else env.my_step)(a_dev, t)
            obs = env.obtain_state(chobs, a_dev, rew)
        else:
            obs, rew, done = env.step(a, t)
        o_rew, o_ch = orc.step(mode, a, t)
        if t % 25 == 24:
            d = rng.integers(1, 4, size=(B, N)).astype(np.uint8)
            env.update_velocity(d); orc.update_velocity(d)
        if t % every == every - 1 or t == T - 1:
            got = (obs.cpu().numpy(), rew.cpu().numpy(), chobs.cpu().numpy() if rich else None)
            slot_equal(cfg, mode, got, (orc.obtain_state(a, o_ch, o_rew), o_rew, o_ch), (N, t))
    tables_equal({k: v.cpu().numpy() for k, v in env.export_state().items()}, orc.export(), N)
    metrics_equal(env.metrics().cpu().numpy(), orc.metrics(), N)
    env.check()
    print("soak ok N=%d A=%d L=%g B=%d T=%d mode=%d vary=%s rc=%g rich=%s  %.1fs" % (N, A, L, B, T, mode, vary, rc, rich, time.time() - t0), flush=True)

SCHEDULES = [(64, 32, 2000.0, 8, 6000, STEP_MY_STEP, True, 250.0), (64, 32, 2000.0, 8, 3000, STEP_MY_STEP_CH, False, 250.0),
             (64, 32, 6000.0, 6, 3000, STEP_MY_STEP, True, 120.0), (256, 64, 4000.0, 3, 1200, STEP_MY_STEP, False, 250.0),
             (128, 64, 4000.0, 4, 2000, STEP_MY_STEP, True, 250.0), (128, 64, 9000.0, 3, 1500, STEP_MY_STEP_CH, True, 150.0),
             (200, 40, 12000.0, 2, 1200, STEP_MY_STEP, True, 140.0)]
RICH_SCHEDULES = [(64, 32, 2000.0, 8, 3000, STEP_MY_STEP, True, 250.0), (48, 16, 1500.0, 6, 2000, STEP_MY_STEP_CH, False, 200.0),
                  (128, 64, 4000.0, 4, 1500, STEP_MY_STEP, True, 250.0), (256, 64, 4000.0, 2, 800, STEP_MY_STEP, False, 250.0)]


@pytest.mark.parametrize("N,A,L,B,T,mode,vary,rc", SCHEDULES)
def test_soak_vs_oracle(N, A, L, B, T, mode, vary, rc):
    soak(N, A, L, B, T, mode, vary, rc)


@pytest.mark.parametrize("N,A,L,B,T,mode,vary,rc", RICH_SCHEDULES)
def test_soak_two_call_pattern_vs_oracle(N, A, L, B, T, mode, vary, rc):
    soak(N, A, L, B, T, mode, vary, rc, rich=True)


if __name__ == "__main__":
    k = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    for (N, A, L, B, T, mode, vary, rc) in SCHEDULES:
        soak(N, A, L, B, T * k, mode, vary, rc, every=250 * k)
    for (N, A, L, B, T, mode, vary, rc) in RICH_SCHEDULES:
        soak(N, A, L, B, T * k, mode, vary, rc, every=250 * k, rich=True)
