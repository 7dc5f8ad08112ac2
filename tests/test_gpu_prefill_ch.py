"""The driver's `enable_channel` prefill (main_test.py:99-114 with :101-103: sample -> my_step_ch -> obtain_state, every
state kept) as ONE launch of K slots (`diral_env_prefill_mode(DIRAL_STEP_MY_STEP_CH)`, step_fast64_slots_kernel<CH, POL>
with PolParams::prefill) against the loop of one-slot calls it replaces: states, actions, tables, positions, metrics -
bit for bit."""
import ctypes

import pytest
import torch

from diral_amd.config import (ERR_UNSUPPORTED, KERNEL_CH, KERNEL_FAST64, KERNEL_POLICY, STEP_MY_STEP_CH, bench_config,
                              c2_config)
from diral_amd.driver import DriverLoop
from diral_amd.vec_env import DiralError
from tests.kslots_harness import RICH, assert_same_envs, start, twins

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cfg,K,dtype", [
    (c2_config(), 7, torch.float32),
    (c2_config(reward_design=3), 30, torch.float64),
    (bench_config(40, 12, 900.0, State=RICH, mobility_vary=True), 26, torch.float32),        # dense
    (bench_config(64, 8, 9000.0, communication_range=100.0), 9, torch.float32),             # sparse: keyed quads
    (c2_config(State=RICH, reward_design=4), 1, torch.float32),
])
def test_ch_prefill_in_one_launch_equals_the_loop_of_one_slot_calls(cfg, K, dtype):
    B, seed = 24, 77001
    e_loop, e_one = twins(cfg, B, dtype, start(cfg, B, 5))
    loops = [DriverLoop(e, enable_channel=True) for e in (e_loop, e_one)]
    a0 = e_loop.sample(123)
    for lp in loops:
        lp.bootstrap(a0)                                             # my_step: `rews` of main_test.py:92, the stale reward column
    want_s, want_a = [], []
    for k in range(K):
        a = e_loop.sample(seed + k)
        want_a.append(a.clone())
        want_s.append(loops[0].prefill_step(a))                      # my_step_ch + obtain_state
        assert e_loop.last_kernel() & KERNEL_POLICY == 0
    states, acts, nxt = e_one.prefill(e_one.sample(seed), K, seed, rew_in=loops[1]._rews0, mode="my_step_ch")
    torch.cuda.synchronize()
    lk = e_one.last_kernel()
    assert (lk & 15) == KERNEL_FAST64 and (lk & KERNEL_POLICY) and (lk & KERNEL_CH), lk
    assert torch.equal(acts, torch.stack(want_a)) and torch.equal(nxt, e_loop.sample(seed + K))
    for k in range(K):
        assert torch.equal(states[k], want_s[k]), (k, (states[k] != want_s[k]).nonzero()[:5])
    s1, s2 = e_loop.export_state(), e_one.export_state()
    for key in s1:
        assert torch.equal(s1[key], s2[key]), key
    m1, m2 = e_loop.metrics(), e_one.metrics()
    assert torch.equal(m1, m2), (m1 != m2).nonzero()[:4]
    assert float(m2[:, 5].min()) > 0.0                               # DIRAL_M_PRR_CNT: every slot paid the PRR columns
    # ... and the envs go on alike (what the launch wrote back: tables, ring, positions)
    for t in range(3):
        a = e_loop.sample(900 + t)
        o1, r1, _ = e_loop.step(a, t)
        o2, r2, _ = e_one.step(a, t)
        assert torch.equal(o1, o2) and torch.equal(r1, r2)
    e_loop.check(); e_one.check()


def test_ch_driver_loop_prefill_takes_the_launch_where_it_can_and_loops_elsewhere():
    for cfg, fused in ((c2_config(), True), (bench_config(128, 16, 4000.0), False),
                       (c2_config(track_arrival=True), False)):
        e1, e2 = twins(cfg, 6, torch.float64, start(cfg, 6, 9))
        l1, l2 = DriverLoop(e1, enable_channel=True), DriverLoop(e2, enable_channel=True)
        a0 = e1.sample(1)
        l1.bootstrap(a0); l2.bootstrap(a0)
        states, acts = l2.prefill(5, 4400)
        assert bool(e2.last_kernel() & KERNEL_POLICY) == fused
        assert e2.last_kernel() & KERNEL_CH or not fused
        for k in range(5):
            a = e1.sample(4400 + k)
            assert torch.equal(acts[k], a) and torch.equal(states[k], l1.prefill_step(a))
        if not fused:
            with pytest.raises(DiralError) as ei:
                e2.prefill(a0, 3, 1, mode=STEP_MY_STEP_CH)
            assert ei.value.status == ERR_UNSUPPORTED


def test_design_prefill_through_the_new_entry_point_equals_diral_env_prefill():
    """`prefill(mode="my_step_design")` (diral_env_prefill_mode) against `diral_env_prefill` called directly, on a rich
    case: the older symbol is a call of the new one."""
    cfg, K, B, seed = c2_config(State=RICH, enable_fingerprint=True), 12, 24, 31007
    e_new, e_old = twins(cfg, B, torch.float64, start(cfg, B, 5))
    rews = []
    for e in (e_new, e_old):
        lp = DriverLoop(e)
        lp.bootstrap(e.sample(123))
        rews.append(lp._rews0.to(torch.float64).contiguous())
    s_new, a_new, n_new = e_new.prefill(e_new.sample(seed), K, seed, rew_in=rews[0], mode="my_step_design")
    assert e_new.last_kernel() & KERNEL_POLICY and not (e_new.last_kernel() & KERNEL_CH)
    a0 = e_old.sample(seed)
    s_old = torch.empty_like(s_new)
    a_old, n_old = torch.empty_like(a_new), torch.empty_like(n_new)

    def p(t):
        return ctypes.c_void_p(t.data_ptr())
    st = e_old.lib.diral_env_prefill(e_old._h, p(a0), K, seed, p(s_old), e_old._dt, p(a_old), p(n_old), p(rews[1]), 0.0, 1.0,
                                     e_old._stream())
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(s_new, s_old) and torch.equal(a_new, a_old) and torch.equal(n_new, n_old)
    assert_same_envs(e_new, e_old, entries=False)
    e_new.check(); e_old.check()
