"""A second libdiral_env.so in the process (`_lib.bind`, `_lib.use`): a handle built under `use(copy)` runs on the copy, one
built outside on the product's library, both compute the same bit for bit, and the product's library is back afterwards."""
import ctypes
import shutil

import pytest
import torch

from diral_amd import _lib
from diral_amd.config import bench_config
from diral_amd.vec_env import VecV2VEnv

pytestmark = pytest.mark.gpu


def address(lib):
    return ctypes.cast(lib.diral_env_step, ctypes.c_void_p).value


def test_handles_on_two_mappings_of_the_library_agree(tmp_path):
    product = _lib.load()
    copy = _lib.bind(shutil.copy(_lib.LIB_PATH, str(tmp_path / "libdiral_env_copy.so")))
    assert address(copy) != address(product)                        # two mappings, not one library opened twice
    cfg = bench_config(8, 3, 100.0)
    with _lib.use(copy):
        assert _lib.load() is copy
        there = VecV2VEnv(cfg, batch=2, device="cuda:0", out_dtype=torch.float32)
    assert _lib.load() is product
    here = VecV2VEnv(cfg, batch=2, device="cuda:0", out_dtype=torch.float32)
    assert there.lib is copy and here.lib is product
    got = []
    for env in (there, here):
        env.reset_topology(seed=1234)
        outs = []
        for t in range(3):
            obs, rew, done = env.step(env.sample(40 + t), t)
            outs += [obs.clone(), rew.clone(), done.clone()]
        out = env.rollout(torch.stack([env.sample(50 + k) for k in range(3)]), 3, states="all", global_reward_avg=True)
        outs += [out[k].clone() for k in ("states", "reward", "done", "shaped", "sum_r", "collision")]
        st = env.export_state()
        got.append(outs + [st[k] for k in sorted(st)] + [env.metrics()])
        env.check()
    assert len(got[0]) == len(got[1]) and all(torch.equal(a, b) for a, b in zip(*got))
    assert _lib.load() is product
