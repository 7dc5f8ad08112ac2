#!/usr/bin/env python
"""Record the reference's replay memory and batch regrouping as fixtures m1 ... m3.

Runs ONLY where the reference checkout exists (DIRAL_REFERENCE, default /root/reference).  utils/memory.py is loaded by
path; algorithms/drl_drqn.py is loaded with an empty stand-in module named ``tensorflow`` and algorithms/ on the path, and
``DRQN.get_states_user`` and the three like it run unbound on a ``types.SimpleNamespace(num_users=N)``.  A trajectory is
fed to ``Memory.add`` the way the driver does (``state = next_state``, main_test.py:113, 217), ``Memory.sample`` draws - the
``idx`` it draws is recorded by drawing first and putting ``np.random``'s state back -, and the regrouped and reshaped
batch is stored as ``train`` builds it (drl_drqn.py:211-243).  Nothing of the reference's source is stored - only data:

    m1_memory_wrapped.npz  N = 4, S = 23, capacity 16, 23 adds, step 6, batch 5     the deque has wrapped
    m2_memory_dqn.npz      N = 9, S = 5, capacity 12, 10 adds, step 1, batch 6      the DQN form ([-1, S] reshapes)
    m3_memory_batches.npz  N = 4, S = 7, capacity 8, 13 adds, step 3                every batch size 1 ... len - step

Every file holds ``meta`` = [N, S, capacity, adds, step], the trajectory ``state0`` [N, S], ``next_states`` [T, N, S],
``actions`` [T, N] int32, ``rewards`` [T, N] (float64 values that float32 holds exactly), and per batch size M:
``b<M>_idx`` [M], ``b<M>_states``, ``b<M>_actions``, ``b<M>_rewards``, ``b<M>_next_states``.

    python tests/golden/gen_memory_golden.py [outdir]        (default: this directory)
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = os.environ.get("DIRAL_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))


def load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    memory = load("ref_memory", "utils", "memory.py")
    sys.modules.setdefault("tensorflow", types.ModuleType("tensorflow"))
    sys.path.insert(0, os.path.join(REF, "algorithms"))
    try:
        drqn = load("ref_drl_drqn", "algorithms", "drl_drqn.py")
    finally:
        sys.path.pop(0)
    return memory.Memory, drqn.DRQN


def record(Memory, DRQN, rng, N, S, capacity, adds, step, batches, lstm):
    f32 = lambda a: a.astype(np.float32).astype(np.float64)          # noqa: E731
    state0 = f32(rng.standard_normal((N, S)))
    nxt = f32(rng.standard_normal((adds, N, S)))
    actions = rng.integers(0, 32, size=(adds, N)).astype(np.int32)
    rewards = f32(rng.standard_normal((adds, N)) * 3.0)
    mem = Memory(max_size=capacity)
    state = state0
    for j in range(adds):
        mem.add((state, actions[j], rewards[j], nxt[j]))
        state = nxt[j]
    me = types.SimpleNamespace(num_users=N)
    out = dict(meta=np.array([N, S, capacity, adds, step]), state0=state0, next_states=nxt, actions=actions, rewards=rewards)
    for M in batches:
        st = np.random.get_state()
        idx = np.random.choice(np.arange(len(mem.buffer) - step), size=M, replace=False)
        np.random.set_state(st)
        batch = mem.sample(M, step)
        s, a = DRQN.get_states_user(me, batch), DRQN.get_actions_user(me, batch)
        r, n = DRQN.get_rewards_user(me, batch), DRQN.get_next_states_user(me, batch)
        if lstm:                                                     # drl_drqn.py:234-238
            s, n = np.reshape(s, [-1, s.shape[2], s.shape[3]]), np.reshape(n, [-1, n.shape[2], n.shape[3]])
            a, r = np.reshape(a, [-1, a.shape[2]]), np.reshape(r, [-1, r.shape[2]])
        else:                                                        # :240-243
            s, n = np.reshape(s, [-1, s.shape[3]]), np.reshape(n, [-1, n.shape[3]])
            a, r = np.reshape(a, [-1]), np.reshape(r, [-1])
        out.update({"b%d_idx" % M: idx.astype(np.int32), "b%d_states" % M: s, "b%d_actions" % M: a.astype(np.int32),
                    "b%d_rewards" % M: r, "b%d_next_states" % M: n})
    return out


def main(outdir):
    Memory, DRQN = load_reference()
    cases = (("m1_memory_wrapped", dict(N=4, S=23, capacity=16, adds=23, step=6, batches=(5,), lstm=True)),
             ("m2_memory_dqn", dict(N=9, S=5, capacity=12, adds=10, step=1, batches=(6,), lstm=False)),
             ("m3_memory_batches", dict(N=4, S=7, capacity=8, adds=13, step=3, batches=(1, 2, 3, 4, 5), lstm=True)))
    for i, (name, kw) in enumerate(cases):
        np.random.seed(8100 + i)
        data = record(Memory, DRQN, np.random.default_rng(8200 + i), **kw)
        np.savez_compressed(os.path.join(outdir, name + ".npz"), **data)
        print(name, {k: v.shape for k, v in data.items() if k.endswith("_states")})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
