#!/usr/bin/env python
"""Record the reference's TD targets and acting-window feeds as fixtures td1 ... td4 and h1.

Runs ONLY where the reference checkout exists (DIRAL_REFERENCE, default /root/reference).  algorithms/drl_drqn.py is
loaded with an empty stand-in module named ``tensorflow`` and algorithms/ on the path, exactly as gen_memory_golden.py
does.  ``DRQN._calc_target`` runs unbound on a stub ``self`` whose ``sess.run`` returns prepared float32 Q arrays;
``DRQN.infer_action(..., policy="greedy")`` runs unbound on a stub whose ``sess.run`` records the feed.  Nothing of the
reference's source is stored - only data:

    td1_double_lstm.npz   use_double, use_lstm_input: rewards [rows, step]     A = 5
    td2_double_dqn.npz    use_double, DQN form: rewards [rows]                 A = 32
    td3_plain_lstm.npz    np.max of the target net, rewards [rows, step]       A = 5
    td4_plain_dqn.npz     ... rewards [rows]                                   A = 32
    h1_history_feeds.npz  a deque(maxlen=step_size) of states and the per-user feeds of infer_action

td*: ``meta`` = [rows, A, step (0: the DQN form), double], ``gamma`` (float64), ``rewards`` float64 (values float32 does
not hold, 0.1 among them), ``qn_target`` / ``qn_eval`` float32 [rows, A] (coarse rows: ties; rows with -0.0 against +0.0,
a NaN, -inf, +inf), ``targets`` as returned (float64 - the feed into the float32 placeholder rounds them once).
h1: ``meta`` = [T, N, S, step], ``states`` [T, N, S] float64 appended one by one, ``feeds_lstm`` [N, step, S] and
``feeds_dqn`` [N, S] - the arrays fed for user 0 ... N - 1.

    python tests/golden/gen_td_golden.py [outdir]        (default: this directory)
"""
import importlib.util
import os
import sys
import types
from collections import deque

import numpy as np

REF = os.environ.get("DIRAL_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))


def load_drqn():
    sys.modules.setdefault("tensorflow", types.ModuleType("tensorflow"))
    sys.path.insert(0, os.path.join(REF, "algorithms"))
    try:
        spec = importlib.util.spec_from_file_location("ref_drl_drqn", os.path.join(REF, "algorithms", "drl_drqn.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.pop(0)
    return mod.DRQN


class Session:
    """sess.run(fetches, feed_dict): the prepared array of every fetch; the feeds are kept."""

    def __init__(self, tables):
        self.tables, self.feeds = tables, []

    def run(self, fetches, feed_dict=None):
        self.feeds.append(feed_dict)
        if isinstance(fetches, (list, tuple)):
            return [self.tables[f] for f in fetches]
        return self.tables[fetches]


def q_table(rng, rows, A):
    q = (rng.standard_normal((rows, A)) * 4.0).astype(np.float32)
    q[::3] = np.round(q[::3] * 2.0) / 2.0                            # ties
    q[1] = 0.0
    q[1, A // 2] = -0.0
    q[4] = -0.0
    q[4, A - 1] = 0.0
    q[7, 1] = np.nan
    q[10] = -np.inf
    q[13, A - 1] = np.inf
    q[16] = q[16, 0]                                                 # all equal
    return q


def record_targets(DRQN, rng, rows, A, step, double, gamma):
    qn_target, qn_eval = q_table(rng, rows, A), q_table(rng, rows, A)[::-1].copy()
    rewards = rng.standard_normal((rows, step) if step else (rows,)) * 3.0
    rewards[::5] = 0.1
    me = types.SimpleNamespace(use_double=double, use_lstm_input=bool(step), gamma=gamma, target_qvalues="target",
                               qvalues="eval", inputs_="inputs", sess=Session(dict(target=qn_target, eval=qn_eval)))
    next_states = np.zeros((rows, step, 2)) if step else np.zeros((rows, 2))
    with np.errstate(invalid="ignore"):
        targets = DRQN._calc_target(me, rewards, next_states)
    return dict(meta=np.array([rows, A, step, int(double)]), gamma=np.float64(gamma), rewards=rewards, qn_target=qn_target,
                qn_eval=qn_eval, targets=np.asarray(targets))


def record_feeds(DRQN, rng, T, N, S, step, A=3):
    states = rng.standard_normal((T, N, S))
    history = deque(maxlen=step)
    for s in states:
        history.append(s)
    state_vector = np.array(history)
    out = dict(meta=np.array([T, N, S, step]), states=states)
    for name, lstm in (("feeds_lstm", True), ("feeds_dqn", False)):
        me = types.SimpleNamespace(use_lstm_input=lstm, step_size=step, state_size=S, action_size=A, inputs_="inputs",
                                   qvalues="eval", sess=Session(dict(eval=np.zeros((1, A), np.float32))))
        for user in range(N):
            DRQN.infer_action(me, user, state_vector, 0, policy="greedy")
        out[name] = np.array([f["inputs"][0] for f in me.sess.feeds])
    return out


def main(outdir):
    DRQN = load_drqn()
    cases = (("td1_double_lstm", dict(rows=48, A=5, step=4, double=True, gamma=0.99)),
             ("td2_double_dqn", dict(rows=40, A=32, step=0, double=True, gamma=0.9)),
             ("td3_plain_lstm", dict(rows=48, A=5, step=4, double=False, gamma=0.99)),
             ("td4_plain_dqn", dict(rows=40, A=32, step=0, double=False, gamma=0.95)))
    for i, (name, kw) in enumerate(cases):
        data = record_targets(DRQN, np.random.default_rng(8300 + i), **kw)
        np.savez_compressed(os.path.join(outdir, name + ".npz"), **data)
        print(name, data["targets"].dtype, data["targets"].shape)
    data = record_feeds(DRQN, np.random.default_rng(8310), T=9, N=4, S=7, step=3)
    np.savez_compressed(os.path.join(outdir, "h1_history_feeds.npz"), **data)
    print("h1_history_feeds", data["feeds_lstm"].shape, data["feeds_dqn"].shape)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
