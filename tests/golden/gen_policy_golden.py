#!/usr/bin/env python
"""Record the exploration policies of the reference's agent (algorithms/policies.py) as fixtures q1 ... q4.

Runs ONLY where the reference checkout exists (DIRAL_REFERENCE, default /root/reference).  policies.py is loaded by path,
its classes are fed float64 ``Qs`` rows, and every draw a call takes from ``np.random`` is recorded by drawing it first
and putting the generator's state back, so that the call draws the same numbers.  Nothing of the reference's source is
stored - only data:

    q1_greedy.npz      GreedyPolicy.action(Qs)                       np.argmax: ties, -0.0, NaN, +-inf rows among them
    q2_eps_greedy.npz  EpsilonGreedy.action(Qs, episode)             param = eps of the call, draw_u, draw_a
    q3_softmax.npz     SoftmaxPolicy.action(Qs, episode)             param = tmp of the call, draw_u
    q4_boltzmann.npz   BoltzmanPolicy.take_action(Qs, time_slot)     param = explore_p, beta, alpha, draw_u, draw_a

Every file holds, for A in (3, 32): ``A<A>_Qs`` [R, A] float64, ``A<A>_param`` [R], ``A<A>_draw_u`` [R] float64,
``A<A>_draw_a`` [R] int32, ``A<A>_actions`` [R] int32 (q4 also ``A<A>_beta`` and ``A<A>_alpha``; draws a policy does not
take are zeros).  The reference runs float32 when TensorFlow hands it float32; these fixtures pin the float64 statement.

    python tests/golden/gen_policy_golden.py [outdir]        (default: this directory)
"""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np

REF = os.environ.get("DIRAL_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (3, 32)
ROWS = 320


def load_policies():
    spec = importlib.util.spec_from_file_location("ref_policies", os.path.join(REF, "algorithms", "policies.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def q_rows(rng, rows, A, scale):
    """Random rows; every fourth one rounded coarsely so that ties between actions are common."""
    Q = rng.standard_normal((rows, A)) * scale
    Q[::4] = np.round(Q[::4] * 2.0) / 2.0
    return Q


def special_rows(A):
    """np.argmax's corners: all equal, ties first / last, -0.0 against +0.0, NaN before / behind the maximum, +-inf."""
    rows = [np.zeros(A), np.full(A, -np.inf), np.full(A, np.inf), np.full(A, np.nan)]
    for k in range(A):
        r = np.zeros(A); r[k] = -0.0; r[(k + 1) % A] = 0.0; rows.append(r)
        r = np.arange(A, dtype=np.float64); r[k] = float(A); rows.append(r)             # a tie of k with nothing, or the last
        r = np.arange(A, dtype=np.float64); r[k] = np.nan; rows.append(r)
        r = -np.arange(A, dtype=np.float64); r[k] = np.nan; rows.append(r)
        r = np.full(A, -np.inf); r[k] = -1e300; rows.append(r)
        r = np.ones(A); r[k] = np.inf; r[(k + 2) % A] = np.inf; rows.append(r)
        r = np.ones(A); r[k] = 5.0; r[A - 1 - k] = 5.0; rows.append(r)
    return np.array(rows)


def gen_greedy(P, rng):
    out = {}
    for A in SIZES:
        Q = np.concatenate((special_rows(A), q_rows(rng, ROWS, A, 1.0)))
        acts = P.GreedyPolicy(nA=A).action(Qs=Q)
        R = len(Q)
        out.update({"A%d_Qs" % A: Q, "A%d_param" % A: np.zeros(R), "A%d_draw_u" % A: np.zeros(R),
                    "A%d_draw_a" % A: np.zeros(R, np.int32), "A%d_actions" % A: np.asarray(acts, np.int32)})
    return out


def gen_eps(P, rng):
    out = {}
    for A in SIZES:
        Q = q_rows(rng, ROWS, A, 1.0)
        pol = P.EpsilonGreedy(nA=A, eps_init=0.7, eps_decay=0.97)
        par, us, das, acts = [], [], [], []
        for k in range(ROWS):
            st = np.random.get_state()
            u = np.random.random()
            a = np.random.randint(A)
            np.random.set_state(st)
            act = pol.action(Qs=Q[k:k + 1], episode=k // 4)
            par.append(pol.eps); us.append(u); das.append(a); acts.append(int(np.ravel(act)[0]))
        out.update({"A%d_Qs" % A: Q, "A%d_param" % A: np.array(par), "A%d_draw_u" % A: np.array(us),
                    "A%d_draw_a" % A: np.array(das, np.int32), "A%d_actions" % A: np.array(acts, np.int32)})
    return out


def gen_softmax(P, rng):
    out = {}
    for A in SIZES:
        Q = q_rows(rng, ROWS, A, 0.3)
        pol = P.SoftmaxPolicy(nA=A, temperature=0.05, episodes=90)
        par, us, acts = [], [], []
        for k in range(ROWS):
            st = np.random.get_state()
            u = np.random.random_sample()
            np.random.set_state(st)
            act = pol.action(Qs=Q[k:k + 1], episode=k // 3)          # (past the list's end: the final temperature)
            par.append(float(pol.tmp)); us.append(u); acts.append(int(act))
        out.update({"A%d_Qs" % A: Q, "A%d_param" % A: np.array(par), "A%d_draw_u" % A: np.array(us),
                    "A%d_draw_a" % A: np.zeros(ROWS, np.int32), "A%d_actions" % A: np.array(acts, np.int32)})
    return out


def gen_boltzmann(P, rng):
    out = {}
    for A in SIZES:
        Q = q_rows(rng, ROWS, A, 2.0)
        Q[5] *= 400.0                                                # exp overflows: inf / inf, the first NaN wins
        Q[6] = -Q[5]
        pols = [P.BoltzmanPolicy(A, beta=1, explore_start=0.6, explore_stop=0.3, decay_rate=0.001, alpha=0),
                P.BoltzmanPolicy(A, beta=2.5, explore_start=0.5, explore_stop=0.1, decay_rate=0.002, alpha=0.25)]
        par, betas, alphas, us, das, acts = [], [], [], [], [], []
        for k in range(ROWS):
            pol, t = pols[k % 2], 25 * (k // 2)
            st = np.random.get_state()
            u = np.random.rand()
            a = int(np.random.choice(A, size=1)[0])
            np.random.set_state(st)
            with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
                act = pol.take_action(Q[k:k + 1], t)
            par.append(pol.explore_stop + (pol.explore_start - pol.explore_stop) * np.exp(-pol.decay_rate * t))
            betas.append(pol.beta); alphas.append(pol.alpha)
            us.append(u); das.append(a); acts.append(int(np.ravel(act)[0]))
        out.update({"A%d_Qs" % A: Q, "A%d_param" % A: np.array(par), "A%d_beta" % A: np.array(betas, np.float64),
                    "A%d_alpha" % A: np.array(alphas, np.float64), "A%d_draw_u" % A: np.array(us),
                    "A%d_draw_a" % A: np.array(das, np.int32), "A%d_actions" % A: np.array(acts, np.int32)})
    return out


def main(outdir):
    P = load_policies()
    for i, (name, fn) in enumerate((("q1_greedy", gen_greedy), ("q2_eps_greedy", gen_eps), ("q3_softmax", gen_softmax),
                                    ("q4_boltzmann", gen_boltzmann))):
        np.random.seed(7100 + i)
        data = fn(P, np.random.default_rng(7200 + i))
        np.savez_compressed(os.path.join(outdir, name + ".npz"), **data)
        print(name, {k: v.shape for k, v in data.items() if k.endswith("_actions")})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
