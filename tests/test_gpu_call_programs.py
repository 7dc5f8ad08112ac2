"""Random call programs (tests/call_programs.py) on every kernel family against the host model, op by op.

What is under test is the host state that decides what the next launch does and which buffers it trusts
(csrc/diral_env.hip: `plane_valid` / `ring_valid`, `flat_y`, `kernel_path`, the slow-env sets, the replay trace;
diral_amd/vec_env.py: `t`, `_vel_calls`, `_spec`, the output ring): a stale flag reads an old but legal buffer and shows
as a wrong number.  `export_state`, `export_entries`, `observe` and `check` change those flags themselves, so they run
only where the program draws them; one full export + metrics + information age + check closes every program.

Bars (the suite's own, imported): state, reward, channel observation, actions, tables, positions, arrival stamps,
information age and metric counts bit for bit; exp() rewards within the exp() bar of tests/oracle_compare.py and sums built from them within
`_exp_bounds`; metric float sums at rtol 1e-12, atol 1e-9; float32 outputs are the float32 cast of the float64 values.

A failure names the family, the seed, the op index and the ops so far: `draw_program(family, seed)` replays it."""
import numpy as np
import pytest
import torch

from diral_amd.config import ERR_UNSUPPORTED, KERNEL_POLICY, STEP_MY_STEP_CH
from tests import call_programs as P
from tests.call_programs import _exp_bounds, uses_exp
from tests.oracle_compare import exp_atol, metrics_equal
from tests.gpu_util import make_env

pytestmark = pytest.mark.gpu

CASES = [(fam, seed) for fam in P.FAMILIES for seed in P.SEEDS[fam]]
# programs kept by name beside the seeded ones: (family, seed) of a program that once failed
REGRESSIONS = {}


class Run:
    def __init__(self, family, seed, monkeypatch):
        from diral_amd.sps import SpsPolicy
        self.prog, self.expected, self.closing, self.rec, _ = P.run_host(family, seed)
        f = P.FAMILIES[family]
        self.family, self.seed, self.f, self.cfg = family, seed, f, self.prog["cfg"]
        if f["form"]:
            monkeypatch.setenv("DIRAL_TABLE_FORM", f["form"])
        self.B, self.N, self.A = self.prog["B"], self.cfg.num_users, self.cfg.num_channels
        self.dt = torch.float64 if f["f64"] else torch.float32
        self.env = make_env(self.cfg, self.B, mode=f["mode"], dtype=self.dt)
        self.env.reset_topology(self.prog["x0"], None, self.prog["v0"])
        self.pol = SpsPolicy(self.B, self.N, self.A, rssi_threshold=P.POLICY["threshold"], device="cuda:0", seed=P.POLICY["seed"])
        self.pol.keep_prob = P.POLICY["keep_prob"]
        self.pol.counter.remainder_(P.POLICY["counter_mod"])
        self.t, self.i, self.log = 0, -1, []
        self.exp = uses_exp(self.cfg, f["mode"])
        self.sum_atol, self.shaped_atol = _exp_bounds(self.N) if self.exp else (None, None)
        self.rew_atol = exp_atol(self.exp)
        self.state_atol = exp_atol(self.exp and self.cfg.State.add_reward)

    # -- comparison ------------------------------------------------------------------------------------------------
    def where(self, what):
        return "%s seed %d, op %d (%s): %s\nops so far: %s" % (self.family, self.seed, self.i, self.log[-1] if self.log else "-",
                                                              what, " | ".join(self.log))

    def eq(self, what, dev, want, atol=None):
        dev = dev.cpu().numpy() if isinstance(dev, torch.Tensor) else np.asarray(dev)
        want = np.asarray(want)
        assert dev.shape == want.shape, self.where("%s: shape %s, expected %s" % (what, dev.shape, want.shape))
        if atol is None:
            if not np.array_equal(dev, want):
                bad = np.argwhere(dev != want)
                raise AssertionError(self.where("%s: %d of %d differ, first at %s: %r, expected %r" % (
                    what, len(bad), dev.size, bad[0].tolist(), dev[tuple(bad[0])], want[tuple(bad[0])])))
        else:
            err = float(np.abs(dev.astype(np.float64) - want.astype(np.float64)).max()) if dev.size else 0.0
            assert err <= atol, self.where("%s: off by %.3g, allowed %.3g" % (what, err, atol))

    def kernel(self, op, policy=None):
        lk = self.env.last_kernel()
        assert (lk & 15) == op["kernel"], self.where("last_kernel() = %d, the model predicts family %d (flat = %s)" % (lk, op["kernel"], op["flat"]))
        if policy is not None:
            assert bool(lk & KERNEL_POLICY) == policy, self.where("last_kernel() = %d, fused expected: %s" % (lk, policy))

    def dev_acts(self, a):
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device="cuda:0")

    def refused(self, call):
        from diral_amd.vec_env import DiralError
        with pytest.raises(DiralError) as ei:
            call()
        assert ei.value.status == ERR_UNSUPPORTED, self.where("refused with status %d" % ei.value.status)

    # -- the ops ---------------------------------------------------------------------------------------------------
    def one_slot(self, e, chobs, op):
        env, a = self.env, self.dev_acts(e["acts"])
        if chobs:                                                    # the reference's pair: obs, rews = my_step*(a, t); obtain_state
            call = env.my_step_ch if self.f["mode"] == STEP_MY_STEP_CH else env.my_step
            co, rew = call(a, self.t)
            self.kernel(op)
            state = env.obtain_state(co, a, rew)
            self.eq("channel observation", co, e["chobs"])
        else:
            state, rew, _ = env.step(a, self.t)
            self.kernel(op)
        self.eq("state", state, e["state"], self.state_atol)
        self.eq("reward", rew, e["rew"], self.rew_atol)
        self.eq("done", env._done, e["done"])
        self.t += 1

    def op_step(self, op, e):
        self.one_slot(e, op["chobs"], op)

    def op_step_general(self, op, e):
        force = self.env.force_general_kernel if op["op"] == "step_general" else self.env.force_large_path
        force(True)
        for s in e["slots"]:
            self.one_slot(s, False, op)
        force(False)

    op_step_large = op_step_general

    def op_observe(self, op, e):
        got = self.env.obtain_state(op["chobs"], op["acts"], op["rew"], op["episode"], op["eps"])
        self.eq("observe", got, e["state"])

    def op_rollout(self, op, e):
        mode = P.MODE_NAME[self.f["mode"]]
        seq = self.dev_acts(op["acts"])
        call = lambda: self.env.rollout(seq, self.t, mode=mode, states=op["states"], global_reward_avg=True, vel_seed=op["vel_seed"])
        if e.get("refused"):
            return self.refused(call)
        got = call()
        self.kernel(op, True)
        self.eq("shaped", got["shaped"], e["shaped"], self.shaped_atol)
        self.eq("sum_r", got["sum_r"], e["sum_r"], self.sum_atol)
        self.eq("collisions", got["collision"], e["coll"], self.sum_atol)
        self.eq("reward", got["reward"], e["rew"], self.rew_atol)
        self.eq("done", got["done"], e["done"])
        if op["states"] is None:
            assert got["states"] is None
        else:
            self.eq("states", got["states"], e["states"], self.state_atol)
        self.t += op["K"]
        assert self.env.t == self.t, self.where("the handle's slot counter is %d, not %d" % (self.env.t, self.t))

    def op_step_policy(self, op, e):
        env, K, B, N = self.env, op["K"], self.B, self.N
        a = self.dev_acts(op["acts"] if e.get("refused") else e["acts"])
        nxt = torch.empty_like(a)
        lead = (K,) if K > 1 else ()
        sh = torch.zeros(lead + (B, N), dtype=self.dt, device="cuda:0")
        sr = torch.zeros(lead + (B,), dtype=self.dt, device="cuda:0")
        co = torch.zeros(lead + (B,), dtype=self.dt, device="cuda:0")
        call = lambda: env.step_policy(a, self.t, self.pol, nxt, shaped_out=sh, sum_r_out=sr, collision_out=co, slots=K,
                                       vel_seed=op["vel_seed"], mode=self.f["mode"])
        if e.get("refused"):
            return self.refused(call)
        state, rew, done = call()
        self.kernel(op, True if K > 1 else None)
        EI = self.cfg.episode_interval
        if K == 1 and self.cfg.mobility_vary and self.t % EI == EI - 1:
            env.update_velocity(seed=op["vel_seed"] + self.t // EI)  # (a K-slot launch does this inside)
        self.eq("shaped", sh.reshape((K, B, N)), e["shaped"], self.shaped_atol)
        self.eq("sum_r", sr.reshape((K, B)), e["sum_r"], self.sum_atol)
        self.eq("collisions", co.reshape((K, B)), e["coll"], self.sum_atol)
        self.eq("reward", rew, e["rew"], self.rew_atol)
        self.eq("done", done, e["done"])
        self.eq("state", state, e["state"], self.state_atol)
        self.eq("actions_out", nxt, e["actions"])
        self.eq("prev_action", self.pol.prev_action, e["sps"][0])
        self.eq("counter", self.pol.counter, e["sps"][1])
        self.t += K

    def op_prefill(self, op, e):
        call = lambda: self.env.prefill(self.env.sample(op["seed"]), op["K"], op["seed"],
                                        mode="my_step_ch" if self.f["mode"] == STEP_MY_STEP_CH else "my_step_design")
        if e.get("refused"):
            return self.refused(call)
        states, acts, nxt = call()
        self.kernel(op, True)
        self.eq("prefill actions", acts, e["acts_all"])
        self.eq("prefill next actions", nxt, e["next"])
        self.eq("prefill states", states, e["states"], self.state_atol)

    def op_update_velocity(self, op, e):
        self.env.update_velocity(op["draws"])

    def op_load_saved_positions(self, op, e):
        self.env.load_saved_positions(op["trace"])

    def compare_export(self, e, st=None):
        st = self.env.export_state() if st is None else st
        for k in ("pos_x", "pos_y", "vel", "seq", "age", "x"):
            self.eq("export_state " + k, st[k], e[k])
        if "la" in e:
            self.eq("export_state la", st["la"].cpu().numpy().astype(np.int64), e["la"])

    def op_export(self, op, e):
        self.compare_export(e["export"])

    def op_export_import(self, op, e):
        st = self.env.export_state()
        self.env.import_state(st["pos_x"], st["pos_y"], st["vel"], seq=st["seq"], age=st["age"], x=st["x"], la=st.get("la"))
        self.compare_export(e["export"], st)

    def op_export_entries_import(self, op, e):
        self.env.import_entries(self.env.export_entries())

    def op_import_partial(self, op, e):
        if op["what"] == "pos":
            self.env.import_state(pos_x=op["pos_x"], vel=op["vel"])
        else:
            c = e["tables"]
            self.env.import_state(seq=c["seq"], age=c["age"], x=c["x"])

    def op_flat_flip(self, op, e):
        self.env.import_state(pos_y=op["pos_y"])

    def op_restore_flat(self, op, e):
        self.env.import_state(pos_y=np.zeros((self.B, self.N)))

    def op_import_offroad(self, op, e):
        self.env.import_state(pos_x=op["pos_x"], vel=op["vel"])

    def op_reset(self, op, e):
        self.env.reset_topology(op["x0"], None, op["v0"])
        self.t = 0

    def compare_metrics(self, m, want):
        m = m.cpu().numpy()
        metrics_equal(m, want, self.where("metrics"), prr=True)

    def op_metrics(self, op, e):
        self.compare_metrics(self.env.metrics(clear=op["clear"]), e["metrics"])

    def op_info_age(self, op, e):
        self.eq("info_age", self.env.info_age(e["t"]), e["info_age"])

    def op_check(self, op, e):
        self.env.check()

    def run(self):
        for self.i, (op, e) in enumerate(zip(self.prog["ops"], self.expected)):
            self.log.append(P.describe(op))
            try:
                getattr(self, "op_" + op["op"])(op, e)
            except AssertionError:
                raise
            except Exception as err:                                 # an error status where a result was expected
                raise AssertionError(self.where("%s: %s" % (type(err).__name__, err))) from err
        self.i, c = len(self.prog["ops"]), self.closing
        self.log.append("closing")
        self.compare_export(c["export"])
        self.compare_metrics(self.env.metrics(), c["metrics"])
        if "info_age" in c:
            self.eq("info_age", self.env.info_age(c["t"]), c["info_age"])
        self.env.check()


@pytest.mark.parametrize("family,seed", CASES + sorted(REGRESSIONS.values()))
def test_call_program_against_the_host_model(family, seed, monkeypatch):
    Run(family, seed, monkeypatch).run()
