"""Action selection from Q-values (QPolicy -> diral_policy_select) against the torch composition it replaces, timed
interleaved in one process on one box: every round times `--reps` back-to-back calls of every form between two device
events, the figure is the median round's time per call.  A call's time includes its enqueue: at these sizes a form of
several small launches is bound by the host as much as by the device, which is what a training loop pays.  The same
`--reps` calls are then captured into one graph per form and the replays timed the same way: the device's share.

  greedy / eps_greedy / softmax / boltzmann   one launch each (device draws)
  torch argmax                                q.argmax(-1).to(int32)
  torch eps_greedy                            rand, randint, argmax, compare, where, cast
  torch softmax                               softmax(q / tmp) + multinomial + cast

Shapes: C2 (B = 4096, N = 64, A = 32; float32 and bfloat16 Q) and the toy config (N = 4, A = 3) at B = 65536.  `q_tb_per_s_in_graph`
is the Q read alone (agents x A x itemsize) over the call's time inside the graph, next to the 6.29 TB/s of the flat copy in
profiles/copy_envs/copy_bench.txt.

  python profiles/select_actions_bench.py [--rounds 7] [--warm 2] [--reps 50] > profiles/select_actions/select_bench.txt
"""
import argparse

import torch

import ab  # noqa: E402  (puts the repository's root on sys.path)
from diral_amd.qpolicy import QPolicy  # noqa: E402

SHAPES = [("c2 f32", 4096, 64, 32, torch.float32), ("c2 bf16", 4096, 64, 32, torch.bfloat16), ("toy f32", 65536, 4, 3, torch.float32)]
FLAT_COPY_TB_S = 6.29


def run(emit, name, B, N, A, dtype, rounds, warm, reps):
    dev = torch.device("cuda:0")
    q = torch.randn((B, N, A), dtype=torch.float32, device=dev).to(dtype)
    out = torch.empty((B, N), dtype=torch.int32, device=dev)
    clk = torch.zeros((1,), dtype=torch.int64, device=dev)
    pols = {k: QPolicy(B, N, A, k, seed=1, device=dev, eps_init=0.1, temperature=0.5, explore_start=0.1, explore_stop=0.1)
            for k in ("greedy", "eps_greedy", "softmax", "boltzmann")}
    eps, tmp = 0.1, 0.5

    def torch_eps():
        u = torch.rand((B, N), device=dev)
        r = torch.randint(A, (B, N), device=dev)
        return torch.where(u > eps, q.argmax(-1), r).to(torch.int32)

    def torch_softmax():
        p = torch.softmax(q.float() / tmp, -1).reshape(-1, A)
        return torch.multinomial(p, 1).reshape(B, N).to(torch.int32)

    forms = [dict(form=k, body=(lambda p=p: p.act_clocked(q, clk, out=out))) for k, p in pols.items()]
    forms += [dict(form="torch argmax", body=lambda: q.argmax(-1).to(torch.int32)),
              dict(form="torch eps_greedy", body=torch_eps), dict(form="torch softmax", body=torch_softmax)]
    ab.timed_rounds(forms, ab.own_body, rounds, warm, reps=reps)
    # the device's share of a call: the same `reps` calls captured into one graph, its replay timed (multinomial is left
    # out: it is not capturable on every torch build)
    side = torch.cuda.Stream()
    graphs = []
    for f in forms:
        if f["form"] == "torch softmax":
            continue
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(reps):
                f["body"]()
        torch.cuda.current_stream().wait_stream(side)
        graphs.append(dict(form=f["form"], body=g.replay))
    ab.timed_rounds(graphs, ab.own_body, rounds, warm)
    gus, grnd = ab.summary(graphs, reps)
    # what was timed is what the tests compare: the launch agrees with torch's argmax wherever the row has one maximum
    g = pols["greedy"].act(q).long()
    top2 = q.double().topk(min(2, A), -1).values
    unique = (top2[..., 0] > top2[..., -1]) if A > 1 else torch.ones((B, N), dtype=torch.bool, device=dev)
    agree = bool(torch.equal(g[unique], q.argmax(-1)[unique]))
    us, rnd = ab.summary(forms, reps)
    q_bytes = B * N * A * q.element_size()
    rec = dict(shape=name, B=B, N=N, A=A, q_dtype=str(dtype), rounds=rounds, reps=reps, us_per_call=us, us_per_call_in_graph=gus,
               greedy_agrees_with_torch=agree, q_bytes=q_bytes,
               q_tb_per_s_in_graph={k: round(q_bytes / (v * 1e-6) / 1e12, 3) for k, v in gus.items()}, flat_copy_tb_per_s=FLAT_COPY_TB_S,
               us_rounds=rnd, graph_us_rounds=grnd)
    emit("%s B=%d N=%d A=%d, us per call: %s\n%s ... inside a graph:      %s" % (
        name, B, N, A, "  ".join("%s %.1f" % kv for kv in us.items()), name, "  ".join("%s %.1f" % kv for kv in gus.items())), rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    print("device: %s" % torch.cuda.get_device_name(0), flush=True)
    with ab.report() as emit:
        for shape in SHAPES:
            run(emit, *shape, rounds=args.rounds, warm=args.warm, reps=args.reps)


if __name__ == "__main__":
    main()
