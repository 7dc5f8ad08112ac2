"""The dense Q-network forward (QNet.forward -> diral_qnet_forward, ONE launch) against the torch composition it replaces,
timed interleaved in one process on one box: every round times `--reps` back-to-back calls of every form between two
device events, the figure is the median round's time per call (enqueue included, as a training loop pays it).

  qnet             QNet.forward(x, out=out): one launch, float32 MFMA, the activations never leave the workgroup
  torch            per hidden layer addmm, relu, F.layer_norm, then addmm - float32, under no_grad, on the same blob
                   (QNet.torch_module()'s chain with addmm written out)

Shapes: the C2 acting pass (262 144 rows, 52 -> 256 -> 256 -> 32), C2 training batches (4096 and 32 768 rows), the DRQN
head behind an LSTM of 256 (256 -> 256 -> 32, the same row counts) and the toy config's acting pass (262 144 rows,
23 -> 256 -> 256 -> 3).

  python profiles/qnet_bench.py [--rounds 7] [--warm 2] [--reps 10] > profiles/qnet/qnet_bench.txt
"""
import argparse

import torch
import torch.nn.functional as F

import ab  # noqa: E402  (puts the repository's root on sys.path)
from diral_amd.qnet import QNet  # noqa: E402

# (name, rows, D, hidden, A)
SHAPES = [("c2 acting", 262144, 52, (256, 256), 32), ("c2 training 4096", 4096, 52, (256, 256), 32),
          ("c2 training 32768", 32768, 52, (256, 256), 32), ("drqn head acting", 262144, 256, (256,), 32),
          ("drqn head training 4096", 4096, 256, (256,), 32), ("toy acting", 262144, 23, (256, 256), 3)]


def torch_chain(net, dtype=torch.float32):
    v, L, eps = {k: t.to(dtype) for k, t in net.views().items()}, net.L, net.ln_eps
    if dtype == torch.float32:
        v = net.views()                                             # the blob itself, no copy

    def run(x):
        with torch.no_grad():
            h = x.to(dtype)
            for l in range(1, L + 1):
                h = torch.relu(torch.addmm(v["b%d" % l], h, v["W%d" % l]))
                h = F.layer_norm(h, h.shape[-1:], v["gamma%d" % l], v["beta%d" % l], eps=eps)
            return torch.addmm(v["b_out"], h, v["W_out"])
    return run


def run(emit, name, rows, D, hidden, A, rounds, warm, reps):
    dev = torch.device("cuda:0")
    g = torch.Generator(dev).manual_seed(1)
    x = torch.rand((rows, D), device=dev, generator=g) * 1.5 - 0.5
    net = QNet(D, hidden, A, device=dev, seed=2)
    out = torch.empty((rows, A), device=dev)
    theirs = torch_chain(net)
    forms = [dict(form="qnet", body=lambda: net.forward(x, out=out)), dict(form="torch", body=lambda: theirs(x))]
    ab.timed_rounds(forms, ab.own_body, rounds, warm, reps=reps)
    # what was timed, against the same chain in float64: the largest error of either form, relative to max |q|
    ref = torch_chain(net, torch.float64)(x)
    scale = float(ref.abs().max())
    err = {"qnet": float((net.forward(x).double() - ref).abs().max()) / scale,
           "torch": float((theirs(x).double() - ref).abs().max()) / scale}
    us, rnd = ab.summary(forms, reps)
    flop = 2.0 * rows * sum(i * o for i, o in zip(net.widths[:-1], net.widths[1:]))
    rec = dict(shape=name, rows=rows, widths=net.widths, rounds=rounds, reps=reps, us_per_call=us,
               tflops={k: round(flop / (t * 1e-6) / 1e12, 2) for k, t in us.items()}, max_err_vs_float64_rel_to_max_q=err,
               us_rounds=rnd)
    emit("%s rows=%d %s, us per call: %s   (qnet / torch = %.2f; max error against float64, of max |q|: qnet %.1e torch %.1e)" % (
        name, rows, " -> ".join(str(w) for w in net.widths), "  ".join("%s %.1f" % kv for kv in us.items()),
        us["qnet"] / us["torch"], err["qnet"], err["torch"]), rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    print("device: %s" % torch.cuda.get_device_name(0), flush=True)
    with ab.report() as emit:
        for shape in SHAPES:
            run(emit, *shape, rounds=args.rounds, warm=args.warm, reps=args.reps)


if __name__ == "__main__":
    main()
