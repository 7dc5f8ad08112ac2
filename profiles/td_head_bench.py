"""The TD head (QLoss -> diral_td_head) and the acting window (ReplayMemory.history -> diral_memory_history) against the
torch compositions they replace, timed interleaved in one process on one box: every round times `--reps` back-to-back calls
of every form between two device events, the figure is the median round's time per call.  A call's time includes its
enqueue: at these sizes a form of several small launches is bound by the host as much as by the device, which is what a
training loop pays.

  td_head          QLoss.loss(...).backward(): the head's launch, the loss launch, autograd's grad_q * grad_output
  torch td_head    argmax, gather, the mixed-precision target, gather, where, square().mean(), and backward to q.grad
  history          ReplayMemory.history(step): one launch
  torch history    index_select of the ring rows + permute().contiguous() + cast

Shapes: C2 (N = 64, A = 32, S = 52, step 6) at batch 64 and 512 with float32 and bfloat16 Q (rows = N * batch; the window
of B = batch envs), and the toy config (N = 4, A = 3, S = 23) at batch 64, with B = 65536 for `history`.

  python profiles/td_head_bench.py [--rounds 7] [--warm 2] [--reps 50] > profiles/td_head/td_head_bench.txt
"""
import argparse

import torch

import ab  # noqa: E402  (puts the repository's root on sys.path)
from diral_amd.memory import ReplayMemory  # noqa: E402
from diral_amd.qloss import QLoss  # noqa: E402

GAMMA = 0.99
# (name, N, A, S, step, batch, envs of the window, Q dtype)
SHAPES = [("c2 batch 64 f32", 64, 32, 52, 6, 64, 64, torch.float32), ("c2 batch 64 bf16", 64, 32, 52, 6, 64, 64, torch.bfloat16),
          ("c2 batch 512 f32", 64, 32, 52, 6, 512, 512, torch.float32), ("c2 batch 512 bf16", 64, 32, 52, 6, 512, 512, torch.bfloat16),
          ("toy batch 64 f32", 4, 3, 23, 6, 64, 65536, torch.float32)]


def torch_head(q, actions, rewards, qn_target, qn_eval):
    """The composition: double-DQN target in NumPy's mixed precision, the hysteretic loss, backward to q.grad."""
    q.grad = None
    j = qn_eval.float().argmax(-1, keepdim=True)
    nv = qn_target.float().gather(1, j).squeeze(1)
    targets = (rewards.double() + (nv * GAMMA).double()).float()
    h = q.float().gather(1, actions.long().unsqueeze(1)).squeeze(1) - targets
    loss = torch.where(h < 0, h / 10, h).square().mean()
    loss.backward()
    return loss


def run(emit, name, N, A, S, step, batch, envs, dtype, rounds, warm, reps):
    dev = torch.device("cuda:0")
    rows = N * batch
    g = torch.Generator(dev).manual_seed(1)
    q = torch.randn((rows, A), device=dev, generator=g).to(dtype).requires_grad_(True)
    qt, qe = (torch.randn((rows, A), device=dev, generator=g).to(dtype) for _ in range(2))
    actions = torch.randint(0, A, (rows,), dtype=torch.int32, device=dev, generator=g)
    rewards = torch.randn((rows,), device=dev, generator=g)
    head = QLoss(GAMMA, double=True, hysteretic=True, device=dev)

    def ours():
        q.grad = None
        head.loss(q, actions, rewards, qt, qe).backward()

    C = 2 * step
    memory = ReplayMemory(C, envs, N, S, device=dev)
    memory.begin(torch.randn((envs, N, S), device=dev, generator=g))
    for _ in range(C + 3):                                          # past the wrap
        memory.add(torch.zeros((envs, N), dtype=torch.int32, device=dev), torch.zeros((envs, N), device=dev),
                   torch.randn((envs, N, S), device=dev, generator=g))
    out = torch.empty((envs * N, step, S), dtype=dtype, device=dev)
    ring_rows = torch.tensor([(memory.count - step + 1 + s) % (C + 1) for s in range(step)], device=dev)

    def torch_history():
        return memory.states.index_select(0, ring_rows).permute(1, 2, 0, 3).contiguous().view(envs * N, step, S).to(dtype)

    forms = [dict(form="td_head", body=ours), dict(form="torch td_head", body=lambda: torch_head(q, actions, rewards, qt, qe)),
             dict(form="history", body=lambda: memory.history(step, out_dtype=dtype, out=out)),
             dict(form="torch history", body=torch_history)]
    ab.timed_rounds(forms, ab.own_body, rounds, warm, reps=reps)
    # what was timed is what the tests compare
    ours()
    mine, mine_loss = q.grad.clone(), float(head.loss(q, actions, rewards, qt, qe).detach())
    theirs_loss = float(torch_head(q, actions, rewards, qt, qe).detach())
    close = bool(torch.allclose(mine.float(), q.grad.float(), rtol=1e-2 if dtype == torch.bfloat16 else 1e-5, atol=0.0))
    same_window = bool(torch.equal(memory.history(step, out_dtype=dtype), torch_history()))
    us, rnd = ab.summary(forms, reps)
    rec = dict(shape=name, N=N, A=A, S=S, step=step, batch=batch, rows=rows, window_envs=envs, q_dtype=str(dtype), rounds=rounds,
               reps=reps, us_per_call=us, gradient_agrees_with_torch=close, loss=[mine_loss, theirs_loss],
               window_equals_torch=same_window, us_rounds=rnd)
    emit("%s rows=%d A=%d / window B=%d N=%d S=%d step=%d, us per call: %s" % (
        name, rows, A, envs, N, S, step, "  ".join("%s %.1f" % kv for kv in us.items())), rec)


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
