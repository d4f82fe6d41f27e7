"""Golden traces of gradient accumulation (`--gradient_accumulation_steps`, training_script.py:556,680), from the installed
accelerate + torch + transformers on the CPU.

    python tests/golden/make_grad_accum_golden.py      # writes tests/golden/grad_accum.json

The toy problem: one 6-element parameter, loss_i = <w, g_i> with fixed vectors g_i (so micro-step i's gradient is g_i, whatever w
is), `torch.optim.AdamW` with the generator's betas / eps / weight decay, `clip_grad_norm_(0.1)` under `if sync_gradients`, a
scheduler from `transformers.get_scheduler` built - as training_script.py:293-294 does - with warmup * N and total * N, all of it
prepared by an `Accelerator(cpu=True, gradient_accumulation_steps=N)` and run inside `accelerator.accumulate(model)` with
`accelerator.backward(loss)`.

"documented" order (what this project builds; accelerate's documentation): backward, [clip,] optimizer.step(), scheduler.step(),
optimizer.zero_grad().  Cases: N in {1, 2, 3} x {constant, linear with warmup 1}, 7 micro-steps each; after every micro-step the
case records `sync_gradients`, the parameter (float32 values) and `scheduler.get_last_lr()[0]`.  Some gradients are scaled so
small that the clip does not act.  Two more traces, as in lr_schedules.json:
  * "nonfinite": N = 2, the 4th micro-step's gradient (a closing one) holds an inf.  No gradient scaler runs on the CPU, so what a
    scaler does there is done by hand: optimizer.step() is not called and the flag a skipped step leaves behind
    (`AcceleratedOptimizer._is_overflow`) is set before scheduler.step(); the wrappers' own code does the rest.
  * "stride": N = 2, linear, with `num_processes` of the shared state set to 2: two scheduler steps per applied update.

Evidence for INTEGRATION.md only (no test of the product reads it):
  * "reference_order": the loop as training_script.py:658,689 has it - optimizer.zero_grad() BEFORE backward - on the same toy
    (N = 2, constant), and the SGD probe (N = 2, lr 1, w0 = 1, gradients 1 and 2) under both orders.
  * "two_contexts": two `accumulate` contexts per iteration (generator's, then discriminator's) sharing accelerate's one step
    counter: `sync_gradients` inside each, 8 iterations, N = 2 and 3.
Only numbers are stored."""
import json
import math
import os
import warnings

import torch
from transformers import get_scheduler

HERE = os.path.dirname(os.path.abspath(__file__))
LR, BETAS, EPS, WD, MAX_NORM = 5e-3, (0.9, 0.999), 1e-8, 1e-2, 0.1
STEPS, NPARAM, TOTAL = 7, 6, 4
GRAD_SCALE = (1.0, 0.01, 0.5, 1.0, 0.02, 0.01, 1.0)  # per micro-step: with and without the clip acting


class Toy(torch.nn.Module):
    def __init__(self, w0):
        super().__init__()
        self.w = torch.nn.Parameter(w0.clone())

    def forward(self, g):
        return (self.w * g).sum()


def fresh_accelerator(N):
    from accelerate import Accelerator
    from accelerate.state import AcceleratorState, GradientState
    AcceleratorState._reset_state(True)
    GradientState._reset_state()
    return Accelerator(cpu=True, gradient_accumulation_steps=N)


def inputs():
    gen = torch.Generator().manual_seed(20)
    w0 = torch.randn(NPARAM, generator=gen)
    grads = [torch.randn(NPARAM, generator=gen) * s for s in GRAD_SCALE]
    return w0, grads


def run(N, kind, warmup, order="documented", inf_at=None, num_processes=1):
    from accelerate.state import AcceleratorState, PartialState
    acc = fresh_accelerator(N)
    shared = (PartialState._shared_state, AcceleratorState._shared_state)
    before = PartialState._shared_state["num_processes"]
    w0, grads = inputs()
    if inf_at is not None:
        grads[inf_at] = grads[inf_at].clone()
        grads[inf_at][2] = float("inf")
    model = Toy(w0)
    opt = torch.optim.AdamW(model.parameters(), lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    sched = get_scheduler(kind, opt, num_warmup_steps=warmup * N, num_training_steps=TOTAL * N)
    model, opt, sched = acc.prepare(model, opt, sched)
    for s in shared:
        s["num_processes"] = num_processes
    trace = []
    try:
        for g in grads:
            with acc.accumulate(model):
                if order == "reference":
                    opt.zero_grad()
                loss = model(g)
                acc.backward(loss)
                skipped = False
                if acc.sync_gradients:
                    finite = bool(torch.isfinite(model.w.grad).all())
                    if finite:
                        acc.clip_grad_norm_(model.parameters(), MAX_NORM)
                    skipped = not finite
                if not skipped:
                    opt.step()
                opt._is_overflow = skipped
                sched.step()
                if order == "documented":
                    opt.zero_grad()
            trace.append(dict(sync_gradients=bool(acc.sync_gradients), skipped=skipped,
                              params=[float(x) for x in model.w.detach().float()], lr=float(sched.get_last_lr()[0])))
    finally:
        for s in shared:
            s["num_processes"] = before
    return dict(accum_steps=N, kind=kind, warmup=warmup * N, total=TOTAL * N, num_processes=num_processes, order=order,
                lr0=LR, grads=[[float(x) if math.isfinite(float(x)) else "inf" for x in g] for g in grads], trace=trace)


def sgd_probe(order):
    acc = fresh_accelerator(2)
    model = Toy(torch.ones(1))
    opt = torch.optim.SGD(model.parameters(), lr=1.0)
    model, opt = acc.prepare(model, opt)
    for g in (1.0, 2.0):
        with acc.accumulate(model):
            if order == "reference":
                opt.zero_grad()
            acc.backward(model(torch.tensor([g])))
            opt.step()
            if order == "documented":
                opt.zero_grad()
    return float(model.w.detach()[0])


def two_contexts(N, iterations=8):
    acc = fresh_accelerator(N)
    G, D = Toy(torch.ones(1)), Toy(torch.ones(1))
    oG, oD = torch.optim.SGD(G.parameters(), lr=1.0), torch.optim.SGD(D.parameters(), lr=1.0)
    G, D, oG, oD = acc.prepare(G, D, oG, oD)
    seen = dict(G=[], D=[])
    for _ in range(iterations):
        with acc.accumulate(G):
            seen["G"].append(bool(acc.sync_gradients))
        with acc.accumulate(D):
            seen["D"].append(bool(acc.sync_gradients))
    return seen


def main():
    warnings.simplefilter("ignore")
    import accelerate
    import transformers
    cases = [run(N, kind, warmup) for N in (1, 2, 3) for kind, warmup in (("constant", 0), ("linear", 1))]
    out = dict(hyper=dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, max_norm=MAX_NORM), w0=[float(x) for x in inputs()[0]],
               torch=torch.__version__.split("+")[0], transformers=transformers.__version__, accelerate=accelerate.__version__,
               cases=cases,
               nonfinite=run(2, "linear", 1, inf_at=3),
               stride=run(2, "linear", 1, num_processes=2),
               evidence=dict(reference_order=run(2, "constant", 0, order="reference"),
                             sgd_probe=dict(documented=sgd_probe("documented"), reference=sgd_probe("reference")),
                             two_contexts={str(N): two_contexts(N) for N in (2, 3)}))
    with open(os.path.join(HERE, "grad_accum.json"), "w") as f:
        json.dump(out, f, indent=1)
    for c in cases + [out["nonfinite"], out["stride"]]:
        print(c["accum_steps"], c["kind"], [t["sync_gradients"] for t in c["trace"]], [t["lr"] for t in c["trace"]])
    print(out["evidence"]["sgd_probe"], out["evidence"]["two_contexts"])


if __name__ == "__main__":
    main()
