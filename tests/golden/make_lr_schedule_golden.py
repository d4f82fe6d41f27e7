"""Golden learning rates of the schedules `--lr_scheduler` names (training_script.py:290-295: `get_scheduler(name, optimizer,
num_warmup_steps, num_training_steps)`), from the installed `transformers.optimization` (diffusers' `optimization.py` is a copy
of it; diffusers is not installed in the build container).

    python tests/golden/make_lr_schedule_golden.py      # writes tests/golden/lr_schedules.json

For each of constant, constant_with_warmup, linear, cosine, cosine_with_restarts and polynomial, on a `torch.optim.AdamW` at
lr 5e-5: `scheduler.get_last_lr()[0]` as a double after c calls of `scheduler.step()`, c = 0 .. T + 2, for (warmup W, total T)
in {(0, 10), (3, 10), (4, 4)}; cosine_with_restarts also with num_cycles = 2, polynomial also with power = 2; cosine once more
at (2, 6), the schedule of the whole-step tests.  A clock at which
the library itself raises (polynomial with W == T divides by zero at c == T) ends that case: the case records the exception's
name and the rates before it.

Two traces through `accelerate.scheduler.AcceleratedScheduler` (constructed on the CPU after `Accelerator(cpu=True)`) pin the
two rules of training_script.py:664 under accelerate:
  * "skip":   an optimizer step that was skipped does not advance the scheduler.  No gradient scaler runs on the CPU, so the
              flag a skipped step leaves behind (`AcceleratedOptimizer._is_overflow`, read through `step_was_skipped`) is set by
              hand before that step's `scheduler.step()`; the wrapper's own code does the rest.
  * "stride": without `split_batches` the scheduler advances `num_processes` times per optimizer step; `num_processes` of the
              shared accelerator state is set to 2 for the trace and put back.
Only numbers are stored."""
import json
import os
import warnings

import torch
from transformers import get_scheduler

HERE = os.path.dirname(os.path.abspath(__file__))
BASE_LR = 5e-5
KINDS = ("constant", "constant_with_warmup", "linear", "cosine", "cosine_with_restarts", "polynomial")
WT = ((0, 10), (3, 10), (4, 4))


def make(kind, W, T, extra):
    opt = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=BASE_LR)
    return opt, get_scheduler(kind, opt, num_warmup_steps=W, num_training_steps=T, scheduler_specific_kwargs=extra or None)


def record(kind, W, T, extra):
    case = dict(kind=kind, warmup=W, total=T, lr=[], raises=None, **extra)
    try:
        opt, sched = make(kind, W, T, extra)
        for c in range(T + 3):
            case["lr"].append(float(sched.get_last_lr()[0]))
            if c < T + 2:
                opt.step()
                sched.step()
    except (ZeroDivisionError, ValueError) as e:
        case["raises"] = type(e).__name__
    return case


def accelerate_traces():
    from accelerate import Accelerator
    from accelerate.optimizer import AcceleratedOptimizer
    from accelerate.scheduler import AcceleratedScheduler
    from accelerate.state import AcceleratorState, PartialState
    Accelerator(cpu=True)
    out = {}
    # an optimizer step skipped at update 3 of 6 (cosine, W = 2, T = 8)
    opt, sched = make("cosine", 2, 8, {})
    aopt = AcceleratedOptimizer(opt)
    asched = AcceleratedScheduler(sched, aopt)
    skipped, lrs = [False, False, False, True, False, False], []
    for skip in skipped:
        lrs.append(float(asched.get_last_lr()[0]))
        if not skip:
            aopt.step()
        aopt._is_overflow = skip
        asched.step()
    lrs.append(float(asched.get_last_lr()[0]))
    out["skip"] = dict(kind="cosine", warmup=2, total=8, skipped=skipped, lr=lrs)
    # two processes: two scheduler steps per optimizer step (linear, W = 3, T = 10)
    shared = (PartialState._shared_state, AcceleratorState._shared_state)  # the second is refreshed from the first
    before = PartialState._shared_state["num_processes"]
    for s in shared:
        s["num_processes"] = 2
    try:
        assert AcceleratorState().num_processes == 2
        opt, sched = make("linear", 3, 10, {})
        aopt = AcceleratedOptimizer(opt)
        asched = AcceleratedScheduler(sched, aopt)
        lrs = []
        for _ in range(6):
            lrs.append(float(asched.get_last_lr()[0]))
            aopt.step()
            asched.step()
        lrs.append(float(asched.get_last_lr()[0]))
    finally:
        for s in shared:
            s["num_processes"] = before
    out["stride"] = dict(kind="linear", warmup=3, total=10, num_processes=2, lr=lrs)
    return out


def main():
    warnings.simplefilter("ignore")
    cases = []
    for kind in KINDS:
        for W, T in WT:
            cases.append(record(kind, W, T, {}))
            if kind == "cosine_with_restarts":
                cases.append(record(kind, W, T, dict(num_cycles=2)))
            if kind == "polynomial":
                cases.append(record(kind, W, T, dict(power=2)))
    cases.append(record("cosine", 2, 6, {}))  # the schedule of the whole-step tests (graph replay, checkpoint)
    import accelerate
    import transformers
    out = dict(base_lr=BASE_LR, transformers=transformers.__version__, accelerate=accelerate.__version__, cases=cases,
               accelerate_traces=accelerate_traces())
    with open(os.path.join(HERE, "lr_schedules.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(f"{len(cases)} cases, {sum(len(c['lr']) for c in cases)} rates; raising: "
          f"{[(c['kind'], c['warmup'], c['total']) for c in cases if c['raises']]}")
    for k, t in out["accelerate_traces"].items():
        print(k, t["lr"])


if __name__ == "__main__":
    main()
