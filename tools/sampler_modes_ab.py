"""Same-box, alternating A/B of the C3 trainer step (bench.build_world(..., "c3"): SD1.5 512x512, bs 1, N = 50, K = 5) under the
sampler's modes: default, early_exit, fast_training, double_laststep.

    python tools/sampler_modes_ab.py [--steps 7] [--warmup 3] [--arms default,early_exit,...] [--tree DIR] [--out FILE]

One process, one set of models; every arm is a CoMatTrainer with its own StepConfig and its own SegmentedStep (segments mode: the
no-grad UNet forwards replay from per-timestep graphs, the trained calls, the head and the D step from segment graphs).  After
`--warmup` steps per arm (the first ones capture) the arms take turns, one step each, `--steps` rounds; a step is timed by the
host clock between two device synchronisations.  Per arm: the median and the spread of its steps, next to the number of UNet
forwards and backwards the mode runs (counted from N, K and the trained steps; the call log itself is pinned by
tests/test_sampler_modes.py).  The trained steps are fixed to [4, 14, 24, 34, 44] - the middle draw of
step.sample_training_steps(50, 5) - so that every step of an arm does the same work; attribute concentration is off in every
arm (double_laststep trains no loop step, so there is no map to concentrate).
--tree DIR: import comat_amd and bench from another checkout (the parent commit's, for the yardstick: arm `default` only)."""
import argparse
import dataclasses
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS = [4, 14, 24, 34, 44]
ARMS = {"default": {}, "early_exit": dict(early_exit=True), "fast_training": dict(fast_training=True),
        "double_laststep": dict(double_laststep=True)}


def unet_calls(arm, n, ts):
    """(no-grad forwards, trained forwards, backwards) of one step"""
    k = len(ts)
    if arm == "early_exit":
        return max(ts) + 1 - k, k, k
    if arm == "fast_training":
        return 0, k, k
    if arm == "double_laststep":
        return n, 1, 1
    return n - k, k, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    os.environ["COMAT_C3_ATTRCON"] = "0"
    import torch

    import bench
    from comat_amd import _hip, ops
    from comat_amd.segments import SegmentedStep
    from comat_amd.step import CoMatTrainer
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    ops.set_kernel_backend(_hip.HipKernels())
    trainer, batch, fixed, scfg, _, setup_s = bench.build_world(dev, torch.bfloat16, 0, "c3")
    fixed = dict(fixed, training_steps=TS)
    steppers, batches = {}, {}
    for arm in args.arms.split(","):
        kw = ARMS[arm]
        tr = trainer if not kw else CoMatTrainer(trainer.pipe, trainer.bank, trainer.blip, trainer.D,
                                                 dataclasses.replace(scfg, **kw), seed=0)
        steppers[arm] = SegmentedStep(tr)
        b = dict(batch)
        if arm == "double_laststep":  # one more step noise for the extra step, and the re-noising draw
            g = torch.Generator().manual_seed(151)
            b["noises"] = list(b["noises"]) + [torch.randn(b["noises"][0].shape, generator=g).to(dev)]
            b["renoise"] = torch.randn(b["latents"].shape, generator=g).to(dev)
        batches[arm] = b
    for arm, st in steppers.items():
        for _ in range(args.warmup):
            st(batches[arm], **fixed)
        torch.cuda.synchronize()
        assert st.failed is None, st.failed
    times = {arm: [] for arm in steppers}
    for _ in range(args.steps):
        for arm, st in steppers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            logs = st(batches[arm], **fixed)
            torch.cuda.synchronize()
            times[arm].append((time.perf_counter() - t0) * 1e3)
            assert torch.isfinite(logs["step_loss"]), arm
    lines = [f"C3 trainer step, segments mode, bf16, trained steps {TS}, attribute concentration off; tree {os.path.basename(tree)}",
             f"{torch.cuda.get_device_name(0)}; {args.warmup} warm-up steps per arm, then {args.steps} alternating rounds; "
             f"set-up {setup_s:.0f} s",
             f"{'arm':18s} {'median ms':>10s} {'min':>8s} {'max':>8s}   UNet calls per step (no-grad fwd / trained fwd / bwd)"]
    for arm, t in times.items():
        ng, tf, tb = unet_calls(arm, scfg.total_step, TS)
        lines.append(f"{arm:18s} {statistics.median(t):10.1f} {min(t):8.1f} {max(t):8.1f}   {ng} / {tf} / {tb}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
