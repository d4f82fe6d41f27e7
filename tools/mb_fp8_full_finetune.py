"""`--full_finetuning` with the fp8 forward (UNetBank(fp8=True), UNet(bank=, fp8_forward=True)) in numbers, on one MI355X.

    python tools/mb_fp8_full_finetune.py [--steps 3] [--reps 20] [--out profiles/fp8_full_finetuning.txt]

One process, bench.py's C2 world (SD1.5, 512 x 512, bf16, batch 1, K = total_step = 5):
  * one fully trained step with and without the fp8 forward (delayed scaling, calibrated), eager and segmented, with peak memory.
    Both worlds stay alive to the end: nothing that holds captured graphs is destroyed while the process goes on capturing;
  * comat_weights_refresh_q8 over the whole SD1.5 bank next to the plain comat_weights_refresh on the same tables, and next to what
    it replaces for the bytes: comat_fp8_scale + comat_fp8_quantize (two launches) per eligible holder.  Bytes per element in bf16
    mode: 8 for every weight (4 read, 2 x 2 written) + 3 for the quantised ones (2 read, 1 written).
Times are medians of HIP-event intervals over `--reps` launches after a warm-up (steps: wall clock around a synchronise); every
buffer is far larger than the caches.  Every line is printed as soon as it is measured."""
import argparse
import dataclasses
import faulthandler
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mb_full_finetune_step import event_ms, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    faulthandler.enable()  # a native crash (GPU runtime, extension) leaves the Python stack on stderr, as in bench.py
    import bench
    from comat_amd import _hip, config, ops, refresh, weights
    from comat_amd.pipeline import TrainableSDPipeline
    from comat_amd.segments import SegmentedStep
    from comat_amd.step import CoMatTrainer
    from comat_amd.unet import UNet, UNetBank
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    ops.set_kernel_backend(_hip.HipKernels())
    k = ops.kernels()
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)
    say(f"one MI355X, library {_hip.build_id()}; medians of {args.reps} HIP-event intervals (min, max)")
    trainer, batch, fixed, scfg, _, _ = bench.build_world(dev, dtype, 0, "c2")
    vae, blip, disc = trainer.pipe.vae, trainer.blip, trainer.D
    usd = weights.make_unet_weights(config.SD15_UNET, seed=1234)
    cfg = dataclasses.replace(scfg, full_finetuning=True)
    say("C2-shaped step (SD1.5, 512 x 512, bf16, batch 1, K = total_step = 5), every UNet parameter trained")
    keep = [trainer]
    for fp8 in (False, True):
        ops.set_fp8_scaling("delayed" if fp8 else "jit")
        ubank = UNetBank(config.SD15_UNET, usd, dtype, dev, fp8=fp8)
        pipe = TrainableSDPipeline(UNet(config.SD15_UNET, usd, dtype, dev, bank=ubank, fp8_forward=fp8), vae)
        full = CoMatTrainer(pipe, ubank, blip, disc, cfg, seed=0)
        if fp8:
            full.fp8_calibrate(batch)
        tag = "fp8 forward " if fp8 else "bf16 forward"
        say(f"{tag}, eager:     {timed(full.train_step, batch, fixed, args.steps)}")
        stepper = SegmentedStep(full)
        say(f"{tag}, segmented: {timed(stepper, batch, fixed, args.steps)}" + (f"  [{stepper.failed}]" if stepper.failed else ""))
        keep += [ubank, pipe, full, stepper]
    # ---- the refresh (the fp8 bank of the last world) ----
    ubank.ensure_compute_copy()
    plan, n = ubank._plan, len(ubank._slot)
    nw = sum(h.w.numel() for h in ubank.holders)
    q = [h for h in ubank.holders if getattr(h, "_w8", None) is not None]
    nq = sum(h.w.numel() for h in q)
    say(f"SD1.5 bank: {nw / 1e6:.1f} M weight elements in {len(ubank.holders)} holders, {len(plan.problems)} matrices, "
        f"{plan.tiles.shape[0]} tiles; {nq / 1e6:.1f} M elements in {n} quantised weights")
    plain = refresh.RefreshPlan(ubank._problems, dev)
    med0, lo, hi = event_ms(lambda: plain.run(ubank.flat, ubank.flat_c, ubank.flat_t), args.reps)
    say(f"comat_weights_refresh (one launch):           {med0:7.3f} ms ({lo:.3f}, {hi:.3f}), {8 * nw / med0 / 1e9:6.2f} TB/s at 8 B/element")
    med, lo, hi = event_ms(lambda: plan.run(ubank.flat, ubank.flat_c, ubank.flat_t, ubank.flat_q8, ubank.w_scale[:n], ubank.w_amax[:n]),
                           args.reps)
    by = 8 * nw + 3 * nq
    say(f"comat_weights_refresh_q8 (three launches):    {med:7.3f} ms ({lo:.3f}, {hi:.3f}), {by / med / 1e9:6.2f} TB/s at "
        f"{by / nw:.2f} B/element (8 + 3 for the quantised ones); {med / med0:.3f} x the plain launch, byte model {by / (8 * nw):.3f} x")
    outs = [(torch.empty(h.w.shape, dtype=torch.uint8, device=dev), torch.empty(1, device=dev)) for h in q]

    def per_holder():
        for h, (o, s) in zip(q, outs):
            k.fp8_quantize(h.w, out=o, scale=s)
    medh, lo, hi = event_ms(per_holder, max(3, args.reps // 4))
    say(f"what the bytes would cost per holder (comat_fp8_scale + comat_fp8_quantize, {2 * len(q)} launches): {medh:7.3f} ms "
        f"({lo:.3f}, {hi:.3f}); plain refresh + per-holder = {med0 + medh:.3f} ms against {med:.3f} ms")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
