"""`--full_finetuning` (StepConfig.full_finetuning) in numbers.

    python tools/mb_full_finetune_step.py [--steps 3] [--out FILE]          one MI355X
    python tools/mb_full_finetune_step.py --oracle-distance [--out FILE]    CPU only

On the GPU (bench.py's C2 world: SD1.5, 512 x 512, bf16, batch 1, K = total_step = 5), one process:
  * comat_weights_refresh over the whole SD1.5 bank: time and bytes/s (8 bytes per element in bf16 mode: 4 read, 2 x 2 written),
    next to UN_COPY moving the same number of bytes and to the per-holder torch refresh it replaces (one cast of the flat buffer +
    one transposing copy per holder);
  * the two reductions at the SD1.5 shapes: comat_layernorm_bwd_affine on 8192 x 320 ... 128 x 1280 rows, comat_colsum_batched on
    64^2 x 320;
  * eager and segmented step time and peak memory of the LoRA step and of the fully trained UNet on the same box.
Times are medians of HIP-event intervals over `--reps` launches after a warm-up; every buffer is far larger than the caches.

--oracle-distance: the figures the bounds of tests/test_full_finetuning.py come from, on the tiny world: the distance of two oracle
runs that differ only in the convolution algorithm, and the distance of the ABI simulator from the oracle in fp32 and bf16."""
import argparse
import dataclasses
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def oracle_distance():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_full_finetuning as T
    from comat_amd import ops
    from helpers import rel_l2
    from sim_backend import SimKernels
    lines = ["tiny world of tests/test_full_finetuning.py (TINY_UNET, batch 2, K = 2 of 3 steps, GAN loss on), CPU"]
    a, b = T.oracle_step(torch.float32, True), T.oracle_step(torch.float32, False)
    cat = lambda d: torch.cat([d[k].reshape(-1) for k in a["g"]])
    keep = cat(a["clipped"]).abs() >= 10 * T.StepConfig().adam_epsilon
    lines.append(f"two oracle runs, mkldnn on / off: |g| {a['gnorm']:.4e}; gradient rel-L2 {rel_l2(cat(b['g']), cat(a['g'])):.3e}; "
                 f"update rel-L2 {rel_l2(cat(b['update'])[keep], cat(a['update'])[keep]):.3e} over the {100 * float(keep.float().mean()):.1f} % "
                 f"of {keep.numel()} elements with |clipped g| >= 10 eps, {rel_l2(cat(b['update']), cat(a['update'])):.3e} unrestricted")
    for dtype in (torch.float32, torch.bfloat16):
        ops.set_kernel_backend(SimKernels())
        cfg, batch, W, tr = T.make_step_world(dtype, torch.device("cpu"))
        _, e = T.step_errors(tr, batch, T.oracle_step(dtype), cfg)
        ops.set_kernel_backend(None)
        lines.append(f"ABI simulator, {str(dtype).split('.')[-1]} storage, against the fp32 oracle on the same weights: gradient rel-L2 "
                     f"{e['grad']:.3e}, exp_avg {e['m']:.3e}, exp_avg_sq {e['v']:.3e}, restricted update {e['update']:.3e} "
                     f"({100 * e['excluded']:.1f} % excluded), unrestricted {e['update_all']:.3e}")
    return lines


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms), min(ms), max(ms)


def timed(step, batch, fixed, steps):
    step(batch, **fixed)  # warm-up: workspaces, memos, captures
    step(batch, **fixed)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step(batch, **fixed)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return f"median {statistics.median(ms):8.1f} ms/step (min {min(ms):.1f}, max {max(ms):.1f}); peak above resident " \
           f"{(torch.cuda.max_memory_allocated() - base) / 2 ** 20:8.0f} MiB"


def on_gpu(args):
    import bench
    from comat_amd import _hip, config, ops, weights
    from comat_amd.pipeline import TrainableSDPipeline
    from comat_amd.segments import SegmentedStep
    from comat_amd.step import CoMatTrainer
    from comat_amd.unet import UNet, UNetBank
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    ops.set_kernel_backend(_hip.HipKernels())
    k = ops.kernels()
    lines = [f"one MI355X, library {_hip.build_id()}; medians of {args.reps} HIP-event intervals (min, max)"]
    # ---- the reductions ----
    for M, C in ((8192, 320), (2048, 640), (512, 1280), (128, 1280)):
        dy, x = torch.randn(M, C, device=dev).to(dtype), torch.randn(M, C, device=dev).to(dtype)
        st = torch.stack([torch.zeros(M, device=dev), torch.ones(M, device=dev)], 1).contiguous()
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        med, lo, hi = event_ms(lambda: k.layernorm_bwd_affine(dy, x, st, dg, db, M, C), args.reps)
        lines.append(f"comat_layernorm_bwd_affine {M:5d} x {C:4d} bf16: {1e3 * med:7.1f} us ({1e3 * lo:.1f}, {1e3 * hi:.1f}), "
                     f"{(2 * M * C * 2 + M * 8) / med / 1e6:7.1f} GB/s")
    B, M, C = 2, 64 * 64, 320
    g, out = torch.randn(B * M, C, device=dev).to(dtype), torch.zeros(B, C, device=dev)
    med, lo, hi = event_ms(lambda: k.colsum_batched(g, out, B, M, C, C), args.reps)
    lines.append(f"comat_colsum_batched {B} x {M} x {C} bf16: {1e3 * med:7.1f} us ({1e3 * lo:.1f}, {1e3 * hi:.1f}), {B * M * C * 2 / med / 1e6:7.1f} GB/s")
    # ---- the LoRA step, then the same world with the fully trained UNet ----
    trainer, batch, fixed, scfg, _, _ = bench.build_world(dev, dtype, 0, "c2")
    lines.append("C2-shaped step (SD1.5, 512 x 512, bf16, batch 1, K = total_step = 5)")
    lines.append(f"LoRA, eager:                {timed(trainer.train_step, batch, fixed, args.steps)}")
    lines.append(f"LoRA, segmented:            {timed(SegmentedStep(trainer), batch, fixed, args.steps)}")
    usd = weights.make_unet_weights(config.SD15_UNET, seed=1234)
    ubank = UNetBank(config.SD15_UNET, usd, dtype, dev)
    pipe = TrainableSDPipeline(UNet(config.SD15_UNET, usd, dtype, dev, bank=ubank), trainer.pipe.vae)
    blip, disc = trainer.blip, trainer.D
    del trainer
    torch.cuda.empty_cache()
    full = CoMatTrainer(pipe, ubank, blip, disc, dataclasses.replace(scfg, full_finetuning=True), seed=0)
    n = ubank.flat.numel()
    ubank.ensure_compute_copy()  # builds the refresh tables
    lines.append(f"fully trained UNet: {n / 1e6:.1f} M elements in the bank ({len(ubank.holders)} weight holders, "
                 f"{len(ubank._plan.problems) if ubank._plan else 0} matrices, {ubank._plan.tiles.shape[0] if ubank._plan else 0} tiles)")
    lines.append(f"full_finetuning, eager:     {timed(full.train_step, batch, fixed, args.steps)}")
    stepper = SegmentedStep(full)
    lines.append(f"full_finetuning, segmented: {timed(stepper, batch, fixed, args.steps)}" + (f"  [{stepper.failed}]" if stepper.failed else ""))
    # ---- the refresh ----
    nw = sum(h.w.numel() for h in ubank.holders)
    med, lo, hi = event_ms(lambda: ubank._plan.run(ubank.flat, ubank.flat_c, ubank.flat_t), args.reps)
    lines.append(f"comat_weights_refresh, SD1.5 bank ({nw / 1e6:.1f} M weight elements, one launch): {med:7.3f} ms ({lo:.3f}, {hi:.3f}), "
                 f"{8 * nw / med / 1e9:6.2f} TB/s at 8 bytes per element")
    src, dst = torch.empty(nw, device=dev), torch.empty(nw, device=dev)  # 4 read + 4 written per element: the same bytes
    med, lo, hi = event_ms(lambda: k.unary(ops.UN_COPY, src, dst, nw), args.reps)
    lines.append(f"UN_COPY of the same bytes (fp32 -> fp32, {nw / 1e6:.1f} M elements): {med:7.3f} ms ({lo:.3f}, {hi:.3f}), {8 * nw / med / 1e9:6.2f} TB/s")

    def per_holder():
        k.unary(ops.UN_COPY, ubank.flat, ubank.flat_c, n)
        for h in ubank.holders:
            h.refresh()
    med, lo, hi = event_ms(per_holder, max(3, args.reps // 4))
    lines.append(f"per-holder torch refresh it replaces (1 cast + {len(ubank.holders)} transposing copies): {med:7.3f} ms ({lo:.3f}, {hi:.3f})")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--oracle-distance", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    text = "\n".join(oracle_distance() if args.oracle_distance else on_gpu(args))
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
