"""ms per C2-shaped eager step (bench.py's C2 world: SD1.5, 512 x 512, bf16, batch 1) with and without StepConfig.tune_vae, and the
peak memory each arm adds over the resident set - what the saved conv inputs of the trained decoder cost.

    python tools/mb_tune_vae_step.py [--steps 3] [--out FILE]

One process; the frozen arm first, then the same UNet / BLIP / discriminator objects with a bank-backed decoder."""
import argparse
import dataclasses
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from comat_amd import _hip, config, ops, weights  # noqa: E402
from comat_amd.step import CoMatTrainer  # noqa: E402
from comat_amd.unet import VAEBank, VAEDecoder  # noqa: E402


def timed(trainer, batch, fixed, steps):
    trainer.train_step(batch, **fixed)  # warm-up: workspaces, memos
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        trainer.train_step(batch, **fixed)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms, (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    ops.set_kernel_backend(_hip.HipKernels())
    trainer, batch, fixed, scfg, _, _ = bench.build_world(dev, dtype, 0, "c2")
    lines = [f"C2-shaped eager step (SD1.5, 512 x 512, bf16, batch 1, K = total_step = 5), {args.steps} steps after one warm-up; "
             f"library {_hip.build_id()}"]
    ms, peak = timed(trainer, batch, fixed, args.steps)
    lines.append(f"tune_vae off: median {statistics.median(ms):8.1f} ms/step (min {min(ms):.1f}, max {max(ms):.1f}); peak above resident {peak:8.0f} MiB")
    vsd = weights.make_vae_weights(config.SD15_VAE, seed=2345)
    vbank = VAEBank(config.SD15_VAE, vsd, dtype, dev)
    trainer.pipe.vae = VAEDecoder(config.SD15_VAE, vsd, dtype, dev, bank=vbank)
    tuned = CoMatTrainer(trainer.pipe, trainer.bank, trainer.blip, trainer.D, dataclasses.replace(scfg, tune_vae=True), seed=0)
    ms, peak = timed(tuned, batch, fixed, args.steps)
    lines.append(f"tune_vae on:  median {statistics.median(ms):8.1f} ms/step (min {min(ms):.1f}, max {max(ms):.1f}); peak above resident {peak:8.0f} MiB")
    lines.append(f"trained VAE parameters: {vbank.flat.numel() / 1e6:.1f} M (fp32 master + gradient + two moments + bf16 copy)")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
