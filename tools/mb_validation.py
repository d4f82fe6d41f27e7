"""Validation sampling in numbers (profiles/validation.txt), one MI355X, bf16:

  * the wall time of CoMatTrainer.validate for 1 prompt x 4 images at SD1.5, 512 x 512, 40 DDPM steps, batch_size 1 - with the eager
    no-grad UNet, and with its graphs prepared for the call's key (pipeline.prepare_graphs(1, 512, 512, 77, 40));
  * comat_image_u8 at B = 4, 512 x 512, C = 3, bf16: HIP-event time per launch and the rate against the bytes it must move
    (2 bytes read + 1 byte written per element).

Seeded synthetic weights (as bench.py); nothing here is part of a timed training step.  python tools/mb_validation.py [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from comat_amd import _hip, config, ops, weights  # noqa: E402
from comat_amd.pipeline import TrainableSDPipeline  # noqa: E402
from comat_amd.step import CoMatTrainer, StepConfig  # noqa: E402
from comat_amd.unet import LoRABank, UNet, VAEDecoder  # noqa: E402
from comat_amd.validate import ValidationConfig  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    ops.set_kernel_backend(_hip.HipKernels())
    lines = [f"library {_hip.build_id()}, {torch.cuda.get_device_name(0)}, bf16"]

    # ---- comat_image_u8 alone ----
    B, H, W, C = 4, 512, 512, 3
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(B * H * W, C, generator=g) * 0.6).to(dtype).to(dev)
    out = torch.empty((B, H, W, C), dtype=torch.uint8, device=dev)
    bad = torch.zeros(B, dtype=torch.int32, device=dev)
    for _ in range(5):
        ops.image_u8(x, B, H, W, out=out.view(B * H, W, C), bad=bad)
    torch.cuda.synchronize()
    times = []
    for _ in range(50):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        ops.image_u8(x, B, H, W, out=out.view(B * H, W, C), bad=bad)
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    moved = x.numel() * (x.element_size() + 1)
    med = statistics.median(times)
    lines.append(f"comat_image_u8, B = {B}, {H} x {W}, C = {C}, bf16: {med * 1e3:.1f} us per launch (min {min(times) * 1e3:.1f}, max "
                 f"{max(times) * 1e3:.1f}; median of 50, HIP events), {moved / 1e6:.2f} MB moved -> {moved / med / 1e6:.0f} GB/s")

    # ---- trainer.validate ----
    ucfg, vcfg = config.SD15_UNET, config.SD15_VAE
    bank = LoRABank(ucfg, weights.make_lora_weights(ucfg, seed=4321), dtype, dev)
    pipe = TrainableSDPipeline(UNet(ucfg, weights.make_unet_weights(ucfg, seed=1234), dtype, dev, bank),
                               VAEDecoder(vcfg, weights.make_vae_weights(vcfg, seed=2345), dtype, dev))
    trainer = CoMatTrainer(pipe, bank, None, None, StepConfig(resolution=512, total_step=40, K=5, gan_loss=False), seed=0)
    cfg = ValidationConfig(num_inference_steps=40, num_validation_images=4, seed=7, height=512, width=512, batch_size=1)
    batch = dict(prompt_embeds=torch.randn(1, 77, ucfg.cross_attention_dim, generator=g),
                 negative_prompt_embeds=torch.randn(1, 77, ucfg.cross_attention_dim, generator=g))

    def timed(label):
        trainer.validate(cfg, batch)  # warm-up: memoised time embeddings, workspaces
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            res = trainer.validate(cfg, batch)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        lines.append(f"trainer.validate, 1 prompt x 4 images, SD1.5 512 x 512, 40 steps, batch_size 1, {label}: "
                     f"{statistics.median(ts):.3f} s (min {min(ts):.3f}, max {max(ts):.3f}; {args.reps} calls, wall time incl. the copy "
                     f"to the host), {int(res.bad.sum())} images flagged non-finite")

    graphed = pipe.graphed
    pipe.graphed = None
    timed("eager no-grad UNet")
    pipe.graphed = graphed
    if graphed is not None:
        t0 = time.perf_counter()
        n = pipe.prepare_graphs(1, 512, 512, 77, 40)
        lines.append(f"prepare_graphs(1, 512, 512, 77, 40): {n} graphs in {time.perf_counter() - t0:.1f} s (once, before training)")
        timed("replayed no-grad UNet graphs")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
