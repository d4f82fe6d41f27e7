"""One eager step of the denoising fine-tune (comat_amd/denoise.py) in numbers: SD1.5 and SDXL at 512 x 512, batch 4, every UNet
parameter trained, bf16, synthetic weights and inputs resident in HBM.

    python tools/mb_denoise_step.py [--steps 5] [--models sd15,sdxl] [--out FILE]     one MI355X
    python tools/mb_denoise_step.py --rehearse                                        anywhere: tiny models on the ABI simulator, no timing

Each timed step is one HIP-event interval around `DenoiseTrainer.train_step` (encoder, prepare, UNet forward and backward, MSE, clip +
AdamW, weight refresh) after two warm-up steps; timesteps and noises are drawn on the device, as in a real run.  The encoder alone and
the three new entry points alone are timed the same way."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn, reps):
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return f"median {statistics.median(ms):9.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}, {reps} intervals)"


def world(name, dev, dtype, B, size, tiny):
    from comat_amd import config, weights
    from comat_amd.denoise import DenoiseConfig, DenoiseTrainer
    from comat_amd.unet import UNet, UNetBank, VAEEncoder
    ucfg, vcfg = {"sd15": (config.SD15_UNET, config.SD15_VAE), "sdxl": (config.SDXL_UNET, config.SDXL_VAE)}[name]
    if tiny:
        ucfg, vcfg = {"sd15": config.TINY_UNET, "sdxl": config.TINY_SDXL_UNET}[name], config.TINY_VAE
    usd = weights.make_unet_weights(ucfg, seed=1234)
    bank = UNetBank(ucfg, usd, dtype, dev)
    unet = UNet(ucfg, usd, dtype, dev, bank=bank)
    del usd
    enc = VAEEncoder(vcfg, weights.make_vae_encoder_weights(vcfg), dtype, dev)
    trainer = DenoiseTrainer(unet, bank, enc, DenoiseConfig(lr=1e-5), seed=0)
    g = torch.Generator().manual_seed(1)
    batch = dict(pixel_values=(torch.rand(B, 3, size, size, generator=g) * 2 - 1).to(dev),
                 prompt_embeds=torch.randn(B, 77, ucfg.cross_attention_dim, generator=g).to(dev))
    if ucfg.addition_embed:
        batch["pooled_prompt_embeds"] = torch.randn(B, ucfg.pooled_dim, generator=g).to(dev)
        batch["add_time_ids"] = (size, size, 0, 0, size, size)
    return trainer, batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--models", default="sd15,sdxl")
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from comat_amd import _hip, ops
    if args.rehearse:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from denoise_sim import DenoiseSimKernels
        ops.set_kernel_backend(DenoiseSimKernels())
        for name in args.models.split(","):
            trainer, batch = world(name, torch.device("cpu"), torch.float32, 2, 64, True)
            logs = [trainer.train_step(batch) for _ in range(2)]
            print(f"rehearsal {name} (tiny, simulator, no timing): loss {float(logs[0]['loss']):.4f} -> {float(logs[1]['loss']):.4f}")
        return
    if not torch.cuda.is_available():
        raise SystemExit("mb_denoise_step: no GPU - nothing is measured without one (--rehearse checks the host logic)")
    dev, dtype, B, size = torch.device("cuda:0"), torch.bfloat16, 4, 512
    ops.set_kernel_backend(_hip.HipKernels())
    lines = [f"one MI355X, library {_hip.build_id()}; eager launches, bf16, batch {B}, {size} x {size}, every UNet parameter trained; "
             "a FIRST measurement, no target attached"]
    for name in args.models.split(","):
        trainer, batch = world(name, dev, dtype, B, size, False)
        for _ in range(2):
            logs = trainer.train_step(batch)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        lines.append(f"{name}: {trainer.bank.flat.numel() / 1e6:.1f} M trained elements")
        lines.append(f"  train_step:            {event_ms(lambda: trainer.train_step(batch), args.steps)}; peak above resident "
                     f"{(torch.cuda.max_memory_allocated() - base) / 2 ** 20:.0f} MiB; loss {float(logs['loss']):.4f}")
        px = ops.nchw_to_tokens(batch["pixel_values"])
        lines.append(f"  VAE encoder alone:     {event_ms(lambda: trainer.vae(px, B, size, size), args.steps)}")
        m, h, w = trainer.vae(px, B, size, size)
        n = B * h * w
        t = torch.randint(0, 1000, (B,), device=dev, dtype=torch.int32)
        z, noise = torch.randn(n, 4, device=dev), torch.randn(n, 4, device=dev)
        prep = lambda: ops.denoise_prepare(trainer.tab, t, noise, dtype, moments=m, z=z, scaling=trainer.vae.cfg.scaling_factor)
        prep()
        lines.append(f"  comat_denoise_prepare: {event_ms(prep, 20)}  ({n * 4} elements)")
        pred = torch.randn(n, 4, device=dev).to(dtype).requires_grad_(True)

        def mse():
            loss, _ = ops.mse_loss(pred, noise, B)
            loss.backward()
        mse()
        lines.append(f"  comat_mse_fwd + _bwd:  {event_ms(mse, 20)}  (3 launches, with torch's autograd around them)")
        del trainer, batch, m, pred
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
