"""`--train_text_encoder_lora` (StepConfig.train_text_encoder_lora) in numbers.

    python tools/mb_text_encoder_step.py [--steps 6] [--out FILE]          one MI355X

bench.py's C2 world (SD1.5, 512 x 512, bf16, batch 1, K = total_step = 5), one process, the eager step:
  * flag off: the world as bench.py builds it (frozen prompt embeddings in the batch);
  * flag on: the same UNet, VAE, BLIP and discriminator; CLIP ViT-L/14's text tower (config.CLIP_L_TEXT, seeded synthetic weights)
    with rank-4 LoRA on its attention projections, input ids in the batch.  `--rank` sets the rank;
  * the tower alone: one encode of [null; prompt] (2 x 77 tokens) with and without its backward, HIP-event medians.
Step times are wall-clock medians over `--steps` steps after two warm-up steps, each step synchronised."""
import argparse
import dataclasses
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(step, batch, fixed, steps):
    step(batch, **fixed)  # warm-up: workspaces, memos, merged weights
    step(batch, **fixed)
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step(batch, **fixed)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return f"median {statistics.median(ms):8.2f} ms/step (min {min(ms):.2f}, max {max(ms):.2f})"


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rank", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from comat_amd import _hip, config, ops, weights
    from comat_amd.clip import ClipLoRABank, ClipTextEncoder
    from comat_amd.step import CoMatTrainer
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    ops.set_kernel_backend(_hip.HipKernels())
    lines = [f"one MI355X, library {_hip.build_id()}; C2-shaped eager step (SD1.5, 512 x 512, bf16, batch 1, K = total_step = 5)"]
    trainer, batch, fixed, scfg, _, _ = bench.build_world(dev, dtype, 0, "c2")
    lines.append(f"flag off:                      {timed(trainer.train_step, batch, fixed, args.steps)}")
    ccfg = config.CLIP_L_TEXT
    g = torch.Generator().manual_seed(7)
    fsd = ClipLoRABank.init(ccfg, args.rank, g)
    fsd = {k: (torch.randn(v.shape, generator=g) * 0.02 if k.endswith("up.weight") else v) for k, v in fsd.items()}
    tbank = ClipLoRABank(ccfg, fsd, dtype, dev)
    enc = ClipTextEncoder(ccfg, weights.make_clip_text_weights(ccfg), dtype, dev, tbank)
    bs, L = batch["prompt_embeds"].shape[:2]
    ids = torch.randint(1000, ccfg.vocab_size - 2, (bs, L), generator=g)
    ids[:, 0], ids[:, 12:] = ccfg.vocab_size - 2, ccfg.vocab_size - 1
    null = torch.full((bs, L), ccfg.vocab_size - 1)
    null[:, 0] = ccfg.vocab_size - 2
    on_batch = {k: v for k, v in batch.items() if k not in ("prompt_embeds", "negative_prompt_embeds")}
    on_batch.update(prompt_input_ids=ids.to(dev), null_input_ids=null.to(dev))
    on = CoMatTrainer(trainer.pipe, trainer.bank, trainer.blip, trainer.D, dataclasses.replace(scfg, train_text_encoder_lora=True),
                      seed=0, text_encoder=enc, text_bank=tbank)
    lines.append(f"flag on (rank {args.rank:3d}, {tbank.flat.numel() / 1e6:.2f} M factors): {timed(on.train_step, on_batch, fixed, args.steps)}")
    both = torch.cat([null, ids]).to(dev)

    def fwd():
        with torch.no_grad():
            enc(both)

    def fwd_bwd():
        tbank.zero_grad()
        out = enc(both)
        out.backward(torch.ones_like(out))

    med, lo, hi = event_ms(fwd, args.reps)
    lines.append(f"the tower alone, [null; prompt] = {both.shape[0]} x {L} tokens, no grad:      {med:6.3f} ms ({lo:.3f}, {hi:.3f})")
    med, lo, hi = event_ms(fwd_bwd, args.reps)
    lines.append(f"the tower alone, forward + backward into the factors:          {med:6.3f} ms ({lo:.3f}, {hi:.3f})")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
