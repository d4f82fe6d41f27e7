"""`--tune_text_encoder` (StepConfig.tune_text_encoder) in numbers.

    python tools/mb_tune_text_encoder_step.py [--steps 6] [--rounds 3] [--out FILE]          one MI355X

bench.py's C2 world (SD1.5, 512 x 512, bf16, batch 1, K = total_step = 5, guidance on), one process, the eager step, three trainers
over the same UNet, VAE, BLIP and discriminator, measured ALTERNATING (`--rounds` rounds of `--steps` steps each, medians over all):
  * neither flag: the world as bench.py builds it (frozen prompt embeddings in the batch);
  * train_text_encoder_lora: CLIP ViT-L/14's text tower (config.CLIP_L_TEXT, seeded synthetic weights), rank-4 LoRA, ids in the batch;
  * tune_text_encoder: the same tower over a clip.ClipTextBank (123 M fp32 parameters), ids in the batch.
Then the pieces the flag adds, HIP-event medians: the bank's AdamW segment alone (sumsq + update + tick), its gradient zeroing, the
refresh launch, and comat_embed_grad at n = 154 and 616, dim 768, vocab 49408 (the null-prompt pattern: every sequence of 77 is a
start token, a few ids, then the end token repeated) next to a plain copy of n x dim elements as its floor."""
import argparse
import dataclasses
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step_ms(step, batch, fixed, steps):
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step(batch, **fixed)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


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
    return f"{statistics.median(ms):8.4f} ms (min {min(ms):.4f}, max {max(ms):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from comat_amd import _hip, config, ops, weights
    from comat_amd.clip import ClipLoRABank, ClipTextBank, ClipTextEncoder
    from comat_amd.step import CoMatTrainer, FlatAdamW
    dev, dtype = torch.device("cuda:0"), torch.bfloat16
    ops.set_kernel_backend(_hip.HipKernels())
    lines = [f"one MI355X, library {_hip.build_id()}; C2-shaped eager step (SD1.5, 512 x 512, bf16, batch 1, K = total_step = 5, guidance on)"]
    trainer, batch, fixed, scfg, _, _ = bench.build_world(dev, dtype, 0, "c2")
    ccfg = config.CLIP_L_TEXT
    csd = weights.make_clip_text_weights(ccfg)
    g = torch.Generator().manual_seed(7)
    fsd = ClipLoRABank.init(ccfg, 4, g)
    fsd = {k: (torch.randn(v.shape, generator=g) * 0.02 if k.endswith("up.weight") else v) for k, v in fsd.items()}
    lbank = ClipLoRABank(ccfg, fsd, dtype, dev)
    lenc = ClipTextEncoder(ccfg, csd, dtype, dev, lbank)
    tbank = ClipTextBank(ccfg, csd, dtype, dev)
    tenc = ClipTextEncoder(ccfg, None, dtype, dev, tbank)
    bs, L = batch["prompt_embeds"].shape[:2]
    end = ccfg.vocab_size - 1
    ids = torch.randint(1000, ccfg.vocab_size - 2, (bs, L), generator=g)
    ids[:, 0], ids[:, 12:] = end - 1, end
    null = torch.full((bs, L), end)
    null[:, 0] = end - 1
    on_batch = {k: v for k, v in batch.items() if k not in ("prompt_embeds", "negative_prompt_embeds")}
    on_batch.update(prompt_input_ids=ids.to(dev), null_input_ids=null.to(dev))
    parts = (trainer.pipe, trainer.bank, trainer.blip, trainer.D)
    lora = CoMatTrainer(*parts, dataclasses.replace(scfg, train_text_encoder_lora=True), seed=0, text_encoder=lenc, text_bank=lbank)
    tune = CoMatTrainer(*parts, dataclasses.replace(scfg, tune_text_encoder=True), seed=0, text_encoder=tenc, text_bank=tbank)
    runs = (("neither flag", trainer.train_step, batch), ("train_text_encoder_lora (rank 4)", lora.train_step, on_batch),
            (f"tune_text_encoder ({tbank.flat.numel() / 1e6:.1f} M parameters)", tune.train_step, on_batch))
    for _, step, b in runs:  # warm-up: workspaces, memos, merged weights
        step(b, **fixed)
        step(b, **fixed)
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in runs}
    for _ in range(args.rounds):
        for name, step, b in runs:
            ms[name] += step_ms(step, b, fixed, args.steps)
    for name, v in ms.items():
        lines.append(f"{name:45s} median {statistics.median(v):8.2f} ms/step (min {min(v):.2f}, max {max(v):.2f}, {len(v)} steps)")

    opt = FlatAdamW([(tbank.flat, tbank.flat_grad)], 1e-6, (0.9, 0.999), 1e-8, 1e-2, 1.0)
    lines.append(f"AdamW over the text segment alone (sumsq, update, tick): {event_ms(opt.step, args.reps)}")
    lines.append(f"zeroing its gradient ({tbank.flat_grad.numel() * 4 / 1e6:.0f} MB):                   {event_ms(tbank.zero_grad, args.reps)}")

    def refresh():
        tbank.mark_updated()
        tbank.ensure_compute_copy()
    lines.append(f"the refresh launch (72 Linear weights):                  {event_ms(refresh, args.reps)}")
    both = torch.cat([null, ids]).to(dev)

    def fwd_bwd():
        out = tenc(both)
        out.backward(torch.ones_like(out))
    lines.append(f"the tower alone, [null; prompt] forward + backward:      {event_ms(fwd_bwd, args.reps)}")
    k, dim, vocab = ops.table_kernels(), ccfg.hidden, ccfg.vocab_size
    table = tbank.params["embeddings.token_embedding.weight"].grad
    for n in (154, 616):
        seq = torch.cat([null, ids] * (n // (2 * L)))[: n // L].reshape(-1).to(dev)
        dy = torch.randn(n, dim, generator=g).to(device=dev, dtype=dtype)
        out = torch.empty_like(dy)
        lines.append(f"comat_embed_grad n = {n:3d}, dim {dim}, bf16 dy:            {event_ms(lambda: k.embed_grad(seq, dy, table, n, dim, vocab), args.reps)}")
        lines.append(f"  a plain copy of {n} x {dim} bf16 elements:              {event_ms(lambda: ops.kernels().unary(ops.UN_COPY, dy, out, n * dim), args.reps)}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
