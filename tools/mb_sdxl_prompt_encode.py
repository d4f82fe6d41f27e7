"""SDXL's prompt encoding from ids (clip.encode_prompt_sdxl) and the pooled-row kernel (comat_eos_pool) in numbers.

    python tools/mb_sdxl_prompt_encode.py [--reps 20] [--out FILE]          one MI355X

  * encode_prompt_sdxl at the real sizes: CLIP ViT-L (config.CLIP_L_TEXT) + OpenCLIP bigG (config.CLIP_BIGG_TEXT), seeded synthetic
    weights, L = 77, bf16, frozen towers under no_grad, B = 2 ([null; prompt] of a batch-1 step) and B = 8; and each tower alone -
    what a step with a text flag pays for the second tower's half every step;
  * comat_eos_pool at B = 8, L = 77, C = 1280 against the form it replaces: comat_layernorm_fwd over all 8 x 77 rows plus the index
    (argmax + gather).
HIP-event medians over `--reps` calls after a warm-up call (min, max in brackets)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    return f"{statistics.median(ms):8.3f} ms ({min(ms):.3f}, {max(ms):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from comat_amd import _hip, config, ops, weights
    from comat_amd.clip import ClipTextEncoder, encode_prompt_sdxl
    dev, dtype, L = torch.device("cuda:0"), torch.bfloat16, 77
    ops.set_kernel_backend(_hip.HipKernels())
    c1, c2 = config.CLIP_L_TEXT, config.CLIP_BIGG_TEXT
    enc1 = ClipTextEncoder(c1, weights.make_clip_text_weights(c1), dtype, dev)
    sd2 = weights.make_clip_text_weights(c2)
    n2 = sum(v.numel() for v in sd2.values())
    enc2 = ClipTextEncoder(c2, sd2, dtype, dev)
    del sd2
    lines = [f"one MI355X, library {_hip.build_id()}; frozen towers, bf16, L = {L}, no grad; second tower: {n2 / 1e6:.0f} M parameters"]
    g = torch.Generator().manual_seed(7)
    for B in (2, 8):
        ids = torch.randint(1000, c1.vocab_size - 2, (B, L), generator=g)
        ids[:, 0] = c1.vocab_size - 2
        ids_1, ids_2 = ids.clone(), ids.clone()
        ids_1[:, 12:] = c1.vocab_size - 1  # the first tokenizer pads with the end token
        ids_2[:, 12], ids_2[:, 13:] = c2.vocab_size - 1, 0  # the second with 0
        ids_1, ids_2 = ids_1.to(dev), ids_2.to(dev)

        def both():
            with torch.no_grad():
                encode_prompt_sdxl(enc1, enc2, ids_1, ids_2)

        def first():
            with torch.no_grad():
                enc1(ids_1, output="penultimate")

        def second():
            with torch.no_grad():
                enc2(ids_2, output="pooled")

        lines.append(f"B = {B}: encode_prompt_sdxl (CLIP-L + bigG)         {event_ms(both, args.reps)}")
        lines.append(f"B = {B}:   CLIP-L alone, hidden_states[-2]          {event_ms(first, args.reps)}")
        lines.append(f"B = {B}:   bigG alone, hidden_states[-2] + pooled   {event_ms(second, args.reps)}")
    B, C = 8, c2.hidden
    h = torch.randn(B * L, C, generator=g).to(dev, dtype)
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    out, y, stats = h.new_empty(B, C), torch.empty_like(h), torch.empty(B * L, 2, device=dev)
    k = ops.kernels()

    def pooled():
        _hip.eos_pool(ids_2, h, gamma, beta, out, None, B, L, C, c2.eos_token_id, c2.eps)

    def replaced():
        k.layernorm_fwd(h, gamma, beta, y, stats, B * L, C, c2.eps)
        return y.reshape(B, L, C)[torch.arange(B, device=dev), ids_2.argmax(-1)]

    pooled()
    assert torch.equal(out, replaced())  # the bit contract, at the real width
    lines.append(f"comat_eos_pool, B = {B}, L = {L}, C = {C}:                    {event_ms(pooled, args.reps)}")
    lines.append(f"comat_layernorm_fwd over {B * L} rows + argmax + gather:     {event_ms(replaced, args.reps)}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
