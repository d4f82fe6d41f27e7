"""Fingerprints of the trained banks after three seeded eager steps of the tiny step world, once per training flag.

    python tools/dump_bank_step.py [--flags none tune_vae full_finetuning tune_text_encoder] [--out FILE]      one MI355X
    python tools/dump_bank_step.py --sim                                                    the CPU simulator of the tests

Per flag a fresh world (tiny UNet / VAE / BLIP / discriminator, bf16, batch 2, K = 2 of 3 sampler steps, GAN loss on; with
tune_text_encoder the tiny CLIP tower and ids in the batch), three `train_step` calls on the same batch, then per trained bank
sha256 of `flat` and `flat_grad` and - where the bank has weight holders - of every holder's `w` and `wt` / `wd` in `holders`
order, after ensure_compute_copy(); and the logged scalars of the last step as exact hex floats.  Two commits compute the same
values if and only if their outputs are equal line for line.  Only the trainer's public surface is used (`bank`, `vae_bank`,
`text_bank`, `holders`), so the tool runs unchanged on older commits."""
import argparse
import dataclasses
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLAGS = ("none", "tune_vae", "full_finetuning", "tune_text_encoder")
FIXED = dict(training_steps=[1, 2], crop=(1, 0, 63, 63))


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def make_world(flag, dtype, dev):
    from comat_amd import config, weights
    from comat_amd.blip import Blip
    from comat_amd.clip import ClipTextBank, ClipTextEncoder
    from comat_amd.gan import D_sd
    from comat_amd.pipeline import TrainableSDPipeline
    from comat_amd.step import CoMatTrainer, StepConfig
    from comat_amd.unet import LoRABank, UNet, UNetBank, VAEBank, VAEDecoder
    ccfg, vcfg, bcfg = config.TINY_CLIP_TEXT, config.TINY_VAE, config.TINY_BLIP
    ucfg = dataclasses.replace(config.TINY_UNET, cross_attention_dim=ccfg.hidden)
    q = lambda d: {k: v.to(dtype).float() for k, v in d.items()}
    up5 = lambda d: {k: (v * 5 if k.endswith("up.weight") else v) for k, v in d.items()}
    usd, vsd = q(weights.make_unet_weights(ucfg, perturb_norms=True)), q(weights.make_vae_weights(vcfg, perturb_norms=True))
    lsd, bsd = q(up5(weights.make_lora_weights(ucfg))), q(weights.make_blip_weights(bcfg, perturb_norms=True))
    dsd, dl = q(weights.make_unet_weights(ucfg, seed=77, perturb_norms=True)), q(up5(weights.make_lora_weights(ucfg, seed=78)))
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g)
    head_w, head_b = r(4) * 0.5, r(1) * 0.1
    text, full, tune_vae = flag == "tune_text_encoder", flag == "full_finetuning", flag == "tune_vae"
    cfg = StepConfig(resolution=64, total_step=3, K=2, gan_loss=True, attrcon=False, lr=1e-2, lr_D=1e-2, tune_text_encoder=text,
                     tune_vae=tune_vae, full_finetuning=full)
    bs, L, end = 2, 9, ccfg.vocab_size - 1
    bids = torch.randint(1, bcfg.vocab_size, (bs, 9), generator=g)
    batch = dict(gan_null_embeds=r(bs, L, ccfg.hidden), latents=r(bs, 4, 8, 8), noises=[r(bs, 4, 8, 8) for _ in range(3)],
                 real_latents=r(bs, 4, 8, 8), blip_input_ids=bids, blip_attention_mask=torch.ones_like(bids))
    if text:
        ids = torch.randint(3, end - 1, (bs, L), generator=g)
        ids[:, L - 2:] = ids[:, :1]  # a repeated id inside every prompt: rows of the token table collide
        null = torch.full((bs, L), end)
        null[:, 0] = 1
        batch.update(prompt_input_ids=ids, null_input_ids=null)
    else:
        batch.update(prompt_embeds=r(bs, L, ccfg.hidden), negative_prompt_embeds=r(bs, L, ccfg.hidden))
    bank = UNetBank(ucfg, usd, dtype, dev) if full else LoRABank(ucfg, lsd, dtype, dev)
    unet = UNet(ucfg, usd, dtype, dev, bank=bank) if full else UNet(ucfg, usd, dtype, dev, bank)
    vae = VAEDecoder(vcfg, vsd, dtype, dev, bank=VAEBank(vcfg, vsd, dtype, dev) if tune_vae else None)
    dbank = LoRABank(ucfg, dl, dtype, dev)
    disc = D_sd(UNet(ucfg, dsd, dtype, dev, dbank), dbank, head_w, head_b)
    kw = {}
    if text:
        tbank = ClipTextBank(ccfg, q(weights.make_clip_text_weights(ccfg, perturb_norms=True)), dtype, dev)
        kw = dict(text_encoder=ClipTextEncoder(ccfg, None, dtype, dev, tbank), text_bank=tbank)
    return CoMatTrainer(TrainableSDPipeline(unet, vae), bank, Blip(bcfg, bsd, dtype, dev), disc, cfg, seed=0, **kw), batch


def dump(flag, dtype, dev):
    trainer, batch = make_world(flag, dtype, dev)
    for _ in range(3):
        logs = trainer.train_step(batch, **FIXED)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    lines = []
    for role, bank in (("generator", trainer.bank), ("vae", trainer.vae_bank), ("text", trainer.text_bank)):
        if bank is None:
            continue
        name = f"{flag} {role} {type(bank).__name__}"
        lines.append(f"{name} flat[{bank.flat.numel()}] {sha(bank.flat)}")
        lines.append(f"{name} flat_grad {sha(bank.flat_grad)}")
        hs = [h for h in getattr(bank, "holders", []) if hasattr(h, "w")]
        if hs:
            bank.ensure_compute_copy()
            lines.append(f"{name} {len(hs)} holders w, wt / wd {sha(*(t for h in hs for t in (h.w, h.wt if hasattr(h, 'wt') else h.wd)))}")
    for k in sorted(logs):
        if torch.is_tensor(logs[k]) and logs[k].numel() == 1:
            lines.append(f"{flag} log {k} {float(logs[k]).hex()}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flags", nargs="+", default=list(FLAGS), choices=FLAGS)
    ap.add_argument("--sim", action="store_true", help="the CPU simulator of tests/ instead of the HIP kernels")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from comat_amd import ops
    if args.sim:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from clip_tune_sim import ClipTuneSimKernels
        ops.set_kernel_backend(ClipTuneSimKernels())
        dev = torch.device("cpu")
    else:
        from comat_amd import _hip
        ops.set_kernel_backend(_hip.HipKernels())
        dev = torch.device("cuda:0")
    lines = []
    for flag in args.flags:
        lines += dump(flag, torch.bfloat16, dev)
        ops.drop_side_stream_state()
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
