"""comat_amd.denoise (DenoiseConfig, DenoiseTrainer, encode_images) against a plain-torch restatement of the loop body of diffusers'
train_text_to_image_sdxl.py: AutoencoderKL.encode (tests/test_vae_encoder.py::encode_ref) -> latent_dist.sample() * scaling_factor ->
add_noise at a timestep per sample -> the oracle's UNet (oracle/sd.py, called sample by sample: it takes one timestep) ->
F.mse_loss on fp32 -> clip_grad_norm_ + torch.optim.AdamW.  Timesteps, noise and posterior noise are given and differ per sample.

Bounds: the loss to helpers.check (the step tests' tolerance); every trained parameter's gradient within 1e-3 relative L2 in fp32 (the
project's parity bound) for a UNetBank and a LoRABank; bf16 to the bounds tests/test_models.py holds LoRA
gradients to (0.25, the worst parameter).  The restricted AdamW update (|clipped gradient| >= 10 eps, as tests/test_full_finetuning.py)
within 1e-3."""
import dataclasses
import functools
import sys

import pytest
import torch
import torch.nn.functional as F

from comat_amd import checkpoint, config, ops, weights
from comat_amd.denoise import DenoiseConfig, DenoiseTrainer, denoise_tables, encode_images, snr_weights
from comat_amd.pipeline import DDPMScheduler
from comat_amd.unet import LoRABank, UNet, UNetBank, VAEEncoder, timestep_embedding
from denoise_sim import denoise_dev  # noqa: F401 - fixture
from helpers import check, rel_l2
from oracle import sd as O
from test_vae_encoder import encode_ref

F32, BF16 = torch.float32, torch.bfloat16
CFGS = {"sd": config.TINY_UNET, "sdxl": config.TINY_SDXL_UNET}
VCFG = config.TINY_VAE
B, L = 2, 7
TSTEPS = (37, 912)  # one timestep per sample
# 64 x 64 images -> 8 x 8 latents, the size the UNet parity tests use.  Smaller does not test this step: 16 x 16 -> 2 x 2 latents cannot
# pass the tiny UNet's two downsamplers (2 -> 1 -> 1 does not come back up to 2: the skip concat fails in the oracle and the product
# alike), and at 32 x 32 -> 4 x 4 the mid block sees ONE token, whose self-attention has an exactly zero to_q / to_k gradient.
IMG = 64
TIME_IDS = (IMG, IMG, 0, 0, IMG, IMG)


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def world(kind, dtype, source):
    """weights (rounded to dtype) and one batch; shared and never written"""
    cfg = CFGS[kind]
    q = lambda d: {k: v.to(dtype).float() for k, v in d.items()}
    usd = q(weights.make_unet_weights(cfg, perturb_norms=True))
    lsd = {k: (v * 5 if k.endswith("up.weight") else v) for k, v in weights.make_lora_weights(cfg).items()}
    esd = q(weights.make_vae_encoder_weights(VCFG, perturb_norms=True))
    hw = IMG // 8 if source == "pixels" else 8
    batch = dict(prompt_embeds=rnd(B, L, cfg.cross_attention_dim, seed=2).to(dtype).float(), timesteps=torch.tensor(TSTEPS),
                 noise=rnd(B, 4, hw, hw, seed=3))
    if source == "pixels":
        batch["pixel_values"] = rnd(B, 3, IMG, IMG, seed=4).clamp(-1, 1).to(dtype).float()
        batch["posterior_noise"] = rnd(B, 4, hw, hw, seed=5)
    else:
        batch["latents"] = rnd(B, 4, hw, hw, seed=6)
    if cfg.addition_embed:
        batch["pooled_prompt_embeds"] = rnd(B, cfg.pooled_dim, seed=7).to(dtype).float()
        batch["add_time_ids"] = TIME_IDS
    return usd, q(lsd), esd, batch


def oracle_loss(kind, usd, lora, esd, batch, snr_gamma=None):
    """the loop body in plain torch -> (loss, per-sample losses)"""
    cfg, sch = CFGS[kind], DDPMScheduler()
    ocfg = O.UNetConfig(**dataclasses.asdict(cfg))
    if "pixel_values" in batch:
        mean, logvar = encode_ref(esd, VCFG, batch["pixel_values"]).chunk(2, dim=1)
        x0 = VCFG.scaling_factor * (mean + torch.exp(0.5 * logvar.clamp(-30, 20)) * batch["posterior_noise"])
    else:
        x0 = batch["latents"]
    per = []
    for b in range(B):
        t = int(batch["timesteps"][b])
        sa, sb = sch.add_noise_coefficients(t)
        noisy = sa * x0[b:b + 1] + sb * batch["noise"][b:b + 1]
        added = None
        if cfg.addition_embed:
            added = (batch["pooled_prompt_embeds"][b:b + 1], torch.tensor([list(batch["add_time_ids"])], dtype=torch.float32))
        eps = O.unet_forward(usd, ocfg, noisy, t, batch["prompt_embeds"][b:b + 1], lora, None, added)
        per.append(F.mse_loss(eps.float(), batch["noise"][b:b + 1].float()))
    per = torch.stack(per)
    w = torch.from_numpy(snr_weights(sch, snr_gamma))[list(TSTEPS)].float()
    return (per * w).mean(), per


@functools.lru_cache(maxsize=None)
def oracle_step(kind, full, dtype, source, lr=1e-3, max_norm=0.05):
    """gradients of the trained leaves, then clip + one AdamW step; shared and never written"""
    usd, lsd, esd, batch = world(kind, dtype, source)
    leaves = {k: v.clone().requires_grad_(True) for k, v in (usd if full else lsd).items()}
    loss, per = oracle_loss(kind, leaves if full else usd, None if full else leaves, esd, batch)
    loss.backward()
    params = list(leaves.values())
    res = dict(loss=loss.detach(), per=per.detach(), g={k: v.grad.clone() for k, v in leaves.items()})
    before = {k: v.detach().clone() for k, v in leaves.items()}
    opt = torch.optim.AdamW(params, lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    res["gnorm"] = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    res["clipped"] = {k: v.grad.clone() for k, v in leaves.items()}
    opt.step()
    res["update"] = {k: v.detach() - before[k] for k, v in leaves.items()}
    return res


def make_trainer(kind, full, dtype, source, dev, **cfg_kw):
    usd, lsd, esd, batch = world(kind, dtype, source)
    cfg = CFGS[kind]
    if full:
        bank = UNetBank(cfg, usd, dtype, dev)
        unet = UNet(cfg, usd, dtype, dev, bank=bank)
    else:
        bank = LoRABank(cfg, lsd, dtype, dev)
        unet = UNet(cfg, usd, dtype, dev, bank)
    enc = VAEEncoder(VCFG, esd, dtype, dev) if source == "pixels" else None
    kw = dict(lr=1e-3, max_grad_norm=0.05)
    kw.update(cfg_kw)
    return DenoiseTrainer(unet, bank, enc, DenoiseConfig(**kw), seed=0), batch


def grads_by_name(bank, full):
    """{diffusers name: (got, layout the oracle's tensor must be brought to)}"""
    if full:
        return {n: bank._view(bank.flat_grad, n).detach().cpu() for n in bank.names}
    return {n: p.grad.detach().cpu() for n, p in bank.params.items()}


def oracle_in_bank_layout(bank, full, tensors):
    return {n: (bank._stored(n, tensors[n].detach()) if full else tensors[n].detach()) for n in bank.names}


def worst_grad(bank, full, ref_g):
    got, want = grads_by_name(bank, full), oracle_in_bank_layout(bank, full, ref_g)
    errs = {n: rel_l2(got[n].reshape(-1), want[n].reshape(-1)) for n in got}
    n = max(errs, key=errs.get)
    return errs[n], n


def flat_of(bank, full, tensors):
    want = oracle_in_bank_layout(bank, full, tensors)
    return torch.cat([want[n].reshape(-1) for n in bank.names])


def bank_vec(bank, full, buf):
    if full:
        return torch.cat([bank._view(buf, n).detach().reshape(-1).cpu() for n in bank.names])
    return buf.detach().cpu()[:sum(p.numel() for p in bank.params.values())].clone()


CASES = [("sd", True, "pixels"), ("sd", False, "pixels"), ("sdxl", True, "pixels"), ("sdxl", False, "latents"), ("sd", True, "latents")]
case_id = lambda c: f"{c[0]}-{'full' if c[1] else 'lora'}-{c[2]}"


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_step_matches_the_restatement_fp32(denoise_dev, case):
    kind, full, source = case
    trainer, batch = make_trainer(kind, full, F32, source, denoise_dev)
    ref = oracle_step(kind, full, F32, source)
    assert ref["gnorm"] > 2 * 0.05, "the clip is meant to be active"
    bank = trainer.bank
    p0 = bank_vec(bank, full, bank.flat)
    logs = trainer.train_step(batch)
    check(logs["loss"], ref["loss"].reshape(1), F32, "loss")
    check(logs["per_sample_loss"], ref["per"], F32, "per-sample loss")
    worst, name = worst_grad(bank, full, ref["g"])
    print(f"{case_id(case)} fp32 {denoise_dev.type}: loss {float(logs['loss']):.6f} (restatement {float(ref['loss']):.6f}), worst "
          f"gradient rel-L2 {worst:.3e} ({name}) over {len(bank.names)} parameters")
    assert worst < 1e-3, f"gradient of {name}: rel-L2 {worst:.3e}"
    check(logs["grad_norm"], torch.tensor([ref["gnorm"]]), F32, "gradient norm")
    assert abs(float(logs["lr"]) - 1e-3) < 1e-9 and logs["timesteps"].tolist() == list(TSTEPS) and int(trainer.oob) == 0
    upd, want = bank_vec(bank, full, bank.flat) - p0, flat_of(bank, full, ref["update"])
    keep = flat_of(bank, full, ref["clipped"]).abs() >= 10 * 1e-8
    assert float(keep.float().mean()) >= 0.95, "more than 5 % of the elements excluded"
    assert rel_l2(upd[keep], want[keep]) < 1e-3, f"AdamW update rel-L2 {rel_l2(upd[keep], want[keep]):.3e}"
    assert trainer.opt.counters.tolist() == [1, 0]


@pytest.mark.parametrize("case", [("sd", False, "pixels"), ("sdxl", True, "pixels")], ids=case_id)
def test_step_bf16(denoise_dev, case):
    kind, full, source = case
    trainer, batch = make_trainer(kind, full, BF16, source, denoise_dev)
    ref = oracle_step(kind, full, BF16, source)
    logs = trainer.train_step(batch)
    check(logs["loss"], ref["loss"].reshape(1), BF16, "loss")
    bank = trainer.bank
    if full:  # one vector: single small parameters of a fully trained tiny UNet are rounding noise in bf16
        worst, name = rel_l2(bank_vec(bank, True, bank.flat_grad), flat_of(bank, True, ref["g"])), "all"
    else:
        worst, name = worst_grad(bank, full, ref["g"])
    print(f"{case_id(case)} bf16 {denoise_dev.type}: worst gradient rel-L2 {worst:.3e} ({name})")
    assert worst < 0.25, f"gradient of {name}: rel-L2 {worst:.3e}"


def test_tables_are_the_schedulers_and_the_unets_values():
    sch = DDPMScheduler()
    tab = denoise_tables(sch, 32, "cpu", snr_gamma=5.0)
    assert tab.T == 1000 and tab.C0 == 32
    for t in (0, 1, 37, 500, 999):
        assert torch.equal(tab.sinus[t], timestep_embedding(t, 32, 1)[0])
        sa, sb = sch.add_noise_coefficients(t)
        assert tab.sab[t].tolist() == [float(torch.tensor(sa, dtype=F32)), float(torch.tensor(sb, dtype=F32))]
        a = float(sch.alphas_cumprod[t].double())
        snr = a / (1.0 - a)
        assert float(tab.wtab[t]) == float(torch.tensor(min(snr, 5.0) / snr, dtype=F32))
    assert bool((denoise_tables(sch, 32, "cpu").wtab == 1).all()) and float(tab.wtab[0]) < 0.01 and float(tab.wtab[999]) == 1.0


def test_snr_gamma_weights_the_samples(denoise_dev):
    trainer, batch = make_trainer("sd", False, F32, "latents", denoise_dev, snr_gamma=5.0)
    usd, lsd, esd, _ = world("sd", F32, "latents")
    with torch.no_grad():
        want, per = oracle_loss("sd", usd, lsd, esd, batch, snr_gamma=5.0)
    w = torch.from_numpy(snr_weights(DDPMScheduler(), 5.0))[list(TSTEPS)]
    assert float(w[0]) < 0.5 and float(w[1]) == 1.0, "the two timesteps are meant to straddle gamma"
    logs = trainer.train_step(batch)
    check(logs["per_sample_loss"], per, F32, "per-sample loss (unweighted)")
    check(logs["loss"], want.reshape(1), F32, "weighted loss")
    assert abs(float(logs["loss"]) - float(per.mean())) > 1e-2 * float(per.mean()), "the weights changed nothing"


@pytest.mark.parametrize("full", [True, False], ids=["full", "lora"])
def test_a_nan_weight_skips_the_update(denoise_dev, full):
    trainer, batch = make_trainer("sd", full, F32, "latents", denoise_dev)
    bank = trainer.bank
    with torch.no_grad():
        bank.flat[5] = float("nan")
    bank.mark_updated()
    before = bank.flat.clone()
    logs = trainer.train_step(batch)
    assert not bool(torch.isfinite(logs["loss"]).all()) and not bool(torch.isfinite(logs["grad_norm"]).all())
    assert trainer.opt.counters.tolist() == [0, 1], "the update was not skipped"
    assert all(float(m.abs().max()) == 0.0 for m in trainer.opt.m + trainer.opt.v), "a skipped update moved the moments"
    assert torch.equal(torch.nan_to_num(bank.flat, nan=7.0), torch.nan_to_num(before, nan=7.0))


def test_checkpoint_round_trip(denoise_dev, tmp_path):
    """unet.pt + optim_state.pt: a trainer built from other weights continues exactly where the saved one stopped"""
    a, batch = make_trainer("sd", True, F32, "latents", denoise_dev, lr_scheduler="cosine", max_train_steps=10, lr_warmup_steps=1)
    a.train_step(batch)
    checkpoint.save_checkpoint(str(tmp_path), a.bank, optim=dict(G=a.opt))
    sd = torch.load(str(tmp_path / "unet.pt"))
    assert set(sd) == set(world("sd", F32, "latents")[0]) and sd["conv_in.weight"].shape == (32, 4, 3, 3)
    other = {k: v + 0.01 for k, v in world("sd", F32, "latents")[0].items()}
    bank = UNetBank(CFGS["sd"], other, F32, denoise_dev)
    b = DenoiseTrainer(UNet(CFGS["sd"], other, F32, denoise_dev, bank=bank), bank, None,
                       DenoiseConfig(lr=1e-3, max_grad_norm=0.05, lr_scheduler="cosine", max_train_steps=10, lr_warmup_steps=1), seed=0)
    checkpoint.load_checkpoint(str(tmp_path), b.bank, optim=dict(G=b.opt))
    assert torch.equal(a.bank.flat, b.bank.flat) and torch.equal(a.opt.counters, b.opt.counters)
    assert all(torch.equal(x, y) for x, y in zip(a.opt.m + a.opt.v, b.opt.m + b.opt.v)) and torch.equal(a.opt.lr_now, b.opt.lr_now)
    la, lb = a.train_step(batch), b.train_step(batch)
    assert torch.equal(la["loss"], lb["loss"]) and torch.equal(a.bank.flat, b.bank.flat) and float(la["lr"]) < 1e-3


def test_refused_configurations_name_their_field(sim):
    for kw, field in ((dict(prediction_type="v_prediction"), "prediction_type"), (dict(use_8bit_adam=True), "use_8bit_adam"),
                      (dict(gradient_checkpointing=True), "gradient_checkpointing"), (dict(fp8_forward=True), "fp8_forward"),
                      (dict(snr_gamma=0.0), "snr_gamma"), (dict(lr_scheduler="linear"), "max_train_steps"),
                      (dict(lr_scheduler="piecewise_constant"), "lr_scheduler")):
        with pytest.raises(ValueError, match=field):
            make_trainer("sd", False, F32, "latents", sim, **kw)
    usd, lsd, _, batch = world("sd", F32, "latents")
    bank = LoRABank(CFGS["sd"], lsd, F32, sim)
    with pytest.raises(ValueError, match="not built over this bank"):
        DenoiseTrainer(UNet(CFGS["sd"], usd, F32, sim, LoRABank(CFGS["sd"], lsd, F32, sim)), bank, None, DenoiseConfig())
    trainer, _ = make_trainer("sd", False, F32, "latents", sim)
    with pytest.raises(ValueError, match="vae_encoder"):
        trainer.train_step(dict(world("sd", F32, "pixels")[3]))


def test_encode_images(denoise_dev):
    _, _, esd, batch = world("sd", F32, "pixels")
    enc = VAEEncoder(VCFG, esd, F32, denoise_dev)
    mean, logvar = encode_ref(esd, VCFG, batch["pixel_values"]).chunk(2, dim=1)
    got = encode_images(enc, batch["pixel_values"])
    assert got.shape == (B, 4, IMG // 8, IMG // 8) and got.dtype == F32
    check(got, VCFG.scaling_factor * mean, F32, "mode of the posterior, scaled")
    z = batch["posterior_noise"]
    check(encode_images(enc, batch["pixel_values"], sample=True, noise=z),
          VCFG.scaling_factor * (mean + torch.exp(0.5 * logvar.clamp(-30, 20)) * z), F32, "a sample of the posterior, scaled")
    assert encode_images(enc, batch["pixel_values"], sample=True).shape == (B, 4, IMG // 8, IMG // 8)


def test_a_step_with_drawn_timesteps_reads_nothing_on_the_host(denoise_dev, monkeypatch):
    """timesteps, noise and posterior noise are drawn on the device, and no line of the package turns a tensor into a host value
    while the step runs (the simulator's own kernels, which stand for device work, may)"""
    import os
    trainer, batch = make_trainer("sd", True, F32, "pixels", denoise_dev, lr_scheduler="constant_with_warmup", lr_warmup_steps=2)
    drawn = {k: v for k, v in batch.items() if k not in ("timesteps", "noise", "posterior_noise")}
    trainer.train_step(drawn)  # everything that is built once exists
    pkg = os.path.dirname(os.path.abspath(ops.__file__))
    reads = []

    def guard(name):
        orig = getattr(torch.Tensor, name)

        def wrapped(self, *a, **kw):
            f = sys._getframe(1)
            if os.path.dirname(os.path.abspath(f.f_code.co_filename)) == pkg and f.f_code.co_filename != _hip_file:
                reads.append(f"{name} at {os.path.basename(f.f_code.co_filename)}:{f.f_lineno}")
            return orig(self, *a, **kw)
        return wrapped

    from comat_amd import _hip
    _hip_file = os.path.abspath(_hip.__file__)
    for name in ("item", "cpu", "tolist", "numpy", "__float__", "__int__", "__bool__", "__index__"):
        monkeypatch.setattr(torch.Tensor, name, guard(name))
    logs = trainer.train_step(drawn)
    monkeypatch.undo()
    assert not reads, reads
    assert logs["timesteps"].device.type == denoise_dev.type and logs["timesteps"].dtype == torch.int32
    assert all(torch.is_tensor(logs[k]) for k in ("loss", "per_sample_loss", "lr", "grad_norm"))
    assert bool(torch.isfinite(logs["loss"]).all()) and 0 <= int(logs["timesteps"].min()) and int(logs["timesteps"].max()) < 1000
    again = trainer.train_step(drawn)
    assert not torch.equal(again["timesteps"], logs["timesteps"]) or not torch.equal(again["loss"], logs["loss"])
