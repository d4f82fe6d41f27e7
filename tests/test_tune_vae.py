"""`--tune_vae` (StepConfig.tune_vae): the VAE decoder's parameters are trained next to the generator's LoRA factors
(training_utils/pipeline.py:68,170-171; training_script.py:187-188,402-403).

The world is tests/test_step.make_world's, rebuilt here with VAEDecoder(..., bank=VAEBank(...)) and StepConfig(tune_vae=True).
The oracle side is composed here: oracle.step.g_loss_terms with the VAE tensors as leaves, ONE torch.optim.AdamW over LoRA + VAE
leaves after a JOINT clip_grad_norm_ (oracle.step.train_step clips the LoRA leaves only, so it is not used)."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from comat_amd import checkpoint, config, ops, weights
from comat_amd.blip import Blip
from comat_amd.gan import D_sd
from comat_amd.pipeline import TrainableSDPipeline
from comat_amd.segments import SegmentedStep
from comat_amd.step import CoMatTrainer, GraphedStep, StepConfig
from comat_amd.unet import LoRABank, UNet, VAEBank, VAEDecoder
from helpers import check, oracle_cfgs, rel_l2, tiny_weights
from oracle import blip as OB
from oracle import step as OS

F32, BF16 = torch.float32, torch.bfloat16
TS, CROP = [1, 2], (1, 0, 63, 63)
# bf16 storage against the fp32 oracle on the same (bf16-representable) weights, VAE gradient rel-L2: 2 x the distance the ABI
# simulator shows in bf16 storage on these inputs, measured on the CPU (profiles/tune_vae_bf16_errors.txt: 3.589e-2) - the margin
# tests/test_step.py:23-31 uses for the same comparison of the LoRA gradient
BF16_VAE_GRAD_SIM = 3.589e-2
BF16_VAE_GRAD_LIMIT = 2 * BF16_VAE_GRAD_SIM


def make_inputs(dtype, tune=True, gan=True, bs=2, **cfg_kw):
    """the inputs of tests/test_step.make_world (attrcon off): configuration, batch, the oracle's world, the state dicts"""
    tcfg = config.TINY_UNET
    usd, vsd, lsd = tiny_weights(dtype, tcfg)
    q = lambda d: {k: v.to(dtype).float() for k, v in d.items()}
    bsd = q(weights.make_blip_weights(config.TINY_BLIP, perturb_norms=True))
    dsd = q(weights.make_unet_weights(tcfg, seed=77, perturb_norms=True))
    dl = q({k: (v * 5 if k.endswith("up.weight") else v) for k, v in weights.make_lora_weights(tcfg, seed=78).items()})
    g = torch.Generator().manual_seed(5)
    head_w, head_b = torch.randn(4, generator=g) * 0.5, torch.randn(1, generator=g) * 0.1
    cfg = StepConfig(resolution=64, total_step=3, K=2, gan_loss=gan, attrcon=False, attrcon_train_steps=1,
                     train_layer_ls=("mid_2", "up_4", "up_8"), attn_reses=(8, 4, 2), lr=1e-2, lr_D=1e-2,
                     mask_token_loss_weight=0.5, mask_pixel_loss_weight=0.1, tune_vae=tune, **cfg_kw)
    L, cd, T = 7, config.TINY_UNET.cross_attention_dim, 9
    r = lambda *s: torch.randn(*s, generator=g)
    ids = torch.randint(1, config.TINY_BLIP.vocab_size, (bs, T), generator=g)
    ids[1, 7:] = 0
    masks = []
    for b in range(bs):
        m = np.zeros((2, 64, 64), dtype=bool)
        m[0, 5:30, 8:40] = True
        m[1, 34:60, 20:64] = True
        masks.append(m)
    batch = dict(prompt_embeds=r(bs, L, cd).to(dtype).float(), negative_prompt_embeds=r(bs, L, cd).to(dtype).float(),
                 gan_null_embeds=r(bs, L, cd).to(dtype).float(), latents=r(bs, 4, 8, 8),
                 noises=[r(bs, 4, 8, 8) for _ in range(3)], real_latents=r(bs, 4, 8, 8),
                 blip_input_ids=ids, blip_attention_mask=(ids != 0).long(), masks=masks,
                 attributes=[[[2, 3], [5]], [[1], [4, 6]]] * (bs // 2))
    ucfg, vcfg = oracle_cfgs(tcfg)
    W = dict(unet=usd, vae={k: v.clone() for k, v in vsd.items()}, blip=bsd, d_unet=dsd, ucfg=ucfg, vcfg=vcfg,
             bcfg=OB.BlipConfig(**dataclasses.asdict(config.TINY_BLIP)),
             lora={k: v.clone().requires_grad_(True) for k, v in lsd.items()},
             d_lora={k: v.clone().requires_grad_(True) for k, v in dl.items()},
             head_w=head_w.clone().requires_grad_(True), head_b=head_b.clone().requires_grad_(True))
    return cfg, batch, W, (tcfg, usd, vsd, lsd, bsd, dsd, dl, head_w, head_b)


def make_world(dtype, dev, tune=True, gan=True, bs=2, **cfg_kw):
    """tests/test_step.make_world with the trainable decoder; tune=False builds today's world through the new signatures' defaults"""
    cfg, batch, W, (tcfg, usd, vsd, lsd, bsd, dsd, dl, head_w, head_b) = make_inputs(dtype, tune, gan, bs, **cfg_kw)
    bank = LoRABank(tcfg, lsd, dtype, dev)
    vbank = VAEBank(config.TINY_VAE, vsd, dtype, dev) if tune else None
    vae = VAEDecoder(config.TINY_VAE, vsd, dtype, dev, bank=vbank) if tune else VAEDecoder(config.TINY_VAE, vsd, dtype, dev)
    pipe = TrainableSDPipeline(UNet(tcfg, usd, dtype, dev, bank), vae)
    dbank = LoRABank(tcfg, dl, dtype, dev)
    disc = D_sd(UNet(tcfg, dsd, dtype, dev, dbank), dbank, head_w, head_b)
    trainer = CoMatTrainer(pipe, bank, Blip(config.TINY_BLIP, bsd, dtype, dev), disc, cfg, seed=0)
    return cfg, batch, W, trainer


def stored(t):
    """a diffusers tensor in the bank's layout (conv weights [Cout, KH, KW, Cin])"""
    return t.permute(0, 2, 3, 1) if t.dim() == 4 else t


def vae_vec(vbank, buf):
    """the parameters' elements of one of the bank's flat buffers (or of an optimizer moment), without the alignment pads"""
    return torch.cat([vbank._view(buf, n).detach().reshape(-1).cpu() for n in vbank.names])


def oracle_vec(tensors, names):
    return torch.cat([stored(tensors[n]).reshape(-1) for n in names])


_ORACLE = {}


def oracle_step(dtype, names):
    """the oracle's step on the world's inputs, computed once per dtype of the weights and shared (never written)"""
    if dtype not in _ORACLE:
        cfg, batch, W, _ = make_inputs(dtype)
        for n in names:
            W["vae"][n].requires_grad_(True)
        leaves = list(W["lora"].values()) + [W["vae"][n] for n in names]
        opt = torch.optim.AdamW(leaves, lr=cfg.lr, betas=(cfg.adam_beta1, cfg.adam_beta2), eps=cfg.adam_epsilon,
                                weight_decay=cfg.adam_weight_decay)
        out = OS.g_loss_terms(W, batch, cfg, TS, CROP)
        out["loss"].backward()
        for p in leaves:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        res = dict(out={k: v.detach() for k, v in out.items() if k in ("Blip", "G_loss", "loss")},
                   g_lora={k: v.grad.clone() for k, v in W["lora"].items()},
                   g_vae={n: W["vae"][n].grad.clone() for n in names})
        torch.nn.utils.clip_grad_norm_(leaves, cfg.max_grad_norm)
        res["clipped_vae"] = {n: W["vae"][n].grad.clone() for n in names}
        opt.step()
        res["p_vae"] = {n: W["vae"][n].detach().clone() for n in names}
        res["p_lora"] = {k: v.detach().clone() for k, v in W["lora"].items()}
        res["m_vae"] = {n: opt.state[W["vae"][n]]["exp_avg"].clone() for n in names}
        res["v_vae"] = {n: opt.state[W["vae"][n]]["exp_avg_sq"].clone() for n in names}
        _ORACLE[dtype] = res
    return _ORACLE[dtype]


# ---- the step against the oracle -------------------------------------------------------------------------------------------
def test_tune_vae_step_matches_oracle(dev):
    """fp32 parity mode.  Measured on the simulator (CPU): VAE gradient rel-L2 and [LoRA; VAE] rel-L2 ~1e-6; the parameter
    comparison excludes 10.6 % of the elements (structurally zero gradients: to_k.bias, the biases in front of one-channel
    groups), see the issue's measurement - two oracle runs that differ only in conv algorithm agree to 4e-6 in the gradient
    but only to 8.6e-5 in the unrestricted parameters."""
    dtype = F32
    cfg, batch, W, trainer = make_world(dtype, dev)
    vb = trainer.vae_bank
    ref = oracle_step(dtype, tuple(vb.names))
    logs = trainer.train_step(batch, training_steps=TS, crop=CROP)
    check(logs["Blip"], ref["out"]["Blip"], dtype, "Blip reward")
    check(logs["G_loss"], ref["out"]["G_loss"], dtype, "G_loss")
    check(logs["step_loss"], ref["out"]["loss"], dtype, "step loss")
    gv, gv_ref = vae_vec(vb, vb.flat_grad), oracle_vec(ref["g_vae"], vb.names)
    gl_ref = torch.cat([ref["g_lora"][n].reshape(-1) for n in trainer.bank.names])
    e_v = rel_l2(gv, gv_ref)
    e_j = rel_l2(torch.cat([trainer.bank.flat_grad.cpu(), gv]), torch.cat([gl_ref, gv_ref]))
    print(f"tune_vae fp32 {dev.type}: VAE grad rel-L2 {e_v:.3e}, [LoRA; VAE] {e_j:.3e}, |g_vae| {float(gv_ref.norm()):.3e}, "
          f"|g_lora| {float(gl_ref.norm()):.3e}")
    assert e_v < 1e-3, f"VAE gradient rel-L2 {e_v:.3e}"
    assert e_j < 1e-3, f"[LoRA; VAE] gradient rel-L2 {e_j:.3e}"
    # the moments of the VAE segment: linear / quadratic in the CLIPPED gradient - the joint norm and the segment wiring
    e_m = rel_l2(vae_vec(vb, trainer.opt.m[1]), oracle_vec(ref["m_vae"], vb.names))
    e_s = rel_l2(vae_vec(vb, trainer.opt.v[1]), oracle_vec(ref["v_vae"], vb.names))
    print(f"  exp_avg rel-L2 {e_m:.3e}, exp_avg_sq {e_s:.3e}")
    assert e_m < 1e-3 and e_s < 2e-3, (e_m, e_s)
    # parameters after the update, over the elements whose oracle clipped gradient is >= 100 x adam_epsilon
    keep = oracle_vec(ref["clipped_vae"], vb.names).abs() >= 100 * cfg.adam_epsilon
    excluded = 1.0 - float(keep.float().mean())
    e_p = rel_l2(vae_vec(vb, vb.flat)[keep], oracle_vec(ref["p_vae"], vb.names)[keep])
    print(f"  parameters rel-L2 {e_p:.3e} over {100 * (1 - excluded):.1f} % of the elements")
    assert excluded <= 0.15, f"{100 * excluded:.1f} % of the VAE elements excluded"
    assert e_p < 3e-4, f"VAE parameters rel-L2 {e_p:.3e}"
    p_ref = torch.cat([ref["p_lora"][n].reshape(-1) for n in trainer.bank.names])
    assert rel_l2(trainer.bank.flat, p_ref) < 3e-4


def test_tune_vae_step_bf16(dev):
    """bf16 storage against the fp32 oracle on the same weights: VAE-gradient rel-L2 within 2 x the simulator's distance"""
    dtype = BF16
    cfg, batch, W, trainer = make_world(dtype, dev)
    vb = trainer.vae_bank
    ref = oracle_step(dtype, tuple(vb.names))
    trainer.train_step(batch, training_steps=TS, crop=CROP)
    e_v = rel_l2(vae_vec(vb, vb.flat_grad), oracle_vec(ref["g_vae"], vb.names))
    print(f"tune_vae bf16 {dev.type}: VAE grad rel-L2 {e_v:.3e}")
    path = os.environ.get("COMAT_TEST_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(f"tune_vae_step bf16 {dev.type} vae_grad={e_v:.3e}\n")
    assert e_v < BF16_VAE_GRAD_LIMIT, f"VAE gradient rel-L2 {e_v:.3e}"


# ---- flag off ---------------------------------------------------------------------------------------------------------------
def test_flag_off_changes_nothing(sim):
    """a default world's step is bit-equal to one built without any of the new arguments, and a frozen conv saves no tensor"""
    import test_step
    cfg0, batch0, _, old = test_step.make_world(F32, sim, False)
    la = old.train_step(batch0, training_steps=TS, crop=CROP)
    cfg1, batch1, _, new = make_world(F32, sim, tune=False)
    assert new.vae_bank is None and not cfg1.tune_vae
    lb = new.train_step(batch1, training_steps=TS, crop=CROP)
    for k_ in ("Blip", "G_loss", "D_loss", "step_loss"):
        assert torch.equal(la[k_], lb[k_]), k_
    assert torch.equal(old.bank.flat_grad, new.bank.flat_grad) and torch.equal(old.bank.flat, new.bank.flat)
    conv = new.pipe.vae.conv_in
    x = torch.randn(2 * 8 * 8, conv.cin, requires_grad=True)
    y = ops.conv2d(x, conv, 2, 8, 8)
    assert y.grad_fn.saved_tensors == ()


def test_flag_and_decoder_must_agree(sim):
    with pytest.raises(ValueError, match="tune_vae"):
        cfg, batch, W, tr = make_world(F32, sim, tune=False)
        CoMatTrainer(tr.pipe, tr.bank, tr.blip, tr.D, dataclasses.replace(cfg, tune_vae=True))


# ---- wiring, on the simulator ---------------------------------------------------------------------------------------------------
def test_accumulation_over_two_micro_steps(sim):
    """gradient_accumulation_steps = 2: two micro-steps = the update from the mean gradient; the VAE buffer is cleared only at
    the window's first micro-step"""
    cfg, batch, W, tr = make_world(F32, sim, gan=False, gradient_accumulation_steps=2)
    vb = tr.vae_bank
    p0 = vb.flat.clone()
    tr.train_step(batch, training_steps=TS, crop=CROP)
    g1 = vb.flat_grad.clone()
    assert torch.equal(vb.flat, p0) and float(g1.abs().max()) > 0  # no update yet
    tr.train_step(batch, training_steps=TS, crop=CROP)
    g2 = vb.flat_grad.clone()  # the sum of two micro-gradients (loss / N each): not cleared in between
    assert rel_l2(g2, 2 * g1) < 1e-5
    assert not torch.equal(vb.flat, p0)
    # one step of a plain world on the same batch: its gradient is the mean gradient of the window
    cfg1, batch1, W1, one = make_world(F32, sim, gan=False)
    one.train_step(batch1, training_steps=TS, crop=CROP)
    assert rel_l2(g2, one.vae_bank.flat_grad) < 1e-5
    assert rel_l2(vb.flat, one.vae_bank.flat) < 1e-6
    # cleared at the window's first micro-step and only there: a mark in an alignment pad (which no kernel writes) survives the
    # closing micro-step and is gone after the next window's first
    pad = next(o + vb.sd[n].numel() for n, (o, _, _) in vb.layout.items() if vb.sd[n].numel() % 8)
    tr.train_step(batch, training_steps=TS, crop=CROP)
    assert float(vb.flat_grad[pad]) == 0.0
    vb.flat_grad[pad] = 7.0
    tr.train_step(batch, training_steps=TS, crop=CROP)
    assert float(vb.flat_grad[pad]) == 7.0
    tr.train_step(batch, training_steps=TS, crop=CROP)
    assert float(vb.flat_grad[pad]) == 0.0


def test_cosine_schedule_moves_both_segments(sim):
    cfg, batch, W, tr = make_world(F32, sim, gan=False, lr_scheduler="cosine", max_train_steps=4)
    cfgc, batchc, Wc, const = make_world(F32, sim, gan=False)
    for _ in range(2):
        tr.train_step(batch, training_steps=TS, crop=CROP)
        const.train_step(batchc, training_steps=TS, crop=CROP)
    assert not torch.equal(tr.vae_bank.flat, const.vae_bank.flat) and not torch.equal(tr.bank.flat, const.bank.flat)


def test_non_finite_vae_gradient_skips_the_update(sim):
    cfg, batch, W, tr = make_world(F32, sim, gan=False)
    vb = tr.vae_bank
    tr._forward_backward(batch, dict(training_steps=TS, crop=CROP))
    vb.flat_grad[3] = float("inf")
    p_l, p_v = tr.bank.flat.clone(), vb.flat.clone()
    counters = tr.opt.counters.clone()
    tr._apply_updates()
    assert torch.equal(tr.bank.flat, p_l) and torch.equal(vb.flat, p_v)  # the whole generator update is skipped
    assert int(tr.opt.counters[0]) == int(counters[0]) and int(tr.opt.counters[1]) == int(counters[1]) + 1


# ---- graphs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_segmented_step_matches_eager(hip, dtype):
    """three calls of SegmentedStep = three eager steps under the flag, bit for bit, parameters included; the whole-step graph
    declines the flag"""
    cfg, batch, W, eager = make_world(dtype, hip)
    cfg2, batch2, W2, tr = make_world(dtype, hip)
    assert GraphedStep(tr).supported(batch2) is False
    eager.pipe.share_text_kv = False  # replayed segments project the text keys / values once per call (as tests/test_segments.py)
    stepper = SegmentedStep(tr)
    for i in range(3):
        la = eager.train_step(batch, training_steps=TS, crop=CROP)
        lb = stepper(batch2, training_steps=TS, crop=CROP)
        torch.cuda.synchronize()
        assert stepper.failed is None, stepper.failed
        for k_ in ("Blip", "G_loss", "D_loss", "step_loss"):
            assert torch.equal(la[k_], lb[k_]), (i, k_)
        assert torch.equal(eager.vae_bank.flat_grad, tr.vae_bank.flat_grad), i
        assert torch.equal(eager.vae_bank.flat, tr.vae_bank.flat) and torch.equal(eager.bank.flat, tr.bank.flat), i


# ---- checkpoint -------------------------------------------------------------------------------------------------------------------
def test_vae_checkpoint_round_trip(sim, tmp_path):
    cfg, batch, W, tr = make_world(F32, sim, gan=False)
    vb = tr.vae_bank
    tr.train_step(batch, training_steps=TS, crop=CROP)  # trained entries differ from the input state dict
    checkpoint.save_checkpoint(str(tmp_path), tr.bank, vae=vb)
    sd = torch.load(os.path.join(str(tmp_path), "vae.pt"), map_location="cpu")
    assert list(sd) == list(vb.sd) and all(tuple(sd[k_].shape) == tuple(vb.sd[k_].shape) for k_ in sd)
    assert any(not torch.equal(sd[n], vb.sd[n].float()) for n in vb.names)
    fresh = VAEBank(config.TINY_VAE, vb.sd, F32, sim)
    lora2 = LoRABank(config.TINY_UNET, {n: p.detach().clone() for n, p in tr.bank.params.items()}, F32, sim)
    checkpoint.load_checkpoint(str(tmp_path), lora2, vae=fresh)
    assert torch.equal(fresh.flat, vb.flat)
    short = {k_: v for k_, v in sd.items() if k_ != "decoder.conv_in.weight"}
    torch.save(short, os.path.join(str(tmp_path), "vae.pt"))
    with pytest.raises(KeyError, match="decoder"):
        checkpoint.load_checkpoint(str(tmp_path), lora2, vae=fresh)


# ---- data parallel ------------------------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, out_dir):
    """after tests/test_dist.py: two ranks over gloo on the simulator, each with its own latents and prompt"""
    import sys

    import torch.distributed as dist
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    from comat_amd import dist as cdist
    from sim_backend import SimKernels
    ops.set_kernel_backend(SimKernels())
    r, w, dev = cdist.init(backend="gloo")
    cfg, batch, W, trainer = make_world(F32, dev, gan=False)
    g = torch.Generator().manual_seed(100 + rank)
    batch["latents"] = torch.randn(batch["latents"].shape, generator=g)
    batch["prompt_embeds"] = torch.randn(batch["prompt_embeds"].shape, generator=g)
    vb = trainer.vae_bank
    trainer.bank.zero_grad()
    vb.zero_grad()
    trainer.compute_losses(batch, training_steps=TS, crop=CROP)["loss"].backward()
    local = torch.cat([trainer.bank.flat_grad, vb.flat_grad]).clone()
    gathered = [torch.zeros_like(local) for _ in range(world)]
    dist.all_gather(gathered, local)
    p0 = torch.cat([trainer.bank.flat, vb.flat]).clone()
    trainer.train_step(batch, training_steps=TS, crop=CROP)
    torch.save(dict(mean=torch.stack(gathered).mean(0), local=local, p0=p0, n_lora=trainer.bank.flat.numel(),
                    reduced=torch.cat([trainer.bank.flat_grad, vb.flat_grad]).clone() / world,
                    params=torch.cat([trainer.bank.flat, vb.flat]).detach().clone()), os.path.join(out_dir, f"rank{rank}.pt"))
    cdist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_vae_parameters(tmp_path):
    """both ranks hold equal VAE (and LoRA) parameters after a step, equal to the one-process update on the mean gradient under
    the joint clip"""
    import socket

    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    world = 2
    mp.spawn(_dp_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r = [torch.load(os.path.join(tmp_path, f"rank{i}.pt")) for i in range(world)]
    n = r[0]["n_lora"]
    assert not torch.allclose(r[0]["local"][n:], r[1]["local"][n:])  # the ranks saw different data
    for i in range(world):
        assert torch.allclose(r[i]["reduced"], r[i]["mean"], rtol=1e-5, atol=1e-7)  # the VAE gradient is exchanged with the LoRA one
    assert torch.equal(r[0]["params"], r[1]["params"])
    assert not torch.equal(r[0]["params"][n:], r[0]["p0"][n:])
    c = StepConfig()
    p = r[0]["p0"].clone().requires_grad_(True)
    p.grad = r[0]["mean"].clone()
    opt = torch.optim.AdamW([p], lr=1e-2, betas=(c.adam_beta1, c.adam_beta2), eps=c.adam_epsilon, weight_decay=c.adam_weight_decay)
    torch.nn.utils.clip_grad_norm_([p], c.max_grad_norm)  # ONE norm over [LoRA; VAE]
    opt.step()
    assert torch.allclose(p.detach(), r[0]["params"], rtol=1e-5, atol=1e-7)
