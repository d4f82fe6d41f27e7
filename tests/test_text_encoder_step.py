"""StepConfig.train_text_encoder_lora: the CLIP text tower inside the optimisation step, its LoRA factors trained - on the tiny
step world of tests/test_step.py with the tiny tower of tests/test_clip_text.py, simulator and real kernels.

The checker of the gradients is torch autograd on the CPU through transformers' CLIPTextModel (W + U D in its four projections)
into oracle/step.py: the oracle's `prompt_embeds` is a plain tensor, autograd flows through it unchanged.  fp32 storage, 1e-3
relative, the project's parity bar."""
import dataclasses
import os
import types

import numpy as np
import pytest
import torch
from safetensors.torch import load_file, save_file

from clip_sim import clip_dev  # noqa: F401 - fixture
from comat_amd import checkpoint, config, ops, weights
from comat_amd.blip import Blip
from comat_amd.clip import LORA_FILE_PREFIX, ClipLoRABank, ClipTextEncoder, lora_key
from comat_amd.gan import D_sd
from comat_amd.pipeline import TrainableSDPipeline, TrainableSDXLPipeline
from comat_amd.segments import SegmentedStep
from comat_amd.step import CoMatTrainer, GraphedStep, StepConfig
from comat_amd.unet import LoRABank, UNet, UNetBank, VAEDecoder
from helpers import check, rel_l2
from oracle import blip as OB
from oracle import sd as O
from oracle import step as OS
from test_clip_text import CFG as CLIP
from test_clip_text import END, hf_model, lora_factors, model_with_lora

UCFG = dataclasses.replace(config.TINY_UNET, cross_attention_dim=CLIP.hidden)
C2 = 16  # channels of the stand-in for SDXL's second encoder
XCFG = dataclasses.replace(config.TINY_SDXL_UNET, cross_attention_dim=CLIP.hidden + C2)
TS, CROP, ACS = [1, 2], (1, 0, 63, 63), [2]
FIXED = dict(training_steps=TS, crop=CROP, attrcon_steps=ACS)
BS, L = 2, 9


def _ids(bs, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, CLIP.vocab_size - 2, (bs, L), generator=g)
    for b in range(bs):
        ids[b, 4 + b:] = END  # the end token, then a run of pads
    null = torch.full((bs, L), END)
    null[:, 0] = 1  # start token, then the end token repeated: the empty prompt
    return ids, null


def make_world(dtype, dev, attrcon=False, flag=True, sdxl=False, bs=BS, rank=4, **cfg_kw):
    """the tiny step world with the context width of the tiny tower.  flag: ids in the batch, tower and text bank in the trainer;
    off: the same prompts as frozen embeddings (the tower's output at the initial factors) and a trainer without the new
    arguments.  -> namespace(cfg, batch, W, tr, factors)"""
    ucfg = XCFG if sdxl else UCFG
    vcfg = dataclasses.replace(config.TINY_VAE, scaling_factor=0.13025) if sdxl else config.TINY_VAE
    q = lambda d: {k: v.to(dtype).float() for k, v in d.items()}
    up5 = lambda d: {k: (v * 5 if k.endswith("up.weight") else v) for k, v in d.items()}
    usd = q(weights.make_unet_weights(ucfg, perturb_norms=True))
    vsd = q(weights.make_vae_weights(vcfg, perturb_norms=True))
    lsd = q(up5(weights.make_lora_weights(ucfg)))
    bsd = q(weights.make_blip_weights(config.TINY_BLIP, perturb_norms=True))
    dsd = q(weights.make_unet_weights(UCFG, seed=77, perturb_norms=True))
    dl = q(up5(weights.make_lora_weights(UCFG, seed=78)))
    fsd = lora_factors(rank, seed=3)
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g)
    rq = lambda *s: r(*s).to(dtype).float()
    head_w, head_b = r(4) * 0.5, r(1) * 0.1
    layers = ("mid_2", "up_2", "up_4") if sdxl else ("mid_2", "up_4", "up_8")
    cfg = StepConfig(**{**dict(resolution=64, total_step=3, K=2, gan_loss=True, attrcon=attrcon, attrcon_train_steps=1,
                               train_layer_ls=layers, attn_reses=(8, 4, 2), lr=1e-2, lr_D=1e-2, mask_token_loss_weight=0.5,
                               mask_pixel_loss_weight=0.1, train_text_encoder_lora=flag), **cfg_kw})
    bids = torch.randint(1, config.TINY_BLIP.vocab_size, (bs, 9), generator=g)
    masks = []
    for _ in range(bs):
        m = np.zeros((2, 64, 64), dtype=bool)
        m[0, 5:30, 8:40] = True
        m[1, 34:60, 20:64] = True
        masks.append(m)
    ids, null = _ids(bs, seed=7)
    batch = dict(gan_null_embeds=rq(bs, L, UCFG.cross_attention_dim), latents=r(bs, 4, 8, 8),
                 noises=[r(bs, 4, 8, 8) for _ in range(3)], real_latents=r(bs, 4, 8, 8), blip_input_ids=bids,
                 blip_attention_mask=torch.ones_like(bids), masks=masks, attributes=([[[2, 3], [5]], [[1], [4, 6]]] * bs)[:bs])
    if sdxl:
        batch.update(pooled_prompt_embeds=rq(bs, ucfg.pooled_dim), negative_pooled_prompt_embeds=rq(bs, ucfg.pooled_dim),
                     add_time_ids=(64, 64, 0, 0, 64, 64), prompt_embeds_2=rq(bs, L, C2), negative_prompt_embeds_2=rq(bs, L, C2))
    if flag:
        batch.update(prompt_input_ids=ids, null_input_ids=null)
    else:
        with torch.no_grad():
            emb = model_with_lora(torch.cat([null, ids]), fsd)[0].reshape(2 * bs, L, -1)
        batch.update(prompt_embeds=emb[bs:].to(dtype).float(), negative_prompt_embeds=emb[:bs].to(dtype).float())
    oc = lambda c: O.UNetConfig(**dataclasses.asdict(c))
    W = dict(unet=usd, vae=vsd, blip=bsd, d_unet=dsd, ucfg=oc(ucfg), d_ucfg=oc(UCFG), vcfg=O.VAEConfig(**dataclasses.asdict(vcfg)),
             bcfg=OB.BlipConfig(**dataclasses.asdict(config.TINY_BLIP)),
             lora={k: v.clone().requires_grad_(True) for k, v in lsd.items()},
             d_lora={k: v.clone().requires_grad_(True) for k, v in dl.items()},
             head_w=head_w.clone().requires_grad_(True), head_b=head_b.clone().requires_grad_(True))
    bank = LoRABank(ucfg, lsd, dtype, dev)
    pipe = (TrainableSDXLPipeline if sdxl else TrainableSDPipeline)(UNet(ucfg, usd, dtype, dev, bank), VAEDecoder(vcfg, vsd, dtype, dev))
    dbank = LoRABank(UCFG, dl, dtype, dev)
    disc = D_sd(UNet(UCFG, dsd, dtype, dev, dbank), dbank, head_w, head_b)
    blip = Blip(config.TINY_BLIP, bsd, dtype, dev)
    if flag:
        tbank = ClipLoRABank(CLIP, fsd, dtype, dev)
        enc = ClipTextEncoder(CLIP, hf_model().state_dict(), dtype, dev, tbank)
        tr = CoMatTrainer(pipe, bank, blip, disc, cfg, seed=0, text_encoder=enc, text_bank=tbank)
    else:
        tr = CoMatTrainer(pipe, bank, blip, disc, cfg, seed=0)
    return types.SimpleNamespace(cfg=cfg, batch=batch, W=W, tr=tr, factors=fsd, sdxl=sdxl)


def oracle_batch(w, leaves, detach_null=False):
    """the oracle's batch: the embeddings of the ids from the CPU model with W + U D (leaves: the factors, requiring grad)"""
    b = w.batch
    bs = b["prompt_input_ids"].shape[0]
    emb = model_with_lora(torch.cat([b["null_input_ids"], b["prompt_input_ids"]]), leaves)[1 if w.sdxl else 0]
    if w.sdxl:
        emb = torch.cat([emb, torch.cat([b["negative_prompt_embeds_2"], b["prompt_embeds_2"]]).reshape(-1, C2)], dim=1)
    emb = emb.reshape(2 * bs, L, -1)
    null = emb[:bs].detach() if detach_null else emb[:bs]
    ob = {k: v for k, v in b.items() if k not in ("prompt_input_ids", "null_input_ids")}
    ob.update(prompt_embeds=emb[bs:], negative_prompt_embeds=null)
    return ob


def oracle_step(w, detach_null=False):
    leaves = {k: v.clone().requires_grad_(True) for k, v in w.factors.items()}
    ref = OS.train_step(w.W, oracle_batch(w, leaves, detach_null), w.cfg, TS, CROP, ACS)
    return ref, leaves


def flat_of(grads, names):
    return torch.cat([grads[n].reshape(-1) for n in names])


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


# ---- gradients and update ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attrcon", [False, True])
def test_text_factor_gradients_match_autograd_through_the_model(clip_dev, attrcon):
    dtype = torch.float32
    w = make_world(dtype, clip_dev, attrcon)
    ref, leaves = oracle_step(w)
    tr = w.tr
    p0, t0 = tr.bank.flat.clone(), tr.text_bank.flat.clone()
    logs = tr.train_step(w.batch, **FIXED)
    sync(clip_dev)
    for key, rk in (("Blip", "Blip"), ("G_loss", "G_loss"), ("D_loss", "D_loss"), ("step_loss", "loss")) + \
            ((("token_loss", "token_loss"), ("pixel_loss", "pixel_loss")) if attrcon else ()):
        check(logs[key], ref[rk], dtype, key)
    tb = tr.text_bank
    g_ref = flat_of(ref["g_grads"], tr.bank.names)
    t_ref = flat_of({k: v.grad for k, v in leaves.items()}, tb.names)
    print(f"text step attrcon={attrcon}: unet {rel_l2(tr.bank.flat_grad, g_ref):.3e} text {rel_l2(tb.flat_grad, t_ref):.3e}")
    assert rel_l2(tr.bank.flat_grad, g_ref) < 1e-3
    assert rel_l2(tb.flat_grad, t_ref) < 1e-3
    for n in tb.names:
        assert float(leaves[n].grad.norm()) > 0, n
        assert rel_l2(tb.params[n].grad, leaves[n].grad) < 1e-3, (n, rel_l2(tb.params[n].grad, leaves[n].grad))
    # ONE clip norm over both banks (training_script.py:661-662): the hand-computed one
    by_hand = float(tr.bank.flat_grad.double().pow(2).sum() + tb.flat_grad.double().pow(2).sum())
    assert abs(float(tr.opt.gnorm_sq) - by_hand) < 1e-5 * by_hand
    assert abs(float(tr.opt.gnorm_sq) - float(g_ref.double().pow(2).sum() + t_ref.double().pow(2).sum())) < 2e-3 * by_hand
    assert float(tb.flat_grad.double().pow(2).sum()) > 1e-6 * by_hand  # (the text share of the norm is not lost in rounding)
    # the update: torch's clip over both parameter sets + AdamW (the first Adam update is sign-like: 3e-4, as tests/test_step.py)
    cfg = w.cfg
    params = list(w.W["lora"].values()) + list(leaves.values())
    opt = torch.optim.AdamW(params, lr=cfg.lr, betas=(cfg.adam_beta1, cfg.adam_beta2), eps=cfg.adam_epsilon,
                            weight_decay=cfg.adam_weight_decay)
    torch.nn.utils.clip_grad_norm_(params, cfg.max_grad_norm)
    opt.step()
    assert rel_l2(tr.bank.flat, flat_of({k: v.detach() for k, v in w.W["lora"].items()}, tr.bank.names)) < 3e-4
    assert rel_l2(tb.flat, flat_of({k: v.detach() for k, v in leaves.items()}, tb.names)) < 3e-4
    assert not torch.equal(tb.flat, t0) and not torch.equal(tr.bank.flat, p0)


def test_the_unconditional_half_trains_the_factors(clip_dev):
    """training_script.py:571 re-encodes the null prompt with gradients enabled: with its upstream gradient zeroed (the null
    embedding detached in the checker) the factors' gradient is another one, and the step's is the full one"""
    w = make_world(torch.float32, clip_dev)
    full, leaves = oracle_step(w)
    cut, leaves_cut = oracle_step(w, detach_null=True)
    names = w.tr.text_bank.names
    t_full, t_cut = flat_of({k: v.grad for k, v in leaves.items()}, names), flat_of({k: v.grad for k, v in leaves_cut.items()}, names)
    assert rel_l2(t_cut, t_full) > 0.05, "the checker's unconditional half carries no gradient: the case shows nothing"
    w.tr.train_step(w.batch, **FIXED)
    sync(clip_dev)
    assert rel_l2(w.tr.text_bank.flat_grad, t_full) < 1e-3
    assert rel_l2(w.tr.text_bank.flat_grad, t_cut) > 0.04


def test_textenc_lora_lr_moves_only_the_text_segment(clip_dev):
    """under a warm-up schedule: the UNet's factors move as without the option, the text factors by the ratio of the rates"""
    ratio = 0.25
    kw = dict(lr_scheduler="constant_with_warmup", lr_warmup_steps=4)
    a = make_world(torch.float32, clip_dev, **kw)
    b = make_world(torch.float32, clip_dev, textenc_lora_lr=ratio * 1e-2, **kw)
    before = a.tr.text_bank.flat.clone()
    for w in (a, b):
        w.tr.train_step(w.batch, **FIXED)  # the rate of the first update is 0 / 4
    sync(clip_dev)
    assert torch.equal(a.tr.text_bank.flat, before) and torch.equal(b.tr.text_bank.flat, before)
    assert float(a.tr.opt.lr_now) == float(np.float32(1e-2 * 0.25))
    idx = len(b.tr.opt.segments) - 1
    assert list(b.tr.opt.own_lr) == [idx] and not a.tr.opt.own_lr
    assert float(b.tr.opt.own_word[idx][1]) == float(np.float32(ratio * 1e-2 * 0.25)) and float(b.tr.opt.lr_now) == float(a.tr.opt.lr_now)
    for w in (a, b):
        w.tr.train_step(w.batch, **FIXED)
    sync(clip_dev)
    assert torch.equal(a.tr.bank.flat, b.tr.bank.flat)  # the UNet's segment: the same bits
    da, db = a.tr.text_bank.flat - before, b.tr.text_bank.flat - before
    assert float(da.abs().max()) > 0
    # p - lr (wd p + m^ / (sqrt(v^) + eps)) is linear in lr; a difference of two fp32 parameters carries 2^-24 |p| of rounding,
    # |p| < 1 against steps of 6e-4: 1e-4 relative.  Held to 1e-3
    assert rel_l2(db, ratio * da) < 1e-3
    assert float(b.tr.opt.own_word[idx][1]) == float(np.float32(ratio * 1e-2 * 0.5))


def test_a_non_finite_norm_skips_both_segments(clip_dev):
    w = make_world(torch.float32, clip_dev)
    tr = w.tr
    p0, t0 = tr.bank.flat.clone(), tr.text_bank.flat.clone()
    for poisoned in (tr.text_bank, tr.bank):
        tr._forward_backward(w.batch, FIXED)
        poisoned.flat_grad[3] = float("inf")
        tr._apply_updates()
        sync(clip_dev)
        assert torch.equal(tr.bank.flat, p0) and torch.equal(tr.text_bank.flat, t0)
    assert tr.opt.counters.tolist() == [0, 2]
    tr.train_step(w.batch, **FIXED)
    sync(clip_dev)
    assert tr.opt.counters.tolist() == [1, 2]
    assert not torch.equal(tr.bank.flat, p0) and not torch.equal(tr.text_bank.flat, t0)


# ---- gradient checkpointing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("attrcon", [False, True])
def test_gradient_checkpointing_gives_the_same_bits(clip_dev, dtype, attrcon):
    """as tests/test_recompute.py: the baseline is the plain step with the text key / value sharing off"""
    plain, ckpt = make_world(dtype, clip_dev, attrcon), make_world(dtype, clip_dev, attrcon, gradient_checkpointing=True)
    plain.tr.pipe.share_text_kv = False
    assert ckpt.tr.pipe.gradient_checkpointing and not plain.tr.pipe.gradient_checkpointing
    for step in range(2):
        la, lb = plain.tr.train_step(plain.batch, **FIXED), ckpt.tr.train_step(ckpt.batch, **FIXED)
        sync(clip_dev)
        for k in ("Blip", "G_loss", "D_loss", "step_loss", "grad_norm_sq") + (("token_loss", "pixel_loss") if attrcon else ()):
            assert torch.equal(la[k], lb[k]), (step, k)
        for x in ("bank", "text_bank"):
            assert torch.equal(getattr(plain.tr, x).flat_grad, getattr(ckpt.tr, x).flat_grad), (step, x)
            assert torch.equal(getattr(plain.tr, x).flat, getattr(ckpt.tr, x).flat), (step, x)
    assert float(ckpt.tr.text_bank.flat_grad.abs().max()) > 0


# ---- runners and errors ----------------------------------------------------------------------------------------------------------
def test_graph_runners_decline_the_flag(clip_dev):
    w, e = make_world(torch.float32, clip_dev), make_world(torch.float32, clip_dev)
    assert not GraphedStep(w.tr).supported(w.batch)
    stepper = SegmentedStep(w.tr, dry=True)  # dry: the segment hooks run wherever the stepper does not decline
    a = stepper(w.batch, **FIXED)
    b = e.tr.train_step(e.batch, **FIXED)
    sync(clip_dev)
    assert not stepper.unet_segs and stepper.head_seg is None and stepper.failed is None
    assert torch.equal(a["step_loss"], b["step_loss"]) and torch.equal(w.tr.text_bank.flat, e.tr.text_bank.flat)
    graphed = GraphedStep(w.tr)
    graphed(w.batch, training_steps=TS, crop=CROP)
    assert not graphed.graphs and graphed.failed is None


@pytest.mark.gpu
def test_graphed_step_would_take_the_world_without_the_flag(hip):
    """the refusal above is the flag's: the same world without it is one the whole-step graph supports"""
    off = make_world(torch.float32, hip, flag=False)
    assert GraphedStep(off.tr).supported(off.batch)


def test_every_mismatch_raises(clip_dev):
    w = make_world(torch.float32, clip_dev)
    tr = w.tr
    parts = (tr.pipe, tr.bank, tr.blip, tr.D)
    on, off = w.cfg, dataclasses.replace(w.cfg, train_text_encoder_lora=False)
    with pytest.raises(ValueError, match="train_text_encoder_lora"):
        CoMatTrainer(*parts, on)
    with pytest.raises(ValueError, match="train_text_encoder_lora"):
        CoMatTrainer(*parts, off, text_encoder=tr.text_encoder, text_bank=tr.text_bank)
    with pytest.raises(ValueError, match="text_bank"):
        CoMatTrainer(*parts, on, text_encoder=tr.text_encoder)
    with pytest.raises(ValueError, match="text_bank"):
        CoMatTrainer(*parts, on, text_bank=tr.text_bank)
    other = ClipLoRABank(CLIP, w.factors, torch.float32, clip_dev)
    with pytest.raises(ValueError, match="text_bank"):
        CoMatTrainer(*parts, on, text_encoder=tr.text_encoder, text_bank=other)
    with pytest.raises(ValueError, match="textenc_lora_lr.*train_text_encoder_lora"):
        StepConfig(textenc_lora_lr=1e-5)
    with pytest.raises(ValueError, match="train_text_encoder_lora.*full_finetuning"):
        StepConfig(train_text_encoder_lora=True, full_finetuning=True)
    with pytest.raises(ValueError, match="train_text_encoder_lora.*use_8bit_adam"):
        StepConfig(train_text_encoder_lora=True, use_8bit_adam=True)
    with pytest.raises(ValueError, match="textenc_lora_lr.*polynomial"):
        StepConfig(train_text_encoder_lora=True, textenc_lora_lr=1e-5, lr_scheduler="polynomial", max_train_steps=10)
    emb = torch.zeros(BS, L, CLIP.hidden)
    with pytest.raises(ValueError, match="prompt_embeds"):
        tr.train_step(dict(w.batch, prompt_embeds=emb, negative_prompt_embeds=emb), **FIXED)
    with pytest.raises(ValueError, match="null_input_ids"):
        tr.train_step({k: v for k, v in w.batch.items() if k != "null_input_ids"}, **FIXED)
    with pytest.raises(ValueError, match="prompt_input_ids"):
        tr.train_step({k: v for k, v in w.batch.items() if k != "prompt_input_ids"}, **FIXED)
    x = make_world(torch.float32, clip_dev, sdxl=True, bs=1)
    with pytest.raises(ValueError, match="prompt_embeds_2"):
        x.tr.train_step({k: v for k, v in x.batch.items() if k != "prompt_embeds_2"}, **FIXED)


# ---- SDXL ------------------------------------------------------------------------------------------------------------------------
def test_sdxl_concatenated_context(clip_dev):
    """[encoder-1 "penultimate" | frozen encoder-2 tensors] along the channels: the gradient reaches the factors the penultimate
    state depends on - against the checker - and none is asked of the second encoder's tensors"""
    w = make_world(torch.float32, clip_dev, attrcon=True, sdxl=True, bs=1)
    for k in ("prompt_embeds_2", "negative_prompt_embeds_2"):
        w.batch[k].requires_grad_(True)
    ref, leaves = oracle_step(w)
    second = {k: w.batch[k].grad.clone() for k in ("prompt_embeds_2", "negative_prompt_embeds_2")}
    assert all(float(g.abs().max()) > 0 for g in second.values())  # (the checker's graph does reach them)
    for k in second:
        w.batch[k].grad = None
    logs = w.tr.train_step(w.batch, **FIXED)
    sync(clip_dev)
    check(logs["step_loss"], ref["loss"], torch.float32, "step loss")
    assert all(w.batch[k].grad is None for k in second)
    tb = w.tr.text_bank
    assert rel_l2(w.tr.bank.flat_grad, flat_of(ref["g_grads"], w.tr.bank.names)) < 1e-3
    last = f"layers.{CLIP.layers - 1}."
    for n in tb.names:
        if last in n:  # hidden_states[-2] does not pass through the last layer
            assert leaves[n].grad is None or not leaves[n].grad.any()
            assert not tb.params[n].grad.any(), n
        else:
            assert float(leaves[n].grad.norm()) > 0 and rel_l2(tb.params[n].grad, leaves[n].grad) < 1e-3, n


# ---- checkpoint ------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_and_key_names(clip_dev, tmp_path):
    w = make_world(torch.float32, clip_dev)
    tr = w.tr
    tr.train_step(w.batch, **FIXED)
    sync(clip_dev)
    d = str(tmp_path / "ck")
    checkpoint.save_checkpoint(d, tr.bank, tr.D, optim=dict(G=tr.opt, D=tr.opt_D), text=tr.text_bank)
    saved = tr.bank.flat.clone()
    sd = load_file(os.path.join(d, checkpoint.LORA_WEIGHT_NAME))
    text_keys = sorted(k for k in sd if k.startswith(LORA_FILE_PREFIX))
    want = sorted(LORA_FILE_PREFIX + lora_key(i, p, f) for i in range(CLIP.layers) for p in ("q_proj", "k_proj", "v_proj", "out_proj")
                  for f in ("down", "up"))
    assert text_keys == want
    assert "text_encoder.text_model.encoder.layers.0.self_attn.q_proj.lora_linear_layer.down.weight" in sd
    assert sorted(k for k in sd if not k.startswith(LORA_FILE_PREFIX)) == sorted("unet." + n for n in tr.bank.names)
    f = make_world(torch.float32, clip_dev)
    assert not torch.equal(f.tr.text_bank.flat, tr.text_bank.flat)
    checkpoint.load_checkpoint(d, f.tr.bank, f.tr.D, optim=dict(G=f.tr.opt, D=f.tr.opt_D), text=f.tr.text_bank)
    assert torch.equal(f.tr.text_bank.flat, tr.text_bank.flat) and torch.equal(f.tr.bank.flat, tr.bank.flat)
    # optim_state.pt carries the extra segment: the resumed run continues bit for bit
    assert len(f.tr.opt.m) == len(tr.opt.m) == 2 and all(torch.equal(x, y) for x, y in zip(f.tr.opt.m + f.tr.opt.v, tr.opt.m + tr.opt.v))
    tr.train_step(w.batch, **FIXED)
    f.tr.train_step(f.batch, **FIXED)
    sync(clip_dev)
    assert torch.equal(f.tr.text_bank.flat, tr.text_bank.flat) and torch.equal(f.tr.bank.flat, tr.bank.flat)
    # ... and an optimizer without the segment refuses the file
    off = make_world(torch.float32, clip_dev, flag=False)
    with pytest.raises(ValueError, match="segments"):
        checkpoint.load_checkpoint(d, off.tr.bank, off.tr.D, optim=dict(G=off.tr.opt, D=off.tr.opt_D))
    # a UNet-only reader ignores the text entries
    checkpoint.load_checkpoint(d, off.tr.bank, off.tr.D)
    assert torch.equal(off.tr.bank.flat, saved)


def test_checkpoint_without_text_is_what_it_was_and_is_refused_by_a_text_reader(clip_dev, tmp_path):
    w = make_world(torch.float32, clip_dev)
    tr = w.tr
    a, b, c = (str(tmp_path / n) for n in "abc")
    checkpoint.save_checkpoint(a, tr.bank, tr.D)
    checkpoint.save_checkpoint(b, tr.bank, tr.D, text=None)
    os.makedirs(c)
    # the parent's writer: the UNet's factors alone, through safetensors
    save_file(checkpoint.lora_state_dict(tr.bank), os.path.join(c, checkpoint.LORA_WEIGHT_NAME), metadata={"format": "pt"})
    read = lambda d: open(os.path.join(d, checkpoint.LORA_WEIGHT_NAME), "rb").read()
    assert read(a) == read(b) == read(c)
    with pytest.raises(KeyError, match=r"text_encoder\.text_model\.encoder\.layers\.0\.self_attn\.q_proj"):
        checkpoint.load_checkpoint(a, tr.bank, tr.D, text=tr.text_bank)
    # another rank: a shape mismatch names the key
    checkpoint.save_checkpoint(a, tr.bank, tr.D, text=tr.text_bank)
    other = ClipLoRABank(CLIP, lora_factors(16, seed=3), torch.float32, clip_dev)
    with pytest.raises(ValueError, match=r"text_encoder\.text_model\.encoder\.layers\.0\.self_attn\.q_proj.*shape"):
        checkpoint.load_checkpoint(a, tr.bank, tr.D, text=other)
    with pytest.raises(ValueError, match="full_finetuning"):
        checkpoint.save_checkpoint(a, UNetBank.__new__(UNetBank), text=tr.text_bank)


# ---- flag off --------------------------------------------------------------------------------------------------------------------
class _Recorded:
    """a kernel backend that notes the name of every entry point called through it"""

    def __init__(self, inner):
        self._inner, self.calls = inner, []

    def __getattr__(self, name):
        fn = getattr(self._inner, name)  # (AttributeError for what the backend lacks: `hasattr` answers as before)
        if not callable(fn):
            return fn

        def call(*a, **kw):
            self.calls.append(name)
            return fn(*a, **kw)
        return call


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_flag_off_is_the_step_it_was(clip_dev, dtype):
    """a trainer handed the new arguments at their defaults issues the launches, and gives the bits, of one built without them"""
    a, b = make_world(dtype, clip_dev, flag=False), make_world(dtype, clip_dev, flag=False)
    assert not a.cfg.train_text_encoder_lora and a.cfg.textenc_lora_lr is None
    b.tr = CoMatTrainer(b.tr.pipe, b.tr.bank, b.tr.blip, b.tr.D, dataclasses.replace(b.cfg, train_text_encoder_lora=False,
                                                                                      textenc_lora_lr=None),
                        seed=0, text_encoder=None, text_bank=None)
    inner = ops.kernels()
    runs = []
    for w in (a, b):
        rec = _Recorded(inner)
        ops.set_kernel_backend(rec)
        try:
            logs = [w.tr.train_step(w.batch, **FIXED) for _ in range(2)]
            sync(clip_dev)
        finally:
            ops.set_kernel_backend(inner)
        runs.append((rec.calls, logs))
    assert runs[0][0] == runs[1][0] and len(runs[0][0]) > 100
    assert a.tr.text_bank is None and len(a.tr.opt.segments) == 1
    for la, lb in zip(runs[0][1], runs[1][1]):
        for k in ("Blip", "G_loss", "D_loss", "step_loss", "grad_norm_sq"):
            assert torch.equal(la[k], lb[k]), k
    assert torch.equal(a.tr.bank.flat, b.tr.bank.flat) and torch.equal(a.tr.D.bank.flat, b.tr.D.bank.flat)
    assert "segment_lrs" not in a.tr.opt.state_dict()
