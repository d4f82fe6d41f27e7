"""StepConfig.tune_text_encoder: the CLIP text tower trained in full inside the optimisation step - the tiny step world of
tests/test_text_encoder_step.py with a clip.ClipTextBank where that file has LoRA factors, simulator and (the first two tests) real
kernels.

The checker of the gradients is torch autograd on the CPU through transformers' CLIPTextModel, every parameter a leaf, into
oracle/step.py: the oracle's `prompt_embeds` is a plain tensor, autograd flows through it unchanged.  fp32 storage, 1e-3 relative
per tensor, the project's parity bar."""
import dataclasses
import os
import types

import pytest
import torch

from clip_tune_sim import ClipTuneSimKernels, tune_dev  # noqa: F401 - fixture
from comat_amd import checkpoint, config, ops, weights
from comat_amd.blip import Blip
from comat_amd.clip import POS_NAME, TOK_NAME, ClipLoRABank, ClipTextBank, ClipTextEncoder
from comat_amd.gan import D_sd
from comat_amd.pipeline import TrainableSDPipeline
from comat_amd.segments import SegmentedStep
from comat_amd.step import CoMatTrainer, GraphedStep, StepConfig
from comat_amd.unet import LoRABank, UNet, UNetBank, VAEBank, VAEDecoder
from helpers import check, rel_l2
from oracle import blip as OB
from oracle import sd as O
from oracle import step as OS
from test_clip_tune import CFG as CLIP
from test_clip_tune import END, bare, hf_model

UCFG = dataclasses.replace(config.TINY_UNET, cross_attention_dim=CLIP.hidden)
TS, CROP = [1, 2], (1, 0, 63, 63)
FIXED = dict(training_steps=TS, crop=CROP)
BS, L = 2, 9
F32 = torch.float32


@pytest.fixture
def tune_sim(sim):
    """the simulator that knows comat_embed_fwd / comat_embed_grad, CPU only"""
    ops.set_kernel_backend(ClipTuneSimKernels())
    return sim


def _ids(bs, seed):
    """prompts WITHOUT the end token (random ids to the last position): the only rows of the batch that name it are the null prompt's"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, CLIP.vocab_size - 2, (bs, L), generator=g)
    ids[:, L - 2:] = ids[:, :1]  # a repeated id inside every prompt: rows of the table collide without the end token
    null = torch.full((bs, L), END)
    null[:, 0] = 1  # start token, then the end token repeated: the empty prompt
    return ids, null


def model_embeds(ids, leaves=None):
    """last_hidden_state of the checker as [B, L, hidden]; leaves: {parameter name: tensor} to differentiate"""
    m = hf_model()
    kw = dict(input_ids=ids, attention_mask=None)
    out = m(**kw) if leaves is None else torch.func.functional_call(m, leaves, args=(), kwargs=kw)
    return out.last_hidden_state


def make_world(dtype, dev, flag=True, tune_vae=False, full=False, bs=BS, **cfg_kw):
    """the tiny step world with the context width of the tiny tower.  flag: ids in the batch, tower and ClipTextBank in the trainer;
    off: the same prompts as frozen embeddings and a trainer without the text arguments"""
    q = lambda d: {k: v.to(dtype).float() for k, v in d.items()}
    up5 = lambda d: {k: (v * 5 if k.endswith("up.weight") else v) for k, v in d.items()}
    usd = q(weights.make_unet_weights(UCFG, perturb_norms=True))
    vsd = q(weights.make_vae_weights(config.TINY_VAE, perturb_norms=True))
    lsd = q(up5(weights.make_lora_weights(UCFG)))
    bsd = q(weights.make_blip_weights(config.TINY_BLIP, perturb_norms=True))
    dsd = q(weights.make_unet_weights(UCFG, seed=77, perturb_norms=True))
    dl = q(up5(weights.make_lora_weights(UCFG, seed=78)))
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g)
    rq = lambda *s: r(*s).to(dtype).float()
    head_w, head_b = r(4) * 0.5, r(1) * 0.1
    cfg = StepConfig(**{**dict(resolution=64, total_step=3, K=2, gan_loss=True, attrcon=False, lr=1e-2, lr_D=1e-2,
                               tune_text_encoder=flag, tune_vae=tune_vae, full_finetuning=full), **cfg_kw})
    bids = torch.randint(1, config.TINY_BLIP.vocab_size, (bs, 9), generator=g)
    ids, null = _ids(bs, seed=7)
    batch = dict(gan_null_embeds=rq(bs, L, UCFG.cross_attention_dim), latents=r(bs, 4, 8, 8),
                 noises=[r(bs, 4, 8, 8) for _ in range(3)], real_latents=r(bs, 4, 8, 8), blip_input_ids=bids,
                 blip_attention_mask=torch.ones_like(bids))
    guided = cfg.cfg_scale > 1.0
    if flag:
        batch.update(prompt_input_ids=ids, **(dict(null_input_ids=null) if guided else {}))
    else:
        with torch.no_grad():
            emb = model_embeds(torch.cat([null, ids]))
        batch.update(prompt_embeds=emb[bs:].to(dtype).float(), negative_prompt_embeds=emb[:bs].to(dtype).float())
    oc = lambda c: O.UNetConfig(**dataclasses.asdict(c))
    W = dict(unet=usd, vae=vsd, blip=bsd, d_unet=dsd, ucfg=oc(UCFG), d_ucfg=oc(UCFG),
             vcfg=O.VAEConfig(**dataclasses.asdict(config.TINY_VAE)), bcfg=OB.BlipConfig(**dataclasses.asdict(config.TINY_BLIP)),
             lora={k: v.clone().requires_grad_(True) for k, v in lsd.items()},
             d_lora={k: v.clone().requires_grad_(True) for k, v in dl.items()},
             head_w=head_w.clone().requires_grad_(True), head_b=head_b.clone().requires_grad_(True))
    bank = UNetBank(UCFG, usd, dtype, dev) if full else LoRABank(UCFG, lsd, dtype, dev)
    unet = UNet(UCFG, usd, dtype, dev, bank=bank) if full else UNet(UCFG, usd, dtype, dev, bank)
    vae = VAEDecoder(config.TINY_VAE, vsd, dtype, dev, bank=VAEBank(config.TINY_VAE, vsd, dtype, dev)) if tune_vae else \
        VAEDecoder(config.TINY_VAE, vsd, dtype, dev)
    pipe = TrainableSDPipeline(unet, vae)
    dbank = LoRABank(UCFG, dl, dtype, dev)
    disc = D_sd(UNet(UCFG, dsd, dtype, dev, dbank), dbank, head_w, head_b)
    blip = Blip(config.TINY_BLIP, bsd, dtype, dev)
    kw = {}
    if flag:
        tbank = ClipTextBank(CLIP, hf_model().state_dict(), dtype, dev)
        kw = dict(text_encoder=ClipTextEncoder(CLIP, None, dtype, dev, tbank), text_bank=tbank)
    return types.SimpleNamespace(cfg=cfg, batch=batch, W=W, tr=CoMatTrainer(pipe, bank, blip, disc, cfg, seed=0, **kw))


def oracle_step(w, batch=None):
    """the oracle's step on the embeddings of the checker, every parameter of the tower a leaf -> (ref, {bare name: gradient})"""
    b = w.batch if batch is None else batch
    bs = b["prompt_input_ids"].shape[0]
    leaves = {n: p.detach().clone().requires_grad_(True) for n, p in hf_model().named_parameters()}
    guided = "null_input_ids" in b
    emb = model_embeds(torch.cat([b["null_input_ids"], b["prompt_input_ids"]]) if guided else b["prompt_input_ids"], leaves)
    ob = {k: v for k, v in b.items() if k not in ("prompt_input_ids", "null_input_ids")}
    ob.update(prompt_embeds=emb[bs:] if guided else emb, **(dict(negative_prompt_embeds=emb[:bs]) if guided else {}))
    ref = OS.train_step(w.W, ob, w.cfg, TS, CROP, None)
    return ref, {bare(n): p.grad for n, p in leaves.items()}


def flat_of(grads, names):
    return torch.cat([grads[n].reshape(-1) for n in names])


def params_vec(tb, buf):
    """the parameters' elements of one of the text bank's flat buffers, without the alignment pads"""
    return torch.cat([tb._view(buf, n).detach().reshape(-1).cpu() for n in tb.names])


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


_ORACLE = {}


def cached_oracle(w):
    """the guided fp32 world's oracle step: computed once, shared, never changed"""
    if "ref" not in _ORACLE:
        _ORACLE["ref"] = oracle_step(w)
    return _ORACLE["ref"]


# ---- gradients and update (simulator and MI355X) ---------------------------------------------------------------------------------
def test_tower_gradients_match_autograd_through_the_model(tune_dev):
    w = make_world(F32, tune_dev)
    ref, grads = cached_oracle(w)
    tr = w.tr
    p0, t0 = tr.bank.flat.clone(), tr.text_bank.flat.clone()
    logs = tr.train_step(w.batch, **FIXED)
    sync(tune_dev)
    for key, rk in (("Blip", "Blip"), ("G_loss", "G_loss"), ("D_loss", "D_loss"), ("step_loss", "loss")):
        check(logs[key], ref[rk], F32, key)
    tb = tr.text_bank
    g_ref = flat_of(ref["g_grads"], tr.bank.names)
    t_ref = flat_of(grads, tb.names)
    t_got = params_vec(tb, tb.flat_grad)
    print(f"tune text step: unet {rel_l2(tr.bank.flat_grad, g_ref):.3e} text {rel_l2(t_got, t_ref):.3e}")
    assert rel_l2(tr.bank.flat_grad, g_ref) < 1e-3 and rel_l2(t_got, t_ref) < 1e-3
    q_scale = {n: float(grads[n.replace("k_proj", "q_proj")].norm()) for n in tb.names if n.endswith("k_proj.bias")}
    for n in tb.names:
        if n.endswith("k_proj.bias"):  # zero in exact arithmetic (softmax does not see a constant added to every key)
            assert float(grads[n].norm()) < 1e-4 * q_scale[n] and float(tb.params[n].grad.norm()) < 1e-3 * q_scale[n], n
            continue
        assert float(grads[n].norm()) > 0, n
        assert rel_l2(tb.params[n].grad, grads[n]) < 1e-3, (n, rel_l2(tb.params[n].grad, grads[n]))
    # ONE clip norm over both banks (training_script.py:661-662): the hand-computed one
    by_hand = float(tr.bank.flat_grad.double().pow(2).sum() + tb.flat_grad.double().pow(2).sum())
    assert abs(float(tr.opt.gnorm_sq) - by_hand) < 1e-5 * by_hand
    assert float(tb.flat_grad.double().pow(2).sum()) > 1e-6 * by_hand  # (the text share of the norm is not lost in rounding)
    assert len(tr.opt.segments) == 2 and tr.opt.segments[-1][0] is tb.flat
    assert not torch.equal(tb.flat, t0) and not torch.equal(tr.bank.flat, p0) and tr.opt.counters.tolist() == [1, 0]
    # every row of the token table that an id names has a gradient and moved; no other row has one
    tok0, tok1 = tb._view(t0, TOK_NAME), tb.params[TOK_NAME].detach()
    named = torch.zeros(CLIP.vocab_size, dtype=torch.bool)
    named[torch.cat([w.batch["prompt_input_ids"], w.batch["null_input_ids"]]).reshape(-1)] = True
    assert not tb.params[TOK_NAME].grad.cpu()[~named].any()
    assert (tok1.cpu()[named] != tok0.cpu()[named]).any(dim=1).all()


def test_the_null_prompt_alone_moves_the_end_token_row(tune_dev):
    """no prompt of this world holds the end token: with guidance on, its row of the token table gets its gradient from the null
    prompt's 8 repeats (training_script.py:571 re-encodes it under autograd); with guidance off no id names it and the row stays"""
    w = make_world(F32, tune_dev)
    assert not (w.batch["prompt_input_ids"] == END).any() and (w.batch["null_input_ids"][:, 1:] == END).all()
    _, grads = cached_oracle(w)
    tb = w.tr.text_bank
    row0 = tb.params[TOK_NAME][END].detach().clone()
    w.tr.train_step(w.batch, **FIXED)
    sync(tune_dev)
    g_end = tb.params[TOK_NAME].grad[END]
    assert float(grads[TOK_NAME][END].norm()) > 0 and rel_l2(g_end, grads[TOK_NAME][END]) < 1e-3
    assert not torch.equal(tb.params[TOK_NAME][END].detach(), row0)
    off = make_world(F32, tune_dev, cfg_scale=1.0)
    assert "null_input_ids" not in off.batch
    tb = off.tr.text_bank
    off.tr.train_step(off.batch, **FIXED)
    sync(tune_dev)
    assert not tb.params[TOK_NAME].grad[END].any() and float(tb.params[TOK_NAME].grad.abs().max()) > 0
    if off.cfg.adam_weight_decay == 0.0:
        assert torch.equal(tb.params[TOK_NAME][END].detach(), row0)


# ---- one optimizer (simulator) -------------------------------------------------------------------------------------------------
def test_text_unet_and_vae_segments_share_one_clip_norm_and_one_skip(tune_sim):
    w = make_world(F32, tune_sim, tune_vae=True)
    tr = w.tr
    banks = (tr.bank, tr.vae_bank, tr.text_bank)
    assert [s[0] is b.flat for s, b in zip(tr.opt.segments, banks)] == [True] * 3
    before = [b.flat.clone() for b in banks]
    tr.train_step(w.batch, **FIXED)
    by_hand = sum(float(b.flat_grad.double().pow(2).sum()) for b in banks)
    assert abs(float(tr.opt.gnorm_sq) - by_hand) < 1e-5 * by_hand
    assert all(float(b.flat_grad.abs().max()) > 0 for b in banks)
    assert all(not torch.equal(b.flat, x) for b, x in zip(banks, before)) and tr.opt.counters.tolist() == [1, 0]
    # a non-finite gradient anywhere skips all of them
    before = [b.flat.clone() for b in banks]
    for poisoned in banks:
        tr._forward_backward(w.batch, FIXED)
        poisoned.flat_grad[3] = float("inf")
        tr._apply_updates()
        assert all(torch.equal(b.flat, x) for b, x in zip(banks, before)), "a segment moved under a non-finite norm"
    assert tr.opt.counters.tolist() == [1, 3]


def test_full_finetuning_with_the_tuned_tower(tune_sim):
    w = make_world(F32, tune_sim, full=True)
    tr = w.tr
    assert isinstance(tr.bank, UNetBank) and len(tr.opt.segments) == 2
    t0, u0, e0 = tr.text_bank.flat.clone(), tr.bank.flat.clone(), tr.text_bank.epoch
    tr.train_step(w.batch, **FIXED)
    by_hand = float(tr.bank.flat_grad.double().pow(2).sum() + tr.text_bank.flat_grad.double().pow(2).sum())
    assert abs(float(tr.opt.gnorm_sq) - by_hand) < 1e-5 * by_hand
    assert not torch.equal(tr.text_bank.flat, t0) and not torch.equal(tr.bank.flat, u0)
    assert tr.text_bank._fresh and tr.text_bank.epoch > e0  # refreshed behind the update


@pytest.mark.gpu
def test_8bit_adam_takes_the_text_segment(hip):
    """use_8bit_adam runs on the HIP kernels only: the text bank is one more 8-bit segment"""
    w = make_world(torch.bfloat16, hip, use_8bit_adam=True)
    tr = w.tr
    t0 = tr.text_bank.flat.clone()
    tr.train_step(w.batch, **FIXED)
    torch.cuda.synchronize()
    assert tr.opt.seg8[-1] and tr.opt.counters.tolist() == [1, 0]
    assert not torch.equal(tr.text_bank.flat, t0) and bool(torch.isfinite(tr.text_bank.flat).all())


@pytest.mark.parametrize("dtype", [F32, torch.bfloat16], ids=["fp32", "bf16"])
def test_gradient_checkpointing_gives_the_same_bits(tune_sim, dtype):
    """as tests/test_recompute.py: the baseline is the plain step with the text key / value sharing off"""
    plain, ckpt = make_world(dtype, tune_sim), make_world(dtype, tune_sim, gradient_checkpointing=True)
    plain.tr.pipe.share_text_kv = False
    assert ckpt.tr.pipe.gradient_checkpointing and not plain.tr.pipe.gradient_checkpointing
    for step in range(2):
        la, lb = plain.tr.train_step(plain.batch, **FIXED), ckpt.tr.train_step(ckpt.batch, **FIXED)
        for k in ("Blip", "G_loss", "D_loss", "step_loss", "grad_norm_sq"):
            assert torch.equal(la[k], lb[k]), (step, k)
        for x in ("bank", "text_bank"):
            assert torch.equal(getattr(plain.tr, x).flat_grad, getattr(ckpt.tr, x).flat_grad), (step, x)
            assert torch.equal(getattr(plain.tr, x).flat, getattr(ckpt.tr, x).flat), (step, x)
    assert float(ckpt.tr.text_bank.flat_grad.abs().max()) > 0


def test_accumulation_over_two_micro_steps_is_the_mean_of_two_gradients(tune_sim):
    a, b, acc = make_world(F32, tune_sim), make_world(F32, tune_sim), make_world(F32, tune_sim, gradient_accumulation_steps=2)
    g = torch.Generator().manual_seed(99)
    second = dict(acc.batch, latents=torch.randn(BS, 4, 8, 8, generator=g))
    a.tr._forward_backward(a.batch, FIXED)
    b.tr._forward_backward(second, FIXED)
    ops.join_side_streams()
    start = acc.tr.text_bank.flat.clone()
    acc.tr.train_step(acc.batch, **FIXED)
    assert torch.equal(acc.tr.text_bank.flat, start) and acc.tr.opt.counters.tolist() == [0, 0]  # the window is open
    acc.tr.train_step(second, **FIXED)
    assert not torch.equal(acc.tr.text_bank.flat, start) and acc.tr.opt.counters.tolist() == [1, 0]
    ga, gb = a.tr.text_bank.flat_grad, b.tr.text_bank.flat_grad
    assert rel_l2(gb, ga) > 1e-3, "the two micro-steps have the same gradient: the case shows nothing"
    mean = (ga.double() + gb.double()) / 2
    # halving the loss is exact in binary floating point, the two sums differ by the rounding of one fp32 addition per element
    assert rel_l2(acc.tr.text_bank.flat_grad, mean) < 1e-6
    for name in (TOK_NAME, POS_NAME):
        v = lambda buf: acc.tr.text_bank._view(buf, name)
        assert rel_l2(v(acc.tr.text_bank.flat_grad), v(mean)) < 1e-6, name


# ---- runners and errors ----------------------------------------------------------------------------------------------------------
def test_graph_runners_decline_the_flag(tune_sim):
    w, e = make_world(F32, tune_sim), make_world(F32, tune_sim)
    assert not GraphedStep(w.tr).supported(w.batch)
    stepper = SegmentedStep(w.tr, dry=True)  # dry: the segment hooks run wherever the stepper does not decline
    a = stepper(w.batch, **FIXED)
    b = e.tr.train_step(e.batch, **FIXED)
    assert not stepper.unet_segs and stepper.head_seg is None and stepper.failed is None
    assert torch.equal(a["step_loss"], b["step_loss"]) and torch.equal(w.tr.text_bank.flat, e.tr.text_bank.flat)
    graphed = GraphedStep(w.tr)
    graphed(w.batch, **FIXED)
    assert not graphed.graphs and graphed.failed is None


def test_every_mismatch_raises(tune_sim):
    w = make_world(F32, tune_sim)
    tr = w.tr
    parts = (tr.pipe, tr.bank, tr.blip, tr.D)
    on, off = w.cfg, dataclasses.replace(w.cfg, tune_text_encoder=False)
    with pytest.raises(ValueError, match="tune_text_encoder"):
        CoMatTrainer(*parts, on)
    with pytest.raises(ValueError, match="text_encoder"):
        CoMatTrainer(*parts, off, text_encoder=tr.text_encoder, text_bank=tr.text_bank)
    with pytest.raises(ValueError, match="tune_text_encoder.*text_bank"):
        CoMatTrainer(*parts, on, text_encoder=tr.text_encoder)
    with pytest.raises(ValueError, match="tune_text_encoder.*text_encoder"):
        CoMatTrainer(*parts, on, text_bank=tr.text_bank)
    other = ClipTextBank(CLIP, hf_model().state_dict(), F32, tune_sim)
    with pytest.raises(ValueError, match="tune_text_encoder.*text_bank"):
        CoMatTrainer(*parts, on, text_encoder=tr.text_encoder, text_bank=other)
    # the other flag's objects under this flag, and the reverse
    from test_clip_text import lora_factors
    lbank = ClipLoRABank(CLIP, lora_factors(4, seed=3), F32, tune_sim)
    lenc = ClipTextEncoder(CLIP, hf_model().state_dict(), F32, tune_sim, lbank)
    with pytest.raises(ValueError, match="tune_text_encoder.*ClipLoRABank"):
        CoMatTrainer(*parts, on, text_encoder=lenc, text_bank=lbank)
    with pytest.raises(ValueError, match="train_text_encoder_lora.*ClipTextBank"):
        CoMatTrainer(*parts, dataclasses.replace(off, train_text_encoder_lora=True), text_encoder=tr.text_encoder, text_bank=tr.text_bank)
    with pytest.raises(ValueError, match="tune_text_encoder.*train_text_encoder_lora.*not built"):
        StepConfig(tune_text_encoder=True, train_text_encoder_lora=True)
    emb = torch.zeros(BS, L, CLIP.hidden)
    with pytest.raises(ValueError, match="tune_text_encoder.*prompt_embeds"):
        tr.train_step(dict(w.batch, prompt_embeds=emb, negative_prompt_embeds=emb), **FIXED)
    with pytest.raises(ValueError, match="tune_text_encoder.*null_input_ids"):
        tr.train_step({k: v for k, v in w.batch.items() if k != "null_input_ids"}, **FIXED)
    with pytest.raises(ValueError, match="tune_text_encoder.*prompt_input_ids"):
        tr.train_step({k: v for k, v in w.batch.items() if k != "prompt_input_ids"}, **FIXED)


# ---- checkpoint ------------------------------------------------------------------------------------------------------------------
def test_text_encoder_pt_round_trips_and_resumes_bit_for_bit(tune_sim, tmp_path):
    w = make_world(F32, tune_sim)
    tr = w.tr
    tr.train_step(w.batch, **FIXED)
    d = str(tmp_path / "ck")
    checkpoint.save_checkpoint(d, tr.bank, tr.D, optim=dict(G=tr.opt, D=tr.opt_D), text=tr.text_bank)
    assert sorted(os.listdir(d)) == sorted(["D_sd", checkpoint.LORA_WEIGHT_NAME, "optim_state.pt", "text_encoder.pt"])
    sd = torch.load(os.path.join(d, checkpoint.TEXT_WEIGHT_NAME))
    src = {k: v for k, v in hf_model().state_dict().items() if v.is_floating_point() and not k.endswith("position_ids")}
    assert set(sd) == set(src) and all(v.dtype == torch.float32 and v.shape == src[k].shape for k, v in sd.items())
    assert all(torch.equal(sd[k], tr.text_bank.state_dict()[k]) for k in sd) and any(not torch.equal(sd[k], src[k]) for k in sd)
    f = make_world(F32, tune_sim)
    assert not torch.equal(f.tr.text_bank.flat, tr.text_bank.flat)
    checkpoint.load_checkpoint(d, f.tr.bank, f.tr.D, optim=dict(G=f.tr.opt, D=f.tr.opt_D), text=f.tr.text_bank)
    assert torch.equal(f.tr.text_bank.flat, tr.text_bank.flat) and torch.equal(f.tr.bank.flat, tr.bank.flat)
    assert len(f.tr.opt.m) == 2 and all(torch.equal(x, y) for x, y in zip(f.tr.opt.m + f.tr.opt.v, tr.opt.m + tr.opt.v))
    la, lb = tr.train_step(w.batch, **FIXED), f.tr.train_step(f.batch, **FIXED)
    assert torch.equal(la["step_loss"], lb["step_loss"])
    assert torch.equal(f.tr.text_bank.flat, tr.text_bank.flat) and torch.equal(f.tr.bank.flat, tr.bank.flat)
    # a file that lacks an entry, or holds another shape, is refused by name
    key = next(k for k in sd if k.endswith("final_layer_norm.bias"))
    torch.save({k: v for k, v in sd.items() if k != key}, os.path.join(d, checkpoint.TEXT_WEIGHT_NAME))
    with pytest.raises(KeyError, match="final_layer_norm.bias"):
        checkpoint.load_checkpoint(d, f.tr.bank, f.tr.D, text=f.tr.text_bank)
    torch.save(dict(sd, **{key: torch.zeros(3)}), os.path.join(d, checkpoint.TEXT_WEIGHT_NAME))
    with pytest.raises(ValueError, match="final_layer_norm.bias"):
        checkpoint.load_checkpoint(d, f.tr.bank, f.tr.D, text=f.tr.text_bank)


def test_a_checkpoint_written_without_the_flag_is_unchanged(tune_sim, tmp_path):
    w, off = make_world(F32, tune_sim), make_world(F32, tune_sim, flag=False)
    a, b, c = (str(tmp_path / n) for n in "abc")
    checkpoint.save_checkpoint(a, off.tr.bank, off.tr.D)
    checkpoint.save_checkpoint(b, off.tr.bank, off.tr.D, text=None)
    checkpoint.save_checkpoint(c, w.tr.bank, w.tr.D, text=w.tr.text_bank)

    def files(d):
        return {os.path.relpath(os.path.join(r, f), d): open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(d) for f in fs}
    assert files(a) == files(b) and "text_encoder.pt" not in files(a)
    # with the flag: the same files (the worlds hold the same LoRA factors) and text_encoder.pt beside them
    assert {k: v for k, v in files(c).items() if k != "text_encoder.pt"} == files(a) and "text_encoder.pt" in files(c)


# ---- flag off --------------------------------------------------------------------------------------------------------------------
class _Recorded:
    """a kernel backend that notes the name of every entry point called through it"""

    def __init__(self, inner):
        self._inner, self.calls = inner, []

    def __getattr__(self, name):
        fn = getattr(self._inner, name)
        if not callable(fn):
            return fn

        def call(*a, **kw):
            self.calls.append(name)
            return fn(*a, **kw)
        return call


@pytest.mark.parametrize("dtype", [F32, torch.bfloat16], ids=["fp32", "bf16"])
def test_flag_off_is_the_step_of_a_trainer_without_text_objects(tune_sim, dtype):
    """flag off: the launches and the bits of a trainer built without any text argument; neither new entry point is called"""
    a, b = make_world(dtype, tune_sim, flag=False), make_world(dtype, tune_sim, flag=False)
    assert not a.cfg.tune_text_encoder and a.cfg.text_flag is None
    b.tr = CoMatTrainer(b.tr.pipe, b.tr.bank, b.tr.blip, b.tr.D, dataclasses.replace(b.cfg, tune_text_encoder=False), seed=0,
                        text_encoder=None, text_bank=None)
    inner = ops.kernels()
    runs = []
    for w in (a, b):
        rec = _Recorded(inner)
        ops.set_kernel_backend(rec)
        try:
            logs = [w.tr.train_step(w.batch, **FIXED) for _ in range(2)]
        finally:
            ops.set_kernel_backend(inner)
        runs.append((rec.calls, logs))
    assert runs[0][0] == runs[1][0] and len(runs[0][0]) > 100
    assert not {"embed_fwd", "embed_grad"} & set(runs[0][0])
    assert a.tr.text_bank is None and len(a.tr.opt.segments) == 1
    for la, lb in zip(runs[0][1], runs[1][1]):
        for k in ("Blip", "G_loss", "D_loss", "step_loss", "grad_norm_sq"):
            assert torch.equal(la[k], lb[k]), k
    assert torch.equal(a.tr.bank.flat, b.tr.bank.flat) and torch.equal(a.tr.D.bank.flat, b.tr.D.bank.flat)
    # and with the flag on the recorded step does call them: one forward, two gradient launches per step
    on = make_world(dtype, tune_sim)
    rec = _Recorded(ops.kernels())
    ops.set_kernel_backend(rec)
    try:
        on.tr.train_step(on.batch, **FIXED)
    finally:
        ops.set_kernel_backend(rec._inner)
    assert rec.calls.count("embed_fwd") == 1 and rec.calls.count("embed_grad") == 2
