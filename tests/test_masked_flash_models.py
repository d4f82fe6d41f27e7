"""The fused masked attention inside the models that carry a mask: the CLIP text tower (causal) and BLIP's decoder (causal +
key padding), the process-wide switch on against the switch off, and one tiny C2-style step under
StepConfig(fused_masked_attention=True) run eagerly, from segment graphs and from the whole-step graph.

Bounds.  Switch on and switch off are two evaluations of the same function, each held to a reference by its own file; the
difference between them is held here to the bound that file sets against its reference, taken from there: test_clip_text.py's
FP32_BOUND / BF16_LORA_OUT_BOUND / BF16_GRAD_BOUND (relative L2 per tensor), test_blip.py's helpers.check with its factors (1 and 3
on gradients, times 3 in bf16).

Head dims.  The tiny CLIP tower has the real head dim, 64.  The tiny BLIP decoder has head dim 12: fp32 takes the fused kernels
(multiples of 4), bf16 does not (multiples of 8) and must return the same bits with the switch on; a decoder of width 32 (head dim
16) runs the bf16 kernels."""
import dataclasses

import pytest
import torch

from comat_amd import _hip, config, ops, weights
from comat_amd.blip import Blip
from comat_amd.clip import ClipLoRABank, ClipTextEncoder
from comat_amd.config import TINY_CLIP_TEXT as CFG
from helpers import check
from masked_attn_sim import MaskedAttnSimKernels, masked_dev  # noqa: F401 - masked_dev is a fixture

F32, BF16 = torch.float32, torch.bfloat16
CLIP_FP32_BOUND, CLIP_BF16_OUT_BOUND, CLIP_BF16_GRAD_BOUND = 1e-3, 1.59e-2, 5.48e-2  # test_clip_text.py


def rel(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((got - ref).norm() / ref.norm())


@pytest.fixture
def masked_calls(masked_dev, monkeypatch):
    """() -> (forward calls, backward calls) of the masked entry points so far, on either leg"""
    k = ops.kernels()
    if isinstance(k, MaskedAttnSimKernels):
        return lambda: (k.masked_calls["fwd"], k.masked_calls["bwd"])
    n = dict(fwd=0, bwd=0)
    fwd, bwd = _hip.flash_attn_masked_fwd, _hip.flash_attn_masked_bwd

    def cf(*a):
        n["fwd"] += 1
        return fwd(*a)

    def cb(*a):
        n["bwd"] += 1
        return bwd(*a)
    monkeypatch.setattr(_hip, "flash_attn_masked_fwd", cf)
    monkeypatch.setattr(_hip, "flash_attn_masked_bwd", cb)
    return lambda: (n["fwd"], n["bwd"])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_clip_text_tower_switch_on_against_off(masked_dev, masked_calls, dtype):
    """ClipTextEncoder of the tiny config with LoRA factors, B = 2, L = 77: outputs and factor gradients"""
    from comat_amd.weights import make_clip_text_weights
    B, L, rank = 2, 77, 4
    g = torch.Generator().manual_seed(3)
    q = lambda t: t.to(BF16).float()
    sd = {k: (q(v) if v.is_floating_point() else v) for k, v in make_clip_text_weights(CFG, perturb_norms=True).items()}
    # factors that matter as much as the weights they sit on, as test_clip_text.lora_factors draws them (up factors are not zero)
    fsd = {k: q(torch.randn(v.shape, generator=g) * CFG.hidden ** -0.5 if k.endswith("up.weight") else v * rank ** 0.5)
           for k, v in ClipLoRABank.init(CFG, rank, g).items()}
    ids = torch.randint(3, CFG.vocab_size - 2, (B, L), generator=g)
    ids[0, 40:] = CFG.vocab_size - 1
    gout = q(torch.randn(B * L, CFG.hidden, generator=g))
    res = {}
    for on in (False, True):
        ops.set_fused_masked_attention(on)
        bank = ClipLoRABank(CFG, fsd, dtype, masked_dev)
        enc = ClipTextEncoder(CFG, sd, dtype, masked_dev, bank)
        bank.zero_grad()
        before = masked_calls()
        out = enc(ids)
        out.backward(gout.to(device=masked_dev, dtype=dtype))
        if masked_dev.type == "cuda":
            torch.cuda.synchronize()
        after = masked_calls()
        assert (after[0] - before[0], after[1] - before[1]) == ((CFG.layers, CFG.layers) if on else (0, 0))
        res[on] = (out.detach().clone(), {n: bank.params[n].grad.detach().clone() for n in bank.names})
    out_bound, grad_bound = (CLIP_FP32_BOUND, CLIP_FP32_BOUND) if dtype == F32 else (CLIP_BF16_OUT_BOUND, CLIP_BF16_GRAD_BOUND)
    e = rel(res[True][0], res[False][0])
    print(f"clip tower, fused against materialised, {dtype}: outputs rel {e:.3e}")
    assert e < out_bound
    worst = max(rel(res[True][1][n], res[False][1][n]) for n in res[True][1] if float(res[False][1][n].norm()) > 0)
    print(f"clip tower, fused against materialised, {dtype}: worst factor-gradient rel {worst:.3e}")
    assert worst < grad_bound


@pytest.mark.parametrize("dtype,t_hidden", [(F32, 24), (BF16, 24), (F32, 32), (BF16, 32)], ids=["f32-d12", "bf16-d12", "f32-d16", "bf16-d16"])
def test_blip_decoder_switch_on_against_off(masked_dev, masked_calls, dtype, t_hidden):
    """Blip.decoder_logits under a right-padded attention_mask: logits and the gradient of the image embeddings"""
    cfg = dataclasses.replace(config.TINY_BLIP, t_hidden=t_hidden)
    bsd = {k: v.to(dtype).float() for k, v in weights.make_blip_weights(cfg, perturb_norms=True).items()}
    model = Blip(cfg, bsd, dtype, masked_dev)
    B, T, N = 3, 9, 17
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(1, cfg.vocab_size, (B, T), generator=g)
    ids[1, 7:] = 0
    ids[2, 3:] = 0
    am = (ids != 0).long()
    emb = torch.randn(B * N, cfg.v_hidden, generator=g).to(dtype)
    gout = torch.randn(B * T, cfg.vocab_size, generator=g).to(dtype)
    fused = ops.flash_ok(cfg.t_hidden // cfg.t_heads, dtype)
    assert fused == (not (dtype == BF16 and t_hidden == 24))
    res = {}
    for on in (False, True):
        ops.set_fused_masked_attention(on)
        e = emb.to(masked_dev).clone().requires_grad_(True)
        before = masked_calls()
        logits = model.decoder_logits(ids, am, e, B, N)
        logits.backward(gout.to(masked_dev))
        if masked_dev.type == "cuda":
            torch.cuda.synchronize()
        after = masked_calls()
        n = cfg.t_layers if on and fused else 0
        # (the first layer's self-attention sits on frozen embeddings alone: autograd never asks for its backward)
        assert (after[0] - before[0], after[1] - before[1]) == (n, max(n - 1, 0))
        res[on] = (logits.detach().clone(), e.grad.detach().clone())
    if not fused:
        assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
        return
    f = 1.0 if dtype == F32 else 3.0
    check(res[True][0], res[False][0], dtype, "decoder logits, fused against materialised", factor=f)
    check(res[True][1], res[False][1], dtype, "d logits / d image embeddings, fused against materialised", factor=3 * f)


@pytest.mark.gpu
def test_step_with_the_flag_replays_bit_identically(hip, monkeypatch):
    """one tiny C2-style world (fp32: the tiny BLIP decoder's head dim 12 takes the fused masked kernels) under
    StepConfig(fused_masked_attention=True): eager steps, SegmentedStep replays and GraphedStep replays give the same bits - losses,
    parameters of G and D, optimizer moments - and the masked kernels are what ran"""
    from comat_amd.segments import SegmentedStep
    from comat_amd.step import CoMatTrainer, GraphedStep
    from test_segments import vary
    from test_step import make_world
    dtype = F32
    n = dict(fwd=0, bwd=0)
    fwd, bwd = _hip.flash_attn_masked_fwd, _hip.flash_attn_masked_bwd
    monkeypatch.setattr(_hip, "flash_attn_masked_fwd", lambda *a: (n.__setitem__("fwd", n["fwd"] + 1), fwd(*a))[1])
    monkeypatch.setattr(_hip, "flash_attn_masked_bwd", lambda *a: (n.__setitem__("bwd", n["bwd"] + 1), bwd(*a))[1])
    worlds = [make_world(dtype, hip, False) for _ in range(4)]
    batch = worlds[0][1]
    try:
        trs = [CoMatTrainer(t.pipe, t.bank, t.blip, t.D, dataclasses.replace(cfg, fused_masked_attention=True), seed=0)
               for cfg, _, _, t in worlds]
        assert ops.fused_masked_attention() and all(t.fused_masked_attention for t in trs)
        tr_e, tr_s, tr_e2, tr_w = trs
        tr_e.pipe.share_text_kv = False  # replayed segments project the text keys / values once per call
        st, gs = SegmentedStep(tr_s), GraphedStep(tr_w)
        gen = torch.Generator().manual_seed(11)
        for it, (ts, crop) in enumerate([([1, 2], (1, 0, 63, 63)), ([1, 2], (0, 1, 63, 63)), ([1, 2], (1, 1, 63, 63))]):
            b = vary(batch, gen, dtype)
            le, lg = tr_e.train_step(b, training_steps=ts, crop=crop), st(b, training_steps=ts, crop=crop)
            torch.cuda.synchronize()
            for k in ("step_loss", "Blip", "G_loss", "D_loss"):
                assert torch.equal(le[k], lg[k]), f"segments, step {it}: {k}"
            assert torch.equal(tr_e.bank.flat, tr_s.bank.flat) and torch.equal(tr_e.D.bank.flat, tr_s.D.bank.flat)
            assert torch.equal(tr_e.opt.m[0], tr_s.opt.m[0]) and torch.equal(tr_e.opt.v[0], tr_s.opt.v[0])
        assert st.failed is None and st.stats()["replays"] >= 2
        assert n["fwd"] >= config.TINY_BLIP.t_layers and n["bwd"] >= config.TINY_BLIP.t_layers
        for it in range(3):
            b = vary(batch, gen, dtype)
            kw = dict(training_steps=[0, 1, 2], crop=(it % 2, 1, 63, 63))
            le, lg = tr_e2.train_step(b, **kw), gs(b, **kw)
            torch.cuda.synchronize()
            assert gs.failed is None, gs.failed
            for k in ("step_loss", "Blip", "G_loss", "D_loss"):
                assert torch.equal(le[k], lg[k]), f"whole-step graph, step {it}: {k}"
            assert torch.equal(tr_e2.bank.flat, tr_w.bank.flat) and torch.equal(tr_e2.D.bank.flat, tr_w.D.bank.flat)
        assert len(gs.graphs) == 1
    finally:
        ops.set_fused_masked_attention(False)
