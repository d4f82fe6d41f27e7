"""Gradient checkpointing of the trained UNet calls (comat_amd/recompute.py, StepConfig.gradient_checkpointing): the step with
recomputation equals the plain step bit for bit - eager, from segment graphs and from the whole-step graph, in every sampler
mode and under the fp8 forward - runs K more UNet forwards, keeps one call's activations instead of K, and needs one segment
per variant in one pool instead of one per (slot, variant) in K pools.

The baseline of every comparison is the plain step with `pipe.share_text_kv = False`: a checkpointed call projects its own text
keys / values (as a replayed segment does), so the plain step must too for the LoRA gradients to be summed in the same order."""
import dataclasses

import numpy as np
import pytest
import torch

from comat_amd import config, ops, weights
from comat_amd.segments import SegmentedStep
from comat_amd.step import CoMatTrainer, GraphedStep, StepConfig
from comat_amd.unet import UNet
from helpers import fp8_state
from test_segments import PLAN, run_plan, vary
from test_step import make_world

DTYPES = [torch.float32, torch.bfloat16]


def _with_flag(tr, flag=True, **more):
    """the same world under another StepConfig (the trainer sets the pipeline's attribute from it)"""
    cfg = dataclasses.replace(tr.cfg, gradient_checkpointing=flag, **more)
    return CoMatTrainer(tr.pipe, tr.bank, tr.blip, tr.D, cfg, seed=0)


def _pair(dev, dtype, attrcon, **kw):
    """(batch, plain trainer with the text key / value sharing off, checkpointed trainer) on two identical worlds"""
    _, batch, _, tr_p = make_world(dtype, dev, attrcon, **kw)
    _, _, _, tr_c = make_world(dtype, dev, attrcon, **kw)
    tr_p.pipe.share_text_kv = False
    tr_c = _with_flag(tr_c)
    assert tr_c.pipe.gradient_checkpointing and not tr_p.pipe.gradient_checkpointing
    return batch, tr_p, tr_c


class _Eager:
    """a trainer behind the call convention of a stepper (test_segments.run_plan)"""

    def __init__(self, tr):
        self.tr = tr

    def __call__(self, batch, **kw):
        return self.tr.train_step(batch, **kw)


def _sdxl_world(dev, dtype):
    """the world of tests/test_segments.py::test_segmented_step_sdxl_matches_eager -> (batch, make_trainer(flag))"""
    from comat_amd.blip import Blip
    from comat_amd.gan import D_sd
    from comat_amd.pipeline import TrainableSDXLPipeline
    from comat_amd.unet import LoRABank, VAEDecoder
    ucfg = config.TINY_SDXL_UNET
    vcfg = dataclasses.replace(config.TINY_VAE, scaling_factor=0.13025)
    usd, vsd = weights.make_unet_weights(ucfg, perturb_norms=True), weights.make_vae_weights(vcfg, perturb_norms=True)
    lsd, bsd = weights.make_lora_weights(ucfg), weights.make_blip_weights(config.TINY_BLIP, perturb_norms=True)
    dsd, dl = weights.make_unet_weights(config.TINY_UNET, seed=77), weights.make_lora_weights(config.TINY_UNET, seed=78)
    g = torch.Generator().manual_seed(6)
    r = lambda *s: torch.randn(*s, generator=g)
    hw, hb = r(4) * 0.5, r(1) * 0.1
    cfg = StepConfig(resolution=64, total_step=3, K=2, gan_loss=True, attrcon=True, attrcon_train_steps=1,
                     train_layer_ls=("mid_2", "up_2", "up_4"), attn_reses=(8, 4, 2), lr=1e-2, lr_D=1e-2,
                     mask_token_loss_weight=0.5, mask_pixel_loss_weight=0.1)
    bs, L, T = 1, 7, 9
    ids = torch.randint(1, config.TINY_BLIP.vocab_size, (bs, T), generator=g)
    m = np.zeros((2, 64, 64), dtype=bool)
    m[0, 5:30, 8:40] = True
    m[1, 34:60, 20:64] = True
    batch = dict(prompt_embeds=r(bs, L, ucfg.cross_attention_dim), negative_prompt_embeds=r(bs, L, ucfg.cross_attention_dim),
                 pooled_prompt_embeds=r(bs, ucfg.pooled_dim), negative_pooled_prompt_embeds=r(bs, ucfg.pooled_dim),
                 add_time_ids=(64, 64, 0, 0, 64, 64), gan_null_embeds=r(bs, L, config.TINY_UNET.cross_attention_dim),
                 latents=r(bs, 4, 8, 8), noises=[r(bs, 4, 8, 8) for _ in range(3)], real_latents=r(bs, 4, 8, 8),
                 blip_input_ids=ids, blip_attention_mask=torch.ones_like(ids), masks=[m], attributes=[[[2, 3], [5]]])

    def world(flag):
        bank = LoRABank(ucfg, lsd, dtype, dev)
        pipe = TrainableSDXLPipeline(UNet(ucfg, usd, dtype, dev, bank), VAEDecoder(vcfg, vsd, dtype, dev))
        dbank = LoRABank(config.TINY_UNET, dl, dtype, dev)
        disc = D_sd(UNet(config.TINY_UNET, dsd, dtype, dev, dbank), dbank, hw, hb)
        return CoMatTrainer(pipe, bank, Blip(config.TINY_BLIP, bsd, dtype, dev), disc,
                            dataclasses.replace(cfg, gradient_checkpointing=flag), seed=0)
    return batch, world


def _exact(a, b):
    return torch.allclose(a.float(), b.float(), rtol=0, atol=0)


# ---- CPU: the host logic through the ABI simulator --------------------------------------------------------------------------
@pytest.mark.parametrize("attrcon", [False, True])
def test_checkpointed_step_equals_the_plain_step(sim, attrcon):
    """1. six steps of PLAN: every logged loss term, the G and D LoRA parameters, the head and the Adam moments, atol = 0"""
    batch, tr_p, tr_c = _pair(sim, torch.float32, attrcon)
    run_plan(tr_p, _Eager(tr_c), batch, torch.float32, attrcon, _exact)


def _count_forwards(tr):
    """a counting wrapper on the generator UNet's `_forward` -> the list it counts into"""
    n = []
    unet, real = tr.pipe.unet, tr.pipe.unet._forward
    unet._forward = lambda *a, **kw: (n.append(torch.is_grad_enabled()), real(*a, **kw))[1]
    return n


def test_k_more_forwards_per_step_and_none_without_the_flag(sim):
    """2. N = 3 denoise steps, K = 2 trained: 3 forwards plain, 3 + 2 checkpointed; the 2 more run with recording, inside the
    backward pass; one trained call (double_laststep) costs one more"""
    batch, tr_p, tr_c = _pair(sim, torch.float32, False)
    n_p, n_c = _count_forwards(tr_p), _count_forwards(tr_c)
    kw = dict(training_steps=[0, 2], crop=(0, 1, 63, 63))
    for it in range(2):
        tr_p.train_step(batch, **kw)
        tr_c.train_step(batch, **kw)
        assert len(n_p) == 3 * (it + 1) and len(n_c) == 5 * (it + 1), (len(n_p), len(n_c))
    assert n_c[:5] == [True, False, True, True, True] and n_p[:3] == [True, False, True]
    tr_1 = _with_flag(make_world(torch.float32, sim, False)[3], K=1)
    n_1 = _count_forwards(tr_1)
    tr_1.train_step(batch, training_steps=[1], crop=(0, 1, 63, 63))
    assert len(n_1) == 4


@pytest.mark.parametrize("attrcon", [False, True])
def test_segment_hooks_dry_under_the_flag(sim, attrcon):
    """3. SegmentedStep(dry=True) under the flag equals the eager checkpointed step, and its U-segment keys carry no slot"""
    _, batch, _, tr_e = make_world(torch.float32, sim, attrcon)
    _, _, _, tr_g = make_world(torch.float32, sim, attrcon)
    tr_e, tr_g = _with_flag(tr_e), _with_flag(tr_g)
    st = SegmentedStep(tr_g, dry=True)
    run_plan(tr_e, st, batch, torch.float32, attrcon, _exact)
    keys = list(st._map_counts)
    assert keys and all(isinstance(k[0], tuple) and len(k) == 7 for k in keys), keys  # (capture places, wanted, B, H, W, L, grad)
    # ... where the plain stepper's start with the slot
    _, _, _, tr_s = make_world(torch.float32, sim, attrcon)
    st_s = SegmentedStep(tr_s, dry=True)
    st_s(batch, training_steps=[1, 2], crop=(0, 0, 63, 63), **(dict(attrcon_steps=[2]) if attrcon else {}))
    assert sorted(k[0] for k in st_s._map_counts) == [0, 1] and all(len(k) == 8 for k in st_s._map_counts)


def test_environment_override_and_default(sim, monkeypatch):
    """4. a default StepConfig has the feature off; COMAT_GRADIENT_CHECKPOINTING=1 switches it on where the config leaves it off"""
    assert StepConfig().gradient_checkpointing is False and StepConfig.sdxl().gradient_checkpointing is False
    monkeypatch.delenv("COMAT_GRADIENT_CHECKPOINTING", raising=False)
    _, batch, _, tr = make_world(torch.float32, sim, False)
    assert not tr.gradient_checkpointing and not tr.pipe.gradient_checkpointing
    monkeypatch.setenv("COMAT_GRADIENT_CHECKPOINTING", "1")
    tr_on = _with_flag(tr, False)
    assert tr_on.gradient_checkpointing and tr_on.pipe.gradient_checkpointing
    n = _count_forwards(tr_on)
    tr_on.train_step(batch, training_steps=[1, 2], crop=(0, 0, 63, 63))
    assert len(n) == 5
    monkeypatch.setenv("COMAT_GRADIENT_CHECKPOINTING", "0")
    assert not _with_flag(tr, False).gradient_checkpointing and _with_flag(tr, True).gradient_checkpointing


def test_the_latch_of_the_side_stream_join_is_dropped_after_the_step(sim):
    """the nested backward queues weight-gradient groups and the join: when `.backward()` has returned, nothing is left
    queued and the latch is free for the next backward"""
    from comat_amd import streams
    batch, _, tr_c = _pair(sim, torch.float32, False)
    tr_c._forward_backward(batch, dict(training_steps=[1, 2], crop=(0, 0, 63, 63)))
    assert not streams._join_queued and not any(q.items for q in streams._ttq.values()) and not streams._side_keep
    assert float(tr_c.bank.flat_grad.abs().max()) > 0


# ---- GPU: the library -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("attrcon", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_checkpointed_step_equals_the_plain_step_on_the_library(hip, dtype, attrcon):
    """5. test 1 through libcomat_hip.so, torch.equal, SD1.5 layout"""
    batch, tr_p, tr_c = _pair(hip, dtype, attrcon)
    run_plan(tr_p, _Eager(tr_c), batch, dtype, attrcon, torch.equal)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_checkpointed_sdxl_step_equals_the_plain_step_on_the_library(hip, dtype):
    """5. SDXL layout: no input of a trained call requires grad (the outputs hang on the anchor alone), attribute concentration"""
    batch, world = _sdxl_world(hip, dtype)
    tr_p, tr_c = world(False), world(True)
    tr_p.pipe.share_text_kv = False
    run_plan(tr_p, _Eager(tr_c), batch, dtype, True, torch.equal)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["early_exit", "fast_training", "double_laststep", "guidance_off"])
def test_sampler_modes_under_the_flag(hip, mode):
    """6. each of the sampler's other modes for one step, plain against checkpointed"""
    from test_sampler_modes import MODES, _worlds
    dtype = torch.bfloat16
    batch, tr_p, tr_c = _worlds(hip, dtype, mode)
    assert set(MODES) == {"early_exit", "fast_training", "double_laststep", "guidance_off"}
    tr_p.pipe.share_text_kv = False
    tr_c = _with_flag(tr_c)
    b = vary(batch, torch.Generator().manual_seed(11), dtype)
    ts, crop, _ = PLAN[0]
    lp, lc = tr_p.train_step(b, training_steps=ts, crop=crop), tr_c.train_step(b, training_steps=ts, crop=crop)
    torch.cuda.synchronize()
    for k in ("step_loss", "Blip", "G_loss", "D_loss"):
        assert torch.equal(lp[k], lc[k]), f"{mode}: {k} {float(lp[k])} vs {float(lc[k])}"
    assert torch.isfinite(lp["step_loss"]) and float(tr_p.bank.flat_grad.abs().max()) > 0
    assert torch.equal(tr_p.bank.flat_grad, tr_c.bank.flat_grad), f"{mode}: LoRA gradients differ"
    assert torch.equal(tr_p.bank.flat, tr_c.bank.flat) and torch.equal(tr_p.D.bank.flat, tr_c.D.bank.flat)


def _segments_against_eager(tr_e, tr_g, batch, dtype):
    """-> (stepper, the variants its trained calls met, the number of those calls)"""
    st = SegmentedStep(tr_g)
    met, calls, hook = set(), [0], st._run_unet

    def spy(slot, xin, B, H, W, t, ctx, L, cap, added, wanted=None):
        met.add((tuple(cap), bool(xin.requires_grad)))
        calls[0] += 1
        return hook(slot, xin, B, H, W, t, ctx, L, cap, added, wanted)
    st._run_unet = spy
    run_plan(tr_e, st, batch, dtype, True, torch.equal)
    assert st.failed is None, st.failed
    return st, met, calls[0]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["sd15", "sdxl"])
def test_segmented_step_under_the_flag(hip, layout):
    """7. segment graphs under the flag equal the eager checkpointed trainer over PLAN; one pool; one U segment per variant met
    (SDXL: the input never requires grad, so the two slots of a step share their variants: 2 segments where the plain stepper
    holds 4); `replays` counts the forward replay of every call and the one more inside its backward"""
    dtype = torch.bfloat16
    if layout == "sd15":
        _, batch, _, tr_e = make_world(dtype, hip, True)
        _, _, _, tr_g = make_world(dtype, hip, True)
        tr_e, tr_g = _with_flag(tr_e), _with_flag(tr_g)
    else:
        batch, world = _sdxl_world(hip, dtype)
        tr_e, tr_g = world(True), world(True)
    st, met, calls = _segments_against_eager(tr_e, tr_g, batch, dtype)
    assert len(st.slot_pools) == 1
    assert len(st.unet_segs) == len(met) == (4 if layout == "sd15" else 2), (list(st.unet_segs), met)
    assert calls == 2 * len(PLAN)
    # the first call of a variant runs eagerly and is captured; every later one replays the forward graph twice
    assert sum(s.replays for s in st.unet_segs.values()) == 2 * (calls - len(met))
    assert all(s.recompute for s in st.unet_segs.values())


@pytest.mark.gpu
def test_whole_step_graph_under_the_flag(hip):
    """8. GraphedStep under the flag: the capture holds the recompute launches; three replayed steps equal eager ones"""
    dtype = torch.bfloat16
    _, batch, _, tr_e = make_world(dtype, hip, False)
    _, _, _, tr_w = make_world(dtype, hip, False)
    tr_e, tr_w = _with_flag(tr_e), _with_flag(tr_w)
    gs = GraphedStep(tr_w)
    assert gs.supported(batch)
    gen = torch.Generator().manual_seed(3)
    for it in range(4):
        b = vary(batch, gen, dtype)
        kw = dict(training_steps=[0, 1, 2], crop=(it % 2, 1, 63, 63))
        le, lg = tr_e.train_step(b, **kw), gs(b, **kw)
        torch.cuda.synchronize()
        assert gs.failed is None, gs.failed
        for k in ("step_loss", "Blip", "G_loss", "D_loss"):
            assert torch.equal(le[k], lg[k]), f"step {it}: {k}"
        assert torch.equal(tr_e.bank.flat, tr_w.bank.flat) and torch.equal(tr_e.D.bank.flat, tr_w.D.bank.flat)
        assert torch.equal(tr_e.opt.m[0], tr_w.opt.m[0]) and torch.equal(tr_e.opt.v[0], tr_w.opt.v[0])
    assert len(gs.graphs) == 1


@pytest.fixture
def fp8_dev(dev):
    with fp8_state():
        yield dev


def test_fp8_forward_under_the_flag(fp8_dev):
    """9. the miniature C5 world, calibrated, delayed scaling under a recipe with clip accounting: two steps with and without
    the flag - losses, gradients, the scale words and `fp8_clipped_sites` are equal (the second pass quantises under the same
    scale words, folds the same abs-maxima into the running maxima, and consumes only the bytes it stamped itself)"""
    from test_fp8 import _fp8_step_world
    same = torch.equal
    step = dict(training_steps=[1, 2], crop=(1, 0, 63, 63), attrcon_steps=[2])
    runs = {}
    for flag in (False, True):
        ops.fp8_reset()
        ops.set_fp8_scaling("delayed")
        ops.set_fp8_recipe(history=2, margin=1.0)
        trainer, bank, batch, cfg, _ = _fp8_step_world(fp8_dev, torch.float32)
        trainer = _with_flag(trainer, flag)
        trainer.pipe.share_text_kv = False
        assert trainer.fp8_calibrate(batch)
        out = []
        for it in range(2):
            b = dict(batch, latents=batch["latents"] * (1.0 + 0.5 * it))  # the second step moves the abs-maxima
            logs = trainer.train_step(b, **step)
            st = ops.fp8_state(fp8_dev)
            out.append(dict(losses=[logs[k].detach().clone() for k in ("step_loss", "Blip", "G_loss", "D_loss", "token_loss",
                                                                        "pixel_loss")],
                            grad=bank.flat_grad.detach().clone(), scale=st.scale[:st.n].clone(), hist=st.hist[:st.n].clone(),
                            clipped=logs["fp8_clipped_sites"].clone(), clip_steps=st.clip_steps[:st.n].clone()))
        runs[flag] = out
    for it, (p, c) in enumerate(zip(runs[False], runs[True])):
        assert all(same(a, b) for a, b in zip(p["losses"], c["losses"])), f"step {it}: losses"
        assert same(p["grad"], c["grad"]) and float(p["grad"].abs().max()) > 0, f"step {it}: LoRA gradients"
        assert same(p["scale"], c["scale"]) and same(p["hist"], c["hist"]), f"step {it}: scale words"
        assert same(p["clipped"], c["clipped"]) and same(p["clip_steps"], c["clip_steps"]), f"step {it}: clip accounting"
    assert not same(runs[False][0]["scale"], runs[False][1]["scale"])  # the steps really moved the scales


@pytest.mark.gpu
def test_checkpointed_step_keeps_one_call_of_activations(hip):
    """10. peak growth of a step (max_memory_allocated - memory_allocated at its start), no GAN, eager launches:

        trained steps   plain   checkpointed
        [2]             A1      R1
        [0, 1, 2]       A3      R3

    Plain keeps one more call's activations per extra trained step: S = (A3 - A1) / 2 is one call's.
    (a) the world can show the effect: S >= 8 io, io = the bytes of one call's model input, sinusoid and eps;
    (b) R3 - R1 <= (A3 - A1) / 4: legitimate growth is two calls' inputs and outputs plus the scheduler chain, which (a) bounds
        to an eighth of A3 - A1; one call whose activations survived to the backward pass would add a whole S, half of it;
    (c) R3 < A3."""
    dtype = torch.bfloat16
    grow = {}
    for flag in (False, True):
        _, batch, _, tr = make_world(dtype, hip, False, gan=False)
        tr = _with_flag(tr, flag)
        tr.pipe.share_text_kv = False
        tr.pipe.graphed = None  # every call eager: no graph pool grows in the middle of a measured step
        crop = (0, 1, 63, 63)
        tr.train_step(batch, training_steps=[0, 1, 2], crop=crop)  # warm-up: workspaces, memos, compute copies
        for ts in ([2], [0, 1, 2]):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            tr.train_step(batch, training_steps=ts, crop=crop)
            torch.cuda.synchronize()
            grow[(flag, len(ts))] = torch.cuda.max_memory_allocated() - base
    A1, A3, R1, R3 = grow[(False, 1)], grow[(False, 3)], grow[(True, 1)], grow[(True, 3)]
    B, hw, c0 = 2 * batch["latents"].shape[0], 8 * 8, config.TINY_UNET.block_out_channels[0]
    io = 2 * B * hw * 4 * 2 + B * c0 * 4  # model input and eps [B h w, 4] bf16, sinusoid [B, C0] fp32
    S = (A3 - A1) / 2
    print(f"peak growth in bytes: A1 {A1} A3 {A3} R1 {R1} R3 {R3}; S {S:.0f}; io {io}")
    assert S >= 8 * io, (A1, A3, io)
    assert R3 - R1 <= (A3 - A1) / 4, (A1, A3, R1, R3)
    assert R3 < A3, (A3, R3)
