"""CoMatTrainer(..., text_encoder_2=...): SDXL's frozen second text tower inside the optimisation step, the prompts encoded from
the two tokenizers' ids - on the tiny SDXL step world of tests/test_text_encoder_step.py (rebuilt here with the context width of
the two tiny towers) with a real tiny second tower (config.TINY_CLIP_TEXT_2), simulator and real kernels.

The check is an identity, not a tolerance: a step fed the four id tensors gives the logs, the gradients and the updated parameters,
bit for bit, of the same trainer fed the four tensors clip.encode_prompt_sdxl made from those ids beforehand (one call over
[null; cond], as the step encodes them).  The towers themselves are held to transformers' in tests/test_clip_text_projection.py."""
import dataclasses
import types

import pytest
import torch

from clip2_sim import clip2_dev  # noqa: F401 - fixture
from comat_amd import config, weights
from comat_amd.blip import Blip
from comat_amd.clip import ClipLoRABank, ClipTextBank, ClipTextEncoder, encode_prompt_sdxl
from comat_amd.config import TINY_CLIP_TEXT_2 as CLIP2
from comat_amd.gan import D_sd
from comat_amd.pipeline import TrainableSDPipeline, TrainableSDXLPipeline
from comat_amd.segments import SegmentedStep
from comat_amd.step import CoMatTrainer, GraphedStep, StepConfig
from comat_amd.unet import LoRABank, UNet, VAEDecoder
from test_clip_text import CFG as CLIP
from test_clip_text import END, hf_model, lora_factors
from test_clip_text_projection import hf_model2, make_ids2
from test_text_encoder_step import UCFG, sync

XCFG = dataclasses.replace(config.TINY_SDXL_UNET, cross_attention_dim=CLIP.hidden + CLIP2.hidden)
FIXED = dict(training_steps=[1, 2], crop=(1, 0, 63, 63))
BS, L = 2, 9
FLAGS = {"train_text_encoder_lora": "lora", "tune_text_encoder": "tune"}
TENSOR_KEYS = ("prompt_embeds_2", "negative_prompt_embeds_2", "pooled_prompt_embeds", "negative_pooled_prompt_embeds")
assert CLIP2.projection_dim == XCFG.pooled_dim and CLIP2.hidden != CLIP.hidden


class CountingEncoder(ClipTextEncoder):
    """the second tower, noting the shape of every id tensor it is called with"""
    seen = ()

    def __call__(self, input_ids, output="last"):
        self.seen = self.seen + ((tuple(input_ids.shape), output),)
        return super().__call__(input_ids, output)


def _ids(bs):
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(3, CLIP.vocab_size - 2, (bs, L), generator=g)
    for b in range(bs):
        ids[b, 4 + b:] = END  # the first tokenizer pads with the end token
    null = torch.full((bs, L), END)
    null[:, 0] = 1
    ids_2 = make_ids2(bs, L, CLIP2.eos_token_id, seed=8)  # the second pads with 0
    null_2 = torch.zeros((bs, L), dtype=torch.int64)
    null_2[:, 0], null_2[:, 1] = 1, CLIP2.vocab_size - 1
    return dict(prompt_input_ids=ids, null_input_ids=null, prompt_input_ids_2=ids_2, null_input_ids_2=null_2)


def make_world(dtype, dev, flag, second=True, bs=BS, cfg2=CLIP2, **cfg_kw):
    """second: the trainer holds the second tower and the batch its ids; off: the same world without either (the four tensors are
    the caller's to add).  -> namespace(cfg, batch, tr, enc2, parts)"""
    q = lambda d: {k: v.to(dtype).float() for k, v in d.items()}
    up5 = lambda d: {k: (v * 5 if k.endswith("up.weight") else v) for k, v in d.items()}
    vcfg = dataclasses.replace(config.TINY_VAE, scaling_factor=0.13025)
    usd = q(weights.make_unet_weights(XCFG, perturb_norms=True))
    vsd = q(weights.make_vae_weights(vcfg, perturb_norms=True))
    lsd = q(up5(weights.make_lora_weights(XCFG)))
    bsd = q(weights.make_blip_weights(config.TINY_BLIP, perturb_norms=True))
    dsd = q(weights.make_unet_weights(UCFG, seed=77, perturb_norms=True))
    dl = q(up5(weights.make_lora_weights(UCFG, seed=78)))
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g)
    head_w, head_b = r(4) * 0.5, r(1) * 0.1
    cfg = StepConfig(**{**dict(resolution=64, total_step=3, K=2, gan_loss=True, attrcon=False, train_layer_ls=("mid_2", "up_2", "up_4"),
                               attn_reses=(8, 4, 2), lr=1e-2, lr_D=1e-2, **{flag: True}), **cfg_kw})
    bids = torch.randint(1, config.TINY_BLIP.vocab_size, (bs, 9), generator=g)
    batch = dict(gan_null_embeds=r(bs, L, UCFG.cross_attention_dim).to(dtype).float(), latents=r(bs, 4, 8, 8),
                 noises=[r(bs, 4, 8, 8) for _ in range(3)], real_latents=r(bs, 4, 8, 8), blip_input_ids=bids,
                 blip_attention_mask=torch.ones_like(bids), add_time_ids=(64, 64, 0, 0, 64, 64))
    ids = _ids(bs)
    guided = cfg.cfg_scale > 1.0
    keys = [k for k in ids if (second or not k.endswith("_2")) and (guided or not k.startswith("null"))]
    batch.update({k: ids[k] for k in keys})
    bank = LoRABank(XCFG, lsd, dtype, dev)
    pipe = TrainableSDXLPipeline(UNet(XCFG, usd, dtype, dev, bank), VAEDecoder(vcfg, vsd, dtype, dev))
    dbank = LoRABank(UCFG, dl, dtype, dev)
    disc = D_sd(UNet(UCFG, dsd, dtype, dev, dbank), dbank, head_w, head_b)
    blip = Blip(config.TINY_BLIP, bsd, dtype, dev)
    if FLAGS[flag] == "lora":
        tbank = ClipLoRABank(CLIP, lora_factors(4, seed=3), dtype, dev)
        enc = ClipTextEncoder(CLIP, hf_model().state_dict(), dtype, dev, tbank)
    else:
        tbank = ClipTextBank(CLIP, hf_model().state_dict(), dtype, dev)
        enc = ClipTextEncoder(CLIP, None, dtype, dev, tbank)
    enc2 = CountingEncoder(cfg2, hf_model2(cfg2.eos_token_id).state_dict(), dtype, dev)
    parts = (pipe, bank, blip, disc)
    tr = CoMatTrainer(*parts, cfg, seed=0, text_encoder=enc, text_bank=tbank, **(dict(text_encoder_2=enc2) if second else {}))
    return types.SimpleNamespace(cfg=cfg, batch=batch, tr=tr, enc2=enc2, parts=parts, ids=ids)


def four_tensors(w):
    """what a caller without text_encoder_2 brings: from ONE encode_prompt_sdxl call over [null; cond] (or the prompt alone)"""
    guided, i = w.cfg.cfg_scale > 1.0, w.ids
    cat = lambda a, b: torch.cat([i[a], i[b]]) if guided else i[b]
    with torch.no_grad():
        emb, pooled = encode_prompt_sdxl(w.tr.text_encoder, w.enc2, cat("null_input_ids", "prompt_input_ids"),
                                         cat("null_input_ids_2", "prompt_input_ids_2"))
    e2, bs = emb[..., CLIP.hidden:].contiguous(), i["prompt_input_ids"].shape[0]
    if not guided:
        return dict(prompt_embeds_2=e2, pooled_prompt_embeds=pooled)
    return dict(prompt_embeds_2=e2[bs:], negative_prompt_embeds_2=e2[:bs], pooled_prompt_embeds=pooled[bs:],
                negative_pooled_prompt_embeds=pooled[:bs])


def assert_same_step(a, b, dev):
    la, lb = a.tr.train_step(a.batch, **FIXED), b.tr.train_step(b.batch, **FIXED)
    sync(dev)
    for k in ("Blip", "G_loss", "D_loss", "step_loss", "grad_norm_sq"):
        assert torch.equal(la[k], lb[k]), k
    assert bool(torch.isfinite(la["grad_norm_sq"]).all())
    for x in ("bank", "text_bank"):
        ga, gb = getattr(a.tr, x), getattr(b.tr, x)
        assert float(ga.flat_grad.abs().max()) > 0, x
        assert torch.equal(ga.flat_grad, gb.flat_grad), f"{x}: gradients differ"
        assert torch.equal(ga.flat, gb.flat), f"{x}: updated parameters differ"
    assert a.tr.opt.counters.tolist() == b.tr.opt.counters.tolist() == [1, 0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("flag", list(FLAGS))
def test_a_step_from_ids_is_the_step_from_the_four_tensors(clip2_dev, flag, dtype):
    a, b = make_world(dtype, clip2_dev, flag), make_world(dtype, clip2_dev, flag, second=False)
    b.batch.update(four_tensors(b))
    before = a.tr.text_bank.flat.clone()
    assert_same_step(a, b, clip2_dev)
    assert not torch.equal(a.tr.text_bank.flat, before)
    assert a.enc2.seen == (((2 * BS, L), "pooled"),)  # [null; cond] in ONE call of the second tower
    assert a.tr.text_encoder_2 is a.enc2 and b.tr.text_encoder_2 is None


def test_with_guidance_off_only_the_prompt_is_encoded(clip2_dev):
    flag = "train_text_encoder_lora"
    a = make_world(torch.float32, clip2_dev, flag, cfg_scale=1.0)
    b = make_world(torch.float32, clip2_dev, flag, second=False, cfg_scale=1.0)
    assert "null_input_ids_2" not in a.batch and "null_input_ids" not in a.batch
    b.batch.update(four_tensors(b))
    assert_same_step(a, b, clip2_dev)
    assert a.enc2.seen == (((BS, L), "pooled"),)


def test_graph_runners_go_on_declining(clip2_dev):
    w = make_world(torch.float32, clip2_dev, "train_text_encoder_lora")
    assert not GraphedStep(w.tr).supported(w.batch)
    stepper = SegmentedStep(w.tr, dry=True)
    stepper(w.batch, **FIXED)
    sync(clip2_dev)
    assert not stepper.unet_segs and stepper.head_seg is None and stepper.failed is None


def test_every_mis_binding_raises(clip2_dev):
    dev, flag = clip2_dev, "train_text_encoder_lora"
    w = make_world(torch.float32, dev, flag)
    tr, enc2 = w.tr, w.enc2
    text = dict(text_encoder=tr.text_encoder, text_bank=tr.text_bank)
    # ids and tensors together: each of the four by name
    given = four_tensors(w)
    for k in TENSOR_KEYS:
        with pytest.raises(ValueError, match=rf"\['{k}'\]"):
            tr.train_step(dict(w.batch, **{k: given[k]}), **FIXED)
    # ids missing
    for k in ("prompt_input_ids_2", "null_input_ids_2"):
        with pytest.raises(ValueError, match=rf"lacks \['{k}'\]"):
            tr.train_step({n: v for n, v in w.batch.items() if n != k}, **FIXED)
    # a tower without a projection, one with a bank, and something that is no tower
    sd2 = hf_model2().state_dict()
    with pytest.raises(ValueError, match="projection_dim"):
        CoMatTrainer(*w.parts, w.cfg, **text, text_encoder_2=ClipTextEncoder(dataclasses.replace(CLIP2, projection_dim=None), sd2, torch.float32, dev))
    with pytest.raises(ValueError, match="projection_dim"):
        CoMatTrainer(*w.parts, w.cfg, **text, text_encoder_2=tr.text_encoder)
    with pytest.raises(ValueError, match="projection_dim"):
        CoMatTrainer(*w.parts, w.cfg, **text, text_encoder_2=object())
    # wrong widths
    proj = torch.zeros(XCFG.pooled_dim + 4, CLIP2.hidden)
    wide = ClipTextEncoder(dataclasses.replace(CLIP2, projection_dim=XCFG.pooled_dim + 4), dict(sd2, **{"text_projection.weight": proj}),
                           torch.float32, dev)
    with pytest.raises(ValueError, match="pooled_dim"):
        CoMatTrainer(*w.parts, w.cfg, **text, text_encoder_2=wide)
    narrow_cfg = dataclasses.replace(config.TINY_CLIP_TEXT, act="gelu", projection_dim=XCFG.pooled_dim)  # hidden 128, not 192
    narrow = ClipTextEncoder(narrow_cfg, dict(hf_model().state_dict(), **{"text_projection.weight": torch.zeros(XCFG.pooled_dim, CLIP.hidden)}),
                             torch.float32, dev)
    with pytest.raises(ValueError, match="cross_attention_dim"):
        CoMatTrainer(*w.parts, w.cfg, **text, text_encoder_2=narrow)
    # without a flag; on an SD1.5 pipeline
    off = dataclasses.replace(w.cfg, train_text_encoder_lora=False)
    with pytest.raises(ValueError, match="text_encoder_2.*train_text_encoder_lora"):
        CoMatTrainer(*w.parts, off, text_encoder_2=enc2)
    pipe, bank, blip, disc = w.parts
    with pytest.raises(ValueError, match="text_encoder_2.*SDXL"):
        CoMatTrainer(TrainableSDPipeline(pipe.unet, pipe.vae), bank, blip, disc, w.cfg, **text, text_encoder_2=enc2)
    # and without the second tower the contract is the one it was
    plain = make_world(torch.float32, dev, flag, second=False, bs=1)
    with pytest.raises(ValueError, match="prompt_embeds_2"):
        plain.tr.train_step(plain.batch, **FIXED)


@pytest.mark.parametrize("where", ["tower", "projection"])
def test_a_non_finite_weight_of_the_second_tower_reaches_the_skipped_update(clip2_dev, where):
    """the contract of tests/test_nonfinite.py for the new path: one NaN in a frozen weight of the second tower - in its first MLP,
    which every token passes, or in text_projection, which only the pooled embedding passes - makes the gradient norm non-finite;
    the update is counted as skipped and parameters and moments keep their bits"""
    w = make_world(torch.float32, clip2_dev, "train_text_encoder_lora")
    tr = w.tr
    lin = w.enc2.layers[0]["fc1"] if where == "tower" else w.enc2.proj
    lin.w[1, 2] = float("nan")
    lin.wt[2, 1] = float("nan")
    before = [t.clone() for t in (tr.bank.flat, tr.text_bank.flat, *tr.opt.m, *tr.opt.v)]
    logs = tr.train_step(w.batch, **FIXED)
    sync(clip2_dev)
    assert not bool(torch.isfinite(logs["grad_norm_sq"].cpu()).all()), "the NaN did not reach comat_sumsq: the gradient norm is finite"
    assert tr.opt.counters.tolist() == [0, 1]
    for a, b in zip((tr.bank.flat, tr.text_bank.flat, *tr.opt.m, *tr.opt.v), before):
        assert torch.equal(a, b)
