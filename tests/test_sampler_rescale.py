"""The sampler with rescaled guidance (`forward(..., guidance_rescale=phi)`) against the reference's own
`TrainableSDPipeline.forward` / `TrainableSDXLPipeline.forward` run with `guidance_rescale = 0.7` on stand-ins
(tests/golden/make_sampler_rescale_golden.py -> sampler_rescale.npz), driven exactly as
tests/test_models.py::test_sampler_loop_against_the_reference_loop drives the unrescaled one and held to the same bounds; then
the same sampler on the tiny real UNet + VAE through eager calls, the no-grad forward graphs and the step graphs."""
import os
import types

import numpy as np
import pytest
import torch

from comat_amd.pipeline import TrainableSDPipeline, TrainableSDXLPipeline
from helpers import check, tok, untok

GOLD = os.path.join(os.path.dirname(__file__), "golden", "sampler_rescale.npz")


def _stand_in(state, spread, xl):
    """the stand-in 'UNet' of the fixture (`stub_unet` / `spread_unet` of the generators) in the channels-last token layout"""
    def unet(x, B, H, W_, t, ctx, L_, capture_places=(), added=None, kv_cache=None):
        state["calls"].append((int(t), bool(torch.is_grad_enabled()), bool(x.requires_grad)))
        xn, c = untok(x, B, H, W_), ctx.reshape(B, L_, -1)
        shift = c.mean(dim=(1, 2)).reshape(-1, 1, 1, 1)
        y = torch.tanh(torch.einsum("oc,bchw->bohw", state["W"], xn)) * (1.0 + 1e-3 * float(t)) + 0.3 * shift + 0.1 * xn.roll(1, dims=3)
        if spread:
            y = y + 2.0 * shift * xn.roll(1, dims=2)
        if xl:
            text_embeds, time_ids = added
            y = y + 0.2 * (text_embeds.mean(dim=1) + 1e-3 * time_ids.float().sum(dim=1)).reshape(-1, 1, 1, 1)
        return tok(y), {}
    return unet


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "sa", "sb", "sd"])
def test_rescaled_sampler_loop_against_the_reference_loop(dev, name):
    gold = np.load(GOLD)
    T = lambda k: torch.from_numpy(gold[k]).to(dev)
    V, n, phi = T("V"), int(gold["n_steps"]), float(gold["guidance_rescale"])
    bs, _, h, w = gold["latents"].shape
    state = {"calls": []}
    unet = _stand_in(state, name.startswith("s"), False)
    unet.dtype, unet.device = torch.float32, dev
    unet.cfg = types.SimpleNamespace(addition_embed=False)

    def vae(z, B, H, W_):
        return tok(torch.einsum("oc,bchw->bohw", V, untok(z, B, H, W_))), H, W_
    vae.cfg = types.SimpleNamespace(scaling_factor=float(gold["scaling_factor"]))
    pipe = TrainableSDPipeline(unet, vae)
    state["W"] = T("W").clone().requires_grad_(True)
    x0 = T("latents").clone().requires_grad_(True)
    image, latents = pipe.forward(T("cond"), T("uncond"), height=8 * h, width=8 * w,
                                  training_timesteps=[int(i) for i in gold[f"{name}:train"]], num_inference_steps=n,
                                  guidance_scale=7.5, guidance_rescale=phi, latents=x0 * 1.0, noises=list(T("noises")),
                                  return_latents=True)
    ((image * T("gimg")).sum() + (latents * T("glat")).sum()).backward()
    calls = state["calls"]
    check(image, T(f"{name}:image"), torch.float32, f"{name}: image")
    check(latents, T(f"{name}:latents"), torch.float32, f"{name}: latents")
    check(state["W"].grad if state["W"].grad is not None else torch.zeros_like(state["W"]), T(f"{name}:dW"), torch.float32,
          f"{name}: dW", factor=3)
    check(x0.grad if x0.grad is not None else torch.zeros_like(x0), T(f"{name}:dx0"), torch.float32, f"{name}: dx0", factor=3)
    assert [c[0] for c in calls] == list(gold[f"{name}:t"])
    assert [c[1] for c in calls] == list(gold[f"{name}:unet_grad_mode"]), name
    assert [c[2] for c in calls] == list(gold[f"{name}:unet_input_requires_grad"]), name


def test_spread_cases_have_a_rescale_factor_away_from_one(sim):
    """what the `s` cases are for: in them the rescaled run differs from the unrescaled arithmetic by far more than the bound
    of the test above (in `a`-`d` the stand-in's two halves differ by a constant and the factor is 1 up to rounding)"""
    gold = np.load(GOLD)
    base = np.load(os.path.join(os.path.dirname(__file__), "golden", "sampler_loop.npz"))
    assert np.abs(gold["a:latents"] - base["a:latents"]).max() < 1e-4
    state = {"calls": [], "W": torch.from_numpy(gold["W"])}
    unet = _stand_in(state, True, False)
    unet.dtype, unet.device = torch.float32, torch.device("cpu")
    unet.cfg = types.SimpleNamespace(addition_embed=False)
    vae = lambda z, B, H, W_: (z, H, W_)
    vae.cfg = types.SimpleNamespace(scaling_factor=1.0)
    bs, _, h, w = gold["latents"].shape
    T = lambda k: torch.from_numpy(gold[k])
    with torch.no_grad():
        plain = TrainableSDPipeline(unet, vae).forward(T("cond"), T("uncond"), height=8 * h, width=8 * w, num_inference_steps=5,
                                                       latents=T("latents"), noises=list(T("noises")), output_type="latent")
    diff = (plain - T("sd:latents")).abs().max() / T("sd:latents").abs().max()
    assert diff > 0.05, float(diff)


@pytest.mark.parametrize("name", ["xa", "xb", "sxa"])
def test_rescaled_sdxl_sampler_loop_against_the_reference_loop(dev, name):
    """bounds of tests/test_models.py::test_sdxl_sampler_loop_against_the_reference_loop (the reference runs its tail in fp16)"""
    gold = np.load(GOLD)
    T = lambda k: torch.from_numpy(gold[k]).to(dev)
    V, n, phi = T("V"), int(gold["n_steps"]), float(gold["guidance_rescale"])
    bs, _, h, w = gold["latents"].shape
    state = {"calls": []}
    unet = _stand_in(state, name.startswith("s"), True)
    unet.dtype, unet.device = torch.float32, dev
    unet.cfg = types.SimpleNamespace(addition_embed=True)
    unet.added_embedding = lambda text_embeds, ids: (text_embeds.to(dev), torch.tensor(ids, dtype=torch.float32, device=dev))

    def vae(z, B, H, W_):
        return tok(torch.einsum("oc,bchw->bohw", V, untok(z, B, H, W_))), H, W_
    vae.cfg = types.SimpleNamespace(scaling_factor=float(gold["xl_scaling_factor"]))
    pipe = TrainableSDXLPipeline(unet, vae)
    state["W"] = T("W").clone().requires_grad_(True)
    x0 = T("latents").clone().requires_grad_(True)
    image, latents = pipe.forward(T("cond"), T("uncond"), height=8 * h, width=8 * w,
                                  training_timesteps=[int(i) for i in gold[f"{name}:train"]], num_inference_steps=n,
                                  guidance_scale=7.5, guidance_rescale=phi, latents=x0 * 1.0, noises=list(T("noises")),
                                  return_latents=True, pooled_prompt_embeds=T("pooled"), negative_pooled_prompt_embeds=T("npooled"))
    ((image * T("gimg")).sum() + (latents * T("glat")).sum()).backward()
    for got, key, tol in ((image, "image", 2e-3), (latents, "latents", 2e-3), (state["W"].grad, "dW", 2e-2),
                          (x0.grad if x0.grad is not None else torch.zeros_like(x0), "dx0", 2e-2)):
        ref = T(f"{name}:{key}")
        assert (got - ref).abs().max() <= tol * (ref.abs().max() + 1e-6), (name, key, float((got - ref).abs().max()))
    assert [c[1] for c in state["calls"]] == list(gold[f"{name}:unet_grad_mode"]), name
    assert [c[2] for c in state["calls"]] == [False] * n, name


# ---- tiny real UNet + VAE: eager calls, no-grad forward graphs, step graphs ----------------------------------------------------
def _worlds(dev, dtype):
    """two identical worlds of tests/test_step.py::make_world under StepConfig(cfg_rescale=0.7, norm_grad=True)"""
    import dataclasses

    from comat_amd.step import CoMatTrainer
    from test_step import make_world
    out = []
    for _ in range(2):
        cfg, batch, W, tr = make_world(dtype, dev, False)
        cfg = dataclasses.replace(cfg, cfg_rescale=0.7, norm_grad=True)
        out.append(CoMatTrainer(tr.pipe, tr.bank, tr.blip, tr.D, cfg, seed=0))
    return batch, out[0], out[1]


def _same_steps(tr_e, stepper, tr_g, batch, dtype, n_steps):
    from test_segments import PLAN, vary
    gen = torch.Generator().manual_seed(11)
    for it, (ts, crop, _) in enumerate(PLAN[:n_steps]):
        b = vary(batch, gen, dtype)
        le = tr_e.train_step(b, training_steps=ts, crop=crop)
        def sample(tr):
            # a REPLAYED whole-step graph updates the LoRA parameters on the device; the host-side freshness flag of their
            # derived copies (compute-dtype / transposed / merged weights) only moves when the optimizer is issued by the
            # host.  Say so before the pipeline is used outside the stepper, as GraphedStep does after its own eager step.
            tr.bank.mark_updated()
            return tr.pipe.forward(b["prompt_embeds"], b["negative_prompt_embeds"], height=64, width=64, num_inference_steps=3,
                                   latents=b["latents"], noises=b["noises"], output_type="latent", guidance_rescale=0.7)
        with torch.no_grad():
            lat_e = sample(tr_e)
        lg = stepper(b, training_steps=ts, crop=crop)
        with torch.no_grad():
            lat_g = sample(tr_g)
        torch.cuda.synchronize()
        for k in ("step_loss", "Blip", "G_loss", "D_loss", "reward_norm"):
            assert torch.equal(le[k], lg[k]), f"step {it}: {k} {float(le[k])} vs {float(lg[k])}"
        assert torch.equal(lat_e, lat_g), f"step {it}: sampled latents differ"
        assert torch.equal(tr_e.bank.flat_grad, tr_g.bank.flat_grad), f"step {it}: LoRA gradients differ"
        assert torch.equal(tr_e.bank.flat, tr_g.bank.flat) and torch.equal(tr_e.D.bank.flat, tr_g.D.bank.flat)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rescaled_sampler_forward_graphs_match_eager_calls(hip, dtype):
    """(a) every UNet call eager against (b) the untrained denoise steps replayed from the no-grad forward graphs"""
    batch, tr_e, tr_g = _worlds(hip, dtype)
    assert tr_g.pipe.graphed is not None
    tr_e.pipe.graphed = None
    _same_steps(tr_e, lambda b, **kw: tr_g.train_step(b, **kw), tr_g, batch, dtype, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rescaled_segmented_step_matches_eager(hip, dtype):
    """(c) trained UNet calls, head (with the image-gradient hook inside its backward graph) and D step from segment graphs"""
    from comat_amd.segments import SegmentedStep
    batch, tr_e, tr_g = _worlds(hip, dtype)
    tr_e.pipe.share_text_kv = False  # replayed segments project the text keys / values once per call
    tr_g.pipe.share_text_kv = False
    st = SegmentedStep(tr_g)
    _same_steps(tr_e, st, tr_g, batch, dtype, 4)
    assert st.stats()["replays"] >= 4 and st.head_seg is not None and st.head_seg.replays >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rescaled_graphed_step_matches_eager(hip, dtype):
    """(c) the whole step, rescaled denoise steps and normalised image gradient included, replayed from one graph"""
    from comat_amd.step import GraphedStep
    batch, tr_e, tr_g = _worlds(hip, dtype)
    gs = GraphedStep(tr_g)
    assert gs.supported(batch)
    _same_steps(tr_e, gs, tr_g, batch, dtype, 4)
    assert gs.failed is None and len(gs.graphs) == 2
