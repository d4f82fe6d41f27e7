"""The sampler's other modes - `early_exit`, `double_laststep`, `fast_training`, `bp_on_trained=False`, `detach_gradient=False`,
guidance off - against the reference's own `TrainableSDPipeline.forward` / `TrainableSDXLPipeline.forward` run on stand-ins
(tests/golden/make_sampler_modes_golden.py -> sampler_modes.npz), driven as tests/test_sampler_rescale.py drives its cases and
held to the same bounds; then the modes on the tiny real world of tests/test_step.py::make_world: an eager step against a
SegmentedStep and against the no-grad forward graphs, bit for bit."""
import dataclasses
import os
import types

import numpy as np
import pytest
import torch

from comat_amd.pipeline import TrainableSDPipeline, TrainableSDXLPipeline
from helpers import check, tok, tol, untok
from test_sampler_rescale import _stand_in

HERE = os.path.dirname(__file__)
GOLD = os.path.join(HERE, "golden", "sampler_modes.npz")

# name -> (spread stand-in, keywords of forward): the settings of tests/golden/make_sampler_modes_golden.py::CASES
CASES = {
    "e1": (False, dict(early_exit=True)),
    "e2": (False, dict(early_exit=True)),
    "e3": (False, dict(early_exit=True)),
    "se1": (True, dict(early_exit=True, guidance_rescale=0.7)),
    "dl1": (False, dict(double_laststep=True)),
    "dl2": (False, dict(double_laststep=True)),
    "f1": (False, dict(fast_training=True)),
    "f2": (False, dict(fast_training=True, early_exit=True)),
    "g1": (False, dict(guidance_scale=1.0)),
    "g2": (False, dict(guidance_scale=1.0, guidance_rescale=0.7)),
    "b1": (False, dict(bp_on_trained=False)),
    "b2": (False, dict(detach_gradient=False)),
}


def _log_matches(calls, gold, name):
    assert [c[0] for c in calls] == list(gold[f"{name}:t"]), (name, [c[0] for c in calls])
    assert [c[1] for c in calls] == list(gold[f"{name}:unet_grad_mode"]), name
    assert [c[2] for c in calls] == list(gold[f"{name}:unet_input_requires_grad"]), name


@pytest.mark.parametrize("name", list(CASES))
def test_sampler_modes_against_the_reference_loop(dev, name):
    gold = np.load(GOLD)
    spread, kw = CASES[name]
    T = lambda k: torch.from_numpy(gold[k]).to(dev)
    V, n = T("V"), int(gold["n_steps"])
    bs, _, h, w = gold["latents"].shape
    state = {"calls": []}
    unet = _stand_in(state, spread, False)
    unet.dtype, unet.device = torch.float32, dev
    unet.cfg = types.SimpleNamespace(addition_embed=False)

    def vae(z, B, H, W_):
        return tok(torch.einsum("oc,bchw->bohw", V, untok(z, B, H, W_))), H, W_
    vae.cfg = types.SimpleNamespace(scaling_factor=float(gold["scaling_factor"]))
    pipe = TrainableSDPipeline(unet, vae)
    state["W"] = T("W").clone().requires_grad_(True)
    x0 = T("latents").clone().requires_grad_(True)
    args = dict(guidance_scale=7.5)
    args.update(kw)
    if kw.get("double_laststep"):
        args["renoise"] = T("renoise")
    image, latents = pipe.forward(T("cond"), T("uncond") if args["guidance_scale"] > 1.0 else None, height=8 * h, width=8 * w,
                                  training_timesteps=[int(i) for i in gold[f"{name}:train"]], num_inference_steps=n,
                                  latents=x0 * 1.0, noises=list(T("noises")) + [T("noise_extra")], return_latents=True, **args)
    loss = (image * T("gimg")).sum() + (latents * T("glat")).sum()
    if loss.requires_grad:
        loss.backward()
    check(image, T(f"{name}:image"), torch.float32, f"{name}: image")
    check(latents, T(f"{name}:latents"), torch.float32, f"{name}: latents")
    check(state["W"].grad if state["W"].grad is not None else torch.zeros_like(state["W"]), T(f"{name}:dW"), torch.float32,
          f"{name}: dW", factor=3)
    check(x0.grad if x0.grad is not None else torch.zeros_like(x0), T(f"{name}:dx0"), torch.float32, f"{name}: dx0", factor=3)
    _log_matches(state["calls"], gold, name)


def test_sdxl_early_exit_against_the_reference_loop(dev):
    """bounds of tests/test_sampler_rescale.py::test_rescaled_sdxl_sampler_loop_against_the_reference_loop (the reference runs
    its tail in fp16); SDXL's early exit is a plain break after the trained step's prev_sample"""
    name = "xe"
    gold = np.load(GOLD)
    T = lambda k: torch.from_numpy(gold[k]).to(dev)
    V, n = T("V"), int(gold["n_steps"])
    bs, _, h, w = gold["latents"].shape
    state = {"calls": []}
    unet = _stand_in(state, False, True)
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
                                  guidance_scale=7.5, latents=x0 * 1.0, noises=list(T("noises")), return_latents=True,
                                  pooled_prompt_embeds=T("pooled"), negative_pooled_prompt_embeds=T("npooled"), early_exit=True)
    ((image * T("gimg")).sum() + (latents * T("glat")).sum()).backward()
    for got, key, tol in ((image, "image", 2e-3), (latents, "latents", 2e-3), (state["W"].grad, "dW", 2e-2),
                          (x0.grad if x0.grad is not None else torch.zeros_like(x0), "dx0", 2e-2)):
        ref = T(f"{name}:{key}")
        assert (got - ref).abs().max() <= tol * (ref.abs().max() + 1e-6), (name, key, float((got - ref).abs().max()))
    _log_matches(state["calls"], gold, name)


def test_sdxl_keeps_refusing_the_modes_its_reference_does_not_have():
    pipe = TrainableSDXLPipeline.__new__(TrainableSDXLPipeline)
    for kw in (dict(double_laststep=True), dict(fast_training=True)):
        with pytest.raises(NotImplementedError):
            pipe.forward(None, None, **kw)


def test_every_mode_fixture_is_away_from_its_default_twin():
    """a case that happened to equal the default-mode run would pin nothing: each differs from its twin of sampler_loop.npz
    (sampler_rescale.npz for `se1`) by more than 20 times the bound of the tests above (helpers.tol: 2e-4 of the largest value
    in fp32, times 3 for gradients) in the quantity its mode changes.  Three must NOT move: `e3` (no trained step: no exit), `g2`
    (no rescale without guidance) and `e2`, which exits at the last step, t = 1, where the scheduler's prev_sample IS its
    pred_original_sample (c_xt = 0, sigma = 1e-10): what `e2` pins is the call log of an exit at the last index."""
    gold = np.load(GOLD)
    base = np.load(os.path.join(HERE, "golden", "sampler_loop.npz"))
    resc = np.load(os.path.join(HERE, "golden", "sampler_rescale.npz"))

    def rel(a, b):
        return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-6))
    far = {"latents": 20 * tol(torch.float32), "dW": 20 * 3 * tol(torch.float32)}
    twins = {"e1": (base, "a", "latents"), "se1": (resc, "sa", "latents"),
             "dl1": (base, "a", "latents"), "f1": (base, "a", "latents"), "g1": (base, "a", "latents"),
             "b1": (base, "a", "dW"), "xe": (base, "xa", "latents")}
    for name, (ref, twin, key) in twins.items():
        assert rel(gold[f"{name}:{key}"], ref[f"{twin}:{key}"]) > far[key], (name, key)
    # no default twin with these trained steps: against the neighbouring mode case instead
    assert rel(gold["dl2:latents"], gold["dl1:latents"]) > far["latents"]
    assert rel(gold["f2:latents"], gold["f1:latents"]) > far["latents"]
    assert rel(gold["se1:latents"], gold["e1:latents"]) > far["latents"]  # the rescale factor reaches pred_original_sample
    # b1: the values are the default's, only the gradient path through the UNet input is cut
    assert rel(gold["b1:latents"], base["a:latents"]) == 0.0
    # b2: an untrained step runs without grad whatever its input: values and gradients are the default's, the call log is not
    assert list(gold["b2:unet_input_requires_grad"]) != list(base["a:unet_input_requires_grad"])
    assert rel(gold["e2:latents"], base["c:latents"]) < tol(torch.float32)
    for key in ("image", "latents", "dW", "dx0"):
        assert np.array_equal(gold[f"e3:{key}"], base[f"d:{key}"]), key
        assert np.array_equal(gold[f"g2:{key}"], gold[f"g1:{key}"]), key
    # the stale-input branch of double_laststep: its trained call sees an input that carries no re-noising
    assert list(gold["dl2:t"])[-1] == 401 and list(gold["dl1:t"])[-1] == 601


# ---- tiny real UNet + VAE: eager steps against segment graphs and no-grad forward graphs ---------------------------------------
MODES = {"early_exit": dict(early_exit=True), "fast_training": dict(fast_training=True),
         "double_laststep": dict(double_laststep=True), "guidance_off": dict(cfg_scale=1.0)}


def _worlds(dev, dtype, mode):
    """two identical worlds of tests/test_step.py::make_world under the mode's StepConfig"""
    from comat_amd.step import CoMatTrainer
    from test_step import make_world
    out = []
    for _ in range(2):
        cfg, batch, W, tr = make_world(dtype, dev, False)
        cfg = dataclasses.replace(cfg, **MODES[mode])
        out.append(CoMatTrainer(tr.pipe, tr.bank, tr.blip, tr.D, cfg, seed=0))
    batch = dict(batch)
    if mode == "double_laststep":  # one more step noise for the extra step, and the re-noising draw
        g = torch.Generator().manual_seed(3)
        batch["noises"] = list(batch["noises"]) + [torch.randn(batch["noises"][0].shape, generator=g)]
        batch["renoise"] = torch.randn(batch["latents"].shape, generator=g)
    if mode == "guidance_off":
        del batch["negative_prompt_embeds"]
    return batch, out[0], out[1]


def _same_steps(tr_e, stepper, tr_g, batch, dtype, n_steps):
    from test_segments import PLAN, vary
    gen = torch.Generator().manual_seed(11)
    for it, (ts, crop, _) in enumerate(PLAN[:n_steps]):
        b = vary(batch, gen, dtype)
        le = tr_e.train_step(b, training_steps=ts, crop=crop)
        lg = stepper(b, training_steps=ts, crop=crop)
        torch.cuda.synchronize()
        for k in ("step_loss", "Blip", "G_loss", "D_loss"):
            assert torch.equal(le[k], lg[k]), f"step {it}: {k} {float(le[k])} vs {float(lg[k])}"
        assert torch.isfinite(le["step_loss"]) and float(tr_e.bank.flat_grad.abs().max()) > 0
        assert torch.equal(tr_e.bank.flat_grad, tr_g.bank.flat_grad), f"step {it}: LoRA gradients differ"
        assert torch.equal(tr_e.bank.flat, tr_g.bank.flat) and torch.equal(tr_e.D.bank.flat, tr_g.D.bank.flat)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("mode", list(MODES))
def test_mode_segmented_step_matches_eager(hip, dtype, mode):
    """(a) an eager step against (b) trained UNet calls, head and D step from segment graphs; the whole-step graph declines"""
    from comat_amd.segments import SegmentedStep
    from comat_amd.step import GraphedStep
    batch, tr_e, tr_g = _worlds(hip, dtype, mode)
    assert not GraphedStep(tr_g).supported(batch)
    tr_e.pipe.share_text_kv = False  # replayed segments project the text keys / values once per call
    tr_g.pipe.share_text_kv = False
    st = SegmentedStep(tr_g)
    _same_steps(tr_e, st, tr_g, batch, dtype, 3)
    assert st.failed is None and st.stats()["replays"] >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_double_laststep_forward_graphs_match_eager_calls(hip, dtype):
    """every loop step of double_laststep is a no-grad step: (a) all of them eager against (b) replayed from the forward graphs"""
    batch, tr_e, tr_g = _worlds(hip, dtype, "double_laststep")
    assert tr_g.pipe.graphed is not None
    tr_e.pipe.graphed = None
    _same_steps(tr_e, lambda b, **kw: tr_g.train_step(b, **kw), tr_g, batch, dtype, 2)
    assert len(tr_g.pipe.graphed.graphs) == 3  # one per timestep: the trained steps of the other modes replay here too
