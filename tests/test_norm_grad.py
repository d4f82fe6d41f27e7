"""`reward_norm` and `--norm_grad` (training_script.py:644-651, :677): the norm of the gradient that reaches the decoded image,
logged every step, and its normalisation to 1e4 before it flows into the VAE - comat_grad_norm_scale behind
ops.grad_norm_hook, switched on by StepConfig.reward_norm / StepConfig.norm_grad."""
import dataclasses
import os
import sys
import types

import numpy as np
import pytest
import torch

from comat_amd import ops
from comat_amd.pipeline import TrainableSDPipeline
from comat_amd.step import CoMatTrainer, StepConfig
from helpers import check, rel_l2, tok, untok
from sim_backend import SimKernels
from test_step import make_world

DTYPES = [torch.float32, torch.bfloat16]


def world(dev, gan, dtype=torch.float32, **flags):
    """the tiny real networks of tests/test_step.py::make_world under a StepConfig with `flags` set"""
    cfg, batch, W, tr = make_world(dtype, dev, False, gan=gan)
    cfg = dataclasses.replace(cfg, **flags)
    return cfg, batch, CoMatTrainer(tr.pipe, tr.bank, tr.blip, tr.D, cfg, seed=0)


FIXED = dict(training_steps=[1, 2], crop=(1, 0, 63, 63))


# ---- the kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [3 * 64 * 64, 3 * 512 * 512, 3 * 1024 * 1024])
def test_grad_norm_scale_kernel(dev, dtype, n):
    """norm: fp32 sums over at most ~12 values per lane, a 256-lane tree and 1 024 partials - a few 1e-6 relative at worst;
    bound 1e-5.  Scaled gradient: helpers.check (the product g * c is rounded once, to fp32 or bf16)."""
    gen = torch.Generator().manual_seed(n % 1000)
    g = (torch.randn(n, generator=gen) * 3e-4).to(dtype)
    want = g.double().norm()
    k = ops.kernels()
    gd = g.to(dev)
    norm = torch.full((1,), -1.0, device=dev)
    k.grad_norm_scale(gd, None, n, norm, 0.0)  # target = 0 only measures
    assert torch.equal(gd.cpu(), g), "target = 0 wrote to the gradient"
    err = abs(float(norm) - float(want)) / float(want)
    print(f"grad_norm_scale n={n} {dtype}: norm rel err {err:.2e}")
    assert err < 1e-5
    out = torch.zeros_like(gd)
    norm2 = torch.zeros(1, device=dev)
    k.grad_norm_scale(gd, out, n, norm2, 1e4)
    assert torch.equal(norm, norm2), "the norm of two runs differs in its bits"
    assert torch.equal(gd.cpu(), g)
    check(out, g.double() * (1e4 / want), dtype, "normalised gradient")
    assert abs(float(out.double().norm()) / 1e4 - 1) < (1e-4 if dtype == torch.float32 else 4e-3)
    again = gd.clone()
    k.grad_norm_scale(again, again, n, norm2, 1e4)  # g_out may alias g
    assert torch.equal(again, out) and torch.equal(norm, norm2)


def test_hook_is_an_identity_that_writes_a_fresh_gradient(dev):
    x = torch.randn(6, 3, device=dev, requires_grad=True)
    norm = torch.zeros(1, device=dev)
    y = ops.grad_norm_hook(x, norm, 1e4)
    assert torch.equal(y, x)
    g = torch.randn(6, 3, device=dev)
    keep = g.clone()
    y.backward(g)
    assert torch.equal(g, keep), "the incoming gradient tensor was modified in place"
    assert abs(float(norm) - float(keep.norm())) < 1e-5 * float(keep.norm())
    check(x.grad, keep * (1e4 / keep.norm()), torch.float32, "normalised gradient")


# ---- the step against the reference's loop body ---------------------------------------------------------------------------
def test_norm_grad_step_against_the_reference_loop_body(dev):
    """twin of tests/test_step.py::test_trainer_step_against_the_reference_loop_body with StepConfig(norm_grad=True,
    cfg_rescale=0.7) against tests/golden/step_body_normgrad.npz (the reference's own loop body with args.norm_grad = True and
    args.cfg_rescale = 0.7 on the same stand-ins): same bounds, plus the logged reward_norm within 1e-4 relative.
    (The stored generator gradient is the CLIPPED one and the caption term dominates it with and without the normalisation, so
    this fixture pins the hook's place, the logged norm and the order of the step; the factor itself is pinned by the linearity
    tests below.)"""
    from comat_amd.gan import D_sd
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "step_body_normgrad.npz"))
    T = lambda k: torch.from_numpy(gold[k]).to(dev)
    V, n = T("V"), int(gold["n_steps"])
    up = torch.nn.Upsample(scale_factor=8, mode="nearest")

    class FlatBank:  # one flat fp32 parameter buffer with a preallocated gradient buffer, as LoRABank exposes them
        def __init__(self, init):
            self.flat = init.reshape(-1).clone().to(dev)
            self.flat_grad = torch.zeros_like(self.flat)
            self.w = self.flat.view(4, 4).requires_grad_(True)
            self.w.grad = self.flat_grad.view(4, 4)

        def set_requires_grad(self, flag):
            self.w.requires_grad_(flag)

        def zero_grad(self):
            self.flat_grad.zero_()

        def mark_updated(self):
            pass
    bank, dbank = FlatBank(T("W0")), FlatBank(T("mix0"))

    def unet(x, B, H, W_, t, ctx, L_, capture_places=(), added=None, kv_cache=None):
        xn, c = untok(x, B, H, W_), ctx.reshape(B, L_, -1)
        shift = c.mean(dim=(1, 2)).reshape(-1, 1, 1, 1)
        y = (torch.tanh(torch.einsum("oc,bchw->bohw", bank.w, xn)) * (1.0 + 1e-3 * float(t)) + 0.3 * shift
             + 0.1 * xn.roll(1, dims=3))
        return tok(y), {}

    def d_unet(x, B, H, W_, t, ctx, L_, capture_places=(), added=None, kv_cache=None):
        xn, c = untok(x, B, H, W_), ctx.reshape(B, L_, -1)
        shift = c.mean(dim=(1, 2)).reshape(-1, 1, 1, 1)
        return tok(torch.einsum("oc,bchw->bohw", dbank.w, xn) + shift + 0.01 * float(t) * xn.flip(1)), {}
    for f in (unet, d_unet):
        f.dtype, f.device, f.cfg = torch.float32, dev, types.SimpleNamespace(addition_embed=False)

    def vae(z, B, H, W_):
        return tok(up(torch.einsum("oc,bchw->bohw", V, untok(z, B, H, W_)))), 8 * H, 8 * W_
    vae.cfg = types.SimpleNamespace(scaling_factor=0.18215)

    def score(img, B, H, W_, ids, mask, crop=None, label_smoothing=None):
        y0, x0, ch, cw = crop
        c = untok(img, B, H, W_)[:, :, y0:y0 + ch, x0:x0 + cw]
        ramp = (torch.linspace(0.5, 1.5, cw).reshape(1, 1, 1, -1) * torch.linspace(1.2, 0.8, ch).reshape(1, 1, -1, 1)).to(dev)
        return (-((c * ramp) ** 2).mean(dim=(1, 2, 3))).mean(), torch.zeros(B, 1, device=dev)
    cfg = StepConfig(resolution=int(gold["resolution"]), total_step=n, K=int(gold["K"]), gan_loss=True, attrcon=False,
                     norm_grad=True, cfg_rescale=float(gold["guidance_rescale"]))
    disc = D_sd(d_unet, dbank, T("head_w0"), T("head_b0"))
    tr = CoMatTrainer(TrainableSDPipeline(unet, vae), bank, types.SimpleNamespace(score=score), disc, cfg)
    batch = dict(prompt_embeds=T("cond"), negative_prompt_embeds=T("null"), gan_null_embeds=T("gan_null"), latents=T("latents"),
                 noises=list(T("noises")), real_latents=T("real"), blip_input_ids=torch.zeros(2, 3, dtype=torch.long),
                 blip_attention_mask=torch.ones(2, 3, dtype=torch.long))
    to_cpu = lambda t: t.detach().float().cpu()
    ox, oy, size = (int(v) for v in gold["crop"])
    logs = tr.train_step(batch, training_steps=[int(i) for i in gold["training_steps"]], crop=(ox, oy, size, size))
    clipped = lambda g, mx: to_cpu(g) * min(1.0, mx / (float(g.norm()) + 1e-6))
    close = lambda a, b, tol: (to_cpu(a) - to_cpu(b)).abs().max() <= tol * (to_cpu(b).abs().max() + 1e-12)
    rn, rn_ref = float(logs["reward_norm"]), float(gold["log:reward_norm"])
    print(f"reward_norm {rn:.8e} vs reference {rn_ref:.8e}: rel {abs(rn - rn_ref) / rn_ref:.2e}")
    assert abs(rn - rn_ref) < 1e-4 * rn_ref
    assert close(clipped(bank.flat_grad, cfg.max_grad_norm).view(4, 4), T("gW"), 1e-3)
    d_all = torch.cat([dbank.flat_grad, disc.head_grad])
    d_clip = clipped(d_all, cfg.max_grad_norm_D)
    assert close(d_clip[:16].view(4, 4), T("gmix"), 1e-3) and close(d_clip[16:20].view(1, 4), T("ghead_w"), 1e-3)
    assert close(d_clip[20:], T("ghead_b"), 1e-3)
    for got, key, start in ((bank.flat.detach().view(4, 4), "W1", "W0"), (dbank.flat.detach().view(4, 4), "mix1", "mix0"),
                            (disc.head[:4].detach().view(1, 4), "head_w1", "head_w0"), (disc.head[4:].detach(), "head_b1", "head_b0")):
        step = (T(key) - T(start)).abs().max()
        assert (got.to(dev) - T(key)).abs().max() <= 2e-3 * step, (key, float((got - T(key)).abs().max()), float(step))
    assert abs(float(logs["step_loss"]) - float(gold["log:step_loss"])) < 1e-4 * abs(float(gold["log:step_loss"]))
    assert abs(float(logs["G_loss"]) - float(gold["log:G_loss"])) < 1e-4 and abs(float(logs["D_loss"]) - float(gold["log:D_loss"])) < 1e-4


# ---- linearity on the tiny real networks -----------------------------------------------------------------------------------
def _grad(dev, gan, **flags):
    cfg, batch, tr = world(dev, gan, **flags)
    logs = tr.train_step(batch, **FIXED)
    return tr.bank.flat_grad.detach().clone(), logs


def test_norm_grad_scales_the_caption_gradient(dev):
    """without the GAN term every path from the loss to the LoRA factors passes the image: the gradient of a norm_grad step is
    1e4 / reward_norm times that of a plain step from the same weights (rel-L2 under the 1e-3 the project uses for LoRA
    gradients against its oracle)"""
    g_plain, logs0 = _grad(dev, False)
    g_norm, logs = _grad(dev, False, norm_grad=True)
    assert "reward_norm" not in logs0
    c = 1e4 / float(logs["reward_norm"])
    err = rel_l2(g_norm, c * g_plain)
    print(f"norm_grad linearity (CM only): c = {c:.4e}, rel-L2 {err:.2e}")
    assert err < 1e-3
    assert float(logs["step_loss"]) == float(logs0["step_loss"])


def test_norm_grad_leaves_the_gan_gradient_alone(dev):
    """with the GAN term: grad = c * grad_CM + (grad_plain - grad_CM) - the generator-side discriminator loss reads the
    latents, not the image, and is not scaled"""
    g_cm, _ = _grad(dev, False)
    g_plain, _ = _grad(dev, True)
    g_norm, logs = _grad(dev, True, norm_grad=True)
    c = 1e4 / float(logs["reward_norm"])
    err = rel_l2(g_norm, c * g_cm + (g_plain - g_cm))
    print(f"norm_grad linearity (CM + GAN): c = {c:.4e}, rel-L2 {err:.2e}")
    assert err < 1e-3


def test_reward_norm_only_measures(dev):
    """reward_norm=True, norm_grad=False: the logged value is the norm a torch hook sees on the same image tensor, and the
    gradients are the bits of a default step"""
    g_plain, _ = _grad(dev, True)
    cfg, batch, tr = world(dev, True, reward_norm=True)
    tr.bank.set_requires_grad(True)
    tr.bank.zero_grad()
    out = tr.compute_losses(batch, **FIXED)
    seen = {}
    out["image"][0].register_hook(lambda g: seen.__setitem__("norm", g.detach().double().norm()))
    out["loss"].backward()
    if dev.type == "cuda":
        ops.join_side_streams()
        torch.cuda.synchronize()
    assert abs(float(tr.reward_norm) - float(seen["norm"])) < 1e-5 * float(seen["norm"])
    assert torch.equal(tr.bank.flat_grad, g_plain)
    cfg, batch, tr2 = world(dev, True, reward_norm=True)
    logs = tr2.train_step(batch, **FIXED)
    assert float(logs["reward_norm"]) == float(tr.reward_norm) and torch.equal(tr2.bank.flat_grad, g_plain)


# ---- host behaviour --------------------------------------------------------------------------------------------------------
def test_norm_grad_step_has_no_host_synchronisation():
    """tests/test_step.py::test_step_has_no_host_synchronisation with norm_grad=True, cfg_rescale=0.7: on the `meta` device any
    attempt to read a tensor's value raises"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from host_overhead import NullKernels
    nk = NullKernels()
    ops.set_kernel_backend(nk)
    try:
        cfg, batch, tr = world(torch.device("meta"), True, dtype=torch.bfloat16, norm_grad=True, cfg_rescale=0.7)
        logs = tr.train_step(batch, **FIXED)
        assert logs["step_loss"].device.type == "meta" and logs["reward_norm"].device.type == "meta"
        tr.train_step(batch)
        assert nk.calls > 0
    finally:
        ops.set_kernel_backend(None)


class _Recorder(SimKernels):
    def __init__(self):
        super().__init__()
        self.seen = []

    def __getattribute__(self, name):
        if name in ("cfg_rescale_ddpm_fwd", "cfg_rescale_ddpm_bwd", "grad_norm_scale", "cfg_ddpm_fwd", "cfg_ddpm_bwd"):
            object.__getattribute__(self, "seen").append(name)
        return object.__getattribute__(self, name)


def test_defaults_issue_no_new_kernel(sim):
    rec = _Recorder()
    ops.set_kernel_backend(rec)  # released by `sim`
    cfg, batch, tr = world(sim, True)
    assert (cfg.cfg_rescale, cfg.norm_grad, cfg.reward_norm) == (0.0, False, False) and tr.reward_norm is None
    logs = tr.train_step(batch, **FIXED)
    assert "reward_norm" not in logs
    assert set(rec.seen) == {"cfg_ddpm_fwd", "cfg_ddpm_bwd"}, set(rec.seen)
    rec.seen.clear()
    cfg, batch, tr = world(sim, True, norm_grad=True, cfg_rescale=0.7)
    tr.train_step(batch, **FIXED)
    # 3 denoise steps, all rescaled; the last two run with grad (trained steps 1 and 2), one image gradient
    assert rec.seen.count("cfg_rescale_ddpm_fwd") == 3 and rec.seen.count("grad_norm_scale") == 1
    assert 1 <= rec.seen.count("cfg_rescale_ddpm_bwd") <= 2 and "cfg_ddpm_fwd" not in rec.seen
