"""Golden vectors for the sampler loop WITH RESCALED GUIDANCE from the reference's OWN `TrainableSDPipeline.forward` and
`TrainableSDXLPipeline.forward`, run in the build container.

    python tests/golden/make_sampler_rescale_golden.py      # writes tests/golden/sampler_rescale.npz

The twin of make_sampler_golden.py, whose pieces (`reference_forward`, `stub_unet`, `StubScheduler`) it imports unchanged: the
same stand-ins, seed and cases `a`-`d` (+ the SDXL cases `xa`, `xb`), with `guidance_rescale = 0.7`.  The reference's methods
call `rescale_noise_cfg`, which their module imports from diffusers; diffusers is not installed where the fixtures are made,
so the function below - a restatement of the published formula (Lin et al., arXiv 2305.08891, section 3.4, as shipped in
diffusers' Stable Diffusion pipeline) - is put into the globals of the extracted methods under that name.  Only arrays are
stored.  What the vectors pin on top of sampler_loop.npz: the rescale runs on trained AND untrained steps, after the guidance
combine and before the scheduler step, with statistics per sample over (C, H, W), and the gradient passes through both
standard deviations on the steps that run with grad.

The two conditioning halves of `stub_unet` differ by a per-sample CONSTANT, so in the cases above the two standard deviations
agree and the rescale factor is 1 up to rounding: those cases pin where the call sits and what runs with grad, not its
arithmetic.  The cases `sa`, `sb`, `sd` (SD1.5) and `sxa` (SDXL) therefore repeat `a`, `b`, `d` and `xa` with `spread_unet` =
`stub_unet` plus a term in which the condition scales a shifted copy of the input: the halves then differ in shape, the
factor is away from 1 and the gradient through the statistics is not cancelled."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_sampler_golden as samp  # noqa: E402

PHI = 0.7


def rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale=0.0):
    std_text = noise_pred_text.std(dim=list(range(1, noise_pred_text.ndim)), keepdim=True)
    std_cfg = noise_cfg.std(dim=list(range(1, noise_cfg.ndim)), keepdim=True)
    noise_pred_rescaled = noise_cfg * (std_text / std_cfg)
    return guidance_rescale * noise_pred_rescaled + (1 - guidance_rescale) * noise_cfg


def spread_unet(W, x, t, ctx):
    shift = ctx.mean(dim=(1, 2)).reshape(-1, 1, 1, 1)
    return samp.stub_unet(W, x, t, ctx) + 2.0 * shift * x.roll(1, dims=2)


def with_rescale(forward):
    forward.__globals__["rescale_noise_cfg"] = rescale_noise_cfg
    return forward


def main():
    forward = with_rescale(samp.reference_forward())
    g = torch.Generator().manual_seed(33)  # the draws of make_sampler_golden.main, in its order
    bs, h, w, L, C, N = 2, 4, 5, 6, 8, 5
    W0 = torch.randn(4, 4, generator=g) * 0.6
    V = torch.randn(3, 4, generator=g) * 0.5
    lat0 = torch.randn(bs, 4, h, w, generator=g)
    noises = [torch.randn(bs, 4, h, w, generator=g) for _ in range(N)]
    cond, uncond = torch.randn(bs, L, C, generator=g), torch.randn(bs, L, C, generator=g)
    gimg, glat = torch.randn(bs, 3, h, w, generator=g), torch.randn(bs, 4, h, w, generator=g)
    out = dict(W=W0, V=V, latents=lat0, noises=torch.stack(noises), cond=cond, uncond=uncond, gimg=gimg, glat=glat,
               n_steps=np.int64(N), scaling_factor=np.float64(0.18215), guidance_rescale=np.float64(PHI))
    base = np.load(os.path.join(HERE, "sampler_loop.npz"))
    for k in ("W", "V", "latents", "noises", "cond", "uncond", "gimg", "glat"):
        assert np.array_equal(base[k], out[k].numpy()), f"{k}: not the inputs of sampler_loop.npz"

    def record(name, train, image, latents, Wp, x0, calls):
        out[f"{name}:train"] = np.array(train)
        out[f"{name}:image"] = image.detach().float()
        out[f"{name}:latents"] = latents.detach().float()
        out[f"{name}:dW"] = Wp.grad.clone() if Wp.grad is not None else torch.zeros_like(Wp)
        out[f"{name}:dx0"] = x0.grad.clone() if x0.grad is not None else torch.zeros_like(x0)
        out[f"{name}:unet_grad_mode"] = np.array([c[1] for c in calls])
        out[f"{name}:unet_input_requires_grad"] = np.array([c[2] for c in calls])
        out[f"{name}:t"] = np.array([c[0] for c in calls])
        print(name, train, "grad mode", [int(c[1]) for c in calls], "input grad", [int(c[2]) for c in calls],
              "|dW|", float(out[f"{name}:dW"].norm()), "|dx0|", float(out[f"{name}:dx0"].norm()),
              *(("max |image - unrescaled|", float((out[f"{name}:image"] - torch.from_numpy(base[f"{name}:image"])).abs().max()))
                if f"{name}:image" in base else ()))

    for name, train in {"a": [1, 3], "b": [0, 1, 2, 3, 4], "c": [4], "d": [], "sa": [1, 3], "sb": [0, 1, 2, 3, 4], "sd": []}.items():
        net = spread_unet if name.startswith("s") else samp.stub_unet
        Wp = W0.clone().requires_grad_(True)
        x0 = lat0.clone().requires_grad_(True)
        calls = []

        def unet(x, t, encoder_hidden_states=None, cross_attention_kwargs=None, return_dict=False):
            calls.append((int(t), bool(torch.is_grad_enabled()), bool(x.requires_grad)))
            return (net(Wp, x, int(t), encoder_hidden_states),)
        self = types.SimpleNamespace(_execution_device=torch.device("cpu"), unet=unet, scheduler=samp.StubScheduler(noises))
        self.encode_prompt = lambda prompt, device, n, cfg, neg, prompt_embeds=None, negative_prompt_embeds=None, lora_scale=None: \
            (prompt_embeds, negative_prompt_embeds)
        self.prepare_latents = lambda b, c, hh, ww, dtype, device, generator, latents: latents
        self.prepare_extra_step_kwargs = lambda generator, eta: {}
        self.vae = types.SimpleNamespace(dtype=torch.float32, config=types.SimpleNamespace(scaling_factor=0.18215),
                                         decode=lambda z, return_dict=False: (torch.einsum("oc,bchw->bohw", V, z),))
        prev = torch.is_grad_enabled()
        image, latents = forward(self, height=8 * h, width=8 * w, training_timesteps=list(train), detach_gradient=True,
                                 bp_on_trained=True, num_inference_steps=N, guidance_scale=7.5, guidance_rescale=PHI,
                                 latents=x0 * 1.0, prompt_embeds=cond, negative_prompt_embeds=uncond, output_type="image",
                                 return_latents=True)
        torch.set_grad_enabled(prev)  # the reference leaves the global grad mode wherever its last gate put it
        loss = (image * gimg).sum() + (latents * glat).sum()
        if loss.requires_grad:
            loss.backward()
        record(name, train, image, latents, Wp, x0, calls)

    forward_xl = with_rescale(samp.reference_forward("TrainableSDXLPipeline"))
    pooled, npooled = torch.randn(bs, 5, generator=g), torch.randn(bs, 5, generator=g)
    assert np.array_equal(base["pooled"], pooled.numpy()) and np.array_equal(base["npooled"], npooled.numpy())
    out.update(pooled=pooled, npooled=npooled)

    def stub_unet_xl(W, x, t, ctx, text_embeds, time_ids, net):
        extra = (text_embeds.mean(dim=1) + 1e-3 * time_ids.float().sum(dim=1)).reshape(-1, 1, 1, 1)
        return net(W, x, t, ctx) + 0.2 * extra
    for name, train in (("xa", [1, 3]), ("xb", [0, 1, 2, 3, 4]), ("sxa", [1, 3])):
        net = spread_unet if name.startswith("s") else samp.stub_unet
        Wp = W0.clone().requires_grad_(True)
        x0 = lat0.clone().requires_grad_(True)
        calls = []

        def unet(x, t, encoder_hidden_states=None, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False):
            calls.append((int(t), bool(torch.is_grad_enabled()), bool(x.requires_grad)))
            return (stub_unet_xl(Wp, x, int(t), encoder_hidden_states, added_cond_kwargs["text_embeds"], added_cond_kwargs["time_ids"], net),)
        self = types.SimpleNamespace(_execution_device=torch.device("cpu"), unet=unet, scheduler=samp.StubScheduler(noises))
        self.encode_prompt = lambda **kw: (kw["prompt_embeds"], kw["negative_prompt_embeds"], kw["pooled_prompt_embeds"],
                                           kw["negative_pooled_prompt_embeds"])
        self.prepare_latents = lambda b, c, hh, ww, dtype, device, generator, latents: latents
        self.prepare_extra_step_kwargs = lambda generator, eta: {}
        self._get_add_time_ids = lambda osz, crop, tsz, dtype=None: torch.tensor([list(osz) + list(crop) + list(tsz)], dtype=dtype)
        self.vae = types.SimpleNamespace(config=types.SimpleNamespace(scaling_factor=0.13025),
                                         decode=lambda z, return_dict=False: (torch.einsum("oc,bchw->bohw", V.to(z.dtype), z),))
        prev = torch.is_grad_enabled()
        image, latents = forward_xl(self, height=8 * h, width=8 * w, training_timesteps=list(train), detach_gradient=True,
                                    num_inference_steps=N, guidance_scale=7.5, guidance_rescale=PHI, latents=x0 * 1.0,
                                    prompt_embeds=cond, negative_prompt_embeds=uncond, pooled_prompt_embeds=pooled,
                                    negative_pooled_prompt_embeds=npooled, return_latents=True)
        torch.set_grad_enabled(prev)
        ((image.float() * gimg).sum() + (latents.float() * glat).sum()).backward()
        record(name, train, image, latents, Wp, x0, calls)
    out["xl_scaling_factor"] = np.float64(0.13025)
    np.savez_compressed(os.path.join(HERE, "sampler_rescale.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()})


if __name__ == "__main__":
    main()
