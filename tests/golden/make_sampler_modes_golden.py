"""Golden vectors for the sampler's OTHER MODES - `early_exit`, `double_laststep`, `fast_training`, `bp_on_trained=False`,
`detach_gradient=False`, guidance off - from the reference's OWN `TrainableSDPipeline.forward` and
`TrainableSDXLPipeline.forward`, run in the build container.

    python tests/golden/make_sampler_modes_golden.py      # writes tests/golden/sampler_modes.npz

The twin of make_sampler_rescale_golden.py: `reference_forward`, `stub_unet` and `spread_unet` are imported unchanged, with the
same seed and inputs (asserted against sampler_loop.npz).  The scheduler stand-in is this file's own, because the modes read two
things `StubScheduler` does not have: `step(...).pred_original_sample` (what `early_exit` returns) and `add_noise` (the
re-noising of `double_laststep`).  Both are restated here from the `alphas_cumprod` of oracle/sd.py's `DDPM`, as DDPMScheduler
defines them for epsilon prediction: x0 = (x - sqrt(1 - abar_t) eps) / sqrt(abar_t), noisy = sqrt(abar_t) x + sqrt(1 - abar_t)
noise.  `double_laststep` draws its re-noising with `torch.randn_like` from the global generator: it is seeded right before the
call and the same draw is stored as `renoise`; the extra scheduler step of that mode takes one more step noise, `noise_extra`,
drawn after everything the other fixtures draw.  Only arrays are stored.

Cases (N = 5; guidance 7.5, detach_gradient=True, bp_on_trained=True unless said):
    e1   early_exit, train [1, 3]          e2   early_exit, train [4]          e3   early_exit, train []: no exit
    se1  e1 on `spread_unet` with guidance_rescale 0.7: the rescale factor inside pred_original_sample
    dl1  double_laststep, train [1, 3]: the last loop step is untrained -> the detached noisy input
    dl2  double_laststep, train [2, 4]: the last loop step is a trained one -> `do_detach` is False and the reference feeds the
         LAST LOOP STEP's model input to the extra call, not the noisy one
    f1   fast_training, train [1, 3]       f2   fast_training + early_exit, train [0, 2, 4]
    g1   guidance_scale 1.0, negative_prompt_embeds None, train [1, 3]          g2   g1 with guidance_rescale 0.7 (== g1)
    b1   bp_on_trained=False, train [1, 3]          b2   detach_gradient=False, train [1, 3]
    xe   SDXL, early_exit, train [1, 3]: a plain break after the trained step's prev_sample
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_sampler_golden as samp  # noqa: E402
import make_sampler_rescale_golden as resc  # noqa: E402

RENOISE_SEED = 4242


class ModesScheduler(samp.StubScheduler):
    """StubScheduler + the two members the modes read"""

    def step(self, eps, t, x, return_dict=True, **kw):
        z = self.noises[self.i]
        self.i += 1
        prev = self.ddpm.step(eps, int(t), x, z)
        a_t = float(self.ddpm.alphas_cumprod[int(t)])
        x0 = (x - (1.0 - a_t) ** 0.5 * eps) / a_t ** 0.5
        return types.SimpleNamespace(prev_sample=prev, pred_original_sample=x0) if return_dict else (prev,)

    def add_noise(self, x, noise, t):
        a_t = float(self.ddpm.alphas_cumprod[int(t)])
        return a_t ** 0.5 * x + (1.0 - a_t) ** 0.5 * noise


CASES = {  # name: (train, spread, forward keywords)
    "e1": ([1, 3], False, dict(early_exit=True)),
    "e2": ([4], False, dict(early_exit=True)),
    "e3": ([], False, dict(early_exit=True)),
    "se1": ([1, 3], True, dict(early_exit=True, guidance_rescale=resc.PHI)),
    "dl1": ([1, 3], False, dict(double_laststep=True)),
    "dl2": ([2, 4], False, dict(double_laststep=True)),
    "f1": ([1, 3], False, dict(fast_training=True)),
    "f2": ([0, 2, 4], False, dict(fast_training=True, early_exit=True)),
    "g1": ([1, 3], False, dict(guidance_scale=1.0)),
    "g2": ([1, 3], False, dict(guidance_scale=1.0, guidance_rescale=resc.PHI)),
    "b1": ([1, 3], False, dict(bp_on_trained=False)),
    "b2": ([1, 3], False, dict(detach_gradient=False)),
}


def main():
    forward = resc.with_rescale(samp.reference_forward())
    g = torch.Generator().manual_seed(33)  # the draws of make_sampler_golden.main, in its order
    bs, h, w, L, C, N = 2, 4, 5, 6, 8, 5
    W0 = torch.randn(4, 4, generator=g) * 0.6
    V = torch.randn(3, 4, generator=g) * 0.5
    lat0 = torch.randn(bs, 4, h, w, generator=g)
    noises = [torch.randn(bs, 4, h, w, generator=g) for _ in range(N)]
    cond, uncond = torch.randn(bs, L, C, generator=g), torch.randn(bs, L, C, generator=g)
    gimg, glat = torch.randn(bs, 3, h, w, generator=g), torch.randn(bs, 4, h, w, generator=g)
    pooled, npooled = torch.randn(bs, 5, generator=g), torch.randn(bs, 5, generator=g)
    noise_extra = torch.randn(bs, 4, h, w, generator=g)  # the step noise of double_laststep's extra step
    torch.manual_seed(RENOISE_SEED)
    renoise = torch.randn(bs, 4, h, w)
    out = dict(W=W0, V=V, latents=lat0, noises=torch.stack(noises), cond=cond, uncond=uncond, gimg=gimg, glat=glat,
               pooled=pooled, npooled=npooled, noise_extra=noise_extra, renoise=renoise, n_steps=np.int64(N),
               scaling_factor=np.float64(0.18215), xl_scaling_factor=np.float64(0.13025), guidance_rescale=np.float64(resc.PHI))
    base = np.load(os.path.join(HERE, "sampler_loop.npz"))
    for k in ("W", "V", "latents", "noises", "cond", "uncond", "gimg", "glat", "pooled", "npooled"):
        assert np.array_equal(base[k], out[k].numpy()), f"{k}: not the inputs of sampler_loop.npz"

    def record(name, train, kw, image, latents, Wp, x0, calls):
        out[f"{name}:train"] = np.array(train, dtype=np.int64)
        out[f"{name}:image"] = image.detach().float()
        out[f"{name}:latents"] = latents.detach().float()
        out[f"{name}:dW"] = Wp.grad.clone() if Wp.grad is not None else torch.zeros_like(Wp)
        out[f"{name}:dx0"] = x0.grad.clone() if x0.grad is not None else torch.zeros_like(x0)
        out[f"{name}:unet_grad_mode"] = np.array([c[1] for c in calls])
        out[f"{name}:unet_input_requires_grad"] = np.array([c[2] for c in calls])
        out[f"{name}:t"] = np.array([c[0] for c in calls], dtype=np.int64)
        print(name, train, kw, "t", [c[0] for c in calls], "grad mode", [int(c[1]) for c in calls], "input grad",
              [int(c[2]) for c in calls], "|dW|", float(out[f"{name}:dW"].norm()), "|dx0|", float(out[f"{name}:dx0"].norm()))

    for name, (train, spread, kw) in CASES.items():
        net = resc.spread_unet if spread else samp.stub_unet
        Wp = W0.clone().requires_grad_(True)
        x0 = lat0.clone().requires_grad_(True)
        calls = []

        def unet(x, t, encoder_hidden_states=None, cross_attention_kwargs=None, return_dict=False):
            calls.append((int(t), bool(torch.is_grad_enabled()), bool(x.requires_grad)))
            return (net(Wp, x, int(t), encoder_hidden_states),)
        self = types.SimpleNamespace(_execution_device=torch.device("cpu"), unet=unet,
                                     scheduler=ModesScheduler(noises + [noise_extra]))
        self.encode_prompt = lambda prompt, device, n, cfg, neg, prompt_embeds=None, negative_prompt_embeds=None, lora_scale=None: \
            (prompt_embeds, negative_prompt_embeds)
        self.prepare_latents = lambda b, c, hh, ww, dtype, device, generator, latents: latents
        self.prepare_extra_step_kwargs = lambda generator, eta: {}
        self.vae = types.SimpleNamespace(dtype=torch.float32, config=types.SimpleNamespace(scaling_factor=0.18215),
                                         decode=lambda z, return_dict=False: (torch.einsum("oc,bchw->bohw", V, z),))
        args = dict(detach_gradient=True, bp_on_trained=True, guidance_scale=7.5)
        args.update(kw)
        guided = args["guidance_scale"] > 1.0
        prev = torch.is_grad_enabled()
        torch.manual_seed(RENOISE_SEED)  # double_laststep: its torch.randn_like is the first draw from the global generator
        image, latents = forward(self, height=8 * h, width=8 * w, training_timesteps=list(train), num_inference_steps=N,
                                 latents=x0 * 1.0, prompt_embeds=cond, negative_prompt_embeds=uncond if guided else None,
                                 output_type="image", return_latents=True, **args)
        torch.set_grad_enabled(prev)  # the reference leaves the global grad mode wherever its last gate put it
        loss = (image * gimg).sum() + (latents * glat).sum()
        if loss.requires_grad:
            loss.backward()
        record(name, train, kw, image, latents, Wp, x0, calls)

    forward_xl = resc.with_rescale(samp.reference_forward("TrainableSDXLPipeline"))

    def stub_unet_xl(W, x, t, ctx, text_embeds, time_ids):
        extra = (text_embeds.mean(dim=1) + 1e-3 * time_ids.float().sum(dim=1)).reshape(-1, 1, 1, 1)
        return samp.stub_unet(W, x, t, ctx) + 0.2 * extra
    for name, train, kw in (("xe", [1, 3], dict(early_exit=True)),):
        Wp = W0.clone().requires_grad_(True)
        x0 = lat0.clone().requires_grad_(True)
        calls = []

        def unet(x, t, encoder_hidden_states=None, cross_attention_kwargs=None, added_cond_kwargs=None, return_dict=False):
            calls.append((int(t), bool(torch.is_grad_enabled()), bool(x.requires_grad)))
            return (stub_unet_xl(Wp, x, int(t), encoder_hidden_states, added_cond_kwargs["text_embeds"], added_cond_kwargs["time_ids"]),)
        self = types.SimpleNamespace(_execution_device=torch.device("cpu"), unet=unet, scheduler=ModesScheduler(noises))
        self.encode_prompt = lambda **kw_: (kw_["prompt_embeds"], kw_["negative_prompt_embeds"], kw_["pooled_prompt_embeds"],
                                            kw_["negative_pooled_prompt_embeds"])
        self.prepare_latents = lambda b, c, hh, ww, dtype, device, generator, latents: latents
        self.prepare_extra_step_kwargs = lambda generator, eta: {}
        self._get_add_time_ids = lambda osz, crop, tsz, dtype=None: torch.tensor([list(osz) + list(crop) + list(tsz)], dtype=dtype)
        self.vae = types.SimpleNamespace(config=types.SimpleNamespace(scaling_factor=0.13025),
                                         decode=lambda z, return_dict=False: (torch.einsum("oc,bchw->bohw", V.to(z.dtype), z),))
        prev = torch.is_grad_enabled()
        image, latents = forward_xl(self, height=8 * h, width=8 * w, training_timesteps=list(train), detach_gradient=True,
                                    num_inference_steps=N, guidance_scale=7.5, latents=x0 * 1.0, prompt_embeds=cond,
                                    negative_prompt_embeds=uncond, pooled_prompt_embeds=pooled,
                                    negative_pooled_prompt_embeds=npooled, return_latents=True, **kw)
        torch.set_grad_enabled(prev)
        ((image.float() * gimg).sum() + (latents.float() * glat).sum()).backward()
        record(name, train, kw, image, latents, Wp, x0, calls)
    np.savez_compressed(os.path.join(HERE, "sampler_modes.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()})


if __name__ == "__main__":
    main()
