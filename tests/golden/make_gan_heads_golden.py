"""Golden vectors for the discriminator's other two shapes from the reference's OWN code, run in the build container.

    python tests/golden/make_gan_heads_golden.py      # writes tests/golden/gan_heads.npz

As tests/golden/make_gan_golden.py does for the default discriminator, `D_sd.D_sd_pipeline_forward` and
`D_sdxl.D_sd_pipeline_forward` are pulled out of `training_utils/gan_sdxl.py` with `ast` (with `set_D_sd_pipeline_lora` and
`get_D_gt_noise`, which they call) and executed as they are on stand-in objects; nothing of them is stored here, only inputs
and outputs.

Case `lastlayer` (`--gan_unet_lastlayer_cls`, gan_sdxl.py:27-30,81-82,122-123): `D_args.gan_unet_lastlayer_cls = True`.  The
stand-in UNet is a deterministic feature function of (latents, t, condition) to C = 8 channels with one trainable matrix,
followed by `self.mlp = nn.Conv2d(8, 1, 3, 1, 1)` with fixed weights - the reference puts that conv in the UNet's `conv_out`
place, so the UNet's output IS the logit map.  Pinned: the logit map is not passed through another head, its targets and
reduction, who receives a gradient on which side.

Case `sdxl` (`--gan_model_arch gansdxl`, gan_sdxl.py:207-295): `D_sdxl`'s forward with the 4 -> 1 head.  The stand-in UNet also
depends on `added_cond_kwargs["time_ids"]` (per position) and `["text_embeds"]`, so their order and duplication are pinned; what
the UNet was handed for both is stored."""
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_gan_golden as G  # noqa: E402


def reference_methods(cls_name, *names):
    import ast
    import textwrap
    src = open(os.path.join(G.REF, "training_utils", "gan_sdxl.py")).read()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == cls_name)
    ns = {"torch": torch, "nn": nn}
    for name in names:
        fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == name)
        exec(compile(textwrap.dedent(ast.get_source_segment(src, fn)), f"gan_sdxl.py:{cls_name}.{name}", "exec"), ns)
    return [ns[name] for name in names]


def feature_fn(mix, latents, t, cond):
    """[B,4,h,w], scalar t, [B,L,C] -> [B,8,h,w]: channel mix (the trainable matrix [8, 4]) + a per-sample shift from the
    condition + a timestep term, through a tanh (the conv that follows must not commute with it)"""
    lat = latents.float()
    shift = cond.float().mean(dim=(1, 2)).reshape(-1, 1, 1, 1)
    return torch.tanh(torch.einsum("oc,bchw->bohw", mix, lat) + shift + 0.01 * float(t) * torch.cat([lat.flip(1), lat], 1))


def added_term(time_ids, text_embeds, tw, pw):
    """per-sample scalar from the SDXL conditioning: position-sensitive in time_ids, sample-sensitive in text_embeds"""
    return (1e-3 * time_ids.float() @ tw + text_embeds.float() @ pw).reshape(-1, 1, 1, 1)


class FeatureUNet(nn.Module):
    """stand-in for a UNet whose conv_out has been replaced by the classifier conv (gan_sdxl.py:28-30)"""

    def __init__(self, mix, conv):
        super().__init__()
        self.mix = nn.Parameter(mix.clone())
        self.conv_out = conv
        self.calls = []

    def forward(self, latents, t, encoder_hidden_states=None, cross_attention_kwargs=None, return_dict=False):
        self.calls.append(dict(t=int(t), training=self.training, batch=latents.shape[0], cond_batch=encoder_hidden_states.shape[0]))
        return (self.conv_out(feature_fn(self.mix, latents, t, encoder_hidden_states)),)


class AddedUNet(nn.Module):
    def __init__(self, mix, tw, pw):
        super().__init__()
        self.mix = nn.Parameter(mix.clone())
        self.tw, self.pw = tw, pw
        self.calls = []

    def forward(self, latents, t, encoder_hidden_states=None, added_cond_kwargs=None, return_dict=False):
        tid, te = added_cond_kwargs["time_ids"], added_cond_kwargs["text_embeds"]
        self.calls.append(dict(t=int(t), training=self.training, batch=latents.shape[0], cond_batch=encoder_hidden_states.shape[0],
                               time_ids=tid.detach().clone().float(), text_embeds=te.detach().clone().float()))
        return (G.stub_unet_fn(self.mix, latents, t, encoder_hidden_states) + added_term(tid, te, self.tw, self.pw),)


def stand_in(unet, mlp, lastlayer, set_lora, get_gt, flags):
    from oracle import sd as O
    self = types.SimpleNamespace()
    self.unet, self.mlp = unet, mlp
    self.cls_loss_fn = nn.BCEWithLogitsLoss()
    self.D_args = types.SimpleNamespace(condition_discriminator=False, gan_unet_lastlayer_cls=lastlayer)
    self.ori_scheduler = G.StubScheduler(lambda n: O.DDPM().set_timesteps(n))
    self.weight_dtype = torch.float32
    # the discriminator's trainable set (get_trainable_parameters: its LoRA factors - here the stand-in's `mix` - plus the head)
    self.D_parameters = [unet.mix] + list(mlp.parameters())

    def set_and_record(requires_grad=True):
        flags.append(bool(requires_grad))
        set_lora(self, requires_grad=requires_grad)
    self.set_D_sd_pipeline_lora = set_and_record
    self.get_D_gt_noise = lambda device, **kw: get_gt(self, device, **kw)
    return self


def run(fwd, self, fake, kw):
    fake_g = fake.clone().requires_grad_(True)
    g_loss = fwd(self, fake_g, side="G", **kw)
    g_loss.backward()
    touched_g = [p.grad is not None for p in self.D_parameters]
    d_loss = fwd(self, fake.clone().detach(), side="D", **kw)
    d_loss.backward()
    calls = self.unet.calls
    return dict(g_loss=g_loss.detach(), d_loss=d_loss.detach(), g_dfake=fake_g.grad, d_dmix=self.unet.mix.grad.clone(),
                g_side_touched_D=np.array(touched_g), t_used=np.array([c["t"] for c in calls]),
                unet_training=np.array([c["training"] for c in calls]), unet_batch=np.array([c["batch"] for c in calls]),
                cond_batch=np.array([c["cond_batch"] for c in calls]))


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    out = {}
    bs, h, w, L, C, N = 2, 5, 6, 7, 12, 5
    set_lora, get_gt = reference_methods("D_sd", "set_D_sd_pipeline_lora", "get_D_gt_noise")

    # ---- lastlayer: D_sd's forward, the conv in conv_out's place
    (fwd,) = reference_methods("D_sd", "D_sd_pipeline_forward")
    g = torch.Generator().manual_seed(31)
    mix = torch.randn(8, 4, generator=g) * 0.7
    conv = nn.Conv2d(8, 1, 3, 1, 1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(1, 8, 3, 3, generator=g) * 0.4)
        conv.bias.copy_(torch.randn(1, generator=g) * 0.3)
    head_w, head_b = conv.weight.detach().clone(), conv.bias.detach().clone()
    fake, real = torch.randn(bs, 4, h, w, generator=g), torch.randn(bs, 4, h, w, generator=g)
    null = torch.randn(bs, L, C, generator=g)
    flags = []
    self = stand_in(FeatureUNet(mix, conv), conv, True, set_lora, get_gt, flags)
    r = run(fwd, self, fake, dict(negative_prompt_embeds=null, num_inference_steps=N, batch=dict(latents=real)))
    r.update(mix=mix, head_w=head_w, head_b=head_b, fake=fake, real=real, null=null, n_steps=np.int64(N),
             d_dhead_w=conv.weight.grad.clone(), d_dhead_b=conv.bias.grad.clone(), lora_flags=np.array(flags))
    out.update({f"lastlayer:{k}": v for k, v in r.items()})
    print("lastlayer: G loss", float(r["g_loss"]), "D loss", float(r["d_loss"]), "t", r["t_used"], "lora flags", flags)

    # ---- sdxl: D_sdxl's forward, the 4 -> 1 head
    (fwd,) = reference_methods("D_sdxl", "D_sd_pipeline_forward")
    g = torch.Generator().manual_seed(32)
    mix = torch.randn(4, 4, generator=g) * 0.7
    pooled_dim, res = 10, 48
    tw, pw = torch.randn(6, generator=g), torch.randn(pooled_dim, generator=g) * 0.3
    mlp = nn.Sequential(nn.Linear(4, 1))
    with torch.no_grad():
        mlp[0].weight.copy_(torch.randn(1, 4, generator=g) * 0.8)
        mlp[0].bias.copy_(torch.randn(1, generator=g) * 0.3)
    head_w, head_b = mlp[0].weight.detach().clone(), mlp[0].bias.detach().clone()
    fake, real = torch.randn(bs, 4, h, w, generator=g), torch.randn(bs, 4, h, w, generator=g)
    null, pooled = torch.randn(bs, L, C, generator=g), torch.randn(bs, pooled_dim, generator=g)
    flags = []
    self = stand_in(AddedUNet(mix, tw, pw), mlp, False, set_lora, get_gt, flags)
    # D_sdxl.__init__: add_time_ids = [original_size + crops_coords_top_left + target_size] from args.resolution (:193-204)
    self.add_time_ids = torch.tensor([[res, res, 0, 0, res, res]], dtype=torch.float32)
    r = run(fwd, self, fake, dict(negative_prompt_embeds=null, negative_pooled_prompt_embeds=pooled, num_inference_steps=N,
                                  batch=dict(latents=real)))
    calls = self.unet.calls
    r.update(mix=mix, tw=tw, pw=pw, head_w=head_w, head_b=head_b, fake=fake, real=real, null=null, pooled=pooled,
             n_steps=np.int64(N), resolution=np.int64(res), d_dhead_w=mlp[0].weight.grad.clone(),
             d_dhead_b=mlp[0].bias.grad.clone(), lora_flags=np.array(flags),
             g_time_ids=calls[0]["time_ids"], g_text_embeds=calls[0]["text_embeds"],
             d_time_ids=calls[1]["time_ids"], d_text_embeds=calls[1]["text_embeds"])
    out.update({f"sdxl:{k}": v for k, v in r.items()})
    print("sdxl: G loss", float(r["g_loss"]), "D loss", float(r["d_loss"]), "t", r["t_used"], "lora flags", flags)

    np.savez(os.path.join(HERE, "gan_heads.npz"), **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in out.items()})
    print({k: (tuple(v.shape) if hasattr(v, "shape") else v) for k, v in out.items()})


if __name__ == "__main__":
    main()
