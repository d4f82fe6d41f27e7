"""GAN fidelity discriminator: a second UNet (own LoRA) + a per-latent-pixel classifier head + BCE-with-logits.

Mirrors `D_sd` / `D_sd.D_sd_pipeline_forward` (training_utils/gan_sdxl.py:7-132), `D_sdxl.D_sd_pipeline_forward`
(:207-295) and the factory `load_discriminator` (training_utils/gan_sd_model.py:8-14).  G side: discriminator frozen,
target 1, gradient flows to the generated latents.  D side: batch [fake.detach(); real], targets [0; 1], gradient to D's
LoRA factors and the head.  Two heads:
  * Linear(4, 1) on the UNet's output (gan_sdxl.py:32-35).  The UNet output is already channels-last, so the reference's
    `permute(0,2,3,1)` disappears and the head + BCE is one kernel (`comat_disc_head_*`);
  * `--gan_unet_lastlayer_cls` (gan_sdxl.py:27-30,81-82,122-123): the UNet's conv_out IS the head, a trainable
    Conv2d(C, 1, 3, padding=1) whose output is the logit map.  The UNet stops after conv_norm_out + SiLU (`UNet.features`)
    and conv + BCE run in `comat_disc_convhead_*`; the UNet's own conv_out weights are not used.
"""
from __future__ import annotations

import torch

from . import ops
from .pipeline import DDPMScheduler
from .unet import LoRABank, UNet


class D_sd:
    def __init__(self, unet: UNet, bank: LoRABank, head_w: torch.Tensor, head_b: torch.Tensor, lastlayer_cls=False):
        """head_w: [1, 4] / [4] (Linear head) or, with lastlayer_cls, the Conv2d weight [1, C, 3, 3]; head_b: [1]"""
        self.unet, self.bank = unet, bank
        self.lastlayer_cls = bool(lastlayer_cls)
        dev = unet.device
        if self.lastlayer_cls:
            w = ops.conv_weight_to_taps(head_w.float())  # [9, C] tap-major: the layout of comat_disc_convhead_*
            self.head_shape = tuple(w.shape)
        else:
            w = head_w.reshape(4).float()
            self.head_shape = (4,)
        n = w.numel()
        # head parameters live at the tail of one small flat fp32 buffer so that the optimizer/all-reduce see them
        self.head = torch.cat([w.reshape(n), head_b.reshape(1).float()]).to(dev)
        self.head_grad = torch.zeros(n + 1, dtype=torch.float32, device=dev)
        self.w = self.head[:n].view(self.head_shape).requires_grad_(True)
        self.b = self.head[n:].requires_grad_(True)
        self.w.grad, self.b.grad = self.head_grad[:n].view(self.head_shape), self.head_grad[n:]
        self.ori_scheduler = DDPMScheduler()
        self._targets = {}

    def _target(self, bs, side):
        key = (bs, side)
        if key not in self._targets:
            t = torch.ones(bs) if side == "G" else torch.cat([torch.zeros(bs), torch.ones(bs)])
            self._targets[key] = t.to(self.unet.device)
        return self._targets[key]

    def zero_grad(self):
        self.bank.zero_grad()
        self.head_grad.zero_()

    def set_D_sd_pipeline_lora(self, requires_grad=True):
        self.bank.set_requires_grad(requires_grad)
        self.w.requires_grad_(requires_grad)
        self.b.requires_grad_(requires_grad)

    def head_state_dict(self):
        """what `torch.save(self.mlp.state_dict())` writes (training_script.py:426): nn.Sequential(nn.Linear(4, 1)) ->
        "0.weight" [1, 4], "0.bias" [1]; nn.Conv2d(C, 1, 3, padding=1) -> "weight" [1, C, 3, 3], "bias" [1]"""
        b = self.b.detach().reshape(1).cpu().clone()
        if self.lastlayer_cls:
            return {"weight": ops.taps_to_conv_weight(self.w.detach().cpu()), "bias": b}
        return {"0.weight": self.w.detach().reshape(1, 4).cpu().clone(), "0.bias": b}

    def load_head_state_dict(self, sd):
        kw, kb = ("weight", "bias") if self.lastlayer_cls else ("0.weight", "0.bias")
        want = (1, self.head_shape[1], 3, 3) if self.lastlayer_cls else (1, 4)
        if set(sd) != {kw, kb} or tuple(sd[kw].shape) != want or sd[kb].numel() != 1:
            raise ValueError(f"discriminator head: the state dict {({k: tuple(v.shape) for k, v in sd.items()})} is not that of "
                             f"{'Conv2d' if self.lastlayer_cls else 'Sequential(Linear(4, 1))'}: expected {kw} {want}, {kb} (1,)")
        with torch.no_grad():
            w = ops.conv_weight_to_taps(sd[kw].float()) if self.lastlayer_cls else sd[kw].reshape(4)
            self.w.copy_(w.to(self.w.device, torch.float32))
            self.b.copy_(sd[kb].reshape(1).to(self.b.device, torch.float32))

    def _added(self, pooled, B, copies):
        """the UNet's `added` conditioning of a batch of B = copies * bs samples; SD1.5 has none"""
        return None

    def _loss(self, x, B, h, w, t, ctx, L, target, added):
        u = self.unet
        kw = {} if added is None else {"added": added}
        if self.lastlayer_cls:
            return ops.disc_convhead_loss(u.features(x, B, h, w, t, ctx, L, **kw), self.w, self.b, target, B, h, w)
        eps, _ = u(x, B, h, w, t, ctx, L, **kw)
        return ops.disc_head_loss(eps, self.w, self.b, target, h * w)

    def D_sd_pipeline_forward(self, training_latents, side="G", *, negative_prompt_embeds, num_inference_steps,
                              h, w, real_latents=None, negative_pooled_prompt_embeds=None):
        """training_latents: fp32 channels-last tokens [bs*h*w, 4]; negative_prompt_embeds (bs, L, C) null embedding;
        real_latents: tokens [bs*h*w, 4] (D side: `batch['latents']`, gan_sdxl.py:46-48);
        negative_pooled_prompt_embeds (bs, pooled): the null prompt's pooled embedding, D_sdxl only."""
        u = self.unet
        T, dev = u.dtype, u.device
        bs, L, _ = negative_prompt_embeds.shape
        t_last = self.ori_scheduler.set_timesteps(num_inference_steps)[-1]
        null = negative_prompt_embeds.to(dev, torch.float32)
        if side == "G":
            self.set_D_sd_pipeline_lora(False)
            ctx = ops.cast(null.reshape(bs * L, -1).contiguous(), T)
            return self._loss(ops.cast_grad(training_latents, T), bs, h, w, t_last, ctx, L, self._target(bs, "G"),
                              self._added(negative_pooled_prompt_embeds, bs, 1))
        if side == "D":
            self.set_D_sd_pipeline_lora(True)
            with torch.no_grad():
                x = ops.concat_rows(training_latents.detach(), real_latents.to(dev, torch.float32))
                x = ops.cast(x, T)
            ctx = ops.cast(torch.cat([null, null]).reshape(2 * bs * L, -1).contiguous(), T)
            return self._loss(x, 2 * bs, h, w, t_last, ctx, L, self._target(bs, "D"),
                              self._added(negative_pooled_prompt_embeds, 2 * bs, 2))
        raise ValueError(side)


class D_sdxl(D_sd):
    """`--gan_model_arch gansdxl`: the discriminator is an SDXL UNet (`D_sdxl.D_sd_pipeline_forward`, gan_sdxl.py:207-295).
    It takes `added_cond_kwargs`: time_ids = (resolution, resolution, 0, 0, resolution, resolution) for every sample
    (:193-204,219,262), text_embeds = the null prompt's pooled embedding, concatenated twice on the D side (:222,265-269).
    The reference's constructor cannot run (it calls `super().__init__()` without arguments); this one has D_sd's shape
    plus the training resolution."""

    def __init__(self, unet: UNet, bank: LoRABank, head_w, head_b, lastlayer_cls=False, resolution=512):
        super().__init__(unet, bank, head_w, head_b, lastlayer_cls)
        self.resolution = int(resolution)

    def _added(self, pooled, B, copies):
        if pooled is None:
            raise ValueError("D_sdxl needs negative_pooled_prompt_embeds (the null prompt's pooled embedding)")
        res = self.resolution
        pooled = pooled.to(self.unet.device, torch.float32)
        if copies > 1:
            pooled = torch.cat([pooled] * copies)
        return self.unet.added_embedding(pooled, [[res, res, 0, 0, res, res]] * B)


def load_discriminator(arch, unet, bank, head_w, head_b, lastlayer_cls=False, resolution=512):
    """gan_sd_model.py:8-14: 'gan' is stripped from `--gan_model_arch`; 'sd_1_5' -> D_sd, anything with 'sdxl' -> D_sdxl
    (the reference returns None for every other name; here that is an error)"""
    arch = arch.replace("gan", "")
    if arch == "sd_1_5":
        return D_sd(unet, bank, head_w, head_b, lastlayer_cls)
    if "sdxl" in arch:
        return D_sdxl(unet, bank, head_w, head_b, lastlayer_cls, resolution)
    raise ValueError(f"unknown discriminator architecture '{arch}' (sd_1_5 or sdxl)")
