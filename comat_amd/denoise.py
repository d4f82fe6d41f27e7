"""Denoising fine-tune from images (noise-prediction MSE): image -> VAE encoder -> noised latent -> UNet -> MSE against the noise ->
clip + AdamW.  The counterpart of the step the reference's SDXL recipe begins with - diffusers' train_text_to_image_sdxl.py run
"for only 100 steps" on SDXL's own 1024^2 samples resized to 512^2 (reference README.md:78-80), whose result the reference loads as
`--sdxl_unet_path` (training_utils/pipeline.py:27-28).  INTEGRATION.md walks through the recipe with this package.

One step issues: the frozen encoder (unet.VAEEncoder, no autograd), ONE comat_denoise_prepare launch (posterior sample, scaling,
add_noise at a timestep PER SAMPLE, cast, the timesteps' sinusoid rows and loss weights from tables built here once), the UNet with
that [B, C0] sinusoid tensor as its `t`, comat_mse_fwd / comat_mse_bwd, and the generator's update of CoMatTrainer._apply_updates
(step.FlatAdamW: clip by the global norm, AdamW, the schedule, the skip of a non-finite gradient).  Timesteps and noises that the
batch does not carry are drawn on the device; nothing in a step reads a device value on the host.

Eager only.  Not built: hipGraph capture of this step, more than one GPU, the fp8 forward, 8-bit Adam,
noise_offset, v-prediction, EMA, a dataset / image-file reader."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .pipeline import DDPMScheduler
from .step import FlatAdamW, lr_schedule
from .unet import UNetBank, timestep_embedding


@dataclass
class DenoiseConfig:
    """the path-relevant arguments of diffusers' train_text_to_image_sdxl.py, under its names and defaults"""
    lr: float = 1e-4
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_weight_decay: float = 1e-2
    adam_epsilon: float = 1e-8
    max_grad_norm: float = 1.0
    lr_scheduler: str = "constant"     # the fields of step.StepConfig, evaluated by the same kernels
    lr_warmup_steps: int = 0
    max_train_steps: int | None = None
    lr_num_cycles: float | None = None
    lr_power: float = 1.0
    lr_steps_per_update: int = 1
    snr_gamma: float | None = None     # --snr_gamma: the loss weight min(snr_t, gamma) / snr_t per sample; None: 1
    sample_posterior: bool = True      # latent_dist.sample(); False: latent_dist.mode()
    prediction_type: str = "epsilon"
    use_8bit_adam: bool = False
    gradient_checkpointing: bool = False
    fp8_forward: bool = False

    def __post_init__(self):
        if self.prediction_type != "epsilon":
            raise ValueError(f"DenoiseConfig.prediction_type = {self.prediction_type!r}: only 'epsilon' is built (the sampler of this "
                             "package predicts the noise)")
        for flag in ("use_8bit_adam", "gradient_checkpointing", "fp8_forward"):
            if getattr(self, flag):
                raise ValueError(f"DenoiseConfig.{flag} is not built for the denoising step")
        if self.snr_gamma is not None and not self.snr_gamma > 0:
            raise ValueError(f"DenoiseConfig.snr_gamma must be positive or None (got {self.snr_gamma})")


def snr_weights(scheduler: DDPMScheduler, snr_gamma):
    """float64 [T]: min(snr_t, gamma) / snr_t with snr_t = abar_t / (1 - abar_t) (compute_snr + the epsilon branch of
    train_text_to_image_sdxl.py); ones without a gamma"""
    abar = scheduler.alphas_cumprod.double().numpy()
    if snr_gamma is None:
        return np.ones_like(abar)
    snr = abar / (1.0 - abar)
    return np.minimum(snr, float(snr_gamma)) / snr


def denoise_tables(scheduler: DDPMScheduler, C0, device, snr_gamma=None) -> ops.DenoiseTables:
    """the tables comat_denoise_prepare reads, for every training timestep: sab[t] = scheduler.add_noise_coefficients(t) (the
    values ops.add_noise is given), sinus[t] = unet.timestep_embedding(t, C0, 1) (that function's own rows),
    wtab = snr_weights - each rounded to fp32 once"""
    T = scheduler.num_train_timesteps
    sab = np.array([scheduler.add_noise_coefficients(t) for t in range(T)], dtype=np.float64).astype(np.float32)
    sinus = torch.cat([timestep_embedding(t, C0, 1) for t in range(T)]).numpy()
    return ops.DenoiseTables(sab, sinus, snr_weights(scheduler, snr_gamma).astype(np.float32), device)


def _moments(vae_encoder, pixel_values):
    px = pixel_values.to(vae_encoder.device, torch.float32)
    B, _, H, W = px.shape
    m, h, w = vae_encoder(ops.nchw_to_tokens(px), B, H, W)
    return m, B, h, w


def encode_images(vae_encoder, pixel_values, sample=False, noise=None):
    """pixel_values [B, 3, H, W] in [-1, 1] -> latents * scaling_factor, fp32 [B, C, H / f, W / f] - the layout of a stored
    `batch["latents"]` record (gt_latents.write_gt_records, Gan_Dataset), so that the discriminator's "real" latents can come from
    real images.  sample: draw from the posterior (noise [B, C, h, w], or drawn on the device) instead of taking its mean.  A u8
    image becomes pixel_values by `x.float() / 127.5 - 1` at the dataset's edge."""
    m, B, h, w = _moments(vae_encoder, pixel_values)
    C = m.shape[1] // 2
    dev = m.device
    z = None
    if sample:
        z = torch.randn((B * h * w, C), device=dev) if noise is None else ops.nchw_to_tokens(noise.to(dev, torch.float32))
    tab = ops.DenoiseTables([[1.0, 0.0]], [[0.0, 0.0]], [1.0], dev)  # one "timestep" that adds no noise: x0 is what is asked for
    _, _, _, x0 = ops.denoise_prepare(tab, torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros((B * h * w, C), device=dev),
                                      torch.float32, moments=m, z=z, scaling=vae_encoder.cfg.scaling_factor, want_x0=True)
    return ops.tokens_to_nchw(x0, B, h, w)


class DenoiseTrainer:
    """bank: the unet.UNetBank the UNet was built from (the recipe: every parameter trained) or its LoRABank.  vae_encoder: a
    unet.VAEEncoder, or None when every batch carries `latents`."""

    def __init__(self, unet, bank, vae_encoder, cfg: DenoiseConfig, scheduler: DDPMScheduler | None = None, seed=0):
        self.unet, self.bank, self.vae, self.cfg = unet, bank, vae_encoder, cfg
        self.scheduler = scheduler or DDPMScheduler()
        self.full = isinstance(bank, UNetBank)
        if (unet.bank if self.full else unet.lora) is not bank:
            raise ValueError("DenoiseTrainer: the UNet was not built over this bank (UNet(..., bank=ubank) / UNet(..., lora=lbank))")
        if getattr(unet, "fp8", False):
            raise ValueError("DenoiseTrainer: the UNet runs the fp8 forward (fp8_forward), which is not built for the denoising step")
        self.device = dev = torch.device(unet.device)
        self.tab = denoise_tables(self.scheduler, unet.cfg.block_out_channels[0], dev, cfg.snr_gamma)
        self.opt = FlatAdamW([(bank.flat, bank.flat_grad)], cfg.lr, (cfg.adam_beta1, cfg.adam_beta2), cfg.adam_epsilon,
                             cfg.adam_weight_decay, cfg.max_grad_norm,
                             schedule=lr_schedule(cfg.lr_scheduler, cfg.lr, cfg.lr_warmup_steps, cfg.max_train_steps, cfg.lr_num_cycles,
                                                  cfg.lr_power, cfg.lr_steps_per_update))
        self.gen = torch.Generator(device=dev).manual_seed(seed)
        self.oob = torch.zeros(1, dtype=torch.int32, device=dev)  # 1 once a timestep outside the schedule was handed in
        self._lr_const = None if self.opt.lr_now is not None else torch.full((1,), cfg.lr, dtype=torch.float32, device=dev)

    def _tokens(self, x):
        return ops.nchw_to_tokens(x.to(self.device, torch.float32))

    def compute_loss(self, batch):
        """forward of one step -> (loss [1] under autograd, per_sample [B], the timesteps used)"""
        cfg, dev, T = self.cfg, self.device, self.unet.dtype
        randn = lambda *s: torch.randn(s, generator=self.gen, device=dev)
        if batch.get("pixel_values") is not None:
            if self.vae is None:
                raise ValueError("DenoiseTrainer: the batch carries pixel_values but the trainer was built without a vae_encoder")
            m, B, h, w = _moments(self.vae, batch["pixel_values"])
            C = m.shape[1] // 2
            z = None
            if cfg.sample_posterior:
                z = self._tokens(batch["posterior_noise"]) if batch.get("posterior_noise") is not None else randn(B * h * w, C)
            src = dict(moments=m, z=z, scaling=self.vae.cfg.scaling_factor)
            size = tuple(batch["pixel_values"].shape[2:])
        else:
            lat = batch["latents"]
            B, C, h, w = lat.shape
            src = dict(latents=self._tokens(lat))
            size = (8 * h, 8 * w)
        noise = self._tokens(batch["noise"]) if batch.get("noise") is not None else randn(B * h * w, C)
        if batch.get("timesteps") is not None:
            t = batch["timesteps"].to(dev, torch.int32)
        else:
            t = torch.randint(0, self.tab.T, (B,), generator=self.gen, device=dev, dtype=torch.int32)
        xin, temb, wts, _ = ops.denoise_prepare(self.tab, t, noise, T, oob=self.oob, **src)
        pe = batch["prompt_embeds"]
        L = pe.shape[1]
        ctx = ops.cast(pe.to(dev, torch.float32).reshape(B * L, -1).contiguous(), T)
        added = None
        if self.unet.cfg.addition_embed:  # SDXL: the keys CoMatTrainer reads
            ids = batch.get("add_time_ids")
            ids = (size[0], size[1], 0, 0, size[0], size[1]) if ids is None else ids
            added = self.unet.added_embedding(batch["pooled_prompt_embeds"].to(dev, torch.float32), [list(ids)] * B)
        eps, _ = self.unet(xin, B, h, w, temb, ctx, L, added=added)
        loss, per_sample = ops.mse_loss(eps, noise, B, w=None if cfg.snr_gamma is None else wts)
        return loss, per_sample, t

    def train_step(self, batch):
        """batch: `pixel_values` [B, 3, H, W] in [-1, 1] or `latents` [B, C, h, w] (scaled), `prompt_embeds` [B, L, C]; SDXL also
        `pooled_prompt_embeds` and optionally `add_time_ids`; optional `timesteps` int [B], `noise` and `posterior_noise`
        [B, C, h, w].  -> logs of device tensors: loss [1], per_sample_loss [B], lr [1], grad_norm [1] (non-finite: the update was
        skipped), timesteps [B]"""
        ops.reset_side_stream_state()
        self.bank.set_requires_grad(True)
        self.bank.zero_grad()
        loss, per_sample, t = self.compute_loss(batch)
        loss.backward()
        if self.device.type == "cuda":
            ops.join_side_streams()
        self.opt.step()
        self.bank.mark_updated()
        if self.full:
            self.bank.ensure_compute_copy()
        return dict(loss=loss.detach(), per_sample_loss=per_sample, lr=self.opt.lr_now if self._lr_const is None else self._lr_const,
                    grad_norm=torch.sqrt(self.opt.gnorm_sq), timesteps=t)
