"""Validation sampling inside a training run - the counterpart of `save_and_evaluate` (training_script.py:428-494, triggered at
:710): every validation prompt is sampled `num_validation_images` times with the CURRENT weights, `--total_step` DDPM steps,
`--cfg_scale` and `--cfg_rescale`, and the images come out as NHWC uint8 (:489).  The product ends at uint8 arrays and PNG files;
a TensorBoard writer is the caller's business.

    no-grad sampler (its hipGraph replay where the graphs exist) -> VAE decode, RAW -> comat_image_u8: one launch per sampler call
    that denormalises, clamps, scales and rounds as diffusers' VaeImageProcessor.postprocess + numpy_to_pil do.

The contract: a call at any point between two `train_step` calls - inside an open accumulation window too - leaves every later
training result bit-identical to a run without it (`undisturbed` below lists what is put back).

Deviations from the reference: every sample draws from a generator of its own, seeded by (seed, prompt, image) - the reference
runs ONE generator through all of them, so there an image depends on how many came before it; the bf16 decode is denormalised in
fp32 (diffusers does it in the pipeline's fp16); there is no safety checker (the reference installs a `dummy_checker`)."""
from __future__ import annotations

import contextlib
import math
import os
import struct
import zlib
from dataclasses import dataclass

import torch

from . import fp8, ops


@dataclass
class ValidationConfig:
    num_inference_steps: int = 40       # --total_step
    guidance_scale: float = 7.5         # --cfg_scale
    guidance_rescale: float = 0.0       # --cfg_rescale
    num_validation_images: int = 4      # --num_validation_images
    seed: int | None = None             # --seed; None: drawn per run and reported (ValidationResult.seed)
    height: int = 512                   # --resolution
    width: int = 512
    batch_size: int = 1                 # samples per sampler call (the reference: 1, "avoid oom by shrinking bs")
    sheet_pad: int = 2                  # pixels around and between the images of a contact sheet

    def __post_init__(self):
        for name in ("num_inference_steps", "num_validation_images", "batch_size"):
            v = getattr(self, name)
            if not isinstance(v, int) or isinstance(v, bool) or v < 1:
                raise ValueError(f"ValidationConfig.{name} must be an integer >= 1 (got {v!r})")
        for name in ("height", "width"):
            v = getattr(self, name)
            if not isinstance(v, int) or v < 8 or v % 8:
                raise ValueError(f"ValidationConfig.{name} must be a positive multiple of 8 (got {v!r})")
        if not isinstance(self.sheet_pad, int) or self.sheet_pad < 0:
            raise ValueError(f"ValidationConfig.sheet_pad must be an integer >= 0 (got {self.sheet_pad!r})")
        if self.seed is not None and (not isinstance(self.seed, int) or isinstance(self.seed, bool)):
            raise ValueError(f"ValidationConfig.seed must be an integer or None (got {self.seed!r})")

    @classmethod
    def from_args(cls, args, **kw):
        """from the reference's parser (training_utils/arguments.py): --total_step, --cfg_scale, --cfg_rescale,
        --num_validation_images, --seed, --resolution"""
        base = dict(num_inference_steps=args.total_step, guidance_scale=args.cfg_scale, guidance_rescale=args.cfg_rescale,
                    num_validation_images=args.num_validation_images, seed=args.seed, height=args.resolution, width=args.resolution)
        base.update(kw)
        return cls(**base)


@dataclass
class ValidationResult:
    images: torch.Tensor                # uint8 [P, N, H, W, 3], host
    bad: torch.Tensor                   # bool [P, N]: the decode of this sample held an Inf or NaN (its bytes: 255 / 0)
    seed: int                           # the seed the draws came from (ValidationConfig.seed, or the one drawn for this run)
    caption_loss: torch.Tensor | None   # fp32 [P, N]: -Blip.score(...)[0] per sample, where a captioner and ids were given
    sheet_pad: int = 2
    device: str = "cpu"                 # where contact_sheet runs its launches


_M64 = (1 << 64) - 1


def _mix(z):
    """splitmix64's finaliser"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def sample_seed(seed, prompt_index, image_index):
    """the generator seed of one sample: a fixed function of the three integers and of nothing else"""
    z = _mix(int(seed) & _M64)
    z = _mix((z + 0x9E3779B97F4A7C15 * (int(prompt_index) + 1)) & _M64)
    z = _mix((z + 0x9E3779B97F4A7C15 * (int(image_index) + 1)) & _M64)
    return z >> 1  # (a non-negative int64)


def draw_noise(seed, prompt_index, image_index, h, w, steps, channels=4):
    """-> (latents [channels, h, w], noises [steps, channels, h, w]) of ONE sample, fp32 on the host, h x w the LATENT size: from a
    CPU generator seeded by sample_seed(seed, prompt_index, image_index).  The draws depend on nothing else - not on batch_size, on
    the other prompts or on the global generator, which is never advanced."""
    g = torch.Generator(device="cpu").manual_seed(sample_seed(seed, prompt_index, image_index))
    lat = torch.randn((channels, h, w), generator=g, dtype=torch.float32)
    noises = torch.randn((steps, channels, h, w), generator=g, dtype=torch.float32)
    return lat, noises


def fresh_seed():
    """a seed from a fresh generator (the global one is not touched)"""
    return torch.Generator(device="cpu").seed() & ((1 << 63) - 1)


@contextlib.contextmanager
def undisturbed(pipe, blip=None):
    """What a sampling call in the middle of training would leave behind, put back:
      * the fp8 forward's state under delayed scaling: running maxima and `used` marks (ops.fp8_sites_preserved), the scale words (a
        site without a scale yet quantises just in time and writes its own), the maxima of sites first reached inside;
      * the text key / value tensors of the replayed no-grad UNet: marked stale before (they are projected for the validation
        context) and after (and again for training) - GraphedUNetForward.new_sampler_call;
      * `pipe.attn_dict`, `pipe.graphed`, the scheduler's timestep list;
      * the captioner's fixed-address crop tables (captured steps read them): the validation images are scored through tables of
        their own.
    Gradient buffers, accumulation windows, optimizer state and counters are not written by anything a no-grad sampler call
    launches; captured graphs keep their static buffers - the replayed UNet's inputs are copied in again by every replay."""
    sched = pipe.scheduler
    saved = dict(attn_dict=pipe.attn_dict, graphed=pipe.graphed, steps=sched.num_inference_steps, timesteps=sched.timesteps)
    graphed = pipe.graphed
    tables = None if blip is None else (blip.static_tables, blip._static_key)
    st = fp8._states.get(fp8._key(pipe.device)) if fp8.fp8_scaling() == "delayed" else None
    n0 = 0 if st is None else st.n
    scale0 = None if st is None or not n0 else st.scale[:n0].clone()
    used0 = None if st is None else set(st.used)
    if graphed is not None:
        graphed.new_sampler_call()
    if blip is not None:
        blip.static_tables = None
    try:
        with torch.no_grad(), ops.fp8_sites_preserved(pipe.device):
            yield
    finally:
        pipe.attn_dict, pipe.graphed = saved["attn_dict"], saved["graphed"]
        sched.num_inference_steps, sched.timesteps = saved["steps"], saved["timesteps"]
        if graphed is not None:
            graphed.new_sampler_call()
        if blip is not None:
            blip.static_tables, blip._static_key = tables
        if st is not None:
            if scale0 is not None:
                st.scale[:n0].copy_(scale0)
            if st.n > n0:  # sites first reached inside: no maximum, no scale, no mark - the next step meets them as new
                st.amax[n0:st.n].zero_()
                st.scale[n0:st.n].zero_()
            st.used = used0


class Validator:
    """`run(cfg, prompt_embeds, ...)`: prompts outer, images inner (training_script.py:466-478), `batch_size` samples per sampler
    call.  blip: a blip.Blip - with `input_ids` / `attention_mask` the result carries the caption loss of every sample."""

    def __init__(self, pipeline, blip=None):
        self.pipe, self.blip = pipeline, blip

    def _graphs_ready(self, B, h, w, L, steps):
        """does the replayed no-grad UNet have its graphs for this call's key (B, h, w, L) at every timestep?  Nothing is captured
        for a validation call: where one is missing the eager UNet runs."""
        g = self.pipe.graphed
        if g is None or (B, h, w, L) not in g.static:
            return False
        sched = self.pipe.scheduler
        return all((int(t), B, h, w, L) in g.graphs for t in sched.set_timesteps(steps))

    def run(self, cfg: ValidationConfig, prompt_embeds, negative_prompt_embeds=None, pooled_prompt_embeds=None,
            negative_pooled_prompt_embeds=None, add_time_ids=None, input_ids=None, attention_mask=None):
        """prompt_embeds [P, L, C] (negative_prompt_embeds alike; not needed for guidance_scale <= 1); SDXL pipelines also take
        pooled_prompt_embeds / negative_pooled_prompt_embeds [P, pooled_dim] and add_time_ids; input_ids / attention_mask [P, T]:
        the captioner's ids of the prompts.  -> ValidationResult"""
        pipe = self.pipe
        guided = cfg.guidance_scale > 1.0
        if prompt_embeds is None or prompt_embeds.dim() != 3:
            raise ValueError("Validator.run: prompt_embeds must be [P, L, C]")
        P, L, _ = prompt_embeds.shape
        if guided and negative_prompt_embeds is None:
            raise ValueError(f"Validator.run: guidance_scale = {cfg.guidance_scale} needs negative_prompt_embeds")
        if guided and negative_prompt_embeds.shape != prompt_embeds.shape:
            raise ValueError(f"Validator.run: negative_prompt_embeds {tuple(negative_prompt_embeds.shape)} and prompt_embeds "
                             f"{tuple(prompt_embeds.shape)} differ in shape")
        if pipe.is_sdxl:
            if pooled_prompt_embeds is None:
                raise ValueError("Validator.run: an SDXL pipeline needs pooled_prompt_embeds")
            if guided and negative_pooled_prompt_embeds is None:
                raise ValueError("Validator.run: an SDXL pipeline under guidance needs negative_pooled_prompt_embeds")
        if (input_ids is None) != (attention_mask is None):
            raise ValueError("Validator.run: input_ids and attention_mask come together")
        if input_ids is not None and self.blip is None:
            raise ValueError("Validator.run: input_ids were given, but the validator has no captioner (Validator(pipeline, blip))")
        if input_ids is not None and input_ids.shape[0] != P:
            raise ValueError(f"Validator.run: input_ids {tuple(input_ids.shape)} for {P} prompts")
        N, steps = cfg.num_validation_images, cfg.num_inference_steps
        H, W, h, w = cfg.height, cfg.width, cfg.height // 8, cfg.width // 8
        seed = fresh_seed() if cfg.seed is None else cfg.seed
        dev = torch.device(pipe.device)
        ch = getattr(getattr(pipe.unet, "cfg", None), "in_channels", 4)
        samples = [(p, i) for p in range(P) for i in range(N)]
        images = torch.empty((P * N, H, W, 3), dtype=torch.uint8, device=dev)
        bad = torch.zeros(P * N, dtype=torch.int32, device=dev)
        scoring = input_ids is not None
        closs = torch.zeros(P * N, dtype=torch.float32, device=dev) if scoring else None
        pick = lambda t, idx: None if t is None else t[idx]
        with undisturbed(pipe, self.blip if scoring else None):
            for k in range(0, len(samples), cfg.batch_size):
                chunk = samples[k:k + cfg.batch_size]
                bs = len(chunk)
                draws = [draw_noise(seed, p, i, h, w, steps, ch) for p, i in chunk]
                lat0 = torch.stack([d[0] for d in draws])
                noises = [torch.stack([d[1][s] for d in draws]) for s in range(steps)]
                idx = torch.tensor([p for p, _ in chunk])
                sdxl = {}
                if pipe.is_sdxl:
                    sdxl = dict(pooled_prompt_embeds=pooled_prompt_embeds[idx], add_time_ids=add_time_ids,
                                negative_pooled_prompt_embeds=pick(negative_pooled_prompt_embeds, idx) if guided else None)
                if not self._graphs_ready((2 if guided else 1) * bs, h, w, L, steps):
                    pipe.graphed = None  # (undisturbed puts it back)
                lat = pipe.forward(prompt_embeds[idx], pick(negative_prompt_embeds, idx) if guided else None, height=H, width=W,
                                   training_timesteps=(), num_inference_steps=steps, guidance_scale=cfg.guidance_scale,
                                   latents=lat0, noises=noises, output_type="latent_tokens",
                                   guidance_rescale=cfg.guidance_rescale, **sdxl)
                raw, Hd, Wd = pipe.decode_tokens(lat, bs, h, w, raw=True)
                if (Hd, Wd) != (H, W):
                    raise ValueError(f"Validator.run: the VAE decodes {h}x{w} latents to {Hd}x{Wd}, not {H}x{W}")
                ops.image_u8(raw, bs, H, W, denormalize=True, out=images[k:k + bs].view(bs * H, W, 3), bad=bad[k:k + bs])
                if scoring:
                    img01 = ops.affine(raw, 0.5, 0.5)  # what the training step scores (TrainableSDPipeline.py:223), unclamped
                    for j, (p, _) in enumerate(chunk):
                        reward = self.blip.score(img01[j * H * W:(j + 1) * H * W], 1, H, W, input_ids[p:p + 1].to(dev),
                                                 attention_mask[p:p + 1].to(dev))[0]
                        closs[k + j] = -reward.detach().float().reshape(())
        return ValidationResult(images=images.cpu().reshape(P, N, H, W, 3), bad=bad.cpu().bool().reshape(P, N), seed=seed,
                                caption_loss=None if closs is None else closs.cpu().reshape(P, N), sheet_pad=cfg.sheet_pad,
                                device=str(dev))


def contact_sheet(result: ValidationResult, cols=None, background=255):
    """-> one uint8 [Hs, Ws, 3] per prompt (host): its images `cols` a row (default: ceil(sqrt(N))), `result.sheet_pad` pixels
    around and between them, on a sheet filled with `background` first - placed by comat_image_u8 (the bytes / 255 are images in
    [0, 1]; times 255 and rounded they are the bytes again)."""
    P, N, H, W, C = result.images.shape
    cols = int(math.ceil(math.sqrt(N))) if cols is None else int(cols)
    if cols < 1:
        raise ValueError(f"contact_sheet: cols must be >= 1 (got {cols})")
    pad, dev = result.sheet_pad, torch.device(result.device)
    Hs, Ws = ops.sheet_shape(N, H, W, cols, pad)
    sheets = []
    for p in range(P):
        sheet = torch.full((Hs, Ws, C), int(background), dtype=torch.uint8, device=dev)
        tokens = result.images[p].to(dev).reshape(N * H * W, C).to(torch.float32) / 255.0
        ops.image_u8(tokens, N, H, W, denormalize=False, out=sheet, cols=cols, pad=pad)
        sheets.append(sheet.cpu())
    return sheets


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, u8):
    """an 8-bit RGB ([H, W, 3]) or grey ([H, W] / [H, W, 1]) PNG from a uint8 array or tensor; zlib and struct only"""
    a = u8.detach().cpu() if isinstance(u8, torch.Tensor) else torch.as_tensor(u8)
    if a.dtype != torch.uint8 or a.dim() not in (2, 3) or (a.dim() == 3 and a.shape[2] not in (1, 3)) or 0 in a.shape:
        raise ValueError(f"write_png: a uint8 [H, W, 3], [H, W, 1] or [H, W] image, got {a.dtype} {tuple(a.shape)}")
    Hh, Ww = a.shape[:2]
    colour = 2 if (a.dim() == 3 and a.shape[2] == 3) else 0
    rows = a.reshape(Hh, -1)
    raw = torch.cat([torch.zeros((Hh, 1), dtype=torch.uint8), rows], dim=1).contiguous().numpy().tobytes()  # filter 0 a row
    png = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", Ww, Hh, 8, colour, 0, 0, 0))
           + _chunk(b"IDAT", zlib.compress(raw, 6)) + _chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(png)
    return path


def save_images(dir, result: ValidationResult, step, cols=None):
    """<dir>/validation/step_<step>/prompt_<i>_<j>.png for every sample and sheet_<i>.png per prompt -> the paths written"""
    out = os.path.join(dir, "validation", f"step_{int(step)}")
    os.makedirs(out, exist_ok=True)
    paths = []
    P, N = result.images.shape[:2]
    for i in range(P):
        for j in range(N):
            paths.append(write_png(os.path.join(out, f"prompt_{i}_{j}.png"), result.images[i, j]))
    for i, sheet in enumerate(contact_sheet(result, cols)):
        paths.append(write_png(os.path.join(out, f"sheet_{i}.png"), sheet))
    return paths
