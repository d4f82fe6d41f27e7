"""One CoMat optimisation step on MI355X — the counterpart of the step body `training_script.py:556-694`:

    sample K trained steps -> K-of-N differentiable denoise -> VAE decode -> random 510^2 crop -> BLIP reward
    [-> + w_g * G_loss] [-> + 1e-3 * token_loss + 5e-5 * pixel_loss] -> backward -> all-reduce(mean) of the flat LoRA
    gradient -> clip(0.1) + AdamW (one fused pass)  ||  D step: D_loss on [fake.detach(); real] -> backward ->
    all-reduce -> clip(1.0) + AdamW.

MI355X-first scheduling: the D step runs on its own HIP stream under the G backward chain; the G-gradient all-reduce
(RCCL over xGMI) is launched asynchronously as soon as the G backward is queued and overlaps the tail of the D step;
the per-step barrier of the reference (training_script.py:716) is dropped.  Optimizer state lives in flat fp32 buffers next to the flat parameter and
gradient buffers, so clip + AdamW is one HBM pass per buffer.
"""
from __future__ import annotations

import contextlib
import os
import random
import sys
from dataclasses import dataclass

import torch

from . import _hip, ops
from .blip import Blip
from .clip import ClipTextBank, ClipTextEncoder
from .dist import GradReducer
from .gan import D_sd, D_sdxl
from .losses import mask_loss, mask_loss_device
from .pipeline import TrainableSDPipeline
from .unet import LoRABank, UNetBank


@dataclass
class StepConfig:
    """Path-relevant flags of training_utils/arguments.py with the values of scripts/sd15.sh."""
    resolution: int = 512
    total_step: int = 50
    K: int = 5
    cfg_scale: float = 7.5
    gan_loss: bool = True
    gan_loss_weight: float = 1.0
    attrcon: bool = False
    attrcon_train_steps: int = 2
    train_layer_ls: tuple = ("mid_8", "up_16", "up_32", "up_64")
    attn_reses: tuple = (64, 32, 16, 8)
    mask_token_loss_weight: float = 1e-3
    mask_pixel_loss_weight: float = 5e-5
    lr: float = 5e-5
    lr_D: float = 2e-5          # --learning_rate_D 2e-5 (scripts/sd15.sh)
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_beta1_D: float = 0.0
    adam_beta2_D: float = 0.999
    adam_weight_decay: float = 1e-2
    adam_epsilon: float = 1e-8
    max_grad_norm: float = 0.1
    max_grad_norm_D: float = 1.0
    label_smoothing: float = 0.1
    cfg_rescale: float = 0.0    # --cfg_rescale -> guidance_rescale of every denoise step (training_script.py:584)
    norm_grad: bool = False     # --norm_grad: the image gradient is divided by |g|_2 / 1e4 (training_script.py:644-651)
    reward_norm: bool = False   # log |dLoss/dimage|_2 as logs["reward_norm"] (training_script.py:646,677); norm_grad implies it
    # the sampler's cheaper training modes (TrainableSDPipeline.py:25-31; pipeline.TrainableSDPipeline.forward).  cfg_scale <= 1
    # (`--cfg_scale 1`) switches guidance off: the batch may then omit negative_prompt_embeds (training_script.py:585)
    early_exit: bool = False        # stop after the last trained step and decode its pred_original_sample
    double_laststep: bool = False   # all N steps without grad, then re-noise and ONE trained call (batch["renoise"], optional)
    fast_training: bool = False     # run only the K trained denoise steps
    bp_on_trained: bool = True      # --bp_on_trained: the UNet input of a trained step is not detached
    # --gan_unet_lastlayer_cls (gan_sdxl.py:27-30): the discriminator's conv_out is its classifier.  The discriminator object
    # carries the head (gan.D_sd(lastlayer_cls=True)); the flag documents the configuration and must agree with it
    gan_unet_lastlayer_cls: bool = False
    # --gradient_checkpointing (training_utils/pipeline.py:73-74; passed by scripts/sd15.sh:7 and scripts/sdxl.sh:7): each trained
    # UNet call drops its activations after the forward and recomputes them inside the backward pass (comat_amd/recompute.py) -
    # the K calls need the activations of one, for K more UNet forwards per step.  Off by default, unlike the two scripts: on a
    # 288 GB part a per-GPU batch <= 4 does not need the memory.  COMAT_GRADIENT_CHECKPOINTING=1 switches it on
    gradient_checkpointing: bool = False
    # the generator's learning-rate schedule (training_script.py:290-295 get_scheduler; :664 its step; :667 logs["lr"]),
    # evaluated on the device from the count of applied updates.  The discriminator's optimizer has none (:266-275)
    lr_scheduler: str = "constant"          # --lr_scheduler: one of _hip.LR_KINDS (piecewise_constant is not built)
    lr_warmup_steps: int = 0                # --lr_warmup_steps
    max_train_steps: int | None = None      # --max_train_steps: required by the kinds that decay
    lr_num_cycles: float | None = None      # cosine: 0.5, cosine_with_restarts: 1 when None (get_scheduler's defaults)
    lr_power: float = 1.0                   # polynomial
    lr_steps_per_update: int = 1            # accelerate without split_batches: the number of processes of the run mirrored
    # --gradient_accumulation_steps (training_script.py:556,680 `accelerator.accumulate`; :293-294 the schedule's lengths times N;
    # :655,702 train_loss): G and D each update once per N consecutive calls of the step, from the mean of their N gradients.  The
    # window's index lives in device memory (FlatAdamW.window), so one captured graph serves every micro-step.  1, as both shipped
    # scripts pass (the reference parser's default is 4)
    gradient_accumulation_steps: int = 1
    # --tune_vae (training_utils/pipeline.py:68 `vae.requires_grad_(args.tune_vae)`, :170-171 the VAE's parameters join the
    # generator's optimizer; training_script.py:402-403 saves vae.pt): the decoder handed in carries the trainable parameters
    # (unet.VAEDecoder(..., bank=unet.VAEBank(...))); the flag documents the configuration and must agree with it.  The bank's
    # flat buffers are a second segment of the generator's AdamW, under ONE clip norm with the LoRA factors (:661-662)
    tune_vae: bool = False
    # --full_finetuning (training_utils/pipeline.py:60-61,85,125-126: no LoRA layers, every parameter of the generator's UNet goes
    # to its optimizer; training_script.py:392-395 saves unet.pt): the trainer is handed the unet.UNetBank the UNet was built
    # from (UNet(..., bank=ubank)) where it takes the LoRABank; the flag documents the configuration and must agree with it.
    # The bank's flat buffers are the first segment of the generator's AdamW (same clip, window, schedule, skip and exchange);
    # after an update its compute copies are rewritten by one comat_weights_refresh launch.  The discriminator keeps LoRA
    full_finetuning: bool = False
    # --use_8bit_adam (training_script.py:216-223: bnb.optim.AdamW8bit is the optimizer class of the generator, :258-264, and of
    # the discriminator, :269-275): both optimizers keep their moments as 8-bit blockwise codes (optim8.FlatAdamW8bit; segments
    # under 4096 elements keep fp32 moments).  HIP kernels only; the deviations from bitsandbytes are listed in INTEGRATION.md
    use_8bit_adam: bool = False
    # --train_text_encoder_lora (training_script.py:569-573,581 re-encodes the prompts under autograd; training_utils/pipeline.py:
    # 117-119,176-184 LoRA on q / k / v / out_proj of every CLIP layer): the trainer is handed the text tower and its factors
    # (CoMatTrainer(..., text_encoder=clip.ClipTextEncoder(..., bank=tb), text_bank=tb)) and the batch carries input ids
    # (prompt_input_ids / null_input_ids) where it carried embeddings.  The factors are one more segment of the generator's
    # AdamW (one clip norm, :661-662).  --textenc_lora_lr (:227-254): that segment's base rate; None = the generator's
    train_text_encoder_lora: bool = False
    textenc_lora_lr: float | None = None
    # --tune_text_encoder (training_utils/pipeline.py:69 `text_encoder.requires_grad_`, :75-77 its gradient checkpointing, :173-174
    # every parameter of the tower joins the generator's optimizer; training_script.py:304-305 the tower stays fp32, :569-573,581 the
    # prompts are re-encoded under autograd, :405-406 / :189-190 text_encoder.pt): the trainer is handed the tower and the
    # clip.ClipTextBank it was built from (CoMatTrainer(..., text_encoder=clip.ClipTextEncoder(..., bank=tb), text_bank=tb)); the batch
    # carries input ids as under train_text_encoder_lora.  The bank's flat buffers are the last segment of the generator's AdamW
    # (one clip norm, skip, schedule, window and exchange); its Linear copies are refreshed behind the update.  An SDXL pipeline's
    # second-encoder tensors stay frozen inputs (the reference tunes `pipeline.text_encoder` only)
    tune_text_encoder: bool = False
    # the attribute-concentration loss as device work (losses.mask_loss_device: one resize launch per resolution, one batched
    # gather / loss / gradient kernel family per (timestep, layer), no host synchronisation) instead of the per-sample host
    # assembly of losses.mask_loss.  Needs attrcon.  COMAT_ATTRCON_DEVICE=1 switches it on where attrcon is on
    attrcon_on_device: bool = False
    # the masked attentions whose probability map nobody reads - the causal self-attention of the CLIP text towers, BLIP's causal +
    # padding-masked decoder self-attention - on the fused masked kernels (comat_flash_attn_masked_*: no score / probability / dP /
    # dS maps in HBM, 1 launch forward and 2 backward instead of 3 and 5 - 6) instead of the materialised _Attention.  The trainer
    # sets ops.set_fused_masked_attention from it; COMAT_FLASH_MASK=1 switches it on where the config leaves it off
    fused_masked_attention: bool = False

    def __post_init__(self):
        if self.attrcon_on_device and not self.attrcon:
            raise ValueError("StepConfig.attrcon_on_device is set but attrcon is off")
        n = self.gradient_accumulation_steps
        if not isinstance(n, int) or isinstance(n, bool) or n < 1:
            raise ValueError(f"gradient_accumulation_steps must be an integer >= 1 (got {n!r})")
        if self.textenc_lora_lr is not None and not self.train_text_encoder_lora:
            raise ValueError("StepConfig.textenc_lora_lr is set but train_text_encoder_lora is off")
        if self.train_text_encoder_lora:
            if self.full_finetuning:
                raise ValueError("StepConfig.train_text_encoder_lora with full_finetuning is not built")
            if self.use_8bit_adam:
                raise ValueError("StepConfig.train_text_encoder_lora with use_8bit_adam is not built")
            if self.textenc_lora_lr is not None and self.lr_scheduler == "polynomial":
                # get_scheduler's polynomial lambda is computed from the optimizer's default rate, not from the group's
                raise ValueError("StepConfig.textenc_lora_lr with lr_scheduler = 'polynomial' is not built")
            if self.tune_text_encoder:  # (the reference would train both; LoRA holders over trained weights are not built)
                raise ValueError("StepConfig.tune_text_encoder with train_text_encoder_lora is not built")

    @property
    def text_flag(self):
        """the name of the flag that trains the text tower, or None: the step then takes embeddings and no text objects"""
        return "tune_text_encoder" if self.tune_text_encoder else "train_text_encoder_lora" if self.train_text_encoder_lora else None

    @classmethod
    def sdxl(cls, **kw):
        """the values of scripts/sdxl.sh where they differ from scripts/sd15.sh (--learning_rate 2e-5 --learning_rate_D 5e-5
        --gan_loss_weight 0.5) and the SDXL layer list of training_script.py:312 (at 512 x 512)"""
        base = dict(lr=2e-5, lr_D=5e-5, gan_loss_weight=0.5, train_layer_ls=("mid_16", "up_16", "up_32"), attn_reses=(32, 16))
        base.update(kw)
        return cls(**base)


def _dbg(tag):
    """COMAT_DEBUG_SYNC=1: synchronise and print a phase marker (locates asynchronous device faults)."""
    if os.environ.get("COMAT_DEBUG_SYNC") in ("1", "phase"):
        torch.cuda.synchronize()
        print(f"[comat] phase ok: {tag}", file=sys.stderr, flush=True)


LR_END = 1e-7  # get_polynomial_decay_schedule_with_warmup's default; get_scheduler leaves it there


def lr_schedule(kind, base_lr, warmup=0, total=None, num_cycles=None, power=1.0, steps_per_update=1, lr_end=LR_END):
    """The schedule `get_scheduler(kind, optimizer, warmup, total)` builds (training_script.py:290-295), as the struct the
    kernels take by value.  What the library refuses at run time is refused here, naming the StepConfig field."""
    if kind not in _hip.LR_KINDS:
        raise ValueError(f"lr_scheduler = {kind!r}: not one of {sorted(_hip.LR_KINDS)}")
    decays = _hip.LR_KINDS[kind] >= _hip.LR_KINDS["linear"]
    if decays and total is None:
        raise ValueError(f"lr_scheduler = {kind!r} needs max_train_steps")
    if decays and total < 1:
        raise ValueError(f"max_train_steps must be >= 1 (got {total})")
    if warmup < 0 or steps_per_update < 1:
        raise ValueError(f"lr_warmup_steps must be >= 0 and lr_steps_per_update >= 1 (got {warmup}, {steps_per_update})")
    if kind == "polynomial" and (not base_lr > lr_end or total == warmup):
        raise ValueError(f"lr_scheduler = 'polynomial' needs lr > {lr_end} and max_train_steps != lr_warmup_steps")
    if num_cycles is None:
        num_cycles = 1.0 if kind == "cosine_with_restarts" else 0.5
    return _hip.LrSchedule(_hip.LR_KINDS[kind], steps_per_update, warmup, total if decays else 0, base_lr, num_cycles, power,
                           lr_end)


class FlatAdamW:
    """clip_grad_norm_ + AdamW over flat fp32 buffers (one or more segments sharing the global norm).

    The step count of the bias correction lives in device memory (`counters` int32 [2] = applied, skipped) and advances
    only when an update is applied: a non-finite gradient norm skips the update (the inf/NaN check of the reference's
    mixed-precision optimizer step, training_script.py:661-664) WITHOUT moving the bias correction ahead of the
    moments, the skip is visible to the caller (`counters[1]`, `gnorm_sq`), and a captured hipGraph of the whole step
    replays with the right count.  Deliberate deviation: plain torch AdamW would apply a NaN update.

    schedule (`lr_schedule(...)`): the learning rate follows it as a function of the same count.  It lives in the device
    word `lr_now` (fp32 [1], fixed address), which the tick of each step sets to the rate of the NEXT update - what
    `lr_scheduler.get_last_lr()` returns after training_script.py:664 - so a skipped update moves neither, as under
    accelerate, and a captured graph replays with the moving rate.  None, or `constant` at one scheduler step per update:
    the rate is the host value `lr` and the launches are those of an optimizer without a schedule.

    accum_steps N > 1 (`--gradient_accumulation_steps`, used as accelerate documents it): the update is applied on every N-th
    call of `step`, to the gradient the caller has summed over the N micro-steps since `zero_grad()` last cleared it.  The index
    of the micro-step inside its window is the device word `window` (int32 [1]); `zero_grad`, the update and the tick read it when
    they execute, so every micro-step issues the same launches and a captured graph replays through whole windows.  The
    optimizer then always owns `lr_now` (a constant schedule is evaluated into it once) and `train_loss` (fp32 [2]: the running
    sum of loss / N of the open window, and the sum of the last closed one - training_script.py:655,702).  The host keeps a copy
    of the index (`closing`) for what only the host can decide: the gradient exchange.  N = 1: none of this exists.

    segment_lrs (one entry per segment; None = `lr`): a segment with a base rate of its own - a second parameter group of the
    reference's optimizer (`--textenc_lora_lr`, training_script.py:227-254).  The clip norm, the count, the window and the skip
    stay the optimizer's; the rate follows the SAME schedule from its own base (get_scheduler's lambda multiplies every group's
    base rate): where the optimizer keeps its rate in a device word, such a segment has a word of its own, re-evaluated from
    the count (comat_lr_schedule_eval) behind every tick.  Without a schedule and a window it is a host value, like `lr`."""

    def __init__(self, segments, lr, betas, eps, weight_decay, max_norm, schedule=None, accum_steps=1, segment_lrs=None):
        self.segments = segments  # list of (param_flat, grad_flat)
        self.m, self.v = self._alloc_moments()
        self.lr, self.betas, self.eps, self.wd, self.max_norm = lr, betas, eps, weight_decay, max_norm
        dev = segments[0][0].device
        self.gnorm_sq = torch.zeros(1, dtype=torch.float32, device=dev)
        self.counters = torch.zeros(2, dtype=torch.int32, device=dev)
        self.schedule, self.lr_now = None, None
        if schedule is not None and not (schedule.kind == _hip.LR_KINDS["constant"] and schedule.stride == 1):
            if schedule.base_lr != lr:
                raise ValueError(f"schedule.base_lr = {schedule.base_lr} but lr = {lr}")
            self.schedule = schedule
            self.lr_now = torch.zeros(1, dtype=torch.float32, device=dev)
            ops.kernels().lr_schedule_eval(schedule, self.counters, self.lr_now)
        if accum_steps < 1:
            raise ValueError(f"accum_steps must be >= 1 (got {accum_steps})")
        self.accum_steps, self._index = int(accum_steps), 0
        self.window = self.train_loss = None
        if self.accum_steps > 1:
            self.window = torch.zeros(1, dtype=torch.int32, device=dev)
            self.train_loss = torch.zeros(2, dtype=torch.float32, device=dev)
            if self.lr_now is None:
                self.lr_now = torch.zeros(1, dtype=torch.float32, device=dev)
                ops.kernels().lr_schedule_eval(lr_schedule("constant", lr), self.counters, self.lr_now)
        if segment_lrs is not None and len(segment_lrs) != len(segments):
            raise ValueError(f"segment_lrs has {len(segment_lrs)} entries for {len(segments)} segments")
        # segment index -> its base rate, and (where the rate lives on the device) -> (schedule from that base, rate word)
        self.own_lr = {i: float(r) for i, r in enumerate(segment_lrs or ()) if r is not None and float(r) != lr}
        self.own_word = {}
        if self.own_lr and self.lr_now is not None:
            for i, r in self.own_lr.items():
                if self.schedule is None:
                    sched = lr_schedule("constant", r)
                else:
                    sched = _hip.LrSchedule(**dict(self.schedule.fields(), base_lr=r))
                self.own_word[i] = (sched, torch.zeros(1, dtype=torch.float32, device=dev))
            self._eval_own()

    def _eval_own(self):
        """the rate words of the segments with a base rate of their own, from the current count"""
        for sched, word in self.own_word.values():
            ops.kernels().lr_schedule_eval(sched, self.counters, word)

    def _lr_word(self, i):
        return self.own_word[i][1] if i in self.own_word else self.lr_now

    def _alloc_moments(self):
        """(m, v): one fp32 buffer per segment (optim8.FlatAdamW8bit keeps codes and scales instead)"""
        return [torch.zeros_like(p) for p, _ in self.segments], [torch.zeros_like(p) for p, _ in self.segments]

    @property
    def closing(self):
        """does the NEXT call of `step` close its window (accelerate's `sync_gradients`)?  Host copy of the index: read it
        before `step`."""
        return self._index == self.accum_steps - 1

    def advance(self):
        """one micro-step has EXECUTED: `step` calls it unless the stream is capturing; whoever replays a graph that holds the
        optimizer's launches calls it once per replay"""
        self._index = (self._index + 1) % self.accum_steps

    def _capturing(self):
        dev = self.counters.device
        return dev.type == "cuda" and torch.cuda.is_current_stream_capturing()

    def zero_grad(self):
        """optimizer.zero_grad() where accelerate documents it, after the closing step: the gradient buffers are cleared iff the
        window is at its first micro-step (decided on the device)"""
        if self.accum_steps == 1:
            for _, g in self.segments:
                g.zero_()
            return
        k = ops.kernels()
        for _, g in self.segments:
            k.accum_zero(g, g.numel(), self.window)

    @property
    def t(self):
        """number of applied updates (host read: synchronises; for logs and tests)"""
        return int(self.counters[0])

    def step(self, grad_scale=1.0, step_loss=None):
        """grad_scale: 1 / world when the gradient buffers hold the SUM over data-parallel ranks (dist.GradReducer).
        step_loss (accum_steps > 1; fp32 device scalar, may be None): this micro-step's unscaled loss, gathered into `train_loss`.
        With accum_steps > 1 `gnorm_sq` is, on a micro-step that does not close, the squared norm of the partial sum."""
        k = ops.kernels()
        self.gnorm_sq.zero_()
        for _, g in self.segments:
            k.sumsq(g, g.numel(), self.gnorm_sq)
        if self.accum_steps > 1:
            for i, ((p, g), m, v) in enumerate(zip(self.segments, self.m, self.v)):
                k.adamw_window(p, g, m, v, p.numel(), self._lr_word(i), self.betas[0], self.betas[1], self.eps, self.wd,
                               self.counters, self.gnorm_sq, self.max_norm, self.window, self.accum_steps, grad_scale=grad_scale)
            if step_loss is not None and step_loss.dtype != torch.float32:
                step_loss = step_loss.float()
            k.window_tick(self.window, self.accum_steps, self.counters, self.gnorm_sq, self.schedule, self.lr_now, step_loss,
                          None if step_loss is None else self.train_loss)
            if self.schedule is not None:
                self._eval_own()
            if not self._capturing():
                self.advance()
            return
        if self.schedule is not None:
            for i, ((p, g), m, v) in enumerate(zip(self.segments, self.m, self.v)):
                k.adamw_lr(p, g, m, v, p.numel(), self._lr_word(i), self.betas[0], self.betas[1], self.eps, self.wd,
                           self.counters, self.gnorm_sq, self.max_norm, grad_scale=grad_scale)
            k.adamw_tick_lr(self.counters, self.gnorm_sq, self.schedule, self.lr_now)
            self._eval_own()  # from the count the tick left: a skipped update moved neither
            return
        for i, ((p, g), m, v) in enumerate(zip(self.segments, self.m, self.v)):
            k.adamw(p, g, m, v, p.numel(), self.own_lr.get(i, self.lr), self.betas[0], self.betas[1], self.eps, self.wd, 0,
                    self.gnorm_sq, self.max_norm, step_dev=self.counters, grad_scale=grad_scale)
        k.adamw_tick(self.counters, self.gnorm_sq)

    def state_dict(self):
        """moments and counters (copies, on their device), the schedule's fields (None without one) and accum = (accum_steps,
        index).  The partial gradient of an open window is not part of the state: mid-window this raises (the reference saves
        only where sync_gradients holds, training_script.py:710)."""
        if self._index != 0:
            raise ValueError(f"optimizer state asked for at micro-step {self._index} of an open window of {self.accum_steps}: "
                             "save where a window has closed")
        sd = dict(**self._moments_state(), counters=self.counters.clone(),
                  schedule=None if self.schedule is None else self.schedule.fields(), accum=(self.accum_steps, self._index))
        if self.train_loss is not None:
            sd["train_loss"] = self.train_loss.clone()
        if self.own_lr:  # (absent without such a segment: the state of every other optimizer is what it was)
            sd["segment_lrs"] = dict(self.own_lr)
        return sd

    def _moments_state(self):
        return dict(m=[t.detach().clone() for t in self.m], v=[t.detach().clone() for t in self.v])

    def _load_moments(self, sd):
        """a state with `state_bits` = 8 (optim8.FlatAdamW8bit's; a file without the field holds fp32 moments) is dequantised first"""
        if sd.get("state_bits", 32) == 8:
            from . import optim8
            sd = optim8.dequantized_state(sd, self.counters.device)
        if len(sd["m"]) != len(self.m) or any(a.shape != b.shape for a, b in zip(sd["m"] + sd["v"], self.m + self.v)):
            raise ValueError("optimizer state does not match this optimizer's segments")
        for dst, src in zip(self.m + self.v, sd["m"] + sd["v"]):
            dst.copy_(src)

    def load_state_dict(self, sd):
        """Copies INTO the existing buffers - their addresses are what captured graphs hold - and re-evaluates the learning-rate
        word from the loaded count.  The schedule itself is baked into those graphs: a state saved under another one is refused."""
        accum_steps, index = sd.get("accum", (1, 0))  # a file from before gradient accumulation
        if accum_steps != self.accum_steps:
            raise ValueError(f"optimizer state was saved under accum_steps = {accum_steps}, this optimizer has {self.accum_steps}")
        mine = None if self.schedule is None else self.schedule.fields()
        if sd["schedule"] != mine:
            raise ValueError(f"optimizer state was saved under the schedule {sd['schedule']}, this optimizer has {mine}")
        if sd.get("segment_lrs", {}) != self.own_lr:
            raise ValueError(f"optimizer state was saved under the segment rates {sd.get('segment_lrs', {})}, this optimizer "
                             f"has {self.own_lr}")
        self._load_moments(sd)
        self.counters.copy_(sd["counters"])
        if self.schedule is not None:
            ops.kernels().lr_schedule_eval(self.schedule, self.counters, self.lr_now)
        self._eval_own()
        self._index = int(index)
        if self.window is not None:
            self.window.fill_(self._index)
            if sd.get("train_loss") is not None:
                self.train_loss.copy_(sd["train_loss"])


def sample_training_steps(total_step, K, rng: random.Random):
    """training_script.py:563-566"""
    interval = total_step // K
    max_start = total_step - interval * (K - 1) - 1
    start = rng.randint(0, max_start)
    return list(range(start, total_step, interval))


def sample_crop(resolution, rng: random.Random):
    """training_script.py:606-609: offsets in [0, resolution // 224], crop size resolution - offset_range."""
    offset_range = resolution // 224
    ox, oy = rng.randint(0, offset_range), rng.randint(0, offset_range)
    size = resolution - offset_range
    return (ox, oy, size, size)  # the reference slices dim 2 with x and dim 3 with y: (row0, col0, h, w)


@contextlib.contextmanager
def _own_streams_by_design():
    """The generator-side discriminator loss and the D step run on their own streams by design, so the discriminator head's
    AccumulateGrad nodes see gradients from more than one stream - which torch reports as a (once per process) warning about
    an unintended mismatch.  Switched off for the duration of THIS package's forward + backward only, and put back: user code
    around the step keeps torch's check (round-3 advice: it used to be switched off process-wide at import)."""
    get = getattr(torch._C, "_warn_on_accumulate_grad_stream_mismatch", None)
    put = getattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch", None)
    if get is None or put is None:  # older torch: no such check
        yield
        return
    before = get()
    put(False)
    try:
        yield
    finally:
        put(before)


class CoMatTrainer:
    def __init__(self, pipeline: TrainableSDPipeline, bank: LoRABank | UNetBank, blip: Blip, disc: D_sd | None,
                 cfg: StepConfig, seed=0, text_encoder=None, text_bank=None, text_encoder_2=None):
        self.pipe, self.bank, self.blip, self.D, self.cfg = pipeline, bank, blip, disc, cfg
        self.text_encoder, self.text_bank, self.text_encoder_2 = text_encoder, text_bank, text_encoder_2
        self._pooled_2 = None  # (pooled, null pooled) of the step's prompts, from text_encoder_2 (encode_prompts)
        flag = cfg.text_flag or "train_text_encoder_lora"
        if text_encoder_2 is not None:
            self._check_text_encoder_2(pipeline, cfg, text_encoder, text_encoder_2)
        if (cfg.text_flag is not None) != (text_encoder is not None) or (text_encoder is None) != (text_bank is None):
            raise ValueError(f"StepConfig.{flag} = {getattr(cfg, flag)}, but the trainer was handed "
                             f"{'a' if text_encoder is not None else 'no'} text_encoder and "
                             f"{'a' if text_bank is not None else 'no'} text_bank")
        if text_encoder is not None and getattr(text_encoder, "bank", None) is not text_bank:
            raise ValueError(f"{flag}: the text encoder was not built over this text_bank "
                             "(ClipTextEncoder(..., bank=text_bank))")
        if text_bank is not None and isinstance(text_bank, ClipTextBank) != bool(cfg.tune_text_encoder):
            raise ValueError(f"StepConfig.{flag} = True, but text_bank is a {type(text_bank).__name__}: tune_text_encoder takes a "
                             "clip.ClipTextBank, train_text_encoder_lora a clip.ClipLoRABank")
        self.full = isinstance(bank, UNetBank)
        if self.full != bool(cfg.full_finetuning):
            raise ValueError(f"StepConfig.full_finetuning = {cfg.full_finetuning}, but the trainer was handed a "
                             f"{'UNetBank' if self.full else 'LoRABank'}")
        if self.full and getattr(pipeline.unet, "bank", None) is not bank:
            raise ValueError("full_finetuning: the pipeline's UNet was not built from this UNetBank (UNet(..., bank=ubank))")
        # the environment may switch recomputation on where the config leaves it off (read once, here): an unmodified
        # benchmark then times it
        self.gradient_checkpointing = bool(cfg.gradient_checkpointing) or \
            os.environ.get("COMAT_GRADIENT_CHECKPOINTING", "0") not in ("", "0")
        pipeline.gradient_checkpointing = self.gradient_checkpointing
        # likewise the device path of the attribute-concentration loss, where the configuration has that loss at all
        self.attrcon_on_device = bool(cfg.attrcon) and (bool(cfg.attrcon_on_device) or
                                                        os.environ.get("COMAT_ATTRCON_DEVICE", "0") not in ("", "0"))
        # likewise the fused masked attention of the text paths: a process-wide switch of ops (the towers and BLIP call
        # ops.attention, eagerly, under capture and on recomputation alike), set from here
        self.fused_masked_attention = bool(cfg.fused_masked_attention) or os.environ.get("COMAT_FLASH_MASK", "0") not in ("", "0")
        ops.set_fused_masked_attention(self.fused_masked_attention)
        # micro-steps per update; the schedule's lengths are counted in micro-steps, as training_script.py:293-294 builds them
        self.accum = N = cfg.gradient_accumulation_steps
        total = cfg.max_train_steps if cfg.max_train_steps is None else cfg.max_train_steps * N
        self.vae_bank = getattr(pipeline.vae, "bank", None)
        if (self.vae_bank is not None) != bool(cfg.tune_vae):
            raise ValueError(f"StepConfig.tune_vae = {cfg.tune_vae}, but the VAE decoder was built "
                             f"{'with' if self.vae_bank is not None else 'without'} a VAEBank")
        # the banks of the generator's optimizer in segment order (one clip norm over all of them), each with what its role asks
        # for behind an update: the compute copies of a fully trained UNet and of the text tower (of either kind) are rewritten
        # right there, ONE launch each, rather than inside the next step's first call; the generator's LoRA factors and the VAE
        # decoder refresh at their first use
        roles = [(bank, self.full), (self.vae_bank, False), (text_bank, True)]
        self.trained = [b for b, _ in roles if b is not None]
        self._refresh_behind_update = [now for b, now in roles if b is not None]
        g_segments = [(b.flat, b.flat_grad) for b in self.trained]
        more = {}
        if text_bank is not None and cfg.textenc_lora_lr is not None:  # the text bank is the last segment
            more = dict(segment_lrs=[None] * (len(g_segments) - 1) + [cfg.textenc_lora_lr])
        adamw = FlatAdamW
        if cfg.use_8bit_adam:  # training_script.py:216-223: one optimizer class for G and D
            from .optim8 import FlatAdamW8bit as adamw
        self.opt = adamw(g_segments, cfg.lr, (cfg.adam_beta1, cfg.adam_beta2),
                         cfg.adam_epsilon, cfg.adam_weight_decay, cfg.max_grad_norm,
                         schedule=lr_schedule(cfg.lr_scheduler, cfg.lr, cfg.lr_warmup_steps * N, total,
                                              cfg.lr_num_cycles, cfg.lr_power, cfg.lr_steps_per_update),
                         accum_steps=N, **more)
        self.opt_D = None
        if disc is not None and bool(getattr(disc, "lastlayer_cls", False)) != bool(cfg.gan_unet_lastlayer_cls):
            raise ValueError(f"StepConfig.gan_unet_lastlayer_cls = {cfg.gan_unet_lastlayer_cls}, but the discriminator was built "
                             f"with lastlayer_cls = {getattr(disc, 'lastlayer_cls', False)}")
        if disc is not None:
            self.opt_D = adamw([(disc.bank.flat, disc.bank.flat_grad), (disc.head, disc.head_grad)], cfg.lr_D,
                               (cfg.adam_beta1_D, cfg.adam_beta2_D), cfg.adam_epsilon, cfg.adam_weight_decay,
                               cfg.max_grad_norm_D, accum_steps=N)
        self.rng = random.Random(seed)
        self.reducer = GradReducer()
        self.device = torch.device(pipeline.device)
        self._d_stream = None
        self._g_stream = None  # generator-side discriminator loss, next to VAE + BLIP (head_losses)
        self._d_pending = False
        self._d_keep = None
        self._fp8_clipped = None  # fixed-address int32 scalar behind logs["fp8_clipped_sites"] (fp8 recipe with accounting)
        self.fp8_clipped = None
        self.serial_d = False  # GraphedStep: D step in stream order on the main stream
        self.flat_d = False    # GraphedStep: forked D stream, but no second-level fork for its weight gradients
        # hooks of segments.SegmentedStep: replay the head (VAE + BLIP + generator-side D loss) / the D step from graphs
        self.head_runner = None
        self.d_runner = None
        self._last_image_hw = None
        self.grad_scale = 1.0
        # |dLoss/dimage|_2 of the last step (cfg.reward_norm / cfg.norm_grad): fixed address, so that captured graphs write it
        self.reward_norm = torch.zeros(1, dtype=torch.float32, device=self.device) \
            if (cfg.reward_norm or cfg.norm_grad) else None

    NORM_GRAD_TARGET = 1e4  # "1e4 for numerical stability", training_script.py:648

    def drop_forked_streams(self):
        """After a FAILED graph capture: forget every stream this trainer forks from the capturing stream (the D step's,
        the generator-side D loss's).  The runtime may leave them in capture mode or invalidated; the next eager step
        makes fresh ones.  Per-stream workspaces keyed on the dead streams are dropped with them."""
        dead = [st.cuda_stream for st in (self._d_stream, self._g_stream) if st is not None]
        self._d_stream = self._g_stream = None
        self._d_pending, self._d_keep = False, None
        k = ops.kernels()
        if dead and hasattr(k, "forget_streams"):
            k.forget_streams(dead)

    def abandon_capture(self):
        """A graph capture that ran this trainer's code raised.  The eager work that preceded it was that call's step, so
        the failure becomes a state of the stepper and not an exception; here everything the aborted capture may have left
        behind is dropped: the capture stream, the streams forked from it, the weight gradients the aborted pass queued."""
        ops.reset_capture_stream(self.device)
        self.drop_forked_streams()  # _d_stream, _g_stream: forked inside the capture, possibly left capturing
        ops.drop_side_stream_state()
        if self.device.type == "cuda":
            try:
                torch.cuda.synchronize()
            except Exception:  # noqa: BLE001 - the pending error of the failed capture
                pass

    @contextlib.contextmanager
    def d_placement(self, serial_d, flat_d):
        """`serial_d` / `flat_d` for the duration of a block (GraphedStep), then as they were"""
        saved = (self.serial_d, self.flat_d)
        self.serial_d, self.flat_d = serial_d, flat_d
        try:
            yield
        finally:
            self.serial_d, self.flat_d = saved

    def _own_stream(self, switch):
        """does a GAN-side piece of the step (environment switch `switch`) run on a stream of its own?"""
        return (self.cfg.gan_loss and self.device.type == "cuda" and ops.side_streams_enabled() and not self.serial_d
                and os.environ.get(switch, "1") != "0")

    def _fork(self, name):
        """-> (main, stream): the current stream and this trainer's stream `name` (made at its first use), which waits for
        everything queued on the current one"""
        main = torch.cuda.current_stream(self.device)
        st = getattr(self, name)
        if st is None:
            st = torch.cuda.Stream(device=self.device)
            setattr(self, name, st)
        st.wait_stream(main)
        return main, st

    def _join_d(self):
        """the current stream waits for a D step that is still pending on its own stream; what was kept alive for it is released"""
        if self._d_pending:
            if self.device.type == "cuda":
                torch.cuda.current_stream(self.device).wait_stream(self._d_stream)
            self._d_pending, self._d_keep = False, None

    def _d_cond(self, batch):
        """what an SDXL discriminator is conditioned on besides the null embedding: the null prompt's pooled embedding
        (gan_sdxl.py:222,265-269), on both sides.  Nothing for the SD1.5 discriminator."""
        if isinstance(self.D, D_sdxl):
            return dict(negative_pooled_prompt_embeds=batch["gan_pooled_null_embeds"])
        return {}

    def head_losses(self, lat, batch, crop, bs, h, w):
        """final latents (channels-last tokens, fp32) -> VAE decode -> crop + BLIP caption reward [-> generator-side
        discriminator loss]: TrainableSDPipeline.py:219-223, training_script.py:606-623."""
        cfg = self.cfg
        # The generator-side discriminator loss needs the final latents and nothing of the decode / caption chain: on a
        # GPU it runs on its own stream next to VAE + BLIP (both chains are ~1 k latency-bound launches that leave most
        # of the chip idle), forward and - autograd keeps a node on the stream of its forward - backward.  Same kernels,
        # same bits (the two latent gradients are added, a + b == b + a); COMAT_G_STREAM=0 restores one stream.
        fork = self._own_stream("COMAT_G_STREAM")

        def g_loss():
            return self.D.D_sd_pipeline_forward(lat, "G", negative_prompt_embeds=batch["gan_null_embeds"],
                                                num_inference_steps=cfg.total_step, h=h, w=w, **self._d_cond(batch))
        if fork:
            main, g_stream = self._fork("_g_stream")
            with torch.cuda.stream(g_stream):
                G_loss = g_loss()
        img, H, W = self.pipe.decode_tokens(lat, bs, h, w, return_latents=True)
        _dbg("vae")
        self._last_image_hw = (H, W)
        if self.reward_norm is not None:
            # the hook of training_script.py:651 sits on what the reference's pipeline returns (after `/2 + 0.5`; SDXL with
            # return_latents: the raw decode): every consumer of the image sees it through the hook
            img = ops.grad_norm_hook(img, self.reward_norm, self.NORM_GRAD_TARGET if cfg.norm_grad else 0.0)
        reward, logp = self.blip.score(img, bs, H, W, batch["blip_input_ids"], batch["blip_attention_mask"], crop=crop,
                                       label_smoothing=cfg.label_smoothing)
        _dbg("blip")
        o = dict(reward=reward, logp=logp, image=(img, H, W))
        if fork:
            main.wait_stream(g_stream)
            o["G_loss"] = G_loss
        elif cfg.gan_loss:
            o["G_loss"] = g_loss()
            _dbg("G loss")
        return o

    def _sampler_modes(self, batch):
        """the mode flags of StepConfig as keyword arguments of the pipeline's forward"""
        cfg = self.cfg
        kw = dict(early_exit=cfg.early_exit, double_laststep=cfg.double_laststep, fast_training=cfg.fast_training)
        if not cfg.bp_on_trained:
            kw["bp_on_trained"] = False
        if cfg.double_laststep and batch.get("renoise") is not None:
            kw["renoise"] = batch["renoise"]
        return kw

    def _sdxl_kw(self, batch):
        """SDXL conditioning (TrainableSDPipeline.py:772-784) as keyword arguments of the pipeline; nothing for SD1.5.  With a
        text_encoder_2 the pooled halves are the ones encode_prompts made from this batch's ids."""
        if self.text_encoder_2 is not None:
            pooled, null_pooled = self._pooled_2
            return dict(pooled_prompt_embeds=pooled, negative_pooled_prompt_embeds=null_pooled, add_time_ids=batch.get("add_time_ids"))
        keys = ("pooled_prompt_embeds", "negative_pooled_prompt_embeds", "add_time_ids")
        return {k: batch.get(k) for k in keys} if "pooled_prompt_embeds" in batch else {}

    @staticmethod
    def _check_text_encoder_2(pipeline, cfg, enc1, enc2):
        """text_encoder_2: SDXL's frozen second tower (`pipeline.text_encoder_2`, a CLIPTextModelWithProjection), encoded from ids
        inside the step as training_script.py:569-573,581 does - only next to a text flag, on an SDXL pipeline, with fitting widths"""
        if cfg.text_flag is None:
            raise ValueError("text_encoder_2 was handed to the trainer, but neither StepConfig.train_text_encoder_lora nor "
                             "tune_text_encoder is set: without a text flag the batch carries the embeddings")
        if not pipeline.is_sdxl:
            raise ValueError("text_encoder_2 was handed to the trainer, but the pipeline is not an SDXL pipeline")
        if not isinstance(enc2, ClipTextEncoder) or enc2.bank is not None or enc2.proj is None:
            raise ValueError("text_encoder_2 must be a frozen clip.ClipTextEncoder (no bank) with a text_projection "
                             "(ClipTextConfig.projection_dim set)")
        ucfg = pipeline.unet.cfg
        if enc2.cfg.projection_dim != ucfg.pooled_dim:
            raise ValueError(f"text_encoder_2: projection_dim {enc2.cfg.projection_dim}, the UNet's pooled_dim is {ucfg.pooled_dim}")
        if enc1 is not None and enc1.cfg.hidden + enc2.cfg.hidden != ucfg.cross_attention_dim:
            raise ValueError(f"text_encoder_2: hidden {enc1.cfg.hidden} + {enc2.cfg.hidden} of the two towers, the UNet's "
                             f"cross_attention_dim is {ucfg.cross_attention_dim}")

    TEXT_ID_KEYS = ("prompt_input_ids", "null_input_ids")
    TEXT_EMBED_KEYS = ("prompt_embeds", "negative_prompt_embeds")
    TEXT_ID_KEYS_2 = ("prompt_input_ids_2", "null_input_ids_2")
    # what the second tower's ids come INSTEAD of
    TEXT_EMBED_KEYS_2 = ("prompt_embeds_2", "negative_prompt_embeds_2", "pooled_prompt_embeds", "negative_pooled_prompt_embeds")

    def encode_prompts(self, batch, guided=None):
        """train_text_encoder_lora / tune_text_encoder: (prompt_embeds, negative_prompt_embeds) (bs, L, C) from the batch's input
        ids, under autograd.  guided: is the null prompt encoded too (None: StepConfig.cfg_scale > 1; `validate` passes its own).
        The null prompt is encoded with the prompt, [null; cond] in ONE call of the tower: training_script.py:569-573 re-encodes it
        with gradients enabled, so the unconditional half of the guidance trains the factors too.  The gradient comes back through
        the text key / value projections of every trained UNet call (and the captured cross-attention maps), summed by autograd:
        the tower's backward runs once per step.  Guidance off (cfg_scale <= 1): only the prompt is encoded.
        SDXL: the tower is the FIRST encoder (the reference puts LoRA on `pipeline.text_encoder` only, training_utils/pipeline.py:119)
        and gives its penultimate hidden state; the caller's frozen second-encoder tensors prompt_embeds_2 / negative_prompt_embeds_2
        (bs, L, C2) are joined to it along the channels, and no gradient is asked of them.
        With a text_encoder_2 the batch carries prompt_input_ids_2 / null_input_ids_2 (bs, L) INSTEAD of those two tensors and of
        the two pooled ones: the frozen second tower encodes [null; cond] in one no-grad call (clip.encode_prompt_sdxl's second
        half), its hidden_states[-2] is joined along the channels as before, and the two pooled halves go to the sampler (_sdxl_kw)."""
        cfg = self.cfg
        flag = cfg.text_flag
        enc2 = self.text_encoder_2
        given = [k for k in self.TEXT_EMBED_KEYS if batch.get(k) is not None]
        if given:
            raise ValueError(f"{flag}: the batch carries {given}; the step encodes {list(self.TEXT_ID_KEYS)} itself")
        guided = cfg.cfg_scale > 1.0 if guided is None else bool(guided)
        need = self.TEXT_ID_KEYS if guided else self.TEXT_ID_KEYS[:1]
        if enc2 is not None:
            given = [k for k in self.TEXT_EMBED_KEYS_2 if batch.get(k) is not None]
            if given:
                raise ValueError(f"text_encoder_2: the batch carries {given}; the step encodes {list(self.TEXT_ID_KEYS_2)} itself")
            need = need + (self.TEXT_ID_KEYS_2 if guided else self.TEXT_ID_KEYS_2[:1])
        lacking = [k for k in need if batch.get(k) is None]
        if lacking:
            raise ValueError(f"{flag}: the batch lacks {lacking}")
        ids = batch["prompt_input_ids"].to(self.device)
        if guided:
            null = batch["null_input_ids"].to(self.device)
            if null.shape != ids.shape:
                raise ValueError(f"null_input_ids {tuple(null.shape)} and prompt_input_ids {tuple(ids.shape)} differ in shape")
            ids = torch.cat([null, ids])
        bs, L = batch["prompt_input_ids"].shape
        emb = self.text_encoder(ids, output="penultimate" if self.pipe.is_sdxl else "last")
        if enc2 is not None:
            ids2 = batch["prompt_input_ids_2"].to(self.device)
            if guided:
                ids2 = torch.cat([batch["null_input_ids_2"].to(self.device), ids2])
            if ids2.shape != ids.shape:
                raise ValueError(f"the second tower's ids {tuple(ids2.shape)} and the first tower's {tuple(ids.shape)} differ in shape")
            with torch.no_grad():
                e2, pooled = enc2(ids2, output="pooled")
            emb = ops.concat_cols(emb, ops.cast(e2, emb.dtype))
            self._pooled_2 = (pooled[bs:], pooled[:bs]) if guided else (pooled, None)
        elif self.pipe.is_sdxl:
            keys = ("negative_prompt_embeds_2", "prompt_embeds_2") if guided else ("prompt_embeds_2",)
            lacking = [k for k in keys if batch.get(k) is None]
            if lacking:
                raise ValueError(f"{flag} on an SDXL pipeline: the batch lacks {lacking}")
            e2 = torch.cat([batch[k].to(self.device) for k in keys]).detach()
            emb = ops.concat_cols(emb, ops.cast(e2.reshape(ids.shape[0] * L, -1).contiguous(), emb.dtype))
        emb = emb.reshape(ids.shape[0], L, -1)
        return (emb[bs:], emb[:bs]) if guided else (emb, None)

    def compute_losses(self, batch, training_steps=None, crop=None, attrcon_steps=None):
        """Forward graph of the step up to the scalar loss.  batch keys: prompt_embeds, negative_prompt_embeds
        (bs,L,C); blip_input_ids, blip_attention_mask (bs,T); optional latents (bs,4,h,w), noises [N x (bs,4,h,w)],
        gan_null_embeds (bs,L,C_D), real_latents (bs,4,h,w), masks (list of [n_obj,H,W] bool arrays), attributes;
        SDXL pipelines also take pooled_prompt_embeds / negative_pooled_prompt_embeds (bs,1280) [+ add_time_ids].
        train_text_encoder_lora, tune_text_encoder: prompt_input_ids, null_input_ids (bs,L) INSTEAD of the two embeddings (encode_prompts);
        with a text_encoder_2 also prompt_input_ids_2, null_input_ids_2 INSTEAD of the second encoder's and the pooled tensors."""
        cfg = self.cfg
        res = cfg.resolution
        if cfg.text_flag is not None:
            prompt_embeds, negative_prompt_embeds = self.encode_prompts(batch)
        else:
            prompt_embeds, negative_prompt_embeds = batch["prompt_embeds"], batch.get("negative_prompt_embeds")
        if training_steps is None:
            training_steps = sample_training_steps(cfg.total_step, cfg.K, self.rng)
        kw = {}
        if cfg.attrcon:
            if attrcon_steps is None:  # random.choices samples WITH replacement (training_script.py:590)
                attrcon_steps = self.rng.choices(training_steps, k=min(cfg.attrcon_train_steps, len(training_steps)))
            kw = dict(attrcon_train_steps=attrcon_steps, train_layer_ls=cfg.train_layer_ls, attn_reses=cfg.attn_reses)
        kw.update(self._sdxl_kw(batch))
        lat = self.pipe.forward(
            prompt_embeds, negative_prompt_embeds, height=res, width=res,
            training_timesteps=training_steps, num_inference_steps=cfg.total_step, guidance_scale=cfg.cfg_scale,
            latents=batch.get("latents"), noises=batch.get("noises"), return_latents=True, output_type="latent_tokens",
            guidance_rescale=cfg.cfg_rescale, **self._sampler_modes(batch), **kw)
        _dbg("sampler")
        bs = prompt_embeds.shape[0]
        if crop is None:
            crop = sample_crop(res, self.rng)
        h, w = res // 8, res // 8
        head = self.head_runner(lat, batch, crop, bs, h, w) if self.head_runner is not None else \
            self.head_losses(lat, batch, crop, bs, h, w)
        reward = head["reward"]
        out = dict(Blip=reward.detach(), token_logp=head["logp"], training_steps=training_steps, crop=crop)
        loss = -reward
        if cfg.gan_loss:
            loss = loss + cfg.gan_loss_weight * head["G_loss"]
            out["G_loss"] = head["G_loss"].detach()
        img, H, W = head["image"]
        if cfg.attrcon:
            tl, pl = (mask_loss_device if self.attrcon_on_device else mask_loss)(
                self.pipe.attn_dict, batch["masks"], batch["attributes"], cfg.train_layer_ls, bs, self.device)
            loss = loss + cfg.mask_token_loss_weight * tl + cfg.mask_pixel_loss_weight * pl
            out["token_loss"], out["pixel_loss"] = tl.detach(), pl.detach()
            self.pipe.attn_dict = {}
            _dbg("mask loss")
        out["loss"] = loss
        out["training_latents"] = lat
        out["image"] = (img, H, W)
        return out

    def _d_step(self, out, batch):
        if self.d_runner is not None:
            return self.d_runner(out, batch)
        return self._d_step_eager(out, batch)

    def _d_forward(self, out, batch):
        """forward half of the D step: zero the discriminator's gradients, D_loss on [fake.detach(); real] with its autograd
        graph (training_script.py:683-688)"""
        cfg = self.cfg
        h = w = cfg.resolution // 8
        if self.accum > 1:
            self.opt_D.zero_grad()  # only at the first micro-step of a window (decided on the device)
        else:
            self.D.zero_grad()
        real = ops.nchw_to_tokens(batch["real_latents"].to(self.device, torch.float32))
        return self.D.D_sd_pipeline_forward(out["training_latents"].detach(), "D",
                                            negative_prompt_embeds=batch["gan_null_embeds"],
                                            num_inference_steps=cfg.total_step, h=h, w=w, real_latents=real,
                                            **self._d_cond(batch))

    def _d_step_eager(self, out, batch):
        """D forward + backward on [fake.detach(); real] (training_script.py:683-690)."""
        D_loss = self._d_forward(out, batch)
        self._scaled(D_loss).backward()
        return D_loss.detach()

    def _scaled(self, loss):
        """what `accelerator.backward` differentiates: loss / gradient_accumulation_steps (the logs keep the unscaled loss)"""
        return loss if self.accum == 1 else loss * (1.0 / self.accum)

    @_own_streams_by_design()
    def _forward_backward(self, batch, fixed):
        """G forward + backward and the D forward + backward (everything of the step that precedes the exchange and
        the optimizer updates).  Returns a dict of device scalars (no host sync).

        The D step needs only the detached final latents, and it touches only the discriminator's gradient buffers:
        it is issued on its own HIP stream right after the G forward, so its ~1.2 k small kernels run concurrently
        with the G backward chain instead of after it (both are latency-bound at bs=1, neither fills the chip).  The
        results are bit-identical to the serial order (no atomics anywhere); COMAT_D_STREAM=0 restores it."""
        cfg = self.cfg
        ops.reset_side_stream_state()
        # a previous step raised between the D fork and the join in _apply_updates: its D kernels may still read
        # buffers this step is about to reuse - join before anything else is queued
        self._join_d()
        for b in self.trained:
            b.set_requires_grad(True)
        if self.accum > 1:
            self.opt.zero_grad()  # only at the first micro-step of a window (decided on the device)
        else:
            for b in self.trained:
                b.zero_grad()
        out = self.compute_losses(batch, **fixed)
        logs = {k: v for k, v in out.items() if k in ("Blip", "G_loss", "token_loss", "pixel_loss")}
        logs["step_loss"] = self._step_loss = out["loss"].detach()
        if self.reward_norm is not None:
            logs["reward_norm"] = self.reward_norm  # written by the backward pass below (device scalar, fixed address)
        self._last = (out["training_steps"], out["crop"])
        concurrent = self._own_stream("COMAT_D_STREAM")
        if concurrent:
            _, d_stream = self._fork("_d_stream")  # the G forward (latents, the discriminator's compute copies) is queued
            # the D stream reads the final latents: they stay referenced until that stream has been joined
            # (_apply_updates), so the allocator cannot hand their memory to main-stream work in the meantime
            self._d_keep = out["training_latents"]
            self._d_pending = True  # from here on the D stream holds work that must be joined, whatever happens below
            with torch.cuda.stream(d_stream), (ops.no_side_streams() if self.flat_d else contextlib.nullcontext()):
                logs["D_loss"] = self._d_step(out, batch)
        self._scaled(out["loss"]).backward()  # LoRA weight gradients run on the side stream; joined at end of backward
        _dbg("G backward")
        self._d_pending = concurrent  # joined in _apply_updates, after the G all-reduce has been launched
        if not concurrent and cfg.gan_loss:
            logs["D_loss"] = self._d_step(out, batch)
        return logs

    def _forward_backward_joined(self, batch, fixed):
        """_forward_backward with every stream it forked joined again: the capturable part of a data-parallel step (the
        gradient exchange and the optimizer follow outside the graph, see GraphedStep)."""
        logs = self._forward_backward(batch, fixed)
        if self.device.type == "cuda":
            ops.join_side_streams()
            self._join_d()
        return logs

    def _apply_updates(self):
        """all-reduce(mean) of the flat gradient buffers (RCCL, async) + clip + AdamW for G and D.  The G all-reduce is
        launched as soon as the G backward is queued, i.e. before the concurrently running D step is joined: on
        several GPUs it overlaps the tail of the D step; the D buffers follow once that stream has been joined."""
        if self.device.type == "cuda":
            ops.join_side_streams()  # idempotent; does not rely on the end-of-backward callback alone
        # gradient accumulation: the ranks exchange only what an update will read, on the closing micro-step (DDP's no_sync
        # on the others).  Decided by the host's copy of the window index; the optimizers' launches below are the same on
        # every micro-step and decide on the device
        exchange = self.opt.closing
        if exchange:
            self.reducer.start(*(b.flat_grad for b in self.trained))
        self._join_d()
        if self.cfg.gan_loss and exchange:
            self.reducer.start(self.D.bank.flat_grad, self.D.head_grad)
        scale = self.reducer.finish()  # 1 / world: the mean is taken inside the clip + AdamW pass
        # NOTE for readers of the buffers after this point: with more than one rank `flat_grad` / `head_grad` hold the SUM
        # over ranks and `opt.gnorm_sq` its squared norm; only comat_adamw applies `scale` (to the gradient and to the norm
        # it clips by).  The logs carry `grad_scale`: |mean gradient|^2 = grad_norm_sq * grad_scale^2.
        self.grad_scale = scale
        if self.accum > 1:
            self.opt.step(scale, step_loss=self._step_loss)
        else:
            self.opt.step(scale)
        for b, now in zip(self.trained, self._refresh_behind_update):
            b.mark_updated()
            if now:
                b.ensure_compute_copy()
        if self.cfg.gan_loss:
            self.opt_D.step(scale)
            self.D.bank.mark_updated()
        # fp8 forward with delayed scaling: this step's abs-maxima become the next step's scales - unless the generator's update
        # was skipped (a non-finite gradient norm): then the scales keep their values too
        ops.fp8_end_of_step(self.opt.gnorm_sq)
        r = ops.fp8_recipe()
        self.fp8_clipped = None
        if r is not None and r["account"] and ops.fp8_scaling() == "delayed" and getattr(self.pipe.unet, "fp8", False):
            if self._fp8_clipped is None:
                self._fp8_clipped = torch.zeros((), dtype=torch.int32, device=self.device)
            self.fp8_clipped = ops.fp8_clipped_sites(self.device, self._fp8_clipped)  # sites whose abs-max exceeded their scale

    def fp8_calibrate(self, batch):
        """scales of the first step under delayed fp8 scaling (TrainableSDPipeline.fp8_calibrate) from this batch's prompt"""
        cfg = self.cfg
        modes = self._sampler_modes(batch)
        modes.pop("renoise", None)
        modes.pop("bp_on_trained", None)  # a no-grad pass: nothing is detached or not
        return self.pipe.fp8_calibrate(batch["prompt_embeds"], batch.get("negative_prompt_embeds"), cfg.resolution,
                                       cfg.resolution, cfg.total_step, guidance_scale=cfg.cfg_scale, latents=batch.get("latents"),
                                       noises=batch.get("noises"), guidance_rescale=cfg.cfg_rescale, **modes, **self._sdxl_kw(batch))

    def train_step(self, batch, **fixed):
        """Full step: G forward/backward, D forward/backward, gradient exchange, G and D updates.  Returns a dict of
        detached device scalars (no host sync here) plus `training_steps` / `crop`.  The same schedule serves one GPU
        and data-parallel runs (the exchange is a no-op in a single-process run)."""
        logs = self._forward_backward(batch, fixed)
        sync = self.opt.closing  # before the update moves the window on
        self._apply_updates()
        self._window_logs(logs, sync)
        # non-finite => the generator update of this step was skipped.  Under gradient accumulation: the norm of the window's
        # partial sum so far (of loss / N gradients); the one an update is clipped by where sync_gradients holds
        logs["grad_norm_sq"] = self.opt.gnorm_sq
        logs["grad_scale"] = self.grad_scale      # 1 / world: grad_norm_sq is the norm of the SUM over ranks
        if self.opt.lr_now is not None:
            logs["lr"] = self.opt.lr_now          # the rate of the NEXT update (training_script.py:667; device word, fixed address)
        if self.fp8_clipped is not None:
            logs["fp8_clipped_sites"] = self.fp8_clipped
        logs["training_steps"], logs["crop"] = self._last
        return logs

    def validate(self, cfg, batch):
        """Validation sampling with the current weights (training_script.py:428-494; comat_amd/validate.py): cfg a
        validate.ValidationConfig, batch the validation prompts under the training batch's keys - prompt_embeds /
        negative_prompt_embeds [P, L, C] (SDXL: the pooled tensors and add_time_ids too), or, where a text tower is trained,
        prompt_input_ids / null_input_ids, encoded here without grad so that validation sees the trained tower; optional
        blip_input_ids / blip_attention_mask [P, T]: the result then carries the caption loss of every sample.
        Runs on the current (main) stream once the side streams are joined, between two `train_step` calls - inside an open
        accumulation window too - and leaves every later training result bit-identical to a run without it.
        -> validate.ValidationResult"""
        from .validate import Validator
        if self.device.type == "cuda":
            ops.join_side_streams()
        self._join_d()
        # the compute copies of everything trained, from the masters as they are NOW: a replayed whole-step graph rewrites the copies
        # at its start and the masters at its end, and the host's freshness marks know nothing of a replay
        for b in self.trained:
            b.mark_updated()
            b.ensure_compute_copy()
        guided = cfg.guidance_scale > 1.0
        pooled_2 = self._pooled_2
        try:
            if self.cfg.text_flag is not None:
                with torch.no_grad():
                    prompt_embeds, negative_prompt_embeds = self.encode_prompts(batch, guided=guided)
                    prompt_embeds = prompt_embeds.detach()
                    negative_prompt_embeds = None if negative_prompt_embeds is None else negative_prompt_embeds.detach()
            else:
                given = [k for k in self.TEXT_ID_KEYS + self.TEXT_ID_KEYS_2 if batch.get(k) is not None]
                if given:
                    raise ValueError(f"validate: the batch carries {given}, but the trainer has no text tower (neither "
                                     "StepConfig.train_text_encoder_lora nor tune_text_encoder): pass prompt_embeds")
                if batch.get("prompt_embeds") is None:
                    raise ValueError("validate: the batch lacks prompt_embeds")
                prompt_embeds, negative_prompt_embeds = batch["prompt_embeds"], batch.get("negative_prompt_embeds")
            sdxl = self._sdxl_kw(batch) if self.pipe.is_sdxl else {}
            ids = batch.get("blip_input_ids")
            return Validator(self.pipe, self.blip if ids is not None else None).run(
                cfg, prompt_embeds, negative_prompt_embeds, input_ids=ids, attention_mask=batch.get("blip_attention_mask"), **sdxl)
        finally:
            self._pooled_2 = pooled_2

    def _window_logs(self, logs, sync):
        """sync_gradients (host bool: did this call close a window - accelerator.sync_gradients, training_script.py:698,710 log and
        save only there) and, under gradient accumulation, train_loss (device word: the last closed window's sum of loss / N,
        :655,702).  Computed per call: a graph's recorded output dict must not carry them over."""
        logs["sync_gradients"] = sync
        if self.opt.train_loss is not None:
            logs["train_loss"] = self.opt.train_loss[1:]

    GATHERED = ("Blip", "G_loss", "D_loss", "token_loss", "pixel_loss", "train_loss")

    def gather_logs(self, logs):
        """The `accelerator.gather(...).mean()` of training_script.py:654,668-675,684 as floats: the cross-rank means of Blip,
        G_loss, D_loss, token_loss, pixel_loss and train_loss (one packed fp32 vector, one collective, one host read) and this
        rank's step_loss, lr and reward_norm (:667,677).  It synchronises: meant for logging steps, not for every step.  With
        one process it only reads.  Without gradient accumulation train_loss is the step's loss."""
        from .dist import all_reduce_mean
        first = lambda t: t.detach().reshape(-1)[:1].float()
        src = dict(logs)
        src.setdefault("train_loss", logs["step_loss"])
        if self.opt.lr_now is None:
            src["lr"] = torch.tensor([self.cfg.lr], dtype=torch.float32, device=self.device)
        names = [k for k in self.GATHERED if k in src]
        local = [k for k in ("step_loss", "lr", "reward_norm") if k in src]
        mean = all_reduce_mean(torch.cat([first(src[k]) for k in names]))
        vals = torch.cat([mean, torch.cat([first(src[k]) for k in local])]).tolist()
        return dict(zip(names + local, vals))


class GraphedStep:
    """The whole optimisation step as ONE hipGraph: G forward + backward, D forward + backward (on its own stream),
    LoRA weight gradients (side streams), gradient norms, clip + AdamW for G and D — ~17 k kernel launches that cost
    the host ~10 us each when issued one by one (the eager step is host-bound: bench `host_enqueue_ms_per_step` ~= the
    step time) replayed by the GPU's own command processor.

    What makes the step replayable:
      * every host value that changes between steps is a graph INPUT at a fixed device address: the batch tensors, the
        per-step noises, the crop (the crop + resize operator of the BLIP preprocessing is a pair of tap tables:
        `ResampleTables.static_copy / load`), and the AdamW step count (device counter, `FlatAdamW.counters`);
      * what does not change for a given list of trained denoise steps is baked in: timesteps (time-embedding
        projections, DDPM coefficients), the launch topology, every workspace.  One graph per distinct
        `training_steps` tuple (C2: N = K, a single tuple), captured lazily at its first use after one eager step;
      * no host synchronisation and no host-side data dependence inside the step (asserted by
        tests/test_step.py::test_step_is_enqueue_only).
    Streams inside the capture: the LoRA weight gradients of the G backward fork onto a side stream, the D step forks onto
    its own stream (its weight gradients stay on that stream: a fork from a forked stream crashes hipStreamEndCapture on
    ROCm 7.2 - located stage by stage in profiles/r02_c_stepgraph_stages.txt); both rejoin before the optimizer.
    Data-parallel runs (and COMAT_GRAPH_SPLIT=1): the graph ends where the streams have rejoined after the backward passes;
    the RCCL all-reduces and the two clip + AdamW updates (a dozen launches) follow eagerly, exactly as in the eager step -
    no collective is ever captured.
    Gradient checkpointing (StepConfig.gradient_checkpointing): the captured step holds the recompute launches - the nested
    backward of recompute.py captures like the plain one (tests/test_recompute.py::test_whole_step_graph_under_the_flag).
    Not captured (the eager path runs instead): attribute-concentration steps (their masks are resized on the host).
    Results are bit-identical to eager steps (`tests/test_step.py::test_graphed_step_matches_eager`)."""

    def __init__(self, trainer: CoMatTrainer):
        self.tr = trainer
        self.graphs = {}
        self.static = ops.StaticBatch(trainer.device)  # fixed-address copies of the batch
        self.pool = None
        self.failed = None      # message of a failed capture: from then on every call is an eager step

    def supported(self, batch):
        cfg = self.tr.cfg
        # the sampler's other modes (early_exit, double_laststep, fast_training, guidance off) run eagerly or from segments
        modes = cfg.early_exit or cfg.double_laststep or cfg.fast_training or cfg.cfg_scale <= 1.0
        # an SDXL discriminator reads batch["gan_pooled_null_embeds"], which has no fixed-address staging buffer here: eager / segments
        # --tune_vae, --full_finetuning: the step runs eagerly or from segments (the whole-step graph is not offered with trained
        # VAE / UNet weights).  --train_text_encoder_lora, --tune_text_encoder: the eager step (not built inside the graph runners)
        return (self.tr.device.type == "cuda" and not cfg.attrcon and not modes and not isinstance(self.tr.D, D_sdxl)
                and not cfg.tune_vae and not cfg.full_finetuning and cfg.text_flag is None
                and batch.get("noises") is not None and batch.get("latents") is not None)

    @staticmethod
    def split():
        """graph = forward + backward only; exchange + optimizer eager (always so with more than one rank)"""
        from .dist import world_size
        return world_size() > 1 or os.environ.get("COMAT_GRAPH_SPLIT") == "1"

    def __call__(self, batch, training_steps=None, crop=None):
        tr = self.tr
        cfg = tr.cfg
        if self.failed is not None or not self.supported(batch):
            return tr.train_step(batch, **{k: v for k, v in (("training_steps", training_steps), ("crop", crop))
                                            if v is not None})
        if training_steps is None:
            training_steps = sample_training_steps(cfg.total_step, cfg.K, tr.rng)
        if crop is None:
            crop = sample_crop(cfg.resolution, tr.rng)
        sb, reallocated = self.static.stage(batch, strict=True)
        if reallocated:  # the graphs hold the addresses of the buffers they were captured with
            self.graphs = {}
        res = cfg.resolution
        split = self.split()
        # host-side values the capture bakes in are part of the key (SDXL: add_time_ids feed the added time embedding)
        meta = tuple(batch["add_time_ids"]) if batch.get("add_time_ids") is not None else None
        key = (tuple(training_steps), split, meta, os.environ.get("COMAT_GRAPH_D", "fork"))
        # D step inside the capture: forked onto its own stream (it overlaps the G backward chain: 187 -> 168 ms per C2 step
        # on MI355X) with its weight gradients kept on that stream - a fork from a forked stream (nested) crashes
        # hipStreamEndCapture on ROCm 7.2.  COMAT_GRAPH_D=serial runs it in stream order on the main stream instead.
        serial = os.environ.get("COMAT_GRAPH_D", "fork") == "serial"
        with tr.d_placement(serial_d=serial, flat_d=not serial):
            if key not in self.graphs:
                return self._capture(key, sb, training_steps, crop, split)
            g, out = self.graphs[key]
            tr.blip.tables(res, res, crop)  # loads this crop's operator into the fixed-address tables
            sync = tr.opt.closing
            g.replay()
            out = dict(out)
            tr._window_logs(out, sync)
            if not split:  # the replay executed the optimizers' launches: the host's copy of the window index follows
                for o in (tr.opt, tr.opt_D):
                    if o is not None:
                        o.advance()
            if split:
                tr._step_loss = out["step_loss"]  # this graph's word (another key's capture may have run since)
                tr._apply_updates()
                out["grad_norm_sq"] = tr.opt.gnorm_sq
                if tr.opt.lr_now is not None:
                    out["lr"] = tr.opt.lr_now
                if tr.fp8_clipped is not None:
                    out["fp8_clipped_sites"] = tr.fp8_clipped
            out["training_steps"], out["crop"] = list(training_steps), crop
            return out

    def _capture(self, key, sb, training_steps, crop, split):
        """first use of `key`: one eager step (this call's step), then the capture of the graph later calls replay"""
        tr = self.tr
        res = tr.cfg.resolution
        # one eager step with these inputs first: fills every host-side memo (time embeddings, targets, crop
        # tables, workspaces of the default stream) and is a real optimisation step of its own.  The fixed-address
        # crop tables serve the eager step too.
        tr.blip.install_static_tables(res, res, crop)
        logs = tr.train_step(sb, training_steps=list(training_steps), crop=crop)
        tr.bank.mark_updated()
        if tr.D is not None:
            tr.D.bank.mark_updated()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        # captured on the package's capture stream, whose workspaces (and its side stream's) exist and are zeroed
        # already: nothing a later graph on the same stream relies on is initialised by a node of this one
        cap = ops.capture_stream(tr.device)
        if tr._d_stream is not None:
            ops.prepare_capture_stream(tr.device, tr._d_stream)
        try:
            with ops.graph_capture(g, pool=self.pool, stream=cap, **ops.capture_kwargs(thread_local=split)):
                if split:
                    out = tr._forward_backward_joined(sb, dict(training_steps=list(training_steps), crop=crop))
                else:
                    out = tr.train_step(sb, training_steps=list(training_steps), crop=crop)
        except Exception as e:  # noqa: BLE001 - see `failed`
            # A call of this object is ONE optimisation step with ONE gradient exchange, whatever happens: the eager
            # step above was it (its all-reduces are matched on every rank), so a failed capture must not surface
            # as an exception a caller would answer by stepping again.  From here on every call steps eagerly.
            self.failed = f"{type(e).__name__}: {e}"
            # (the fixed-address crop tables stay installed: segment graphs captured earlier read them, and
            # Blip.tables() loads them with whatever crop an eager call asks for)
            tr.abandon_capture()
            return logs
        if self.pool is None:
            self.pool = g.pool()
        self.graphs[key] = (g, out)
        # the capture did not execute anything: the eager step above is this call's step
        return logs
