"""K-of-N differentiable DDPM sampler — the MI355X-native counterpart of `TrainableSDPipeline.forward`
(TrainableSDPipeline.py:20-225) and of its attribute-concentration variant
(AttrConcenTrainableSDPipeline.py:38-279), with the same argument names and gradient topology:

  * UNet runs without grad on non-trained steps, and with grad on a NON-detached input on the K trained steps
    (`bp_on_trained=True`, TrainableSDPipeline.py:138-145);
  * the CFG combine + scheduler step runs with grad for every i >= min(training_timesteps) (:163-167), so the loss
    gradient reaches earlier trained steps through the (affine) DDPM chain;
  * on `attrcon_train_steps` the cross-attention maps of the COND half are handed out per timestep
    (`attn_dict[str(t)] = {place_res: [maps]}`, AttrConcenTrainableSDPipeline.py:239-279).  The reference runs the
    cond and uncond halves as two UNet calls there; here it stays one batched call and the cond half of the
    probability tensor is sliced — same arithmetic, half the launches.
Latents stay fp32 channels-last tokens for the whole loop; CFG + DDPM step is one fused kernel.
"""
from __future__ import annotations

import math

import torch

from . import ops, recompute
import os

from .unet import GraphedUNetForward, UNet, VAEDecoder, _capturing, regroup_maps


class DDPMScheduler:
    """DDPMScheduler with SD1.5's config (scaled_linear betas, steps_offset 1, leading spacing, epsilon prediction,
    fixed_small variance, clip_sample False) — SURVEY.md A.4; forced by training_utils/pipeline.py:50-59."""

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, steps_offset=1):
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        self.alphas_cumprod = torch.cumprod(1.0 - betas, dim=0)
        self.num_train_timesteps = num_train_timesteps
        self.steps_offset = steps_offset
        self.num_inference_steps = None
        self.timesteps = []

    def set_timesteps(self, num_inference_steps):
        self.num_inference_steps = num_inference_steps
        ratio = self.num_train_timesteps // num_inference_steps
        self.timesteps = [i * ratio + self.steps_offset for i in range(num_inference_steps)][::-1]
        return self.timesteps

    def scale_model_input(self, sample, t):
        return sample  # identity for DDPM

    def step_coefficients(self, t):
        """prev_sample = cx * sample + ce * eps + sigma * z (x0 eliminated from DDPMScheduler.step)."""
        prev_t = t - self.num_train_timesteps // self.num_inference_steps
        a_t = float(self.alphas_cumprod[t])
        a_prev = float(self.alphas_cumprod[prev_t]) if prev_t >= 0 else 1.0
        beta_t, beta_prev = 1.0 - a_t, 1.0 - a_prev
        cur_alpha = a_t / a_prev
        cur_beta = 1.0 - cur_alpha
        c_x0 = math.sqrt(a_prev) * cur_beta / beta_t
        c_xt = math.sqrt(cur_alpha) * beta_prev / beta_t
        sigma = math.sqrt(max(beta_prev / beta_t * cur_beta, 1e-20)) if t > 0 else 0.0
        sa, sb = math.sqrt(a_t), math.sqrt(beta_t)
        return c_xt + c_x0 / sa, -c_x0 * sb / sa, sigma

    def x0_coefficients(self, t):
        """pred_original_sample = px * sample + pe * eps of DDPMScheduler.step (epsilon prediction)."""
        a_t = float(self.alphas_cumprod[t])
        return 1.0 / math.sqrt(a_t), -math.sqrt(1.0 - a_t) / math.sqrt(a_t)

    def add_noise_coefficients(self, t):
        """noisy = sa * sample + sb * noise of DDPMScheduler.add_noise."""
        a_t = float(self.alphas_cumprod[t])
        return math.sqrt(a_t), math.sqrt(1.0 - a_t)


class TrainableSDPipeline:
    is_sdxl = False

    def __init__(self, unet: UNet, vae: VAEDecoder, scheduler: DDPMScheduler | None = None):
        self.unet, self.vae = unet, vae
        self.scheduler = scheduler or DDPMScheduler()
        self.dtype, self.device = unet.dtype, unet.device
        self.attn_dict = {}
        # hipGraph replay for the untrained (no-grad) denoise steps; COMAT_GRAPHS=0 disables it (COMAT_GRAPHS_ATTRCON=0
        # only for forwards that also capture attention maps).  History: an early build raised a hardware exception
        # in the second optimisation step when graphs and attribute-concentration steps were combined; it has not
        # reproduced since the attention-map gather kernel was rewritten (fixed-order, no atomics) — see DESIGN.md.
        # SDXL: the prompt-dependent half of the time embedding is an extra graph input (validated on MI355X in round 2;
        # COMAT_SDXL_GRAPHS=0 disables).  One graph per timestep: capture them up front with prepare_graphs() — a
        # capture costs ~3 eager forwards, and lazily captured graphs only pay off after every timestep has been seen
        # (only a real UNet is replayed from graphs: a stand-in callable - the reference-code fixtures of tests/ drive this
        # class with a small torch "UNet" on the device - has no static launch topology to rely on)
        use_graphs = (torch.device(self.device).type == "cuda" and os.environ.get("COMAT_GRAPHS", "1") != "0"
                      and isinstance(unet, UNet)
                      and (not unet.cfg.addition_embed or os.environ.get("COMAT_SDXL_GRAPHS", "1") != "0"))
        self.graphed = GraphedUNetForward(unet) if use_graphs else None
        # hook of segments.SegmentedStep: runs a TRAINED UNet call (slot = its rank among the trained steps) from a pair
        # of replayable graphs instead of eager launches; None = eager
        self.trained_runner = None
        # the text key / value projections are shared by the denoise steps of one sampler call (UNet.__call__); replayed
        # segments recompute them per call, and so does the eager path when asked to match them bit for bit
        self.share_text_kv = True
        # `--gradient_checkpointing` (training_utils/pipeline.py:73-74), per trained call: its activations are dropped after
        # the forward and recomputed inside the backward pass (comat_amd/recompute.py).  step.CoMatTrainer sets it from
        # StepConfig.gradient_checkpointing; whoever drives the pipeline directly may set it too
        self.gradient_checkpointing = False

    def _trained_unet(self, xin, B, h, w, t, ctx, L, cap, added, kv_cache):
        """an eager trained UNet call -> (eps, maps); checkpointed, it projects its own text keys / values"""
        if self.gradient_checkpointing:
            return recompute.unet_call(self.unet, xin, B, h, w, t, ctx, L, cap, added)
        if ctx.requires_grad:
            # a trained text tower (StepConfig.train_text_encoder_lora): the context's gradient is summed per CALL first - through
            # this alias, a node of its own and no launch - and over the calls after that, which is the order the checkpointed
            # call sums it in (its nested backward returns one gradient per call): the two modes give the same bits
            ctx = ctx.view_as(ctx)
        return self.unet(xin, B, h, w, t, ctx, L, capture_places=cap, added=added, kv_cache=kv_cache)

    def prepare_graphs(self, batch_size, height, width, L, num_inference_steps, guidance_scale=7.5):
        """Capture the no-grad UNet forward graph of every timestep up front (before training starts), so that no
        capture — and none of the allocator housekeeping it triggers — happens in the middle of a step.
        guidance_scale <= 1: the UNet batch of a sampler call without guidance (batch_size instead of twice that)."""
        if self.graphed is None:
            return 0
        h, w = height // 8, width // 8
        B = (2 if guidance_scale > 1.0 else 1) * batch_size
        x = torch.zeros((B * h * w, self.unet.cfg.in_channels), dtype=self.dtype, device=self.device)
        ctx = torch.zeros((B * L, self.unet.cfg.cross_attention_dim), dtype=self.dtype, device=self.device)
        added = None
        if self.unet.cfg.addition_embed:
            added = torch.zeros((B, self.unet.cfg.time_embed_dim), dtype=self.dtype, device=self.device)
        # fp8 forward, delayed scaling, before any calibration: the graphs are captured (they hold the delayed launches, which
        # read the scale words at replay time) but not run - a replay waits until every site has a scale (GraphedUNetForward)
        only = self.graphed._fp8_on_trust() and ops.fp8_unready(self.device)
        for t in self.scheduler.set_timesteps(num_inference_steps):
            self.graphed(x, B, h, w, int(t), ctx, L, added=added, capture_only=only)
        torch.cuda.synchronize()
        return len(self.graphed.graphs)

    def fp8_calibrate(self, prompt_embeds, negative_prompt_embeds, height, width, num_inference_steps, guidance_scale=7.5,
                      latents=None, noises=None, guidance_rescale=0.0, early_exit=False, double_laststep=False,
                      fast_training=False, **sdxl_kw):
        """fp8 forward with delayed scaling (ops.set_fp8_scaling('delayed')): the scales of the FIRST optimisation step.  One
        eager no-grad sampler pass over all `num_inference_steps` denoise steps of this prompt in which every quantisation site
        quantises under its own abs-max and records it; the maxima over the pass become the scales (ops.fp8_end_of_step), as
        they will after every later step.  Captured graphs are not touched (they hold the delayed-scaling launches, which read
        the scale words at replay time).  `guidance_rescale`: the step's own value (the calibration runs the trajectory the step
        will run).  guidance_scale <= 1: the pass runs without guidance, as the step will (`negative_prompt_embeds` may be None).
        `early_exit` / `double_laststep` / `fast_training`: accepted and not forwarded - those modes visit a subset of the
        `num_inference_steps` timesteps, which trained steps they keep is drawn per step, and the full pass covers them all.
        -> True when a calibration ran."""
        if not getattr(self.unet, "fp8", False) or ops.fp8_scaling() != "delayed":
            return False
        graphed, runner = self.graphed, self.trained_runner
        self.graphed = self.trained_runner = None
        try:
            with torch.no_grad(), ops.fp8_calibration():
                self.forward(prompt_embeds, negative_prompt_embeds, height=height, width=width, training_timesteps=(),
                             num_inference_steps=num_inference_steps, guidance_scale=guidance_scale, latents=latents,
                             noises=noises, output_type="latent", guidance_rescale=guidance_rescale, **sdxl_kw)
        finally:
            self.graphed, self.trained_runner = graphed, runner
        ops.fp8_end_of_step()
        return True

    def prepare_latents(self, batch_size, height, width, generator=None, latents=None):
        """(bs,4,h/8,w/8) NCHW fp32 -> channels-last tokens [bs*h*w, 4] fp32 on the device."""
        h, w = height // 8, width // 8
        if latents is None:
            latents = torch.randn((batch_size, 4, h, w), generator=generator, dtype=torch.float32)
        latents = latents.to(self.device, torch.float32)
        return ops.nchw_to_tokens(latents), h, w

    def forward(self, prompt_embeds, negative_prompt_embeds, height=512, width=512, training_timesteps=(),
                num_inference_steps=50, guidance_scale=7.5, latents=None, generator=None, noises=None,
                detach_gradient=True, bp_on_trained=True, early_exit=False, double_laststep=False,
                fast_training=False, return_latents=False, attrcon_train_steps=(), train_layer_ls=(),
                attn_reses=(64, 32, 16, 8), output_type="image", pooled_prompt_embeds=None,
                negative_pooled_prompt_embeds=None, add_time_ids=None, guidance_rescale=0.0, renoise=None):
        """prompt_embeds / negative_prompt_embeds: (bs, L, cross_dim) text-encoder outputs (the CLIP text encoder is
        a no-grad preprocessing step outside this path - or, under StepConfig.train_text_encoder_lora, clip.ClipTextEncoder
        with trained LoRA factors: the embeddings then carry a gradient, which the trained UNet calls hand back through their
        text key / value projections; the no-grad denoise steps read the values only).  Returns image/2+0.5 as (bs,3,H,W) [output_type 'image'] or
        as channels-last tokens ([bs*H*W,3], H, W) ['tokens'], plus the final latents when `return_latents`;
        output_type 'latent' returns the final latents (bs,4,h,w) fp32 without decoding.
        guidance_rescale > 0 (`--cfg_rescale`): every denoise step, trained or not, rescales the guided noise of each sample
        towards the standard deviation of its text-conditioned prediction (TrainableSDPipeline.py:159-161, :822-824), fused
        with the scheduler step; 0 runs the plain fused step.
        guidance_scale <= 1 (`--cfg_scale 1`): guidance is off (:70,90,135,155): `negative_prompt_embeds` may be None, the
        context and the UNet batch are bs, `guidance_rescale` is ignored (:159).
        detach_gradient / bp_on_trained (:140-145): the UNet input is detached when `detach_gradient`, except on trained steps
        when `bp_on_trained`.
        fast_training (:96-98): the timestep list becomes its trained entries and every remaining step is trained; `noises[i]`
        is indexed by the new position; the scheduler's stride stays num_train_timesteps // num_inference_steps.
        early_exit (:168,175-177): after the last trained step the loop ends and the latents are that step's
        `pred_original_sample`; that step writes no x_prev and no later UNet call runs.  With no trained step there is no exit.
        double_laststep (:133,138,163,188-213): every loop step runs without grad; then the latents are re-noised to
        t = timesteps[training_timesteps[0]] with the draw `renoise` (bs,4,h,w; drawn here when None) and ONE trained UNet call
        with a plain scheduler step on the noisy latents follows (its step noise is `noises[len(timesteps)]`: `noises` carries
        one more entry).  The input of that call is the reference's `noisy_model_input.detach() if do_detach else
        latent_model_input` with the `do_detach` the LAST loop step left behind: when that step was a trained one (and
        `bp_on_trained`), the reference feeds the last loop step's model input, not the noisy one.  That is mirrored here.
        SDXL (:657-846): `early_exit` is a plain break after the trained step's x_prev (:835-836), `detach_gradient` applies to
        every step; `double_laststep` / `fast_training` are not in that signature."""
        if self.is_sdxl and (double_laststep or fast_training):
            raise NotImplementedError("TrainableSDXLPipeline.forward has no double_laststep / fast_training (TrainableSDPipeline.py:657-694)")
        guided = guidance_scale > 1.0  # do_classifier_free_guidance
        halves = 2 if guided else 1
        phi = guidance_rescale if guided else 0.0
        bs, L, _ = prompt_embeds.shape
        B = halves * bs
        dev, T = self.device, self.dtype
        ctx = (torch.cat([negative_prompt_embeds, prompt_embeds]) if guided else prompt_embeds).to(dev, torch.float32)
        # (cast_grad: the launch of ops.cast, and a node that hands the gradient on when the context carries one - the output of a
        # trained text tower, StepConfig.train_text_encoder_lora)
        ctx = ops.cast_grad(ctx.reshape(B * L, -1).contiguous(), T)
        added = None
        if self.is_sdxl:  # added_cond_kwargs of TrainableSDPipeline.py:772-784,807
            if add_time_ids is None:
                add_time_ids = (height, width, 0, 0, height, width)  # original_size + crop_top_left + target_size
            text_embeds = (torch.cat([negative_pooled_prompt_embeds, pooled_prompt_embeds]) if guided
                           else pooled_prompt_embeds).to(dev, torch.float32)
            # prompt-level constant: computed once here, shared by every denoise step (and a graph input)
            added = self.unet.added_embedding(text_embeds, [list(add_time_ids)] * B)
        timesteps = self.scheduler.set_timesteps(num_inference_steps)
        training_timesteps = list(training_timesteps)
        if fast_training:  # the scheduler keeps its stride: the reference overwrites `.timesteps` and nothing else
            timesteps = [timesteps[i] for i in training_timesteps]
            training_timesteps = list(range(len(timesteps)))
        if double_laststep and not training_timesteps:
            raise ValueError("double_laststep re-noises to timesteps[training_timesteps[0]]: it needs a trained step")
        lat, h, w = self.prepare_latents(bs, height, width, generator, latents)
        tmin = min(training_timesteps) if training_timesteps else 0
        t_exit = max(training_timesteps) if (early_exit and training_timesteps) else None
        loop_grad = not double_laststep  # double_laststep switches all three grad gates of the loop off
        places = sorted({s.split("_")[0] for s in train_layer_ls})
        self.attn_dict = {}
        if self.graphed is not None:
            self.graphed.new_sampler_call()  # this call's context / LoRA factors: its text keys / values are projected once
        # text key / value projections shared by the denoise steps of this call (see UNet.__call__)
        kv_cache = {} if (self.share_text_kv and self.trained_runner is None) else None
        wanted = {(s_.split("_")[0], int(s_.split("_")[1])) for s_ in train_layer_ls}
        slot_of = {i: j for j, i in enumerate(sorted(set(training_timesteps)))}
        do_detach, x2 = detach_gradient, None

        def draw(i):
            if noises is not None:
                return ops.nchw_to_tokens(noises[i].to(dev, torch.float32))
            return torch.randn(lat.shape, generator=generator, dtype=torch.float32,
                               device=dev if generator is None else generator.device).to(dev)

        for i, t in enumerate(timesteps):
            train = i in training_timesteps
            with_grad = train and loop_grad  # this step's UNet call runs with grad
            with torch.set_grad_enabled((len(training_timesteps) == 0 or i > tmin) and loop_grad):
                x2 = ops.concat_rows(lat, lat) if guided else lat
            with torch.set_grad_enabled(with_grad):
                # SDXL has no bp_on_trained exception: with `detach_gradient` it detaches the UNet input on every step
                # (TrainableSDPipeline.py:805-809, AttrConcenTrainableSDXLPipeline.py:393-410)
                do_detach = detach_gradient and not (train and bp_on_trained and not self.is_sdxl)
                xin = x2.detach() if do_detach else x2
                xin = ops.cast_grad(xin, T)
                cap = places if (with_grad and i in attrcon_train_steps) else ()
                graph_ok = not attrcon_train_steps or os.environ.get("COMAT_GRAPHS_ATTRCON", "1") != "0"
                if (not with_grad and self.graphed is not None and graph_ok
                        and not torch.cuda.is_current_stream_capturing()):
                    eps2, maps = self.graphed(xin, B, h, w, int(t), ctx, L, added=added), {}
                elif with_grad and self.trained_runner is not None and not _capturing(dev):
                    eps2, maps = self.trained_runner(slot_of[i], xin, B, h, w, int(t), ctx, L, cap, added, wanted)
                elif with_grad:
                    eps2, maps = self._trained_unet(xin, B, h, w, int(t), ctx, L, cap, added, kv_cache)
                else:
                    eps2, maps = self.unet(xin, B, h, w, int(t), ctx, L, capture_places=cap, added=added,
                                           kv_cache=kv_cache)
                if cap:
                    cond = {p: [m[bs:] if guided else m for m in lst] for p, lst in maps.items()}
                    self.attn_dict[str(int(t))] = regroup_maps(cond, reses=attn_reses)
            exiting = i == t_exit
            want_x0 = exiting and not self.is_sdxl  # the exiting step's x_prev is never read: only x0 is written
            z = None if want_x0 else draw(i)
            dbg = os.environ.get("COMAT_DEBUG_SYNC")
            if dbg == "1" or (dbg == "train" and train) or (dbg == "nograd" and not train):
                torch.cuda.synchronize()
                print(f"[comat] denoise step {i} (t={int(t)}, train={train}, capture={bool(cap)}) ok", flush=True)
            cx, ce, sigma = self.scheduler.step_coefficients(int(t))
            with torch.set_grad_enabled((len(training_timesteps) == 0 or i >= tmin) and loop_grad):
                if guided and not want_x0:
                    lat = ops.cfg_ddpm_step(lat, eps2, z, guidance_scale, cx, ce, sigma, rescale=guidance_rescale, batch=bs)
                else:
                    x_prev, x0 = ops.ddpm_step(lat, eps2, z, guidance_scale, cx, ce, sigma, halves=halves,
                                               x0_coef=self.scheduler.x0_coefficients(int(t)) if want_x0 else None,
                                               want_prev=not want_x0, rescale=phi, batch=bs)
                    lat = x0 if want_x0 else x_prev
            if exiting:
                break
        if double_laststep:
            with torch.enable_grad():
                t = timesteps[training_timesteps[0]]
                if renoise is not None:
                    noise = ops.nchw_to_tokens(renoise.to(dev, torch.float32))
                else:
                    noise = torch.randn(lat.shape, generator=generator, dtype=torch.float32,
                                        device=dev if generator is None else generator.device).to(dev)
                sa, sb = self.scheduler.add_noise_coefficients(int(t))
                noisy, xin = ops.add_noise(lat, noise, sa, sb, halves, T)
                if not do_detach:  # the reference's `latent_model_input`: the model input of the LAST loop step (docstring)
                    xin = ops.cast_grad(x2, T)
                if self.trained_runner is not None and not _capturing(dev):
                    eps2, _ = self.trained_runner(0, xin, B, h, w, int(t), ctx, L, (), added, wanted)
                else:
                    eps2, _ = self._trained_unet(xin, B, h, w, int(t), ctx, L, (), added, kv_cache)
                z = draw(len(timesteps))
                cx, ce, sigma = self.scheduler.step_coefficients(int(t))
                if guided:
                    lat = ops.cfg_ddpm_step(noisy, eps2, z, guidance_scale, cx, ce, sigma, rescale=guidance_rescale, batch=bs)
                else:
                    lat = ops.ddpm_step(noisy, eps2, z, guidance_scale, cx, ce, sigma, halves=1, batch=bs)[0]
        if output_type == "latent":  # TrainableSDPipeline.py:224-225: the final latents, no decode
            return ops.tokens_to_nchw(lat, bs, h, w)
        if output_type == "latent_tokens":  # the same as channels-last tokens [bs*h*w, 4] fp32 (decode_tokens follows)
            return lat
        img, H, W = self.decode_tokens(lat, bs, h, w, return_latents)
        if output_type == "tokens":
            out = (img, H, W)
        else:
            out = ops.tokens_to_nchw(img, bs, H, W)
        if return_latents:
            return out, (lat if output_type == "tokens" else ops.tokens_to_nchw(lat, bs, h, w))
        return out


    def decode_tokens(self, lat, bs, h, w, return_latents=False, raw=False):
        """`vae.decode(latents / scaling_factor)` (+ `/2 + 0.5`, TrainableSDPipeline.py:219-223) on channels-last latent
        tokens -> (image tokens [bs*H*W, 3], H, W).  raw: the decode as it leaves the VAE, without the `/2 + 0.5` launch
        (validation sampling: comat_image_u8 denormalises on its way to bytes)"""
        z0 = ops.cast_grad(ops.affine(lat, 1.0 / self.vae.cfg.scaling_factor, 0.0), getattr(self.vae, "dtype", self.dtype))
        img, H, W = self.vae(z0, bs, h, w)
        if not raw and not (self.is_sdxl and return_latents):  # SDXL + return_latents returns the raw decode (:838-840)
            img = ops.affine(img, 0.5, 0.5)
        return img, H, W


class TrainableSDXLPipeline(TrainableSDPipeline):
    """SDXL variant (TrainableSDPipeline.py:657-846, AttrConcenTrainableSDXLPipeline.py:234-496): pooled text
    embedding + size/crop ids as additional conditioning, UNet input always detached, raw VAE decode returned with
    `return_latents`.  Use with an SDXL_UNET-style UNetConfig and VAEConfig(scaling_factor=0.13025)."""
    is_sdxl = True
