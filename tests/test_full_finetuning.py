"""`--full_finetuning` of the generator UNet, the model side (training_utils/pipeline.py:60-61,85,125-126; training_script.py:177-178,
392-395): unet.UNetBank holds every parameter, UNet(cfg, sd, dtype, device, bank=...) reads them, and ONE call under autograd
accumulates the gradient of EVERY parameter into the bank.

The oracle is oracle.sd.unet_forward(sd, ..., lora=None) with every entry of `sd` a leaf, the loss (eps * w).sum() with a fixed random
w, on B = 2, 8 x 8 latents, L = 7, t = 401; the UNet's input does NOT require grad (the first trained denoise step: conv_in, the text
key / value projections and the first embedding layers have no differentiable input).  In fp32 EACH parameter's gradient is within
1e-3 rel-L2 of the oracle's - the project's fp32 parity bound - and none is left out; the oracle's own gradients are checked to be
non-zero for every parameter, so that a missing gradient cannot hide.

The step (second half of the module): the world is tests/test_tune_vae.make_inputs with W["lora"] = {} and every W["unet"] entry a
leaf; the oracle is oracle.step.g_loss_terms plus ONE torch.optim.AdamW over those leaves after clip_grad_norm_ (max_grad_norm 0.1
against an oracle |g| of 0.4255: the clip is active).  The UPDATE p_after - p_before is compared over the elements whose oracle
clipped gradient is >= 10 x adam_epsilon (elsewhere AdamW's m / (sqrt(v) + eps) amplifies rounding noise to the size of the update).
Its bound is 10 x the distance of two ORACLE runs that differ only in the convolution algorithm
(torch.backends.mkldnn.flags(enabled=False)), re-measured on the CPU with tools/mb_full_finetune_step.py --oracle-distance
(profiles/full_finetuning.txt):
    two oracle runs:   gradient rel-L2 6.671e-6;  restricted update rel-L2 5.810e-6 (98.1 % of 1 460 868 elements kept);
                       unrestricted update 2.054e-4 (which is why it is restricted)
    ABI simulator:     gradient 7.896e-6;  restricted update 6.285e-6;  unrestricted 2.722e-4
so UPDATE_LIMIT = 10 x 5.810e-6 = 5.81e-5 (the product reorders every contraction, the two oracle runs only the convolutions: hence
the factor), and the simulator stays inside it.
bf16 storage against the fp32 oracle on the same (bf16-representable) weights: UNet-gradient rel-L2 within 2 x the distance the ABI
simulator shows on these inputs, 9.662e-2, measured on the CPU (profiles/full_finetuning_bf16_errors.txt) - the convention of
tests/test_tune_vae.BF16_VAE_GRAD_LIMIT.

Every case runs on the ABI simulator (tests/sim_backend.py) and, marked gpu, on the library."""
import dataclasses
import functools

import pytest
import torch

from comat_amd import config, ops, weights
from comat_amd.unet import GraphedUNetForward, LoRABank, UNet, UNetBank
from helpers import rel_l2, tok
from oracle import sd as O

F32, BF16 = torch.float32, torch.bfloat16
CFGS = {"sd": config.TINY_UNET, "sdxl": config.TINY_SDXL_UNET}
B, HW, L, T = 2, 8, 7, 401
FP32_GRAD_LIMIT = 1e-3  # the project's fp32 parity bound (BASELINE.md s. 5), per parameter


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def world(kind):
    """state dict, inputs and the oracle's eps and per-parameter gradients; computed once and shared (never written)"""
    cfg = CFGS[kind]
    sd = weights.make_unet_weights(cfg, perturb_norms=True)
    x, ctx, w = rnd(B, 4, HW, HW, seed=1), rnd(B, L, cfg.cross_attention_dim, seed=2), rnd(B, 4, HW, HW, seed=3)
    added = None
    if cfg.addition_embed:
        added = (rnd(B, cfg.pooled_dim, seed=4), torch.tensor([[64.0, 64.0, 0.0, 0.0, 64.0, 64.0]] * B))
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    eps = O.unet_forward(leaves, O.UNetConfig(**dataclasses.asdict(cfg)), x, T, ctx, None, None, added)
    (eps * w).sum().backward()
    grads = {k: v.grad for k, v in leaves.items()}
    return sd, x, ctx, w, added, eps.detach(), grads


def call(unet, kind, dev, dtype=F32):
    sd, x, ctx, w, added, _, _ = world(kind)
    a = None if added is None else (added[0].to(dev), added[1].tolist())
    cd = ctx.shape[-1]
    return unet(tok(x).to(dev, dtype), B, HW, HW, T, ctx.reshape(-1, cd).to(dev, dtype), L, added=a)[0]


def loss_of(eps, kind, dev):
    return (eps.float() * tok(world(kind)[3]).to(dev)).sum()


def bank_grads(bank):
    """the bank's gradient by diffusers name, in the state dict's layout"""
    keep = bank.flat
    try:
        bank.flat = bank.flat_grad  # state_dict() undoes the layout changes of whatever `flat` is
        return bank.state_dict()
    finally:
        bank.flat = keep


@pytest.mark.parametrize("kind", ["sd", "sdxl"])
def test_unet_call_every_parameter_gradient(dev, kind):
    sd, _, _, _, _, eps_o, grads = world(kind)
    norms = {k: float(g.norm()) for k, g in grads.items() if g is not None}
    assert len(norms) == len(sd) and min(norms.values()) > 0, "the oracle itself leaves a parameter without a gradient"
    print(f"{kind}: {len(sd)} parameters, oracle gradient norms {min(norms.values()):.3g} .. {max(norms.values()):.3g}")
    bank = UNetBank(CFGS[kind], sd, F32, dev)
    unet = UNet(CFGS[kind], sd, F32, dev, bank=bank)
    eps = call(unet, kind, dev)  # the input does not require grad
    assert eps.requires_grad
    assert rel_l2(eps, tok(eps_o)) < FP32_GRAD_LIMIT
    loss_of(eps, kind, dev).backward()
    ops.flush_weight_grads()
    got = bank_grads(bank)
    errs = {k: rel_l2(got[k], grads[k]) for k in sd}
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    print(f"{kind}: worst per-parameter rel-L2 {worst}")
    bad = {k: e for k, e in errs.items() if not e < FP32_GRAD_LIMIT}
    assert not bad, f"{len(bad)} of {len(sd)} parameters miss {FP32_GRAD_LIMIT}: {sorted(bad.items(), key=lambda kv: -kv[1])[:8]}"
    # a second call accumulates
    once = bank.flat_grad.clone()
    loss_of(call(unet, kind, dev), kind, dev).backward()
    ops.flush_weight_grads()
    assert rel_l2(bank.flat_grad, 2 * once) < 1e-5
    if dev.type == "cuda":
        torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["sd", "sdxl"])
def test_no_grad_call_saves_nothing(dev, kind):
    sd = world(kind)[0]
    bank = UNetBank(CFGS[kind], sd, F32, dev)
    unet = UNet(CFGS[kind], sd, F32, dev, bank=bank)
    with torch.no_grad():
        eps = call(unet, kind, dev)
    assert not eps.requires_grad and eps.grad_fn is None
    assert float(bank.flat_grad.abs().max()) == 0.0
    # a bank that is not trained (the discriminator's step): nothing requires grad either
    bank.set_requires_grad(False)
    eps = call(unet, kind, dev)
    assert not eps.requires_grad
    bank.set_requires_grad(True)
    assert call(unet, kind, dev).requires_grad


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_bank_forward_equals_frozen_forward(dev, dtype):
    """the no-grad forward through the bank's holders has the bits of the frozen UNet built from the same state dict"""
    sd = {k: v.to(dtype).float() for k, v in world("sdxl")[0].items()}
    frozen = UNet(CFGS["sdxl"], sd, dtype, dev)
    unet = UNet(CFGS["sdxl"], sd, dtype, dev, bank=UNetBank(CFGS["sdxl"], sd, dtype, dev))
    with torch.no_grad():
        assert torch.equal(call(unet, "sdxl", dev, dtype), call(frozen, "sdxl", dev, dtype))


@pytest.mark.parametrize("kind", ["sd", "sdxl"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_whole_bank_refresh(dev, kind, dtype):
    """after ensure_compute_copy() every holder of the UNet has w == master.to(dtype) and its second orientation, bit for bit; after
    an in-place update of the master and mark_updated() again"""
    sd = world(kind)[0]
    bank = UNetBank(CFGS[kind], sd, dtype, dev)
    UNet(CFGS[kind], sd, dtype, dev, bank=bank)
    assert len(bank.holders) > 50
    for rnd_ in range(2):
        bank.ensure_compute_copy()
        for h in bank.holders:
            m = torch.as_strided(bank.flat, h.w.shape, h.w.stride(), h.w.storage_offset())
            assert torch.equal(h.w, m.to(dtype))
            if isinstance(h, ops.TrainableConv):
                assert torch.equal(h.wd, h.w.flip(1, 2).permute(3, 1, 2, 0))
            else:
                assert torch.equal(h.wt, h.w.t())
        with torch.no_grad():
            bank.flat.mul_(1.25).add_(0.01)
        bank.mark_updated()


def test_state_dict_round_trip(sim):
    """keys, shapes and values of state_dict() equal the dict the bank was built from (what a stock UNet2DConditionModel loads): conv
    weights are OIHW again, GEGLU rows in their original order; the master itself holds the kernel layout"""
    cfg = CFGS["sdxl"]
    sd = world("sdxl")[0]
    bank = UNetBank(cfg, sd, F32, sim)
    out = bank.state_dict()
    assert list(out) == list(sd)
    for k in sd:
        assert out[k].shape == sd[k].shape and torch.equal(out[k], sd[k]), k
    ff = next(k for k in sd if k.endswith("ff.net.0.proj.weight"))
    assert not torch.equal(bank.params[ff].detach(), sd[ff]), "GEGLU rows are kept interleaved"
    assert torch.equal(bank.params[ff].detach(), sd[ff][ops.geglu_perm(sd[ff].shape[0])])
    cw = "down_blocks.0.resnets.0.conv1.weight"
    assert torch.equal(bank.params[cw].detach(), sd[cw].permute(0, 2, 3, 1))
    assert all(bank.layout[n][0] % 8 == 0 for n in bank.names)  # 32-byte boundaries
    assert all(p.grad.data_ptr() == bank._view(bank.flat_grad, n).data_ptr() for n, p in bank.params.items())
    # load: another state dict goes in through the same layout changes; a missing key and a wrong shape are refused
    other = {k: v * 1.5 for k, v in sd.items()}
    bank.load_state_dict(other)
    assert all(torch.equal(v, other[k]) for k, v in bank.state_dict().items())
    lacking = dict(other)
    del lacking[ff]
    with pytest.raises(KeyError):
        bank.load_state_dict(lacking)
    wrong = dict(other)
    wrong[cw] = other[cw][:, :, :1, :1]
    with pytest.raises(ValueError):
        bank.load_state_dict(wrong)
    assert all(torch.equal(v, other[k]) for k, v in bank.state_dict().items()), "a refused load changed the bank"


def test_constructor_refusals(sim):
    cfg = CFGS["sd"]
    sd = world("sd")[0]
    bank = UNetBank(cfg, sd, F32, sim)
    lora = LoRABank(cfg, weights.make_lora_weights(cfg), F32, sim)
    with pytest.raises(ValueError, match="lora"):
        UNet(cfg, sd, F32, sim, lora, bank=bank)
    with pytest.raises(ValueError, match="fp8"):
        UNet(cfg, sd, F32, sim, fp8_forward=True, bank=bank)
    with pytest.raises(ValueError, match="dtype"):
        UNet(cfg, sd, BF16, sim, bank=bank)


def test_update_invalidates_time_embedding_memo(dev):
    """nothing that depends on trained weights is memoised across an update: after an in-place change of the master the no-grad
    forward equals that of a frozen UNet built from the new state dict, bit for bit, and differs from the one before"""
    cfg = CFGS["sd"]
    sd = world("sd")[0]
    bank = UNetBank(cfg, sd, F32, dev)
    unet = UNet(cfg, sd, F32, dev, bank=bank)
    with torch.no_grad():
        before = call(unet, "sd", dev).clone()
        for n in ("time_embedding.linear_2.weight", "down_blocks.0.resnets.0.time_emb_proj.bias", "mid_block.resnets.0.conv1.weight"):
            bank.params[n].add_(0.05)
        bank.mark_updated()
        after = call(unet, "sd", dev)
        fresh = call(UNet(cfg, bank.state_dict(), F32, dev), "sd", dev)
    assert not torch.equal(after, before)
    assert torch.equal(after, fresh)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_graphed_forward_follows_an_update(hip, dtype):
    """a GraphedUNetForward replay at a timestep captured BEFORE an update of the bank equals the eager no-grad forward on the
    updated weights bit for bit, and differs from its own output before the update"""
    cfg = CFGS["sd"]
    sd = {k: v.to(dtype).float() for k, v in world("sd")[0].items()}
    _, x, ctx, _, _, _, _ = world("sd")
    bank = UNetBank(cfg, sd, dtype, hip)
    unet = UNet(cfg, sd, dtype, hip, bank=bank)
    graphed = GraphedUNetForward(unet)
    xd, cd = tok(x).to(hip, dtype), ctx.reshape(-1, ctx.shape[-1]).to(hip, dtype)
    with torch.no_grad():
        before = graphed(xd, B, HW, HW, T, cd, L).clone()
        assert torch.equal(before, unet(xd, B, HW, HW, T, cd, L)[0])
        bank.flat.mul_(1.02)
        bank.mark_updated()  # noticed by itself: no new_sampler_call()
        after = graphed(xd, B, HW, HW, T, cd, L).clone()
        eager = unet(xd, B, HW, HW, T, cd, L)[0]
    torch.cuda.synchronize()
    assert not torch.equal(after, before)
    assert torch.equal(after, eager)


# =================================================================================================================================
# The step: StepConfig.full_finetuning, CoMatTrainer(pipe, ubank, ...), unet.pt
# =================================================================================================================================
# World, oracle and bounds: see the module docstring.
import os  # noqa: E402

import test_tune_vae as TV  # noqa: E402
from comat_amd import checkpoint  # noqa: E402
from comat_amd.blip import Blip  # noqa: E402
from comat_amd.gan import D_sd  # noqa: E402
from comat_amd.pipeline import TrainableSDPipeline  # noqa: E402
from comat_amd.segments import SegmentedStep  # noqa: E402
from comat_amd.step import CoMatTrainer, GraphedStep, StepConfig  # noqa: E402
from comat_amd.unet import VAEBank, VAEDecoder  # noqa: E402
from helpers import check  # noqa: E402
from oracle import step as OS  # noqa: E402

TS, CROP = TV.TS, TV.CROP
ORACLE_GRAD_DISTANCE, ORACLE_UPDATE_DISTANCE = 6.671e-6, 5.810e-6
UPDATE_LIMIT = 10 * ORACLE_UPDATE_DISTANCE
BF16_UNET_GRAD_SIM = 9.662e-2
BF16_UNET_GRAD_LIMIT = 2 * BF16_UNET_GRAD_SIM


def make_step_world(dtype, dev, gan=True, tune_vae=False, full=True, **cfg_kw):
    """tests/test_tune_vae.make_world with the fully trained UNet: UNet(..., bank=ubank), CoMatTrainer(pipe, ubank, ...)"""
    cfg, batch, W, (tcfg, usd, vsd, lsd, bsd, dsd, dl, head_w, head_b) = TV.make_inputs(dtype, tune_vae, gan, full_finetuning=full,
                                                                                        **cfg_kw)
    if full:
        W["lora"] = {}
        W["unet"] = {k: v.clone().requires_grad_(True) for k, v in usd.items()}
        bank = UNetBank(tcfg, usd, dtype, dev)
        unet = UNet(tcfg, usd, dtype, dev, bank=bank)
    else:
        bank = LoRABank(tcfg, lsd, dtype, dev)
        unet = UNet(tcfg, usd, dtype, dev, bank)
    vbank = VAEBank(config.TINY_VAE, vsd, dtype, dev) if tune_vae else None
    vae = VAEDecoder(config.TINY_VAE, vsd, dtype, dev, bank=vbank) if tune_vae else VAEDecoder(config.TINY_VAE, vsd, dtype, dev)
    dbank = LoRABank(tcfg, dl, dtype, dev)
    disc = D_sd(UNet(tcfg, dsd, dtype, dev, dbank), dbank, head_w, head_b)
    trainer = CoMatTrainer(TrainableSDPipeline(unet, vae), bank, Blip(config.TINY_BLIP, bsd, dtype, dev), disc, cfg, seed=0)
    return cfg, batch, W, trainer


def bank_vec(bank, buf):
    """the parameters' elements of one of the bank's flat buffers (or of an optimizer moment), without the alignment pads"""
    return torch.cat([bank._view(buf, n).detach().reshape(-1).cpu() for n in bank.names])


def oracle_vec(bank, tensors):
    """diffusers tensors by name -> one vector in the bank's layout and order"""
    return torch.cat([bank._stored(n, tensors[n].detach()).reshape(-1) for n in bank.names])


_ORACLE = {}


def oracle_step(dtype, mkldnn=True):
    """the oracle's step on the world's inputs, once per dtype of the weights (and conv algorithm), shared and never written"""
    key = (dtype, mkldnn)
    if key not in _ORACLE:
        cfg, batch, W, _ = TV.make_inputs(dtype, False, True, full_finetuning=True)
        W["lora"] = {}
        leaves = W["unet"] = {k: v.clone().requires_grad_(True) for k, v in W["unet"].items()}
        params = list(leaves.values())
        before = {k: v.detach().clone() for k, v in leaves.items()}
        opt = torch.optim.AdamW(params, lr=cfg.lr, betas=(cfg.adam_beta1, cfg.adam_beta2), eps=cfg.adam_epsilon,
                                weight_decay=cfg.adam_weight_decay)
        with torch.backends.mkldnn.flags(enabled=mkldnn):
            out = OS.g_loss_terms(W, batch, cfg, TS, CROP)
            out["loss"].backward()
        assert all(p.grad is not None for p in params)
        res = dict(out={k: v.detach() for k, v in out.items() if k in ("Blip", "G_loss", "loss")},
                   g={k: v.grad.clone() for k, v in leaves.items()})
        res["gnorm"] = float(torch.nn.utils.clip_grad_norm_(params, cfg.max_grad_norm))
        res["clipped"] = {k: v.grad.clone() for k, v in leaves.items()}
        opt.step()
        res["update"] = {k: v.detach() - before[k] for k, v in leaves.items()}
        res["m"] = {k: opt.state[v]["exp_avg"].clone() for k, v in leaves.items()}
        res["v"] = {k: opt.state[v]["exp_avg_sq"].clone() for k, v in leaves.items()}
        _ORACLE[key] = res
    return _ORACLE[key]


def step_errors(trainer, batch, ref, cfg):
    """one step of `trainer` against the oracle's: logs and the distances the tests bound"""
    bank = trainer.bank
    p0 = bank_vec(bank, bank.flat)
    logs = trainer.train_step(batch, training_steps=TS, crop=CROP)
    keep = oracle_vec(bank, ref["clipped"]).abs() >= 10 * cfg.adam_epsilon
    upd = bank_vec(bank, bank.flat) - p0
    return logs, dict(grad=rel_l2(bank_vec(bank, bank.flat_grad), oracle_vec(bank, ref["g"])),
                      m=rel_l2(bank_vec(bank, trainer.opt.m[0]), oracle_vec(bank, ref["m"])),
                      v=rel_l2(bank_vec(bank, trainer.opt.v[0]), oracle_vec(bank, ref["v"])),
                      update=rel_l2(upd[keep], oracle_vec(bank, ref["update"])[keep]),
                      update_all=rel_l2(upd, oracle_vec(bank, ref["update"])),
                      excluded=1.0 - float(keep.float().mean()), n=int(keep.numel()))


def test_full_finetuning_step_matches_oracle(dev):
    """fp32 parity mode: losses, the UNet gradient, both moments and the restricted update"""
    cfg, batch, W, trainer = make_step_world(F32, dev)
    ref = oracle_step(F32)
    assert ref["gnorm"] > 2 * cfg.max_grad_norm, "the clip is meant to be active"
    logs, e = step_errors(trainer, batch, ref, cfg)
    print(f"full_finetuning fp32 {dev.type}: |g| {ref['gnorm']:.3e}, grad rel-L2 {e['grad']:.3e}, exp_avg {e['m']:.3e}, "
          f"exp_avg_sq {e['v']:.3e}, update {e['update']:.3e} over {100 * (1 - e['excluded']):.1f} % of {e['n']} elements "
          f"(unrestricted {e['update_all']:.3e})")
    check(logs["Blip"], ref["out"]["Blip"], F32, "Blip reward")
    check(logs["G_loss"], ref["out"]["G_loss"], F32, "G_loss")
    check(logs["step_loss"], ref["out"]["loss"], F32, "step loss")
    assert e["grad"] < 1e-3, f"UNet gradient rel-L2 {e['grad']:.3e}"
    assert e["m"] < 1e-3 and e["v"] < 2e-3, (e["m"], e["v"])
    assert e["excluded"] <= 0.05, f"{100 * e['excluded']:.1f} % of the elements excluded"
    assert e["update"] < UPDATE_LIMIT, f"update rel-L2 {e['update']:.3e} (limit {UPDATE_LIMIT:.3e})"


def test_full_finetuning_step_bf16(dev):
    """bf16 storage against the fp32 oracle on the same weights: UNet-gradient rel-L2 within 2 x the simulator's distance"""
    cfg, batch, W, trainer = make_step_world(BF16, dev)
    ref = oracle_step(BF16)
    trainer.train_step(batch, training_steps=TS, crop=CROP)
    e = rel_l2(bank_vec(trainer.bank, trainer.bank.flat_grad), oracle_vec(trainer.bank, ref["g"]))
    print(f"full_finetuning bf16 {dev.type}: UNet grad rel-L2 {e:.3e}")
    assert e < BF16_UNET_GRAD_LIMIT, f"UNet gradient rel-L2 {e:.3e}"


# ---- wiring, on the simulator ---------------------------------------------------------------------------------------------------
def test_flag_off_changes_nothing(sim):
    """a LoRA world built through the new signatures' defaults steps bit-equal to tests/test_step.make_world's, and frozen layers
    still save nothing"""
    import test_step
    _, batch0, _, old = test_step.make_world(F32, sim, False)
    la = old.train_step(batch0, training_steps=TS, crop=CROP)
    cfg1, batch1, _, new = make_step_world(F32, sim, full=False)
    assert not cfg1.full_finetuning and not new.full and new.pipe.unet.bank is None
    lb = new.train_step(batch1, training_steps=TS, crop=CROP)
    for k_ in ("Blip", "G_loss", "D_loss", "step_loss"):
        assert torch.equal(la[k_], lb[k_]), k_
    assert torch.equal(old.bank.flat_grad, new.bank.flat_grad) and torch.equal(old.bank.flat, new.bank.flat)
    u = new.pipe.unet
    x = torch.randn(2 * 8 * 8, u.conv_in.cin, requires_grad=True)
    assert ops.conv2d(x, u.conv_in, 2, 8, 8).grad_fn.saved_tensors == ()
    h = torch.randn(6, u.t2.in_features, requires_grad=True)
    assert ops.linear(h, u.t2).grad_fn.saved_tensors == ()


def test_flag_and_bank_must_agree(sim):
    cfg, batch, W, tr = make_step_world(F32, sim, gan=False)
    with pytest.raises(ValueError, match="full_finetuning"):
        CoMatTrainer(tr.pipe, tr.bank, tr.blip, tr.D, dataclasses.replace(cfg, full_finetuning=False))
    cfg2, _, _, lo = make_step_world(F32, sim, gan=False, full=False)
    with pytest.raises(ValueError, match="full_finetuning"):
        CoMatTrainer(lo.pipe, lo.bank, lo.blip, lo.D, dataclasses.replace(cfg2, full_finetuning=True))
    with pytest.raises(ValueError, match="UNetBank"):  # a bank the pipeline's UNet was not built from
        CoMatTrainer(lo.pipe, tr.bank, lo.blip, lo.D, cfg)


def test_tune_vae_and_full_finetuning_share_one_clip(sim):
    """both segments move, under ONE norm: the update equals torch.optim.AdamW on [UNet; VAE] after a joint clip_grad_norm_"""
    cfg, batch, W, tr = make_step_world(F32, sim, gan=False, tune_vae=True)
    ub, vb = tr.bank, tr.vae_bank
    p0 = torch.cat([ub.flat, vb.flat]).clone()
    tr.train_step(batch, training_steps=TS, crop=CROP)
    assert not torch.equal(ub.flat, p0[:ub.flat.numel()]) and not torch.equal(vb.flat, p0[ub.flat.numel():])
    p = p0.clone().requires_grad_(True)
    p.grad = torch.cat([ub.flat_grad, vb.flat_grad]).clone()
    opt = torch.optim.AdamW([p], lr=cfg.lr, betas=(cfg.adam_beta1, cfg.adam_beta2), eps=cfg.adam_epsilon,
                            weight_decay=cfg.adam_weight_decay)
    torch.nn.utils.clip_grad_norm_([p], cfg.max_grad_norm)
    opt.step()
    assert rel_l2(torch.cat([ub.flat, vb.flat]) - p0, p.detach() - p0) < 1e-4


def test_accumulation_over_two_micro_steps(sim):
    cfg, batch, W, tr = make_step_world(F32, sim, gan=False, gradient_accumulation_steps=2)
    ub = tr.bank
    p0 = ub.flat.clone()
    tr.train_step(batch, training_steps=TS, crop=CROP)
    g1 = ub.flat_grad.clone()
    assert torch.equal(ub.flat, p0) and float(g1.abs().max()) > 0  # no update yet
    tr.train_step(batch, training_steps=TS, crop=CROP)
    assert rel_l2(ub.flat_grad, 2 * g1) < 1e-5 and not torch.equal(ub.flat, p0)
    _, batch1, _, one = make_step_world(F32, sim, gan=False)
    one.train_step(batch1, training_steps=TS, crop=CROP)
    assert rel_l2(ub.flat_grad, one.bank.flat_grad) < 1e-5  # the window's sum is the mean gradient
    assert rel_l2(ub.flat - p0, one.bank.flat - p0) < 1e-4


def test_non_finite_gradient_skips_the_update(sim):
    cfg, batch, W, tr = make_step_world(F32, sim, gan=False)
    tr._forward_backward(batch, dict(training_steps=TS, crop=CROP))
    tr.bank.flat_grad[3] = float("inf")
    p = tr.bank.flat.clone()
    counters = tr.opt.counters.clone()
    tr._apply_updates()
    assert torch.equal(tr.bank.flat, p)
    assert int(tr.opt.counters[0]) == int(counters[0]) and int(tr.opt.counters[1]) == int(counters[1]) + 1


def test_gradient_checkpointing_same_bits(dev):
    """each trained call recomputed inside the backward pass: the bank's gradient has the bits of the plain step (whose calls project
    their own text keys / values, as checkpointed calls do) - every weight gradient is accumulated once, not twice"""
    _, batch, _, plain = make_step_world(F32, dev, gan=False)
    plain.pipe.share_text_kv = False
    _, batch2, _, ck = make_step_world(F32, dev, gan=False, gradient_checkpointing=True)
    la = plain.train_step(batch, training_steps=TS, crop=CROP)
    lb = ck.train_step(batch2, training_steps=TS, crop=CROP)
    assert torch.equal(la["step_loss"], lb["step_loss"])
    assert torch.equal(plain.bank.flat_grad, ck.bank.flat_grad)
    assert torch.equal(plain.bank.flat, ck.bank.flat)


def test_unet_checkpoint_round_trip_and_resume(sim, tmp_path):
    """unet.pt: keys and shapes of the dict the bank was built from, values = state_dict() (OIHW, original GEGLU rows), no LoRA
    file; a file lacking a key is refused; with optim_state.pt a resumed trainer continues bit for bit"""
    cfg, batch, W, tr = make_step_world(F32, sim, gan=False)
    tr.train_step(batch, training_steps=TS, crop=CROP)
    d = str(tmp_path)
    checkpoint.save_checkpoint(d, tr.bank, optim=dict(G=tr.opt))
    assert not os.path.exists(os.path.join(d, checkpoint.LORA_WEIGHT_NAME))
    sd = torch.load(os.path.join(d, "unet.pt"), map_location="cpu")
    src = {k: v.detach() for k, v in W["unet"].items()}  # the state dict the bank was built from
    assert list(sd) == list(src) and all(tuple(sd[k].shape) == tuple(src[k].shape) for k in sd)
    want = tr.bank.state_dict()
    assert all(torch.equal(sd[k], want[k]) for k in sd)
    assert all(not torch.equal(sd[k], src[k].float()) for k in sd), "every parameter was trained"
    ff = next(k for k in sd if k.endswith("ff.net.0.proj.weight"))
    assert torch.equal(sd[ff][ops.geglu_perm(sd[ff].shape[0])], tr.bank.params[ff].detach())
    cw = "conv_in.weight"
    assert torch.equal(sd[cw].permute(0, 2, 3, 1), tr.bank.params[cw].detach())
    # resume: a fresh world, loaded; its next step equals the original's next step
    _, batch2, _, fresh = make_step_world(F32, sim, gan=False)
    checkpoint.load_checkpoint(d, fresh.bank, optim=dict(G=fresh.opt))
    assert torch.equal(fresh.bank.flat, tr.bank.flat)
    tr.train_step(batch, training_steps=TS, crop=CROP)
    fresh.train_step(batch2, training_steps=TS, crop=CROP)
    assert torch.equal(fresh.bank.flat, tr.bank.flat) and torch.equal(fresh.opt.m[0], tr.opt.m[0])
    short = {k: v for k, v in sd.items() if k != ff}
    torch.save(short, os.path.join(d, "unet.pt"))
    with pytest.raises(KeyError, match="ff.net.0.proj"):
        checkpoint.load_checkpoint(d, fresh.bank)


# ---- data parallel ------------------------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, out_dir):
    """after tests/test_tune_vae.py: two ranks over gloo on the simulator, each with its own latents and prompt"""
    import sys

    import torch.distributed as dist
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    from comat_amd import dist as cdist
    from sim_backend import SimKernels
    ops.set_kernel_backend(SimKernels())
    r, w, dev = cdist.init(backend="gloo")
    cfg, batch, W, trainer = make_step_world(F32, dev, gan=False)
    g = torch.Generator().manual_seed(100 + rank)
    batch["latents"] = torch.randn(batch["latents"].shape, generator=g)
    batch["prompt_embeds"] = torch.randn(batch["prompt_embeds"].shape, generator=g)
    ub = trainer.bank
    ub.zero_grad()
    trainer.compute_losses(batch, training_steps=TS, crop=CROP)["loss"].backward()
    ops.flush_weight_grads()
    local = ub.flat_grad.clone()
    gathered = [torch.zeros_like(local) for _ in range(world)]
    dist.all_gather(gathered, local)
    p0 = ub.flat.clone()
    trainer.train_step(batch, training_steps=TS, crop=CROP)
    torch.save(dict(mean=torch.stack(gathered).mean(0), local=local, p0=p0, reduced=ub.flat_grad.clone() / world,
                    params=ub.flat.detach().clone()), os.path.join(out_dir, f"rank{rank}.pt"))
    cdist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_unet_parameters(tmp_path):
    """both ranks hold equal UNet parameters after a step, equal to the one-process update on the mean gradient"""
    import socket

    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    world = 2
    mp.spawn(_dp_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r = [torch.load(os.path.join(tmp_path, f"rank{i}.pt")) for i in range(world)]
    assert not torch.allclose(r[0]["local"], r[1]["local"])  # the ranks saw different data
    for i in range(world):
        assert torch.allclose(r[i]["reduced"], r[i]["mean"], rtol=1e-5, atol=1e-7)
    assert torch.equal(r[0]["params"], r[1]["params"]) and not torch.equal(r[0]["params"], r[0]["p0"])
    c = StepConfig()
    p = r[0]["p0"].clone().requires_grad_(True)
    p.grad = r[0]["mean"].clone()
    opt = torch.optim.AdamW([p], lr=1e-2, betas=(c.adam_beta1, c.adam_beta2), eps=c.adam_epsilon, weight_decay=c.adam_weight_decay)
    torch.nn.utils.clip_grad_norm_([p], c.max_grad_norm)
    opt.step()
    assert rel_l2(r[0]["params"] - r[0]["p0"], p.detach() - r[0]["p0"]) < 1e-4


# ---- graphs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_segmented_step_matches_eager(hip, dtype):
    """three calls of SegmentedStep = three eager steps under the flag, bit for bit, parameters included; the whole-step graph
    declines the flag"""
    cfg, batch, W, eager = make_step_world(dtype, hip)
    cfg2, batch2, W2, tr = make_step_world(dtype, hip)
    assert GraphedStep(tr).supported(batch2) is False
    eager.pipe.share_text_kv = False  # replayed segments project the text keys / values once per call (as tests/test_segments.py)
    stepper = SegmentedStep(tr)
    for i in range(3):
        la = eager.train_step(batch, training_steps=TS, crop=CROP)
        lb = stepper(batch2, training_steps=TS, crop=CROP)
        torch.cuda.synchronize()
        assert stepper.failed is None, stepper.failed
        for k_ in ("Blip", "G_loss", "D_loss", "step_loss"):
            assert torch.equal(la[k_], lb[k_]), (i, k_)
        assert torch.equal(eager.bank.flat_grad, tr.bank.flat_grad), i
        assert torch.equal(eager.bank.flat, tr.bank.flat), i


# ---- SDXL: the added embedding is read ahead of the first UNet call -------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_added_embedding_reads_fresh_copies(dev, dtype):
    """UNet.added_embedding called on its own - as TrainableSDPipeline.forward does, before any UNet call - right after construction,
    after an update of the master and after a load: the bits of a frozen UNet built from the same weights (the bank's compute copies
    start as zeros and are refreshed lazily)"""
    cfg = CFGS["sdxl"]
    sd = {k: v.to(dtype).float() for k, v in world("sdxl")[0].items()}
    pooled, tids = world("sdxl")[4]
    pooled, tids = pooled.to(dtype).float().to(dev), tids.tolist()
    bank = UNetBank(cfg, sd, dtype, dev)
    unet = UNet(cfg, sd, dtype, dev, bank=bank)
    with torch.no_grad():
        first = unet.added_embedding(pooled, tids)
        assert torch.equal(first, UNet(cfg, sd, dtype, dev).added_embedding(pooled, tids))
        bank.params["add_embedding.linear_1.weight"].mul_(1.5)
        bank.params["add_embedding.linear_2.weight"].add_(0.25)
        bank.mark_updated()
        second = unet.added_embedding(pooled, tids)
        now = {k: v.to(dtype).float() for k, v in bank.state_dict().items()}
        assert not torch.equal(second, first)
        assert torch.equal(second, UNet(cfg, now, dtype, dev).added_embedding(pooled, tids))
        bank.load_state_dict(sd)  # as checkpoint.load_checkpoint does
        assert torch.equal(unet.added_embedding(pooled, tids), first)
    a1, a2 = unet.a1, unet.a2
    assert torch.equal(a1.wt, a1.w.t()) and torch.equal(a2.wt, a2.w.t()) and float(a2.wt.float().abs().max()) > 0


def test_sdxl_sampler_every_parameter_gradient(dev):
    """the SDXL pipeline under the flag, fp32, in its FIRST call after construction: K = 2 of 3 denoise steps trained, the added
    embedding computed once by the pipeline ahead of the UNet calls.  Every parameter's gradient - add_embedding.* included - within
    the fp32 parity bound of oracle.sd.sample_with_grad with every UNet entry a leaf"""
    from comat_amd.pipeline import TrainableSDXLPipeline
    ucfg = CFGS["sdxl"]
    vcfg = dataclasses.replace(config.TINY_VAE, scaling_factor=0.13025)
    usd = world("sdxl")[0]
    vsd = weights.make_vae_weights(vcfg, perturb_norms=True)
    bs, h = 1, 8
    cd = ucfg.cross_attention_dim
    lat = rnd(bs, 4, h, h, seed=10)
    cu, cc = rnd(bs, L, cd, seed=11), rnd(bs, L, cd, seed=12)
    pu, pc = rnd(bs, ucfg.pooled_dim, seed=13), rnd(bs, ucfg.pooled_dim, seed=14)
    tids = (64, 64, 0, 0, 64, 64)
    noises = [rnd(bs, 4, h, h, seed=20 + i) for i in range(3)]
    leaves = {k: v.clone().requires_grad_(True) for k, v in usd.items()}
    img_o, lat_o, _ = O.sample_with_grad(leaves, O.UNetConfig(**dataclasses.asdict(ucfg)), vsd, O.VAEConfig(**dataclasses.asdict(vcfg)),
                                         None, cu, cc, lat, noises, 3, [1, 2], 7.5,
                                         sdxl_cond=(pu, pc, torch.tensor([tids], dtype=torch.float32)))
    gi = rnd(*img_o.shape, seed=30)
    (img_o * gi).sum().backward()
    assert all(v.grad is not None and float(v.grad.norm()) > 0 for v in leaves.values())
    bank = UNetBank(ucfg, usd, F32, dev)
    pipe = TrainableSDXLPipeline(UNet(ucfg, usd, F32, dev, bank=bank), VAEDecoder(vcfg, vsd, F32, dev))
    img, latf = pipe.forward(cc, cu, height=8 * h, width=8 * h, training_timesteps=[1, 2], num_inference_steps=3, guidance_scale=7.5,
                             latents=lat, noises=noises, return_latents=True, pooled_prompt_embeds=pc,
                             negative_pooled_prompt_embeds=pu, add_time_ids=tids)
    (img.float() * gi.to(dev)).sum().backward()
    ops.flush_weight_grads()
    check(latf, lat_o, F32, "final latents", factor=3)
    got = bank_grads(bank)
    errs = {k: rel_l2(got[k], v.grad) for k, v in leaves.items()}
    print(f"sdxl sampler: worst per-parameter rel-L2 {sorted(errs.items(), key=lambda kv: -kv[1])[:4]}; add_embedding "
          f"{ {k: f'{e:.2e}' for k, e in errs.items() if k.startswith('add_embedding')} }")
    bad = {k: e for k, e in errs.items() if not e < FP32_GRAD_LIMIT}
    assert not bad, f"{len(bad)} of {len(errs)} parameters miss {FP32_GRAD_LIMIT}: {sorted(bad.items(), key=lambda kv: -kv[1])[:8]}"


def test_a_layer_is_built_once_per_name(sim):
    """a second UNet on the same bank shares the first one's holders: no duplicate holder, no weight refreshed twice"""
    cfg = CFGS["sd"]
    sd = world("sd")[0]
    bank = UNetBank(cfg, sd, F32, sim)
    one = UNet(cfg, sd, F32, sim, bank=bank)
    n_h, n_p, n_a = len(bank.holders), len(bank._problems), len(bank._affine)
    two = UNet(cfg, sd, F32, sim, bank=bank)
    assert (len(bank.holders), len(bank._problems), len(bank._affine)) == (n_h, n_p, n_a)
    assert two.conv_in is one.conv_in and two.t1 is one.t1 and two.norm_out[0] is one.norm_out[0]
    bank.ensure_compute_copy()
    from comat_amd import refresh
    n = bank.flat.numel()
    cw, ct = refresh.covered(bank._plan.problems, bank._plan.tiles, n, bank.flat_t.numel())
    assert cw.max() == 1 and ct.max() == 1
    assert int(ct.sum()) == sum(h.w.numel() for h in bank.holders) == int(cw.sum())
    with pytest.raises(ValueError, match="conv_in"):
        bank.conv("conv_in", stride=2)
    assert not hasattr(bank, "sd")  # the source state dict is not kept alive
