"""The discriminator's other two shapes: the conv classifier head (`--gan_unet_lastlayer_cls`: comat_disc_convhead_* ->
ops.disc_convhead_loss -> gan.D_sd(lastlayer_cls=True)) and the SDXL discriminator (gan.D_sdxl).

Kernel level: against F.conv2d + F.binary_cross_entropy_with_logits at shapes that are all border, ragged, more than one
block, and the real channel count; the frozen head; accumulation into dwb; NaN-haloed windows; run-to-run and graph-replay
bits; the contract's refusals.  Assembly: against the reference's own `D_sd.D_sd_pipeline_forward` /
`D_sdxl.D_sd_pipeline_forward` run on stand-ins (tests/golden/make_gan_heads_golden.py -> gan_heads.npz).  Model level: real
tiny UNets against the oracle UNet whose conv_out IS the head (the substitution the reference makes).  Step level: the
trainer's eager step against SegmentedStep and GraphedStep bit for bit, the head's AdamW update, the checkpoint form."""
import dataclasses
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from comat_amd import checkpoint, config, ops
from comat_amd.gan import D_sd, D_sdxl, load_discriminator
from comat_amd.step import CoMatTrainer, GraphedStep
from comat_amd.unet import LoRABank, UNet
from helpers import Window, check, oracle_cfgs, rel_l2, tiny_weights, tok, untok
from oracle import sd as O
from test_step import BF16_D_GRAD_LIMIT, BF16_GRAD_LIMIT, BF16_GRAD_LIMIT_SDXL, make_world

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_gan_heads_golden as MG  # noqa: E402 - the stand-ins' own functions (feature_fn, added_term), nothing of the reference

GOLD = os.path.join(HERE, "golden", "gan_heads.npz")
DTYPES = [torch.float32, torch.bfloat16]
F32 = torch.float32
# (B, H, W, C): non-square with dominating borders; every pixel a border pixel in x; the real channel count; 646 pixels =
# more than one block of the backward pass (11 chunks of 59) and a ragged last one
SHAPES = [(2, 5, 6, 32), (2, 3, 1, 64), (1, 8, 8, 320), (2, 17, 19, 32)]
G_UP = 1.7


def dv(x, dev, dtype=None, grad=False):
    t = x.detach().to(device=dev, dtype=dtype or x.dtype).contiguous()
    return t.clone().requires_grad_(True) if grad else t


@functools.lru_cache(maxsize=None)
def problem(B, H, W, C, dtype):
    """inputs (values representable in `dtype`, held in fp32) and the torch reference of one shape: computed once, shared"""
    g = torch.Generator().manual_seed(B * 1000 + H * 100 + W * 10 + C)
    x = torch.randn(B * H * W, C, generator=g).to(dtype).float()
    w4 = torch.randn(1, C, 3, 3, generator=g) * (2.0 / (9 * C) ** 0.5)
    b = torch.randn(1, generator=g) * 0.3
    target = torch.tensor([0.0, 1.0])[:B].clone()
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w4, b))
    z = F.conv2d(untok(xr, B, H, W), wr, br, padding=1)
    loss = F.binary_cross_entropy_with_logits(z, target.reshape(B, 1, 1, 1).expand(B, 1, H, W))
    (G_UP * loss).backward()
    return types.SimpleNamespace(x=x, w4=w4, b=b, target=target, loss=loss.detach(), z=z.detach().reshape(-1), dx=xr.grad,
                                 dw4=wr.grad, db=br.grad)


def run_op(p, dev, dtype, B, H, W, frozen=False):
    xd = dv(p.x, dev, dtype, grad=True)
    wd, bd = dv(ops.conv_weight_to_taps(p.w4), dev, grad=not frozen), dv(p.b, dev, grad=not frozen)
    loss = ops.disc_convhead_loss(xd, wd, bd, dv(p.target, dev), B, H, W)
    z = loss.grad_fn.saved_tensors[2]
    (G_UP * loss).backward()
    return loss.detach(), z, xd.grad, wd.grad, bd.grad


def check_against_reference(p, got, dtype, what):
    loss, z, dx, dw, db = got
    check(loss, p.loss, F32, f"{what} loss", factor=5)
    check(z, p.z, F32, f"{what} z", factor=5)
    check(dx, p.dx, dtype, f"{what} dx")
    if dw is not None:
        check(ops.taps_to_conv_weight(dw), p.dw4, F32, f"{what} dw", factor=20)
        check(db, p.db, F32, f"{what} db", factor=20)


# ---- 1. kernel against F.conv2d + BCE ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_convhead_matches_conv2d_bce(dev, dtype, shape):
    B, H, W, C = shape
    p = problem(B, H, W, C, dtype)
    check_against_reference(p, run_op(p, dev, dtype, B, H, W), dtype, f"convhead {shape}")


def test_weight_layout_round_trip():
    w4 = torch.randn(1, 16, 3, 3)
    w9 = ops.conv_weight_to_taps(w4)
    assert tuple(w9.shape) == (9, 16) and torch.equal(w9[5], w4[0, :, 1, 2]) and torch.equal(ops.taps_to_conv_weight(w9), w4)


# ---- 2. frozen head ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_frozen_head_produces_dx_only(dev, dtype):
    B, H, W, C = SHAPES[3]
    p = problem(B, H, W, C, dtype)
    seen = []
    k = ops.kernels()
    real = k.disc_convhead_bwd
    k.disc_convhead_bwd = lambda x, w, z, t, g, dx, dwb, *a: (seen.append((dx is not None, dwb is not None)), real(x, w, z, t, g, dx, dwb, *a))[1]
    try:
        trained = run_op(p, dev, dtype, B, H, W)
        frozen = run_op(p, dev, dtype, B, H, W, frozen=True)
    finally:
        k.disc_convhead_bwd = real
    assert seen == [(True, True), (True, False)]
    assert frozen[3] is None and frozen[4] is None
    assert torch.equal(frozen[2], trained[2]), "dx must not depend on whether the weight gradient is asked for"
    check_against_reference(p, frozen, dtype, "frozen head")


# ---- 3. accumulation --------------------------------------------------------------------------------------------------------
def kernel_call(k, p, dev, dtype, B, H, W, C, dwb, want_dx=True):
    x, w, b, t = dv(p.x, dev, dtype), dv(ops.conv_weight_to_taps(p.w4), dev), dv(p.b, dev), dv(p.target, dev)
    z, loss = torch.empty(B * H * W, device=dev), torch.empty(1, device=dev)
    k.disc_convhead_fwd(x, w, b, t, z, loss, B, H, W, C)
    dx = torch.empty_like(x) if want_dx else None
    k.disc_convhead_bwd(x, w, z, t, dv(torch.tensor([G_UP]), dev), dx, dwb, B, H, W, C)
    return loss, z, dx


@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_accumulates_into_dwb_and_never_zeroes_it(dev, dtype):
    B, H, W, C = SHAPES[3]
    p = problem(B, H, W, C, dtype)
    k = ops.kernels()
    once = torch.zeros(9 * C + 1, device=dev)
    kernel_call(k, p, dev, dtype, B, H, W, C, once)
    twice = torch.zeros(9 * C + 1, device=dev)
    kernel_call(k, p, dev, dtype, B, H, W, C, twice)
    kernel_call(k, p, dev, dtype, B, H, W, C, twice, want_dx=False)  # dx may be NULL
    assert torch.equal(twice, once + once)
    pre = torch.full((9 * C + 1,), 3.0, device=dev)
    kernel_call(k, p, dev, dtype, B, H, W, C, pre)
    assert torch.equal(pre, once + 3.0)
    check(ops.taps_to_conv_weight(once[:9 * C].reshape(9, C)), p.dw4, F32, "dw", factor=20)
    check(once[9 * C:], p.db, F32, "db", factor=20)


# ---- 4. windows -------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_windowed_operands_and_guarded_outputs(dev, dtype, shape):
    """every operand a window inside a NaN-filled buffer, every output inside a guard band: finite results, the bits of the
    unwindowed call, guards and halos untouched"""
    B, H, W, C = shape
    P = B * H * W
    p = problem(B, H, W, C, dtype)
    k = ops.kernels()
    plain_dwb = torch.zeros(9 * C + 1, device=dev)
    loss0, z0, dx0 = kernel_call(k, p, dev, dtype, B, H, W, C, plain_dwb)
    flat = lambda v, dt=F32: Window(1, v.numel(), v.numel(), dt, dev).put(v.reshape(1, -1)).arm()
    xw = Window(P, C, C, dtype, dev).put(p.x).arm()
    ww, bw, tw, gw = flat(ops.conv_weight_to_taps(p.w4)), flat(p.b), flat(p.target), flat(torch.tensor([G_UP]))
    zw, lw = Window(1, P, P, F32, dev).arm(), Window(1, 1, 1, F32, dev).arm()
    dxw = Window(P, C, C, dtype, dev).arm()
    dwbw = flat(torch.zeros(9 * C + 1))
    k.disc_convhead_fwd(xw.view, ww.flat.view(9, C), bw.flat, tw.flat, zw.flat, lw.flat, B, H, W, C)
    k.disc_convhead_bwd(xw.view, ww.flat.view(9, C), zw.flat, tw.flat, gw.flat, dxw.view, dwbw.flat, B, H, W, C)
    for name, win in (("x", xw), ("w", ww), ("b", bw), ("target", tw), ("g_up", gw), ("z", zw), ("loss", lw), ("dx", dxw),
                      ("dwb", dwbw)):
        win.assert_guard_intact(f"convhead {name}")
    for name, win in (("z", zw), ("loss", lw), ("dx", dxw), ("dwb", dwbw)):
        win.assert_written(f"convhead {name}")
    assert torch.equal(_bits(xw.get()), _bits(dv(p.x, dev, dtype))), "the input window was written to"
    assert torch.equal(lw.get().reshape(-1), loss0) and torch.equal(zw.get().reshape(-1), z0)
    assert torch.equal(_bits(dxw.get()), _bits(dx0)) and torch.equal(dwbw.get().reshape(-1), plain_dwb)


# ---- 5. reproducibility -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_same_bits_on_every_run_and_in_a_graph_replay(hip, dtype, shape):
    B, H, W, C = shape
    p = problem(B, H, W, C, dtype)
    first = run_op(p, hip, dtype, B, H, W)
    second = run_op(p, hip, dtype, B, H, W)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    xs, ws, bs_ = dv(p.x, hip, dtype, grad=True), dv(ops.conv_weight_to_taps(p.w4), hip, grad=True), dv(p.b, hip, grad=True)
    tg = dv(p.target, hip)
    cap = ops.capture_stream(hip)  # its workspaces exist before the capture begins
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with ops.graph_capture(graph, stream=cap):
        loss = ops.disc_convhead_loss(xs, ws, bs_, tg, B, H, W)
        dx, dw, db = torch.autograd.grad(G_UP * loss, (xs, ws, bs_))
    loss = loss.detach()
    for _ in range(2):
        loss.zero_(), dx.zero_(), dw.zero_(), db.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip((first[0], first[2], first[3], first[4]), (loss, dx, dw, db)):
            assert torch.equal(a, b)


# ---- 6. contract ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_contract_refusals_then_a_valid_call(dev, dtype):
    B, H, W, C = SHAPES[0]
    p = problem(B, H, W, C, dtype)
    k = ops.kernels()
    x, t = dv(p.x, dev, dtype), dv(p.target, dev)
    w, b = dv(ops.conv_weight_to_taps(p.w4), dev), dv(p.b, dev)
    z, loss, g = torch.zeros(B * H * W, device=dev), torch.zeros(1, device=dev), dv(torch.tensor([G_UP]), dev)
    dwb = torch.zeros(9 * C + 1, device=dev)
    x12 = torch.zeros(B * H * W, 12, dtype=dtype, device=dev)
    with pytest.raises(RuntimeError, match="comat_disc_convhead_fwd.*multiple of 8"):
        k.disc_convhead_fwd(x12, w, b, t, z, loss, B, H, W, 12)
    with pytest.raises(RuntimeError, match="comat_disc_convhead_bwd.*multiple of 8"):
        k.disc_convhead_bwd(x12, w, z, t, g, torch.empty_like(x12), dwb, B, H, W, 12)
    with pytest.raises(RuntimeError, match="comat_disc_convhead_fwd.*positive"):
        k.disc_convhead_fwd(x, w, b, t, z, loss, 0, H, W, C)
    with pytest.raises(RuntimeError, match="comat_disc_convhead_bwd.*positive"):
        k.disc_convhead_bwd(x, w, z, t, g, torch.empty_like(x), dwb, B, 0, W, C)
    with pytest.raises(RuntimeError, match="comat_disc_convhead_bwd.*neither dx nor dwb"):
        k.disc_convhead_bwd(x, w, z, t, g, None, None, B, H, W, C)
    assert not dwb.any() and not z.any() and not loss.any(), "a refused call launched something"
    check_against_reference(p, run_op(p, dev, dtype, B, H, W), dtype, "after the refusals")


def test_library_exports_and_validates_the_conv_head():
    """no GPU needed: argument errors come back as COMAT_EINVAL + a message, nothing is launched"""
    import ctypes as C

    from comat_amd import _hip
    lib = _hip.load_library()
    for name in ("comat_disc_convhead_fwd", "comat_disc_convhead_bwd", "comat_disc_convhead_workspace_bytes"):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    buf = (C.c_float * 64)()
    q = C.cast(buf, C.c_void_p)
    assert lib.comat_disc_convhead_fwd(q, q, q, q, q, q, q, 2, 5, 6, 12, 0, None) == -1
    assert b"multiple of 8" in lib.comat_last_error()
    assert lib.comat_disc_convhead_fwd(q, q, q, q, q, q, q, 2, 0, 6, 32, 0, None) == -1
    assert b"positive" in lib.comat_last_error()
    assert lib.comat_disc_convhead_bwd(q, q, q, q, q, None, None, q, 2, 5, 6, 32, 0, None) == -1
    assert b"neither dx nor dwb" in lib.comat_last_error()
    assert lib.comat_disc_convhead_bwd(q, q, q, q, q, q, None, None, 2, 5, 6, 32, 0, None) == -1  # no workspace
    # the workspace holds the 9 tap products of every pixel, the loss partials and the weight-gradient slabs
    assert lib.comat_disc_convhead_workspace_bytes(2, 64, 64, 320) >= 4 * (9 * 8192 + 2 * (9 * 320 + 1))
    assert lib.comat_abi_version() == 8


# ---- 7 / 8. the assembly against the reference's own forward methods ----------------------------------------------------------
class StandInBank:
    def __init__(self, unet):
        self.unet = unet

    def set_requires_grad(self, flag):
        self.unet.mix.requires_grad_(flag)

    def zero_grad(self):
        self.unet.mix.grad = None


class StandInUNet:
    """the device-side twin of the golden script's stand-in UNets, behind this package's UNet interface"""

    def __init__(self, dev, mix, tw=None, pw=None):
        self.dtype, self.device = torch.float32, dev
        self.mix = mix.to(dev).requires_grad_(True)
        self.tw, self.pw = (None if tw is None else tw.to(dev)), (None if pw is None else pw.to(dev))
        self.calls, self.added_calls = [], []

    def _note(self, x, B, t, ctx, L):
        self.calls.append((int(t), B, ctx.shape[0] // L))

    def features(self, x, B, h, w, t, ctx, L, added=None, kv_cache=None):
        self._note(x, B, t, ctx, L)
        return tok(MG.feature_fn(self.mix, untok(x, B, h, w), t, ctx.reshape(B, L, -1)))

    def added_embedding(self, text_embeds, time_ids):
        tid = torch.tensor(time_ids, dtype=torch.float32, device=self.device)
        self.added_calls.append((tid.cpu(), text_embeds.detach().float().cpu()))
        return torch.cat([tid, text_embeds.to(self.device).float()], 1)

    def __call__(self, x, B, h, w, t, ctx, L, added=None):
        self._note(x, B, t, ctx, L)
        e = MG.G.stub_unet_fn(self.mix, untok(x, B, h, w), t, ctx.reshape(B, L, -1))
        if added is not None:
            e = e + MG.added_term(added[:, :6], added[:, 6:], self.tw, self.pw)
        return tok(e), {}


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / ref.abs().max())


def drive_against_gold(dev, case, make_disc):
    gold = np.load(GOLD)
    T = lambda k: torch.from_numpy(gold[f"{case}:{k}"])
    n = int(gold[f"{case}:n_steps"])
    bs, _, h, w = gold[f"{case}:fake"].shape
    disc, unet = make_disc(T)
    kw = dict(negative_prompt_embeds=T("null").to(dev), num_inference_steps=n, h=h, w=w)
    if f"{case}:pooled" in gold:
        kw["negative_pooled_prompt_embeds"] = T("pooled").to(dev)
    fake = tok(T("fake")).to(dev).requires_grad_(True)
    g_loss = disc.D_sd_pipeline_forward(fake, "G", **kw)
    g_loss.backward()
    assert rel(g_loss, T("g_loss")) < 1e-5
    assert rel(fake.grad, tok(T("g_dfake"))) < 1e-5
    # the generator side leaves the discriminator untouched (gan_sdxl.py:55-56)
    assert unet.mix.grad is None and not disc.head_grad.any() and not list(gold[f"{case}:g_side_touched_D"]).count(True)
    disc.zero_grad()
    d_loss = disc.D_sd_pipeline_forward(fake.detach(), "D", real_latents=tok(T("real")).to(dev), **kw)
    d_loss.backward()
    assert rel(d_loss, T("d_loss")) < 1e-5
    assert rel(unet.mix.grad, T("d_dmix")) < 1e-5
    nw = disc.head.numel() - 1
    dw = disc.head_grad[:nw]
    dw = ops.taps_to_conv_weight(dw.reshape(9, -1)) if disc.lastlayer_cls else dw.reshape(1, 4)
    assert rel(dw, T("d_dhead_w")) < 1e-5 and rel(disc.head_grad[nw:], T("d_dhead_b")) < 1e-5
    # what the reference asked of its UNet: timestep, batch sizes (G: bs, D: 2 bs with the condition twice); who trains when
    assert [c[0] for c in unet.calls] == list(gold[f"{case}:t_used"])
    assert [c[1] for c in unet.calls] == list(gold[f"{case}:unet_batch"])
    assert [c[2] for c in unet.calls] == list(gold[f"{case}:cond_batch"])
    assert list(gold[f"{case}:lora_flags"]) == [False, True] and disc.w.requires_grad and unet.mix.requires_grad
    return gold, unet


def test_conv_head_discriminator_matches_the_reference_forward(dev):
    def make(T):
        unet = StandInUNet(dev, T("mix"))
        return D_sd(unet, StandInBank(unet), T("head_w"), T("head_b"), lastlayer_cls=True), unet
    drive_against_gold(dev, "lastlayer", make)


def test_sdxl_discriminator_matches_the_reference_forward(dev):
    def make(T):
        unet = StandInUNet(dev, T("mix"), T("tw"), T("pw"))
        disc = load_discriminator("gansdxl", unet, StandInBank(unet), T("head_w"), T("head_b"), resolution=int(res))
        assert type(disc) is D_sdxl
        return disc, unet
    res = np.load(GOLD)["sdxl:resolution"]
    gold, unet = drive_against_gold(dev, "sdxl", make)
    (g_tid, g_te), (d_tid, d_te) = unet.added_calls
    assert torch.equal(g_tid, torch.from_numpy(gold["sdxl:g_time_ids"])) and torch.equal(d_tid, torch.from_numpy(gold["sdxl:d_time_ids"]))
    assert torch.equal(g_te, torch.from_numpy(gold["sdxl:g_text_embeds"])) and torch.equal(d_te, torch.from_numpy(gold["sdxl:d_text_embeds"]))


def test_load_discriminator_mirrors_the_reference_factory(sim):
    unet = StandInUNet(sim, torch.zeros(4, 4))
    mk = lambda arch: load_discriminator(arch, unet, StandInBank(unet), torch.zeros(1, 4), torch.zeros(1))
    assert type(mk("gansd_1_5")) is D_sd and type(mk("sd_1_5")) is D_sd and type(mk("gansdxl")) is D_sdxl
    with pytest.raises(ValueError):
        mk("sd_2_1")


# ---- 9. real tiny UNets against the oracle UNet whose conv_out is the head ------------------------------------------------------
# Bounds: the project's bar for a tiny step (tests/test_step.py): rel-L2 1e-3 in fp32 storage; in bf16 storage the tiny step's
# limit of the UNet layout at hand - BF16_GRAD_LIMIT (SD1.5 layout), BF16_GRAD_LIMIT_SDXL (SDXL layout: twice the transformer
# layers of a random-weight toy network) - for the LoRA gradients, the head gradients and d G_loss / d fake alike.  The
# SD1.5-layout LoRA gradients are the very comparison tests/test_step.py holds to its tighter BF16_D_GRAD_LIMIT (one UNet call):
# they keep that one.  fp32 storage measures ~1e-5 or less everywhere: the bf16 figures are storage rounding, not arithmetic.


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["sd15-conv", "sdxl-conv", "sdxl-linear"])
def test_real_tiny_discriminators_match_the_oracle(dev, dtype, kind):
    sdxl, conv = kind.startswith("sdxl"), kind.endswith("conv")
    ucfg = config.TINY_SDXL_UNET if sdxl else config.TINY_UNET
    usd, _, lsd = tiny_weights(dtype, ucfg)
    ocfg, _ = oracle_cfgs(ucfg)
    C0 = ucfg.block_out_channels[0]
    bs, h, w, L, N, res = 2, 8, 8, 7, 3, 64
    g = torch.Generator().manual_seed(17)
    r = lambda *s: torch.randn(*s, generator=g)
    head_w = (r(1, C0, 3, 3) * (9 * C0) ** -0.5) if conv else r(1, 4) * 0.5
    head_b = r(1) * 0.1
    fake, real = r(bs, 4, h, w).to(dtype).float(), r(bs, 4, h, w).to(dtype).float()
    null = r(bs, L, ucfg.cross_attention_dim).to(dtype).float()
    pooled = r(bs, ucfg.pooled_dim).to(dtype).float() if sdxl else None
    t_last = O.DDPM().set_timesteps(N)[-1]
    # oracle: the reference's substitution - conv_out IS the classifier (gan_sdxl.py:28-30) - then BCE here
    lo = {k: v.clone().requires_grad_(True) for k, v in lsd.items()}
    hw, hb = head_w.clone().requires_grad_(True), head_b.clone().requires_grad_(True)
    osd = dict(usd, **{"conv_out.weight": hw, "conv_out.bias": hb}) if conv else usd

    def oracle_loss(lat, target):
        B = lat.shape[0]
        added = (torch.cat([pooled] * (B // bs)), torch.tensor([[res, res, 0, 0, res, res]] * B, dtype=torch.float32)) if sdxl else None
        out = O.unet_forward(osd, ocfg, lat, t_last, torch.cat([null] * (B // bs)), lo, None, added)
        pred = out.permute(0, 2, 3, 1)
        if not conv:
            pred = F.linear(pred, hw, hb)
        return F.binary_cross_entropy_with_logits(pred, target.reshape(B, 1, 1, 1).expand_as(pred))
    fo = fake.clone().requires_grad_(True)
    g_ref = oracle_loss(fo, torch.ones(bs))
    (g_dfake_ref,) = torch.autograd.grad(g_ref, fo)
    d_ref = oracle_loss(torch.cat([fake, real]), torch.cat([torch.zeros(bs), torch.ones(bs)]))
    d_ref.backward()
    # product
    bank = LoRABank(ucfg, lsd, dtype, dev)
    unet = UNet(ucfg, usd, dtype, dev, bank)
    disc = load_discriminator("gansdxl" if sdxl else "gansd_1_5", unet, bank, head_w, head_b, lastlayer_cls=conv, resolution=res)
    kw = dict(negative_prompt_embeds=null.to(dev), num_inference_steps=N, h=h, w=w)
    if sdxl:
        kw["negative_pooled_prompt_embeds"] = pooled.to(dev)
    ft = tok(fake).to(dev).requires_grad_(True)
    disc.zero_grad()
    g_loss = disc.D_sd_pipeline_forward(ft, "G", **kw)
    g_loss.backward()
    assert not bank.flat_grad.any() and not disc.head_grad.any()
    d_loss = disc.D_sd_pipeline_forward(ft.detach(), "D", real_latents=tok(real).to(dev), **kw)
    d_loss.backward()
    ops.join_side_streams()
    f = 1.0 if dtype == torch.float32 else 4.0
    check(g_loss, g_ref, dtype, "G loss", factor=f)
    check(d_loss, d_ref, dtype, "D loss", factor=f)
    lora_ref = torch.cat([lo[n].grad.reshape(-1) for n in bank.names])
    hw_ref = ops.conv_weight_to_taps(hw.grad) if conv else hw.grad
    head_ref = torch.cat([hw_ref.reshape(-1), hb.grad.reshape(-1)])
    e_f, e_l, e_h = rel_l2(ft.grad, tok(g_dfake_ref)), rel_l2(bank.flat_grad, lora_ref), rel_l2(disc.head_grad, head_ref)
    print(f"{kind} {dtype} {dev.type}: d/d fake {e_f:.3e}  LoRA {e_l:.3e}  head {e_h:.3e}")
    lim = 1e-3 if dtype == torch.float32 else (BF16_GRAD_LIMIT_SDXL if sdxl else BF16_GRAD_LIMIT)
    lim_l = lim if dtype == torch.float32 or sdxl else BF16_D_GRAD_LIMIT
    assert e_l < lim_l, f"discriminator LoRA gradients rel-L2 {e_l:.3e}"
    assert e_h < lim, f"head gradients rel-L2 {e_h:.3e}"
    assert e_f < lim, f"d G_loss / d fake rel-L2 {e_f:.3e}"


def test_features_share_the_forward_and_leave_default_calls_alone(sim):
    """UNet.features = the forward without conv_out: conv_out applied to it gives the default call's output bit for bit, and
    a default call launches exactly the features call's kernels plus that one convolution"""
    dtype = torch.float32
    usd, _, lsd = tiny_weights(dtype)
    unet = UNet(config.TINY_UNET, usd, dtype, sim, LoRABank(config.TINY_UNET, lsd, dtype, sim))
    B, h, w, L = 1, 8, 8, 7
    g = torch.Generator().manual_seed(3)
    x, ctx = torch.randn(B * h * w, 4, generator=g), torch.randn(B * L, config.TINY_UNET.cross_attention_dim, generator=g)
    k = ops.kernels()
    counts = []
    for fn in (lambda: unet(x, B, h, w, 5, ctx, L)[0], lambda: unet.features(x, B, h, w, 5, ctx, L)):
        n = [0]
        real = k.conv2d
        k.conv2d = lambda *a, **kw: (n.__setitem__(0, n[0] + 1), real(*a, **kw))[1]
        try:
            with torch.no_grad():
                out = fn()
        finally:
            del k.conv2d
        counts.append((n[0], out))
    (n_full, eps), (n_feat, feat) = counts
    assert n_full == n_feat + 1 and tuple(feat.shape) == (B * h * w, config.TINY_UNET.block_out_channels[0])
    with torch.no_grad():
        assert torch.equal(ops.conv2d(feat, unet.conv_out, B, h, w), eps)


# ---- 10. the step ---------------------------------------------------------------------------------------------------------------
def conv_world(dtype, dev, sdxl_disc=False):
    """the tiny world of tests/test_step.py::make_world with the discriminator rebuilt: conv head (SD1.5 layout), or an SDXL
    discriminator with the conv head"""
    cfg, batch, W, tr0 = make_world(dtype, dev, False)
    cfg = dataclasses.replace(cfg, gan_unet_lastlayer_cls=True)
    g = torch.Generator().manual_seed(23)
    ucfg = config.TINY_SDXL_UNET if sdxl_disc else config.TINY_UNET
    C0 = ucfg.block_out_channels[0]
    head_w, head_b = torch.randn(1, C0, 3, 3, generator=g) * (9 * C0) ** -0.5, torch.randn(1, generator=g) * 0.1
    if sdxl_disc:
        dsd, _, dl = tiny_weights(dtype, ucfg)
        batch = dict(batch, gan_pooled_null_embeds=torch.randn(batch["latents"].shape[0], ucfg.pooled_dim, generator=g).to(dtype).float())
    else:
        dsd, dl = W["d_unet"], {k: v.detach().clone() for k, v in W["d_lora"].items()}
    dbank = LoRABank(ucfg, dl, dtype, dev)
    disc = load_discriminator("gansdxl" if sdxl_disc else "gansd_1_5", UNet(ucfg, dsd, dtype, dev, dbank), dbank, head_w, head_b,
                              lastlayer_cls=True, resolution=cfg.resolution)
    return cfg, batch, CoMatTrainer(tr0.pipe, tr0.bank, tr0.blip, disc, cfg, seed=0)


STEP_PLAN = [([1, 2], (1, 0, 63, 63)), ([1, 2], (0, 1, 63, 63)), ([1, 2], (1, 1, 63, 63))]


def vary(batch, gen, dtype):
    b = dict(batch)
    b["latents"] = torch.randn(batch["latents"].shape, generator=gen)
    b["noises"] = [torch.randn(n.shape, generator=gen) for n in batch["noises"]]
    b["real_latents"] = torch.randn(batch["real_latents"].shape, generator=gen)
    return b


def same_over_the_plan(tr_e, stepper, batch, dtype):
    gen = torch.Generator().manual_seed(11)
    for it, (ts, crop) in enumerate(STEP_PLAN):
        b = vary(batch, gen, dtype)
        le = tr_e.train_step(b, training_steps=ts, crop=crop)
        lg = stepper(b, training_steps=ts, crop=crop)
        torch.cuda.synchronize()
        for k in ("step_loss", "G_loss", "D_loss"):
            assert float(le[k]) == float(lg[k]), f"step {it}: {k} {float(le[k])} (eager) vs {float(lg[k])}"
        tr_g = stepper.tr
        assert torch.equal(tr_e.bank.flat, tr_g.bank.flat), f"step {it}: generator LoRA parameters differ"
        assert torch.equal(tr_e.D.bank.flat, tr_g.D.bank.flat), f"step {it}: discriminator LoRA parameters differ"
        assert torch.equal(tr_e.D.head, tr_g.D.head), f"step {it}: discriminator heads differ"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sdxl_disc", [False, True], ids=["sd15", "sdxl"])
def test_train_step_moves_the_conv_head_by_adamw(dev, dtype, sdxl_disc):
    cfg, batch, tr = conv_world(dtype, dev, sdxl_disc)
    D = tr.D
    C0 = D.head_shape[1]
    assert D.head.numel() == 9 * C0 + 1 and tr.opt_D.segments[1][0] is D.head
    head0, dlora0 = D.head.clone(), D.bank.flat.clone()
    logs = tr.train_step(batch, training_steps=[1, 2], crop=(1, 0, 63, 63))
    assert torch.isfinite(logs["G_loss"]) and torch.isfinite(logs["D_loss"])
    gsq = float(tr.opt_D.gnorm_sq)
    g = D.head_grad.detach().cpu().double()
    want_sq = float((D.bank.flat_grad.double() ** 2).sum() + (D.head_grad.double() ** 2).sum())
    assert abs(gsq - want_sq) < 1e-4 * want_sq and g.abs().max() > 0, "one clip norm over the LoRA factors and the head"
    # first AdamW step, restated: clip by the shared norm, m = (1 - b1) g, v = (1 - b2) g^2, bias corrections of step 1
    b1, b2, lr, wd, eps = cfg.adam_beta1_D, cfg.adam_beta2_D, cfg.lr_D, cfg.adam_weight_decay, cfg.adam_epsilon
    gc = g * min(1.0, cfg.max_grad_norm_D / (gsq ** 0.5 + 1e-6))
    m, v = (1 - b1) * gc, (1 - b2) * gc * gc
    want = head0.cpu().double() * (1 - lr * wd) - lr / (1 - b1) * m / (v.sqrt() / (1 - b2) ** 0.5 + eps)
    assert (D.head.cpu().double() - want).abs().max() < 2e-6, "the head did not move by the AdamW update of its gradient"
    assert (D.head - head0).abs().max() > 1e-4 and not torch.equal(D.bank.flat, dlora0)
    with pytest.raises(ValueError, match="gan_unet_lastlayer_cls"):
        CoMatTrainer(tr.pipe, tr.bank, tr.blip, D, dataclasses.replace(cfg, gan_unet_lastlayer_cls=False))


@pytest.mark.gpu
@pytest.mark.parametrize("sdxl_disc", [False, True], ids=["sd15", "sdxl"])
def test_segmented_step_matches_eager(hip, sdxl_disc):
    from comat_amd.segments import SegmentedStep
    dtype = torch.bfloat16
    cfg, batch, tr_e = conv_world(dtype, hip, sdxl_disc)
    _, _, tr_g = conv_world(dtype, hip, sdxl_disc)
    tr_e.pipe.share_text_kv = False
    st = SegmentedStep(tr_g)
    same_over_the_plan(tr_e, st, batch, dtype)
    assert st.failed is None and st.head_seg is not None and st.head_seg.replays == len(STEP_PLAN) - 1


@pytest.mark.gpu
def test_graphed_step_matches_eager(hip):
    dtype = torch.bfloat16
    cfg, batch, tr_e = conv_world(dtype, hip)
    _, _, tr_g = conv_world(dtype, hip)
    gs = GraphedStep(tr_g)
    assert gs.supported(batch)
    same_over_the_plan(tr_e, gs, batch, dtype)
    assert gs.failed is None and len(gs.graphs) == 1
    # an SDXL discriminator reads a batch tensor the whole-step graph has no staging buffer for: declined, the step is eager
    _, batch_x, tr_x = conv_world(dtype, hip, sdxl_disc=True)
    assert not GraphedStep(tr_x).supported(batch_x)


# ---- 11. checkpoint -------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trips_the_conv_head(sim, tmp_path):
    dtype = torch.float32
    usd, _, lsd = tiny_weights(dtype)
    C0 = config.TINY_UNET.block_out_channels[0]
    g = torch.Generator().manual_seed(2)
    hw, hb = torch.randn(1, C0, 3, 3, generator=g), torch.randn(1, generator=g)

    def disc(head_w, head_b, conv=True):
        bank = LoRABank(config.TINY_UNET, lsd, dtype, sim)
        return D_sd(UNet(config.TINY_UNET, usd, dtype, sim, bank), bank, head_w, head_b, lastlayer_cls=conv)
    d1 = disc(hw, hb)
    checkpoint.save_checkpoint(str(tmp_path), d1.bank, d1)
    mlp = torch.load(tmp_path / "D_sd" / "mlp.pt")
    assert sorted(mlp) == ["bias", "weight"] and tuple(mlp["weight"].shape) == (1, C0, 3, 3) and tuple(mlp["bias"].shape) == (1,)
    conv = torch.nn.Conv2d(C0, 1, 3, padding=1)
    conv.load_state_dict(mlp)  # the reference's own module takes the file (training_script.py:196-200)
    assert torch.equal(conv.weight.detach(), hw) and torch.equal(conv.bias.detach(), hb)
    d2 = disc(torch.zeros(1, C0, 3, 3), torch.zeros(1))
    checkpoint.load_checkpoint(str(tmp_path), d2.bank, d2)
    assert torch.equal(d2.head, d1.head) and torch.equal(d2.w, ops.conv_weight_to_taps(hw))
    with pytest.raises(ValueError, match="Linear"):  # a conv file into the Linear head
        d3 = disc(torch.zeros(1, 4), torch.zeros(1), conv=False)
        checkpoint.load_checkpoint(str(tmp_path), d3.bank, d3)
    lin_dir = tmp_path / "lin"
    d3 = disc(torch.ones(1, 4), torch.ones(1), conv=False)
    checkpoint.save_checkpoint(str(lin_dir), d3.bank, d3)
    with pytest.raises(ValueError, match="Conv2d"):  # a Linear file into the conv head
        checkpoint.load_checkpoint(str(lin_dir), d2.bank, d2)
    assert torch.equal(d2.head, d1.head), "a refused load changed the head"
