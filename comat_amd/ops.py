"""Autograd operators of the CoMat step, each a thin `torch.autograd.Function` over the C-ABI kernels.

Activations are channels-last token matrices: an image tensor (B, H, W, C) is the contiguous 2-D tensor
[B*H*W, C].  Frozen weights carry both orientations (`w` [N,K] for the forward GEMM, `wt` [K,N] for the
data-gradient) so that every large contraction runs through the k-contiguous MFMA path; only LoRA factors and
attention use the k-major operand paths.  Nothing here computes on the CPU: the kernel backend is the HIP library
(`comat_amd._hip.HipKernels`); `set_kernel_backend` exists only so that `tests/` can check the host logic on a
machine without a GPU by plugging in a simulator of the C ABI.

Also the facade of the host code: the backend object (backend.py), the stream machinery (streams.py), the fp8 forward's state
(fp8.py) and LoRA (lora.py) are re-exported under the names callers use as `ops.NAME`; their flags are read where they live.
"""
from __future__ import annotations

import os

import torch
from torch.autograd import Function

from . import fp8
from ._hip import ACT_GELU, ACT_NONE, ACT_SILU, EMBED_GRAD_MAX_N, UN_AFFINE, UN_COPY, UN_GELU, UN_QUICK_GELU, UN_SILU  # noqa: F401
from .backend import _c, _uniform_stride, kernels, set_kernel_backend  # noqa: F401
from .fp8 import (clear_fp8_recipe, fp8_act, fp8_calibration, fp8_capture_on_trust, fp8_clipped_sites, fp8_eligible,  # noqa: F401
                  fp8_end_of_step, fp8_forward, fp8_load_state_dict, fp8_pending, fp8_producer_site, fp8_recipe, fp8_report,
                  fp8_reset, fp8_scaling, fp8_site, fp8_sites_preserved, fp8_stamp, fp8_state, fp8_state_dict, fp8_unready,
                  fp8_weight, fp8_weight_group, set_fp8_recipe, set_fp8_scaling, use_fp8)
from .lora import LoRAGroup, LoRAStore, lora_group_linear, lora_linear, set_lora_tail, set_train_merged  # noqa: F401
from .streams import (TT_GROUP, StaticBatch, _queue_join, _tt_enqueue, _TTQueue, capture_kwargs, capture_stream,  # noqa: F401
                      drop_side_stream_state, flush_weight_grads, graph_capture, join_side_streams, no_side_streams,
                      prepare_capture_stream, reset_capture_stream, reset_side_stream_state, run_off_chain,
                      set_side_stream_enabled, set_tt_grouping, side_streams_enabled)


# ----------------------------------------------------------------------------------------------------------------
# parameter holders
# ----------------------------------------------------------------------------------------------------------------
class FrozenLinear:
    """A frozen nn.Linear: weight [N,K] and its transpose [K,N] in the compute dtype, bias fp32."""

    def __init__(self, weight: torch.Tensor, bias, dtype, device):
        w = weight.to(device=device, dtype=torch.float32)
        self.w = w.to(dtype).contiguous()
        self.wt = w.t().contiguous().to(dtype)
        self.bias = None if bias is None else bias.to(device=device, dtype=torch.float32).contiguous()
        self.out_features, self.in_features = self.w.shape


class FrozenGegluLinear:
    """`ff.net.0.proj` of a BasicTransformerBlock followed by its GEGLU (3P diffusers GEGLU: `value, gate = proj(x).chunk(2, -1);
    value * gelu(gate)`): a frozen Linear(in -> 2 D) whose output ROWS are stored interleaved in sixteens - rows 32 t .. 32 t + 15 =
    value channels 16 t .., rows 32 t + 16 .. 32 t + 31 = their gate channels - so that one lane of the GEMM epilogue owns value
    and gate of the same 8 channels and the product leaves the GEMM (comat_gemm_params::epi2).  `w` [2 D, in] / `wt` [in, 2 D]
    / `bias` [2 D] in that order; `out_features` = D."""

    def __init__(self, weight: torch.Tensor, bias, dtype, device):
        n2, k = weight.shape
        D = n2 // 2
        self.perm = geglu_perm(n2)  # interleaved position -> original row
        w = weight.to(device=device, dtype=torch.float32)[self.perm.to(device)]
        self.w = w.to(dtype).contiguous()
        self.wt = w.t().contiguous().to(dtype)
        self.bias = None if bias is None else bias.to(device=device, dtype=torch.float32)[self.perm.to(device)].contiguous()
        self.out_features, self.pre_features, self.in_features = D, n2, k


def frozen_linear_group(weights, biases, dtype, device):
    """FrozenLinears of projections that read the same input (same [N, K] each), allocated as ONE [G, N, K] buffer
    (+ one [G, K, N] for the transposes): the group's forward is then a single batched launch."""
    G = len(weights)
    shp = tuple(weights[0].shape)
    assert all(tuple(w.shape) == shp for w in weights)
    w32 = torch.stack([w.to(device=device, dtype=torch.float32) for w in weights])
    W = w32.to(dtype).contiguous()
    Wt = w32.transpose(1, 2).contiguous().to(dtype)
    out = []
    for i in range(G):
        lin = FrozenLinear.__new__(FrozenLinear)
        lin.w, lin.wt = W[i], Wt[i]
        b = biases[i]
        lin.bias = None if b is None else b.to(device=device, dtype=torch.float32).contiguous()
        lin.out_features, lin.in_features = shp
        out.append(lin)
    return out


class FrozenConv:
    """A frozen conv2d.  `w` is [Cout, KH, KW, Cin]; `wd` is the tap-flipped, channel-transposed weight
    [Cin, KH, KW, Cout] that turns the data-gradient into the same implicit-GEMM gather."""

    def __init__(self, weight_oihw: torch.Tensor, bias, dtype, device, stride=1, pad=1):
        w = weight_oihw.to(device=device, dtype=torch.float32)
        self.cout, self.cin, self.kh, self.kw = w.shape
        self.w = w.permute(0, 2, 3, 1).contiguous().to(dtype)
        self.wd = w.flip(2, 3).permute(1, 2, 3, 0).contiguous().to(dtype)
        self.bias = None if bias is None else bias.to(device=device, dtype=torch.float32).contiguous()
        self.stride, self.pad = stride, pad


class TrainableLinear:
    """A Linear (or 1x1 conv) that is trained in full - the VAE decoder under `--tune_vae` (training_utils/pipeline.py:68).  The
    fields the forward reads are FrozenLinear's: `w` [N, K] in the compute dtype (a view of the owner's compute copy: the fp32
    master itself in fp32), `wt` its transpose, `bias` fp32 (a view of the master).  `w_grad` [N, K] / `bias_grad` are fp32 views
    of the owner's flat gradient buffer, accumulated in place by the backward pass while `requires_grad` is set."""

    trainable = True

    def __init__(self, w, w_grad, bias, bias_grad, wt=None):
        """wt: the owner's storage of the second orientation (unet.UNetBank refreshes every holder's in one launch), else its own"""
        self.w, self.w_grad, self.bias, self.bias_grad = w, w_grad, bias, bias_grad
        self.wt = torch.empty((w.shape[1], w.shape[0]), dtype=w.dtype, device=w.device) if wt is None else wt
        self.out_features, self.in_features = w.shape
        self.requires_grad = True

    def refresh(self):
        """after `w` changed (the owner recast its flat buffer): the derived orientation follows"""
        self.wt.copy_(self.w.t())


class TrainableConv:
    """A conv2d that is trained in full; FrozenConv's fields, with `w` [Cout, KH, KW, Cin] a view of the owner's compute copy -
    the weight is KEPT in the kernel layout, so that comat_conv2d_wgrad accumulates `w_grad` (same layout, fp32) in place."""

    trainable = True

    def __init__(self, w, w_grad, bias, bias_grad, stride=1, pad=1, wd=None):
        self.w, self.w_grad, self.bias, self.bias_grad = w, w_grad, bias, bias_grad
        self.cout, self.kh, self.kw, self.cin = w.shape
        self.wd = torch.empty((self.cin, self.kh, self.kw, self.cout), dtype=w.dtype, device=w.device) if wd is None else wd
        self.stride, self.pad = stride, pad
        self.requires_grad = True

    def refresh(self):
        self.wd.copy_(self.w.flip(1, 2).permute(3, 1, 2, 0))


class TrainableGegluLinear(TrainableLinear):
    """`ff.net.0.proj` + GEGLU trained in full: FrozenGegluLinear's fields, `w` [2 D, in] / `bias` [2 D] and their gradients KEPT in
    its interleaved row order by the owner (unet.UNetBank), so that dW and db are taken from the pre-activation gradient as it is."""

    def __init__(self, w, w_grad, bias, bias_grad, wt=None):
        super().__init__(w, w_grad, bias, bias_grad, wt)
        self.pre_features, self.in_features = w.shape
        self.out_features = self.pre_features // 2


def geglu_perm(n2):
    """interleaved position -> original row of a GEGLU projection with 2 D = n2 output rows (FrozenGegluLinear)"""
    assert n2 % 32 == 0, "GEGLU projection: 2 D must be a multiple of 32"
    t = torch.arange(n2 // 32).reshape(-1, 1, 1)
    j = torch.arange(16).reshape(1, 1, -1)
    half = torch.arange(2).reshape(1, -1, 1)
    return (half * (n2 // 2) + t * 16 + j).reshape(-1)


def trains(holder, ctx):
    """the holder's weight gradient is wanted by the backward pass of this node.  The parameters are not autograd inputs (their
    gradients land in the owner's flat buffer), so the node must have a differentiable input to be run at all: under --tune_vae
    the decoder's input always carries a gradient; under torch.no_grad() nothing does and nothing is saved.  A layer whose input
    may carry none (under --full_finetuning: conv_in, the text key / value projections, the first embedding layers) is handed its
    owner's GATE, a tensor that requires grad for no other purpose (`gate_of`)."""
    return bool(getattr(holder, "trainable", False) and holder.requires_grad and any(ctx.needs_input_grad))


def gate_of(holder):
    """the gate tensor of a trained holder whose owner has one (unet.UNetBank), else None: an extra autograd input that makes the
    node run in the backward pass even when its data input carries no gradient"""
    # (under torch.no_grad() no gate: a Function's needs_input_grad reports an input's requires_grad whatever the grad mode)
    return getattr(holder, "gate", None) if getattr(holder, "requires_grad", False) and torch.is_grad_enabled() else None


# ----------------------------------------------------------------------------------------------------------------
# elementwise
# ----------------------------------------------------------------------------------------------------------------
def cast(x, dtype):
    """dtype conversion (no autograd)."""
    if x.dtype == dtype:
        return x
    x = _c(x)
    y = torch.empty_like(x, dtype=dtype)
    kernels().unary(UN_COPY, x, y, x.numel())
    return y


class _Cast(Function):
    @staticmethod
    def forward(ctx, x, dtype):
        ctx.src_dtype = x.dtype
        return cast(x, dtype)

    @staticmethod
    def backward(ctx, g):
        return cast(_c(g), ctx.src_dtype), None


def cast_grad(x, dtype):
    return x if x.dtype == dtype else _Cast.apply(x, dtype)


class _Unary(Function):
    @staticmethod
    def forward(ctx, x, op):
        x = _c(x)
        y = torch.empty_like(x)
        kernels().unary(op, x, y, x.numel())
        ctx.save_for_backward(x)
        ctx.op = op
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        kernels().unary_bwd(ctx.op, _c(g), x, dx, x.numel())
        return dx, None


def silu(x):
    return _Unary.apply(x, UN_SILU)


def gelu(x):
    return _Unary.apply(x, UN_GELU)


def quick_gelu(x):
    """x * sigmoid(1.702 x): transformers' QuickGELUActivation (CLIP ViT-L/14's text MLP)"""
    return _Unary.apply(x, UN_QUICK_GELU)


class _Axpby(Function):
    @staticmethod
    def forward(ctx, x, y, a, b):
        x, y = _c(x), _c(y)
        out = torch.empty_like(x)
        kernels().axpby(a, x, b, y, out, x.numel())
        ctx.a, ctx.b = a, b
        ctx.ydtype = y.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        gx = gy = None
        if ctx.needs_input_grad[0]:
            if ctx.a == 1.0:
                gx = g
            else:
                gx = torch.empty_like(g)
                kernels().axpby(ctx.a, g, 0.0, None, gx, g.numel())
        if ctx.needs_input_grad[1]:
            if ctx.b == 1.0 and ctx.ydtype == g.dtype:
                gy = g
            else:
                gy = torch.empty_like(g, dtype=ctx.ydtype)
                kernels().axpby(ctx.b, g, 0.0, None, gy, g.numel())
        return gx, gy, None, None


def add(x, y, a=1.0, b=1.0):
    """a*x + b*y (same shape); result has x's dtype."""
    return _Axpby.apply(x, y, float(a), float(b))


class _Affine(Function):
    @staticmethod
    def forward(ctx, x, a, b):
        x = _c(x)
        y = torch.empty_like(x)
        kernels().unary(UN_AFFINE, x, y, x.numel(), a, b)
        ctx.a = a
        return y

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        dx = torch.empty_like(g)
        kernels().unary(UN_AFFINE, g, dx, g.numel(), ctx.a, 0.0)
        return dx, None, None


def affine(x, a, b):
    """a*x + b with scalars."""
    return _Affine.apply(x, float(a), float(b))


class _GradNorm(Function):
    """identity whose backward measures (and optionally normalises) the gradient that passes: the `record_grad` hook of the
    reference's step body (training_script.py:644-651)"""

    @staticmethod
    def forward(ctx, x, norm_out, target):
        ctx.norm_out, ctx.target = norm_out, target
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        # a fresh tensor, never in place: autograd may hand the same gradient tensor to another consumer
        out = torch.empty_like(g) if ctx.target > 0 else None
        kernels().grad_norm_scale(g, out, g.numel(), ctx.norm_out, ctx.target)
        return (g if out is None else out), None, None


def grad_norm_hook(x, norm_out, target=0.0):
    """x unchanged; in the backward pass norm_out[0] (fp32, device, caller-owned) receives |dL/dx|_2 and, with target > 0, the
    gradient continues as g * target / |g|_2 (`--norm_grad`: target = 1e4).  No host synchronisation."""
    return _GradNorm.apply(x, norm_out, float(target))


class _Geglu(Function):
    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        M, D2 = x.shape
        y = x.new_empty((M, D2 // 2))
        kernels().geglu_fwd(x, y, M, D2 // 2)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        kernels().geglu_bwd(_c(g), x, dx, x.shape[0], x.shape[1] // 2)
        return dx


def geglu(x):
    return _Geglu.apply(x)


# COMAT_GEGLU_FUSED=0: the projection and the GEGLU as two launches (A/B runs, tests); both forms use the interleaved layout
_geglu_fused = os.environ.get("COMAT_GEGLU_FUSED", "1") != "0"
# COMAT_GEGLU_BWD_FUSED=0: the GEGLU's gradient as its own launch behind ff.net.2's data-gradient GEMM (A/B runs)
_geglu_bwd_fused = os.environ.get("COMAT_GEGLU_BWD_FUSED", "1") != "0"


def set_geglu_fused(flag: bool):
    global _geglu_fused
    _geglu_fused = bool(flag)


def _geglu_linear_fwd(x, lin, need_pre, fp8_for=None, keep_y=False):
    """(GEGLU(x W^T + b), pre-activations or None, None): ONE launch (the product leaves the GEMM epilogue; the pre-activations are
    stored only when a backward pass will read them) where the library's pipelined kernel takes the problem, else the GEMM and
    the interleaved-layout GEGLU kernel.
    fp8_for: the frozen layer that consumes the result.  Under the fp8 forward with delayed scaling the epilogue writes the e4m3
    bytes that layer multiplies INSTEAD of the bf16 product (comat_gemm_params::q8): -> (None, pre, (bytes, scale)); keep_y: the
    bf16 product is stored as well (a trained `ff.net.2` takes its weight gradient from it)."""
    M, Kd = x.shape
    D, N2 = lin.out_features, lin.pre_features
    k = kernels()
    if use_fp8(lin, Kd):
        a, (w, sw) = fp8_act(x, lin), fp8_weight(lin)
        a, scales = a[0], (a[1], sw)
    else:
        a, w, scales = x, lin.w, None
    fused = _geglu_fused and x.dtype == torch.bfloat16 and k.geglu_gemm_ok(a, w, M, N2, Kd)
    site = fp8_producer_site(fp8_for, D, x.device) if (fused and scales is not None and fp8._geglu_q8) else None
    if site is not None:
        pre = x.new_empty((M, N2)) if need_pre else None
        q8 = torch.empty((M, D), dtype=torch.uint8, device=x.device)
        y = x.new_empty((M, D)) if keep_y else None
        k.gemm(a, w, pre, M, N2, Kd, Kd, Kd, N2, bias=lin.bias, scales=scales, geglu=(y, need_pre), q8=(q8, site[0], site[1]))
        return y, pre, (q8, site[0])
    y = x.new_empty((M, D))
    if fused:
        pre = x.new_empty((M, N2)) if need_pre else None
        k.gemm(a, w, pre, M, N2, Kd, Kd, Kd, N2, bias=lin.bias, scales=scales, geglu=(y, need_pre))
    else:
        pre = x.new_empty((M, N2))
        k.gemm(a, w, pre, M, N2, Kd, Kd, Kd, N2, bias=lin.bias, scales=scales)
        k.geglu_il_fwd(pre, y, M, D)
    return y, (pre if need_pre else None), None


class _GegluLinear(Function):
    """y = GEGLU(x W^T + b) with the interleaved weight of FrozenGegluLinear (see _geglu_linear_fwd)."""

    @staticmethod
    def forward(ctx, x, lin, gate=None):
        x = _c(x)
        ctx.wg = trains(lin, ctx)
        y, pre, _ = _geglu_linear_fwd(x, lin, ctx.needs_input_grad[0] or ctx.wg)
        ctx.lin = lin
        if ctx.wg:
            ctx.save_for_backward(pre, x)
        elif pre is not None:
            ctx.save_for_backward(pre)
        return y

    @staticmethod
    def backward(ctx, g):
        pre = ctx.saved_tensors[0]
        lin = ctx.lin
        M, N2 = pre.shape
        k = kernels()
        dpre = torch.empty_like(pre)
        k.geglu_il_bwd(_c(g), pre, dpre, M, lin.out_features)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = pre.new_empty((M, lin.in_features))
            k.gemm(dpre, lin.wt, dx, M, lin.in_features, N2, N2, N2, lin.in_features)
        if ctx.wg:  # dW, db in the interleaved layout, from the pre-activation gradient
            _linear_weight_grads(lin, dpre, ctx.saved_tensors[1], M, N2, lin.in_features)
        return dx, None, None


class _GegluFeedForward(Function):
    """h = GEGLU(x W1^T + b1) W2^T + b2 + residual - the feed-forward of a BasicTransformerBlock (`ff.net.0.proj` + GEGLU,
    `ff.net.2`; 3P diffusers FeedForward, reached from TrainableSDPipeline.py:144-150) as one autograd node, so that the
    backward pass can run the GEGLU's gradient in the epilogue of `ff.net.2`'s data-gradient GEMM (comat_gemm_params::epi2 = 3):
        forward   two launches (projection + GEGLU epilogue, projection + residual epilogue)  - as before
        backward  d pre = geglu'(g W2; pre) in ONE launch (was: the GEMM, a [M, D] round trip, the elementwise kernel), then
                  dx = d pre W1."""

    @staticmethod
    def forward(ctx, x, residual, ff1, ff2, gate=None):
        x = _c(x)
        ctx.wg = trains(ff1, ctx)  # trained layers (both or neither): their weight gradients need x and the GEGLU output
        need = ctx.needs_input_grad[0] or ctx.wg
        # (fp8 forward, delayed scales: e4m3 bytes instead of f - next to f where the weight gradient of ff2 will read it)
        f, pre, f8q = _geglu_linear_fwd(x, ff1, need, fp8_for=ff2, keep_y=ctx.wg)
        M, D = x.shape[0], ff1.out_features
        N = ff2.out_features
        y = x.new_empty((M, N))
        k = kernels()
        residual = _c(residual) if residual is not None else None
        beta = 1.0 if residual is not None else 0.0
        if use_fp8(ff2, D):
            f8, sf = f8q if f8q is not None else fp8_act(f, ff2)
            w8, sw = fp8_weight(ff2)
            k.gemm(f8, w8, y, M, N, D, D, D, N, bias=ff2.bias, R=residual, ldr=N, beta=beta, scales=(sf, sw))
        else:
            k.gemm(f, ff2.w, y, M, N, D, D, D, N, bias=ff2.bias, R=residual, ldr=N, beta=beta)
        ctx.ff1, ctx.ff2 = ff1, ff2
        ctx.has_res = residual is not None
        if ctx.wg:
            ctx.save_for_backward(pre, x, f)
        elif need:
            ctx.save_for_backward(pre)
        return y

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        ff1, ff2 = ctx.ff1, ctx.ff2
        dx = None
        if ctx.needs_input_grad[0] or ctx.wg:
            pre = ctx.saved_tensors[0]
            M, N2 = pre.shape
            D, N = ff1.out_features, ff2.out_features
            k = kernels()
            dpre = torch.empty_like(pre)
            if _geglu_fused and _geglu_bwd_fused and pre.dtype == torch.bfloat16 and k.geglu_gemm_ok(g, ff2.wt, M, 2 * D, N):
                k.gemm(g, ff2.wt, dpre, M, D, N, N, N, N2, geglu=(pre, "bwd"))
            else:
                df = pre.new_empty((M, D))
                k.gemm(g, ff2.wt, df, M, D, N, N, N, D)
                k.geglu_il_bwd(df, pre, dpre, M, D)
            if ctx.needs_input_grad[0]:
                dx = pre.new_empty((M, ff1.in_features))
                k.gemm(dpre, ff1.wt, dx, M, ff1.in_features, N2, N2, N2, ff1.in_features)
            if ctx.wg:
                # ff.net.2: dW2 += g^T GEGLU(pre), db2 += colsum g;  ff.net.0.proj: dW1 += d pre^T x, db1 += colsum d pre (interleaved)
                _, x, f = ctx.saved_tensors
                _linear_weight_grads(ff2, g, f, M, N, D)
                _linear_weight_grads(ff1, dpre, x, M, N2, ff1.in_features)
        return dx, (g if ctx.has_res else None), None, None, None


def geglu_feed_forward(x, ff1: "FrozenGegluLinear", ff2: "FrozenLinear", residual=None):
    """GEGLU(x W1^T + b1) W2^T + b2 (+ residual): see _GegluFeedForward"""
    return _GegluFeedForward.apply(x, residual, ff1, ff2, gate_of(ff1))


def geglu_linear(x, lin: "FrozenGegluLinear"):
    """GEGLU(x W^T + b) - the feed-forward's first projection and its gate in one operator (see _GegluLinear)"""
    return _GegluLinear.apply(x, lin, gate_of(lin))


def _copy_pair(items, rows):
    """two strided 2-D copies [(src, ld_src, dst, ld_dst, cols)] in one launch where the library takes them (16-byte rows)"""
    k = kernels()
    if hasattr(k, "copy2d_pair") and k.copy2d_pair_ok(items):
        k.copy2d_pair(items, rows)
    else:
        for src, ld_src, dst, ld_dst, cols in items:
            k.copy2d(src, ld_src, dst, ld_dst, rows, cols)


class _ConcatCols(Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _c(a), _c(b)
        M, Ca = a.shape
        Cb = b.shape[1]
        out = a.new_empty((M, Ca + Cb))
        _copy_pair([(a, Ca, out, Ca + Cb, Ca), (b, Cb, out[:, Ca:], Ca + Cb, Cb)], M)
        ctx.ca, ctx.cb = Ca, Cb
        return out

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        M = g.shape[0]
        Ca, Cb = ctx.ca, ctx.cb
        k = kernels()
        ga = gb = None
        if ctx.needs_input_grad[0] and ctx.needs_input_grad[1]:
            ga, gb = g.new_empty((M, Ca)), g.new_empty((M, Cb))
            _copy_pair([(g, Ca + Cb, ga, Ca, Ca), (g[:, Ca:], Ca + Cb, gb, Cb, Cb)], M)
        elif ctx.needs_input_grad[0]:
            ga = g.new_empty((M, Ca))
            k.copy2d(g, Ca + Cb, ga, Ca, M, Ca)
        elif ctx.needs_input_grad[1]:
            gb = g.new_empty((M, Cb))
            k.copy2d(g[:, Ca:], Ca + Cb, gb, Cb, M, Cb)
        return ga, gb


def concat_cols(a, b):
    """channel concat of two [M, C*] token matrices (UNet skip connections)."""
    return _ConcatCols.apply(a, b)


class _ConcatRows(Function):
    """row concat: out = [a; b] (batch concat of token matrices)."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _c(a), _c(b)
        out = a.new_empty((a.shape[0] + b.shape[0], a.shape[1]))
        k = kernels()
        na, nb = a.numel(), b.numel()
        items = [(a, na, out[: a.shape[0]], na, na), (b, nb, out[a.shape[0]:], nb, nb)]
        if a.dtype == b.dtype and hasattr(k, "copy2d_pair") and k.copy2d_pair_ok(items):
            k.copy2d_pair(items, 1)  # both halves in one launch (one "row" each)
        else:
            k.unary(UN_COPY, a, out[: a.shape[0]], na)
            k.unary(UN_COPY, b, out[a.shape[0]:], nb)
        ctx.ma = a.shape[0]
        return out

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        return g[: ctx.ma], g[ctx.ma:]


def concat_rows(a, b):
    return _ConcatRows.apply(a, b)


class _AddRowVec(Function):
    @staticmethod
    def forward(ctx, x, v):
        x, v = _c(x), _c(v)
        out = torch.empty_like(x)
        kernels().add_rowvec(x, v, out, x.shape[0], x.shape[1])
        return out

    @staticmethod
    def backward(ctx, g):
        return g, None  # v is a frozen positional table


def add_rowvec(x, v):
    """x[r, :] + v[:] with a frozen vector/table v (x: [rows, cols], v: [cols])."""
    return _AddRowVec.apply(x, v)


# ----------------------------------------------------------------------------------------------------------------
# dense contractions
# ----------------------------------------------------------------------------------------------------------------
class _Linear(Function):
    @staticmethod
    def forward(ctx, x, residual, lin, act, out_dtype=None, gate=None):
        x = _c(x)
        M, Kd = x.shape
        N = lin.out_features
        y = torch.empty((M, N), dtype=out_dtype or x.dtype, device=x.device)
        if residual is not None:
            residual = _c(residual)
        if use_fp8(lin, Kd):
            k = kernels()
            x8, sx = fp8_act(x, lin)
            w8, sw = fp8_weight(lin)
            k.gemm(x8, w8, y, M, N, Kd, Kd, Kd, N, bias=lin.bias, R=residual, ldr=N,
                   beta=1.0 if residual is not None else 0.0, act=act, scales=(sx, sw))
        else:
            kernels().gemm(x, lin.w, y, M, N, Kd, Kd, Kd, N, bias=lin.bias, R=residual, ldr=N,
                           beta=1.0 if residual is not None else 0.0, act=act)
        ctx.lin = lin
        ctx.has_res = residual is not None
        ctx.shape = (M, N, Kd)
        ctx.wg = trains(lin, ctx)  # a trained layer: the weight gradient needs the input
        if ctx.wg:
            assert act == ACT_NONE
            ctx.save_for_backward(x)
        assert act == ACT_NONE or not ctx.needs_input_grad[0], "fused activation is for no-grad calls only"
        return y

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        M, N, Kd = ctx.shape
        dx = None
        if ctx.needs_input_grad[0]:
            dx = g.new_empty((M, Kd))
            kernels().gemm(g, ctx.lin.wt, dx, M, Kd, N, N, N, Kd)
        if ctx.wg:
            _linear_weight_grads(ctx.lin, g, ctx.saved_tensors[0], M, N, Kd)
        return dx, (g if ctx.has_res else None), None, None, None, None


def _linear_weight_grads(lin, g, x, M, N, Kd):
    """dW [N, K] += g^T x and db += column sums of g, fp32 in place, off the dependent chain: the k-major product joins the grouped
    weight-gradient launches where comat_gemm_tt_grouped takes it, else (fp32 parity mode, the 4 -> 4 post_quant_conv) one
    comat_gemm with both operands k-major, as lora._factor_grads"""
    from . import streams
    k = kernels()
    prob = (g, x, lin.w_grad, N, Kd, M, N, Kd, Kd)

    def bias_grad():
        if lin.bias_grad is not None:
            k.colsum(g, lin.bias_grad, M, N, N)

    if streams._tt_grouping and k.tt_group_ok(*prob):
        streams._tt_enqueue(x.device, [prob], (g, x), pre=bias_grad)
        return

    def weight_grads():
        bias_grad()
        k.gemm(g, x, lin.w_grad, N, Kd, M, N, Kd, Kd, transA=True, transB=True, R=lin.w_grad, ldr=Kd, beta=1.0)

    run_off_chain(x.device, weight_grads, (g, x))


def linear(x, lin: FrozenLinear, residual=None, act=ACT_NONE, out_dtype=None):
    """y = x W^T + b (+ residual); W frozen.  `out_dtype` (no-grad use) lets the GEMM epilogue emit fp32 directly."""
    return _Linear.apply(x, residual, lin, act, out_dtype, gate_of(lin))


class _Conv(Function):
    @staticmethod
    def forward(ctx, x, residual, conv, B, H, W, ups, bias2, gate=None):
        x = _c(x)
        Hs, Ws = H * ups, W * ups
        Ho = (Hs + 2 * conv.pad - conv.kh) // conv.stride + 1
        Wo = (Ws + 2 * conv.pad - conv.kw) // conv.stride + 1
        assert x.shape == (B * H * W, conv.cin), (x.shape, B, H, W, conv.cin)
        y = x.new_empty((B * Ho * Wo, conv.cout))
        if residual is not None:
            residual = _c(residual)
        if use_fp8(conv, conv.cin):
            k = kernels()
            x8, sx = fp8_act(x, conv)
            w8, sw = fp8_weight(conv)
            k.conv2d(x8, w8, y, B, H, W, conv.cin, Ho, Wo, conv.cout, conv.kh, conv.kw, conv.stride, conv.pad, mode=0,
                     ups=ups, bias=conv.bias, bias2=bias2, R=residual, beta=1.0 if residual is not None else 0.0,
                     scales=(sx, sw))
        else:
            kernels().conv2d(x, conv.w, y, B, H, W, conv.cin, Ho, Wo, conv.cout, conv.kh, conv.kw, conv.stride, conv.pad,
                             mode=0, ups=ups, bias=conv.bias, bias2=bias2, R=residual,
                             beta=1.0 if residual is not None else 0.0)
        ctx.conv, ctx.geo = conv, (B, H, W, Ho, Wo, ups)
        ctx.has_res = residual is not None
        ctx.wg = trains(conv, ctx)  # a trained layer: the weight gradient needs the input (a frozen conv saves nothing)
        if ctx.wg:
            ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        conv = ctx.conv
        B, H, W, Ho, Wo, ups = ctx.geo
        dx = None
        if ctx.needs_input_grad[0]:
            k = kernels()
            padd = conv.kh - 1 - conv.pad
            if conv.stride == 1:
                Hs, Ws = H * ups, W * ups
                du = g.new_empty((B * Hs * Ws, conv.cin))
                k.conv2d(g, conv.wd, du, B, Ho, Wo, conv.cout, Hs, Ws, conv.cin, conv.kh, conv.kw, 1, padd, mode=0)
                if ups == 2:
                    dx = g.new_empty((B * H * W, conv.cin))
                    k.sumpool2x2(du, dx, B, H, W, conv.cin)
                else:
                    dx = du
            else:
                assert ups == 1
                dx = g.new_empty((B * H * W, conv.cin))
                k.conv2d(g, conv.wd, dx, B, Ho, Wo, conv.cout, H, W, conv.cin, conv.kh, conv.kw, conv.stride, padd,
                         mode=1)
        if ctx.wg:  # dW and db in fp32, in place, off the dependent chain (nothing reads them before the optimizer)
            x, k = ctx.saved_tensors[0], kernels()

            def weight_grads():
                k.conv2d_wgrad(x, g, conv.w_grad, B, H, W, conv.cin, Ho, Wo, conv.cout, conv.kh, conv.kw, conv.stride, conv.pad, ups)
                if conv.bias_grad is not None:
                    k.colsum(g, conv.bias_grad, B * Ho * Wo, conv.cout, conv.cout)

            run_off_chain(x.device, weight_grads, (x, g))
        db2 = None
        if ctx.needs_input_grad[7]:  # the time-embedding projection is trained: per-sample column sums of g, fp32 [B, Cout]
            db2 = torch.empty((B, conv.cout), dtype=torch.float32, device=g.device)
            kernels().colsum_batched(g, db2, B, Ho * Wo, conv.cout, conv.cout)
        return dx, (g if ctx.has_res else None), None, None, None, None, None, db2, None


def conv2d(x, conv: FrozenConv, B, H, W, ups=1, residual=None, bias2=None):
    """Channels-last conv (frozen weight).  x: [B*H*W, Cin] -> ([B*Ho*Wo, Cout]).  `ups=2` fuses a nearest 2x
    upsample of the input; `bias2` [B, Cout] fp32 is the per-sample time-embedding add (frozen UNet: no gradient, the time
    embedding depends only on t and frozen weights; a fully trained UNet hands in a tensor that requires grad and gets the
    per-sample column sums of the output gradient back); `residual` is added in the epilogue."""
    return _Conv.apply(x, residual, conv, B, H, W, ups, bias2, gate_of(conv))


def conv_out_hw(conv: FrozenConv, H, W, ups=1):
    return ((H * ups + 2 * conv.pad - conv.kh) // conv.stride + 1, (W * ups + 2 * conv.pad - conv.kw) // conv.stride + 1)


# ----------------------------------------------------------------------------------------------------------------
# normalisation
# ----------------------------------------------------------------------------------------------------------------
class _GroupNorm(Function):
    """y = GroupNorm(x) (+ SiLU).  With `fork`, the input is also handed back as a second output (an alias): a branch
    that bypasses the norm (a ResnetBlock's shortcut, the residual around a transformer block) reads THAT output, so
    both gradients of x arrive at this node and dx = norm_bwd(gy) + g_bypass is ONE kernel (the `add` operand of
    comat_groupnorm_bwd) instead of autograd's separate accumulation add."""

    @staticmethod
    def forward(ctx, x, gamma, beta, B, HW, G, eps, silu_, fork, fp8_for=None):
        x = _c(x)
        Cc = x.shape[1]
        assert x.shape[0] == B * HW
        y = torch.empty_like(x)
        stats = torch.empty((B, G, 2), dtype=torch.float32, device=x.device)
        k = kernels()
        site = fp8_producer_site(fp8_for, Cc, x.device)
        if site is not None and k.groupnorm_fwd_q_ok(x, B, HW, Cc, G):
            # fp8 forward, delayed scaling: the e4m3 bytes of y for the layer it feeds leave the same launch (fp8_act finds them)
            q8 = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
            k.groupnorm_fwd_q(x, gamma, beta, y, stats, B, HW, Cc, G, eps, silu_, q8, site[0], site[1])
            fp8_stamp(y, q8, site)
        else:
            k.groupnorm_fwd(x, gamma, beta, y, stats, B, HW, Cc, G, eps, silu_)
        ctx.save_for_backward(x, gamma, beta, stats)
        ctx.cfg = (B, HW, Cc, G, silu_)
        # a trained norm (its affine parameters carry `comat_grad`, fp32 views of the owner's gradient buffer)
        ctx.affine = (gamma.comat_grad, beta.comat_grad) if getattr(gamma, "comat_train", False) and any(ctx.needs_input_grad) else None
        ctx.set_materialize_grads(False)
        return (y, x.view_as(x)) if fork else y

    @staticmethod
    def backward(ctx, g, g_bypass=None):
        x, gamma, beta, stats = ctx.saved_tensors
        B, HW, Cc, G, silu_ = ctx.cfg
        if g is None:  # the normalised branch is unused: only the bypass gradient flows
            return (g_bypass,) + (None,) * 9
        dx = torch.empty_like(x)
        add = None if g_bypass is None else _c(g_bypass)
        g = _c(g)
        kernels().groupnorm_bwd(g, x, gamma, beta, stats, dx, B, HW, Cc, G, silu_, add=add)
        if ctx.affine is not None:  # a pass of its own, off the dependent chain; the data-gradient launch above is unchanged
            dgamma, dbeta = ctx.affine
            run_off_chain(x.device, lambda: kernels().groupnorm_bwd_affine(g, x, gamma, beta, stats, dgamma, dbeta, B, HW, Cc, G, silu_),
                          (g, x, stats))
        return (dx,) + (None,) * 9


def group_norm(x, gamma, beta, B, HW, G=32, eps=1e-5, silu=False, fp8_for=None):
    """fp8_for: the frozen layer (holder) this output feeds - under the fp8 forward with delayed scaling the kernel also stores
    the e4m3 bytes that layer will multiply (ops.fp8_act picks them up); ignored otherwise"""
    return _GroupNorm.apply(x, gamma, beta, B, HW, G, float(eps), bool(silu), False, fp8_for)


def group_norm_fork(x, gamma, beta, B, HW, G=32, eps=1e-5, silu=False, fp8_for=None):
    """(GroupNorm(x), x'): use x' for the branch that bypasses the norm (see _GroupNorm)."""
    return _GroupNorm.apply(x, gamma, beta, B, HW, G, float(eps), bool(silu), True, fp8_for)


class _LayerNorm(Function):
    """y = LayerNorm(x); `fork` as in _GroupNorm (the residual connection around a pre-norm sub-layer)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, fork, fp8_for=None):
        x = _c(x)
        M, Cc = x.shape
        y = torch.empty_like(x)
        stats = torch.empty((M, 2), dtype=torch.float32, device=x.device)
        k = kernels()
        site = fp8_producer_site(fp8_for, Cc, x.device)
        if site is not None and k.layernorm_fwd_q_ok(x):
            q8 = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
            k.layernorm_fwd_q(x, gamma, beta, y, stats, M, Cc, eps, q8, site[0], site[1])
            fp8_stamp(y, q8, site)
        else:
            k.layernorm_fwd(x, gamma, beta, y, stats, M, Cc, eps)
        ctx.save_for_backward(x, gamma, stats)
        # a trained norm (its affine parameters carry `comat_grad`, fp32 views of the owner's gradient buffer), as _GroupNorm
        ctx.affine = (gamma.comat_grad, beta.comat_grad) if getattr(gamma, "comat_train", False) and any(ctx.needs_input_grad) else None
        ctx.set_materialize_grads(False)
        return (y, x.view_as(x)) if fork else y

    @staticmethod
    def backward(ctx, g, g_bypass=None):
        x, gamma, stats = ctx.saved_tensors
        if g is None:
            return g_bypass, None, None, None, None, None
        dx = torch.empty_like(x)
        add = None if g_bypass is None else _c(g_bypass)
        g = _c(g)
        kernels().layernorm_bwd(g, x, gamma, stats, dx, x.shape[0], x.shape[1], add=add)
        if ctx.affine is not None:  # a pass of its own, off the dependent chain; the data-gradient launch above is unchanged
            dgamma, dbeta = ctx.affine
            run_off_chain(x.device, lambda: kernels().layernorm_bwd_affine(g, x, stats, dgamma, dbeta, x.shape[0], x.shape[1]),
                          (g, x, stats))
        return dx, None, None, None, None, None


def layer_norm(x, gamma, beta, eps=1e-5, fp8_for=None):
    return _LayerNorm.apply(x, gamma, beta, float(eps), False, fp8_for)


def layer_norm_fork(x, gamma, beta, eps=1e-5, fp8_for=None):
    """(LayerNorm(x), x'): use x' for the residual that bypasses the norm (see _GroupNorm); fp8_for as in group_norm."""
    return _LayerNorm.apply(x, gamma, beta, float(eps), True, fp8_for)


# ----------------------------------------------------------------------------------------------------------------
# attention with materialised probabilities (the map the reference's AttentionStore captures)
# ----------------------------------------------------------------------------------------------------------------
class _Attention(Function):
    """softmax(scale * Q K^T) V per (batch, head), heads addressed in place inside [tokens, heads*dim] matrices.
    Returns (O [B*Nq, H*d], P [B, H, Nq, Nk]).  P is a differentiable output: an upstream gradient on it (from the
    attribute-concentration loss) is added to dP before the softmax backward (attn_utils/tc_attn_utils.py:140-146)."""

    @staticmethod
    def forward(ctx, q, k_, v, B, Nq, Nk, H, d, scale, causal, key_mask):
        q, k_, v = _c(q), _c(k_), _c(v)
        K = kernels()
        dev = q.device
        HD = H * d
        S = torch.empty((B, H, Nq, Nk), dtype=torch.float32, device=dev)
        K.gemm(q, k_, S, Nq, Nk, d, HD, HD, Nk, batch=(B, H), sA=(Nq * HD, d), sB=(Nk * HD, d),
               sC=(H * Nq * Nk, Nq * Nk), alpha=scale)
        P = torch.empty((B, H, Nq, Nk), dtype=q.dtype, device=dev)
        K.softmax_fwd(S, P, B * H * Nq, Nk, q_len=Nq, causal=causal, causal_offset=Nk - Nq, key_mask=key_mask,
                      rows_per_mask=H * Nq)
        del S
        O = q.new_empty((B * Nq, HD))
        K.gemm(P, v, O, Nq, d, Nk, Nk, HD, HD, transB=True, batch=(B, H), sA=(H * Nq * Nk, Nq * Nk),
               sB=(Nk * HD, d), sC=(Nq * HD, d))
        ctx.save_for_backward(q, k_, v, P)
        ctx.cfg = (B, Nq, Nk, H, d, scale)
        ctx.set_materialize_grads(False)  # an unused probability output must not cost a zero-filled gradient
        return O, P

    @staticmethod
    def backward(ctx, gO, gP):
        q, k_, v, P = ctx.saved_tensors
        B, Nq, Nk, H, d, scale = ctx.cfg
        K = kernels()
        dev = q.device
        HD = H * d
        sP = (H * Nq * Nk, Nq * Nk)
        dV = dQ = dK = None
        if gO is None and gP is None:
            return (None,) * 11
        if gO is None:
            gO = torch.zeros((B * Nq, HD), dtype=q.dtype, device=dev)
        gO = _c(gO)
        # dP = gO V^T  (fp32)
        dP = torch.empty((B, H, Nq, Nk), dtype=torch.float32, device=dev)
        K.gemm(gO, v, dP, Nq, Nk, d, HD, HD, Nk, batch=(B, H), sA=(Nq * HD, d), sB=(Nk * HD, d), sC=sP)
        if gP is not None:
            gP = _c(gP)
            K.axpby(1.0, dP, 1.0, gP, dP, dP.numel())
        if ctx.needs_input_grad[2]:  # dV [Nk, d] = P^T gO
            dV = torch.empty_like(v)
            K.gemm(P, gO, dV, Nk, d, Nq, Nk, HD, HD, transA=True, transB=True, batch=(B, H), sA=sP,
                   sB=(Nq * HD, d), sC=(Nk * HD, d))
        dS = torch.empty((B, H, Nq, Nk), dtype=q.dtype, device=dev)
        K.softmax_bwd(P, dP, dS, B * H * Nq, Nk, scale)
        del dP
        if ctx.needs_input_grad[0]:  # dQ = dS K
            dQ = torch.empty_like(q)
            K.gemm(dS, k_, dQ, Nq, d, Nk, Nk, HD, HD, transB=True, batch=(B, H), sA=sP, sB=(Nk * HD, d),
                   sC=(Nq * HD, d))
        if ctx.needs_input_grad[1]:  # dK = dS^T Q
            dK = torch.empty_like(k_)
            K.gemm(dS, q, dK, Nk, d, Nq, Nk, HD, HD, transA=True, transB=True, batch=(B, H), sA=sP,
                   sB=(Nq * HD, d), sC=(Nk * HD, d))
        return dQ, dK, dV, None, None, None, None, None, None, None, None


class _FlashAttention(Function):
    """Fused attention (scores stay on chip); saves Q, K, V, O and the per-row log-sum-exp for the backward kernels."""

    @staticmethod
    def forward(ctx, q, k_, v, B, Nq, Nk, H, d, scale, fp8_for=None):
        q, k_, v = _c(q), _c(k_), _c(v)
        HD = H * d
        O = q.new_empty((B * Nq, HD))
        lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
        site = fp8_producer_site(fp8_for, HD, q.device) if fp8._flash_q8 else None
        if site is not None:  # fp8 forward, delayed scaling: the e4m3 bytes for the output projection leave the same launch
            q8 = torch.empty((B * Nq, HD), dtype=torch.uint8, device=q.device)
            kernels().flash_attn_fwd(q, k_, v, O, lse, B, H, Nq, Nk, d, HD, HD, HD, HD, scale, q8=(q8, site[0], site[1]))
            fp8_stamp(O, q8, site)
        else:
            kernels().flash_attn_fwd(q, k_, v, O, lse, B, H, Nq, Nk, d, HD, HD, HD, HD, scale)
        ctx.save_for_backward(q, k_, v, O, lse)
        ctx.cfg = (B, Nq, Nk, H, d, scale)
        return O

    @staticmethod
    def backward(ctx, gO):
        q, k_, v, O, lse = ctx.saved_tensors
        B, Nq, Nk, H, d, scale = ctx.cfg
        HD = H * d
        gO = _c(gO)
        # one allocation, constant spacing: the q/k/v (or k/v) projections' backward batches over these gradients
        if q.shape == k_.shape:
            dQ, dK, dV = q.new_empty((3,) + tuple(q.shape)).unbind(0)
        else:
            dQ = torch.empty_like(q)
            dK, dV = k_.new_empty((2,) + tuple(k_.shape)).unbind(0)
        dbuf = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
        kernels().flash_attn_bwd(q, k_, v, O, gO, lse, dbuf, dQ, dK, dV, B, H, Nq, Nk, d, HD, HD, HD, HD, scale)
        return dQ, dK, dV, None, None, None, None, None, None, None


def flash_ok(dim, dtype):
    return dim <= 160 and dim % (8 if dtype == torch.bfloat16 else 4) == 0


def masked_attn_kernels():
    """who runs flash_attn_masked_fwd / _bwd (comat_flash_attn_masked_*): the installed backend where it has them (the simulator of
    tests/masked_attn_sim.py), else the binding's module functions - as pool_kernels()"""
    from . import _hip
    k = kernels()
    return k if hasattr(k, "flash_attn_masked_fwd") else _hip


_fused_masked_attention = False


def set_fused_masked_attention(on: bool):
    """process-wide: attention(..., need_probs=False) under a causal limit or a key-padding mask runs the fused masked kernels
    (off by default: the materialised path of _Attention).  CoMatTrainer sets it from StepConfig.fused_masked_attention."""
    global _fused_masked_attention
    _fused_masked_attention = bool(on)


def fused_masked_attention() -> bool:
    return _fused_masked_attention


class _MaskedFlashAttention(Function):
    """_FlashAttention under a causal limit (offset Nk - Nq, as _Attention) and / or a key-padding mask [B, Nk] int8; saves Q, K, V,
    O, the per-row log-sum-exp and the mask for the backward kernels."""

    @staticmethod
    def forward(ctx, q, k_, v, B, Nq, Nk, H, d, scale, causal, key_mask):
        q, k_, v = _c(q), _c(k_), _c(v)
        key_mask = None if key_mask is None else _c(key_mask)
        HD = H * d
        O = q.new_empty((B * Nq, HD))
        lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
        masked_attn_kernels().flash_attn_masked_fwd(q, k_, v, O, lse, B, H, Nq, Nk, d, HD, HD, HD, HD, scale, causal, Nk - Nq, key_mask)
        ctx.save_for_backward(q, k_, v, O, lse, key_mask)
        ctx.cfg = (B, Nq, Nk, H, d, scale, causal)
        return O

    @staticmethod
    def backward(ctx, gO):
        q, k_, v, O, lse, key_mask = ctx.saved_tensors
        B, Nq, Nk, H, d, scale, causal = ctx.cfg
        HD = H * d
        gO = _c(gO)
        if q.shape == k_.shape:  # one allocation, constant spacing (see _FlashAttention)
            dQ, dK, dV = q.new_empty((3,) + tuple(q.shape)).unbind(0)
        else:
            dQ = torch.empty_like(q)
            dK, dV = k_.new_empty((2,) + tuple(k_.shape)).unbind(0)
        dbuf = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
        masked_attn_kernels().flash_attn_masked_bwd(q, k_, v, O, gO, lse, dbuf, dQ, dK, dV, B, H, Nq, Nk, d, HD, HD, HD, HD, scale,
                                                    causal, Nk - Nq, key_mask)
        return dQ, dK, dV, None, None, None, None, None, None, None, None


class _FusedQKVAttention(Function):
    """Self-attention whose q / k / v projections are one frozen Linear(d -> 3d) (BLIP's ViT, modeling_blip
    BlipAttention.qkv): ONE GEMM writes [M, 3D], the fused attention kernels read q / k / v as column slices of it
    (leading dimension 3D), the backward kernels write dQ / dK / dV into the column slices of one [M, 3D] buffer and
    ONE GEMM (K = 3D) turns it into the input gradient — 2 launches instead of 6, no gradient-accumulation adds."""

    @staticmethod
    def forward(ctx, x, lin, B, N, H, d, scale):
        x = _c(x)
        M, Kd = x.shape
        D = H * d
        assert lin.out_features == 3 * D
        k = kernels()
        qkv = x.new_empty((M, 3 * D))
        k.gemm(x, lin.w, qkv, M, 3 * D, Kd, Kd, Kd, 3 * D, bias=lin.bias)
        O = x.new_empty((M, D))
        lse = torch.empty((B, H, N), dtype=torch.float32, device=x.device)
        k.flash_attn_fwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], O, lse, B, H, N, N, d, 3 * D, 3 * D, 3 * D, D, scale)
        ctx.save_for_backward(qkv, O, lse)
        ctx.cfg = (lin, B, N, H, d, scale, Kd)
        return O

    @staticmethod
    def backward(ctx, gO):
        qkv, O, lse = ctx.saved_tensors
        lin, B, N, H, d, scale, Kd = ctx.cfg
        D = H * d
        M = qkv.shape[0]
        k = kernels()
        gO = _c(gO)
        dqkv = torch.empty_like(qkv)
        dbuf = torch.empty((B, H, N), dtype=torch.float32, device=qkv.device)
        k.flash_attn_bwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], O, gO, lse, dbuf, dqkv[:, :D], dqkv[:, D:2 * D],
                         dqkv[:, 2 * D:], B, H, N, N, d, 3 * D, 3 * D, 3 * D, D, scale)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = qkv.new_empty((M, Kd))
            k.gemm(dqkv, lin.wt, dx, M, Kd, 3 * D, 3 * D, 3 * D, Kd)
        return dx, None, None, None, None, None, None


def fused_qkv_attention(x, lin_qkv: "FrozenLinear", B, N, heads, scale=None):
    """x: [B*N, in] -> attention output [B*N, heads*dim] with q, k, v = split(x W_qkv^T + b_qkv)."""
    D = lin_qkv.out_features // 3
    dim = D // heads
    assert flash_ok(dim, x.dtype), "fused qkv attention needs a head dim the fused kernels support"
    return _FusedQKVAttention.apply(x, lin_qkv, B, N, heads, dim, float(scale if scale is not None else dim ** -0.5))


def attention(q, k, v, B, Nq, Nk, heads, dim, scale=None, causal=False, key_mask=None, need_probs=True, fp8_for=None):
    """q: [B*Nq, heads*dim], k/v: [B*Nk, heads*dim] -> (out [B*Nq, heads*dim], probs [B, heads, Nq, Nk] or None).
    `need_probs=False` selects the fused kernel (no probability map in HBM) when the layer allows it; under `causal` or a
    `key_mask` that is the masked fused kernel, and only while set_fused_masked_attention(True) holds.
    fp8_for: the frozen projection that consumes the output (ops.group_norm): the fused kernel then also emits its e4m3 bytes."""
    if scale is None:
        scale = dim ** -0.5
    if not need_probs and not causal and key_mask is None and flash_ok(dim, q.dtype):
        return _FlashAttention.apply(q, k, v, B, Nq, Nk, heads, dim, float(scale), fp8_for), None
    if not need_probs and _fused_masked_attention and flash_ok(dim, q.dtype):
        return _MaskedFlashAttention.apply(q, k, v, B, Nq, Nk, heads, dim, float(scale), bool(causal), key_mask), None
    return _Attention.apply(q, k, v, B, Nq, Nk, heads, dim, float(scale), bool(causal), key_mask)


# ----------------------------------------------------------------------------------------------------------------
# scheduler step
# ----------------------------------------------------------------------------------------------------------------
class _CfgDdpm(Function):
    @staticmethod
    def forward(ctx, x, eps2, z, s, cx, ce, sigma):
        x, eps2 = _c(x), _c(eps2)
        assert x.dtype == torch.float32 and eps2.numel() == 2 * x.numel()
        xp = torch.empty_like(x)
        kernels().cfg_ddpm_fwd(x, eps2, None if z is None else _c(z), xp, x.numel(), s, cx, ce, sigma)
        ctx.cfg = (s, cx, ce, eps2.dtype, eps2.shape)
        return xp

    @staticmethod
    def backward(ctx, g):
        s, cx, ce, edt, eshape = ctx.cfg
        g = _c(g)
        dx = torch.empty_like(g) if ctx.needs_input_grad[0] else None
        deps = torch.empty(eshape, dtype=edt, device=g.device)
        kernels().cfg_ddpm_bwd(g, dx, deps, g.numel(), s, cx, ce)
        return dx, (deps if ctx.needs_input_grad[1] else None), None, None, None, None, None


class _CfgRescaleDdpm(Function):
    """the same step with rescaled guidance (`rescale_noise_cfg`, TrainableSDPipeline.py:159-161): per-sample statistics and
    the apply pass in one launch; eps2 and the statistics are kept only when a gradient will flow into eps2"""

    @staticmethod
    def forward(ctx, x, eps2, z, s, cx, ce, sigma, phi, batch):
        x, eps2 = _c(x), _c(eps2)
        n = x.numel()
        assert x.dtype == torch.float32 and eps2.numel() == 2 * n and n % batch == 0
        xp = torch.empty_like(x)
        stats = torch.empty((batch, 4), dtype=torch.float32, device=x.device)
        kernels().cfg_rescale_ddpm_fwd(x, eps2, None if z is None else _c(z), xp, n, s, cx, ce, sigma, phi, batch,
                                       n // batch, stats)
        ctx.cfg = (s, cx, ce, phi, batch)
        ctx.trained = bool(ctx.needs_input_grad[1])
        if ctx.trained:
            ctx.save_for_backward(eps2, stats)
        return xp

    @staticmethod
    def backward(ctx, g):
        s, cx, ce, phi, batch = ctx.cfg
        g = _c(g)
        if not ctx.trained:  # untrained step: eps2 is a constant, the step is affine in x
            dx = torch.empty_like(g)
            kernels().unary(UN_AFFINE, g, dx, g.numel(), cx, 0.0)
            return dx, None, None, None, None, None, None, None, None
        eps2, stats = ctx.saved_tensors
        dx = torch.empty_like(g) if ctx.needs_input_grad[0] else None
        deps = torch.empty_like(eps2)
        kernels().cfg_rescale_ddpm_bwd(g, eps2, stats, dx, deps, g.numel(), s, cx, ce, phi, batch, g.numel() // batch)
        return dx, deps, None, None, None, None, None, None, None


def cfg_ddpm_step(x, eps2, z, guidance, cx, ce, sigma, rescale=0.0, batch=None):
    """x_prev = cx*x + ce*(e_u + s(e_c - e_u)) + sigma*z;  x fp32 [n], eps2 = [uncond; cond] in compute dtype.
    rescale = phi > 0 (`guidance_rescale`): the guided noise of each of the `batch` samples (contiguous runs of x) is scaled by
    phi * std(e_c) / std(e) + 1 - phi first (Lin et al., arXiv 2305.08891 s. 3.4)."""
    if rescale == 0.0:
        return _CfgDdpm.apply(x, eps2, z, float(guidance), float(cx), float(ce), float(sigma))
    if batch is None:
        raise ValueError("cfg_ddpm_step: rescaled guidance takes its statistics per sample: pass `batch`")
    return _CfgRescaleDdpm.apply(x, eps2, z, float(guidance), float(cx), float(ce), float(sigma), float(rescale), int(batch))


class _DdpmStep2(Function):
    """the step of the sampler's other modes (comat_ddpm_step2_fwd / _bwd): guidance on (halves = 2) or off (1), x_prev and / or
    the scheduler's x0 (TrainableSDPipeline.py:155-168), rescaled or not; eps and the statistics are kept only when a gradient
    will flow into eps"""

    @staticmethod
    def forward(ctx, x, eps, z, s, cx, ce, sigma, px, pe, phi, batch, halves, want_prev, want_x0):
        x, eps = _c(x), _c(eps)
        n = x.numel()
        assert x.dtype == torch.float32 and eps.numel() == halves * n and n % batch == 0
        xp = torch.empty_like(x) if want_prev else None
        x0 = torch.empty_like(x) if want_x0 else None
        stats = torch.empty((batch, 4), dtype=torch.float32, device=x.device) if phi > 0.0 else None
        kernels().ddpm_step2_fwd(x, eps, None if z is None else _c(z), xp, x0, n, halves, s, cx, ce, sigma, px, pe, phi, batch,
                                 n // batch, stats)
        ctx.cfg = (s, cx, ce, px, pe, phi, batch, halves, eps.dtype, eps.shape)
        ctx.trained = bool(ctx.needs_input_grad[1])
        if ctx.trained and phi > 0.0:
            ctx.save_for_backward(eps, stats)
        ctx.set_materialize_grads(False)
        return xp, x0

    @staticmethod
    def backward(ctx, g_prev, g_x0):
        s, cx, ce, px, pe, phi, batch, halves, edt, eshape = ctx.cfg
        if g_prev is None and g_x0 is None:
            return (None,) * 14
        g_prev, g_x0 = (None if g is None else _c(g) for g in (g_prev, g_x0))
        ref = g_prev if g_prev is not None else g_x0
        n = ref.numel()
        eps, stats = ctx.saved_tensors if (ctx.trained and phi > 0.0) else (None, None)
        dx = torch.empty_like(ref) if ctx.needs_input_grad[0] else None
        deps = torch.empty(eshape, dtype=edt, device=ref.device) if ctx.trained else None
        if dx is not None or deps is not None:
            kernels().ddpm_step2_bwd(g_prev, g_x0, eps, stats, dx, deps, n, halves, s, cx, ce, px, pe, phi, batch, n // batch,
                                     eps_dtype=edt)
        return (dx, deps) + (None,) * 12


def ddpm_step(x, eps, z, guidance, cx, ce, sigma, *, halves=2, x0_coef=None, want_prev=True, rescale=0.0, batch=None):
    """-> (x_prev | None, x0 | None): the scheduler step of the sampler's other modes as ONE op.
    halves = 2: eps = [uncond; cond] and e = e_u + s (e_c - e_u); halves = 1: guidance is off, e = eps, `guidance` is ignored and
    `rescale` must be 0.  x_prev = cx x + ce k e + sigma z (`want_prev`); x0 = px x + pe k e, the scheduler's
    `pred_original_sample`, when x0_coef = (px, pe) is given.  rescale = phi > 0: k = phi std(e_c) / std(e) + 1 - phi per sample
    (as ops.cfg_ddpm_step), shared by both outputs.  `batch`: number of samples (contiguous runs of x), each a multiple of 4 long."""
    if not want_prev and x0_coef is None:
        raise ValueError("ddpm_step: neither x_prev nor x0 is wanted")
    if halves not in (1, 2):
        raise ValueError(f"ddpm_step: halves must be 1 or 2, got {halves}")
    if halves == 1 and rescale != 0.0:
        raise ValueError("ddpm_step: guidance off (halves = 1) takes no rescale")
    if batch is None:
        if rescale != 0.0:
            raise ValueError("ddpm_step: rescaled guidance takes its statistics per sample: pass `batch`")
        batch = 1
    px, pe = (0.0, 0.0) if x0_coef is None else x0_coef
    return _DdpmStep2.apply(x, eps, z, float(guidance), float(cx), float(ce), float(sigma), float(px), float(pe), float(rescale),
                            int(batch), int(halves), bool(want_prev), x0_coef is not None)


def add_noise(x, noise, sa, sb, copies, dtype):
    """-> (noisy, xin): noisy = sa x + sb noise in fp32 and `copies` (1 or 2) stacked copies of it in `dtype`, the UNet input of
    the extra trained call of `double_laststep` (scheduler.add_noise + cat + cast, TrainableSDPipeline.py:191-195), one launch.
    No autograd: nothing in front of it carries a gradient in that mode."""
    x, noise = _c(x.detach()), _c(noise.detach())
    assert x.dtype == torch.float32 and noise.dtype == torch.float32 and x.shape == noise.shape and copies in (1, 2)
    noisy = torch.empty_like(x)
    xin = torch.empty((copies * x.shape[0],) + tuple(x.shape[1:]), dtype=dtype, device=x.device)
    kernels().add_noise_fwd(x, noise, noisy, xin, x.numel(), float(sa), float(sb), int(copies))
    return noisy, xin


# ----------------------------------------------------------------------------------------------------------------
# image path
# ----------------------------------------------------------------------------------------------------------------
class ResampleTables:
    """Device-resident sparse tap tables of a separable linear resampling operator and of its transpose."""

    def __init__(self, fwd, bwd, Hin, Win, Hout, Wout, device):
        # fwd / bwd: dicts with ystart, ywt, xstart, xwt (numpy), KT
        def put(d):
            return dict(ystart=torch.from_numpy(d["ystart"]).to(device), ywt=torch.from_numpy(d["ywt"]).to(device),
                        xstart=torch.from_numpy(d["xstart"]).to(device), xwt=torch.from_numpy(d["xwt"]).to(device),
                        KT=int(d["KT"]))
        self.fwd, self.bwd = put(fwd), put(bwd)
        self.Hin, self.Win, self.Hout, self.Wout = Hin, Win, Hout, Wout

    def static_copy(self, extra_taps=2):
        """A second table set with `extra_taps` spare (zero-weight) taps per row: the fixed-address tables that a
        captured hipGraph of the training step reads.  `load()` refills it with another crop's operator before a
        replay (the resampling kernel skips zero weights, so padded taps cost nothing)."""
        new = ResampleTables.__new__(ResampleTables)
        new.Hin, new.Win, new.Hout, new.Wout = self.Hin, self.Win, self.Hout, self.Wout

        def grow(d):
            KT = d["KT"] + extra_taps
            out = dict(ystart=d["ystart"].clone(), xstart=d["xstart"].clone(), KT=KT)
            for k in ("ywt", "xwt"):
                w = torch.zeros((d[k].shape[0], KT), dtype=d[k].dtype, device=d[k].device)
                w[:, : d["KT"]] = d[k]
                out[k] = w
            return out
        new.fwd, new.bwd = grow(self.fwd), grow(self.bwd)
        return new

    def load(self, other):
        """copy `other`'s operator into these (fixed-address) tables; raises if it needs more taps than there is room"""
        for mine, theirs in ((self.fwd, other.fwd), (self.bwd, other.bwd)):
            if theirs["KT"] > mine["KT"]:
                raise ValueError("resampling operator needs more taps than the static tables hold")
            mine["ystart"].copy_(theirs["ystart"])
            mine["xstart"].copy_(theirs["xstart"])
            for k in ("ywt", "xwt"):
                mine[k].zero_()
                mine[k][:, : theirs["KT"]] = theirs[k]


class _Resample(Function):
    @staticmethod
    def forward(ctx, img, tab, B, Cc, scale, shift, out_dtype):
        img = _c(img)
        out = torch.empty((B * tab.Hout * tab.Wout, Cc), dtype=out_dtype, device=img.device)
        t = tab.fwd
        kernels().resample2d(img, out, B, tab.Hin, tab.Win, tab.Hout, tab.Wout, Cc, t["ystart"], t["ywt"], t["xstart"],
                             t["xwt"], t["KT"], scale, shift)
        ctx.tab, ctx.B, ctx.C, ctx.scale = tab, B, Cc, scale
        ctx.in_dtype = img.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        g = _c(g)
        tab = ctx.tab
        t = tab.bwd
        dimg = torch.empty((ctx.B * tab.Hin * tab.Win, ctx.C), dtype=ctx.in_dtype, device=g.device)
        kernels().resample2d(g, dimg, ctx.B, tab.Hout, tab.Wout, tab.Hin, tab.Win, ctx.C, t["ystart"], t["ywt"],
                             t["xstart"], t["xwt"], t["KT"], ctx.scale, None)
        return dimg, None, None, None, None, None, None


def resample(img, tab: ResampleTables, B, C, scale=None, shift=None, out_dtype=None):
    """out = scale[c] * R(img) + shift[c] with R the separable resampling operator of `tab`."""
    return _Resample.apply(img, tab, B, C, scale, shift, out_dtype or img.dtype)


class _Patchify(Function):
    @staticmethod
    def forward(ctx, img, B, H, W, Cc, P):
        img = _c(img)
        out = img.new_empty((B * (H // P) * (W // P), P * P * Cc))
        kernels().patchify(img, out, B, H, W, Cc, P, False)
        ctx.cfg = (B, H, W, Cc, P)
        return out

    @staticmethod
    def backward(ctx, g):
        B, H, W, Cc, P = ctx.cfg
        g = _c(g)
        dimg = g.new_empty((B * H * W, Cc))
        kernels().patchify(dimg, g, B, H, W, Cc, P, True)
        return dimg, None, None, None, None, None


def patchify(img, B, H, W, C, P):
    return _Patchify.apply(img, B, H, W, C, P)


def embedding(ids, table):
    """rows of a frozen table (no gradient)."""
    ids = _c(ids.reshape(-1))
    out = table.new_empty((ids.numel(), table.shape[1]))
    kernels().embedding(ids, table, out, ids.numel(), table.shape[1], table.shape[0])
    return out


def table_kernels():
    """who runs embed_fwd / embed_grad (comat_embed_fwd / comat_embed_grad): the installed backend where it has them (the
    simulator of tests/clip_tune_sim.py), else the binding's module functions - which refuse anything that is not in HBM"""
    from . import _hip
    k = kernels()
    return k if hasattr(k, "embed_fwd") else _hip


def pool_kernels():
    """who runs eos_pool (comat_eos_pool): the installed backend where it has the entry point (the simulator of
    tests/clip2_sim.py), else the binding's module function - as table_kernels()"""
    from . import _hip
    k = kernels()
    return k if hasattr(k, "eos_pool") else _hip


def eos_pool(ids, h, gamma, beta, L, eos_id, eps=1e-5):
    """the pooled row of a text tower with a projection: LayerNorm(h[b * L + eos_pos(b)]) -> [B, C] in ONE launch, eos_pos by
    transformers' rule for `eos_id` (include/comat_hip.h: comat_eos_pool).  ids [B, L] int64, h [B * L, C] the last layer's output.
    Forward only: the tower it serves is frozen in the reference (training_utils/pipeline.py:119,173-174)."""
    if h.requires_grad:
        raise NotImplementedError("ops.eos_pool: the backward is not built (the second text tower is frozen); h requires grad")
    B = ids.numel() // L
    if ids.numel() != B * L or h.dim() != 2 or h.shape[0] != B * L:
        raise ValueError(f"ops.eos_pool: ids {tuple(ids.shape)} and h {tuple(h.shape)} do not fit L = {L}")
    ids, h = _c(ids.reshape(B, L)), _c(h.detach())
    out = h.new_empty((B, h.shape[1]))
    pool_kernels().eos_pool(ids, h, gamma, beta, out, None, B, L, h.shape[1], int(eos_id), float(eps))
    return out


def image_kernels():
    """who runs image_u8 (comat_image_u8): the installed backend where it has the entry point (the simulator of
    tests/validate_sim.py), else the binding's module function - as pool_kernels()"""
    from . import _hip
    k = kernels()
    return k if hasattr(k, "image_u8") else _hip


def sheet_shape(B, H, W, cols, pad):
    """(rows, columns) in pixels of the contact sheet comat_image_u8 places B images of H x W on, `cols` a row, `pad` pixels around
    and between them"""
    rows = -(-B // cols)
    return pad + rows * (H + pad), pad + min(B, cols) * (W + pad)


def image_u8(tokens, B, H, W, denormalize=True, out=None, cols=1, pad=0, bad=None):
    """image tokens [B * H * W, C] (fp32 or bf16, C 1 .. 4) -> bytes in ONE launch (include/comat_hip.h: comat_image_u8):
    `denormalize` takes the raw VAE decode (x / 2 + 0.5 first), else an image already in [0, 1].  out = None: a fresh uint8
    [B, H, W, C].  out = a contiguous uint8 sheet [Hs, Ws, C] of at least sheet_shape(B, H, W, cols, pad): the images are placed on
    it, `cols` a row and `pad` pixels apart, its other bytes stay.  bad: int32 [B], zeroed by the caller; 1 is stored where an image
    holds a non-finite value.  No autograd: the tokens are detached.  -> out"""
    if tokens.dim() != 2 or tokens.shape[0] != B * H * W:
        raise ValueError(f"ops.image_u8: tokens {tuple(tokens.shape)} do not fit B, H, W = {B}, {H}, {W}")
    C = tokens.shape[1]
    x = _c(tokens.detach())
    if out is None:
        if cols != 1 or pad != 0:
            raise ValueError("ops.image_u8: cols / pad place the images on a sheet: pass it as `out`")
        out = torch.empty((B, H, W, C), dtype=torch.uint8, device=x.device)
        pitch = W * C
    else:
        if cols < 1 or pad < 0:
            raise ValueError(f"ops.image_u8: cols = {cols} must be >= 1 and pad = {pad} >= 0")
        need = sheet_shape(B, H, W, cols, pad)
        if (out.dtype != torch.uint8 or out.dim() != 3 or not out.is_contiguous() or out.shape[2] != C or out.device != x.device
                or out.shape[0] < need[0] or out.shape[1] < need[1]):
            raise ValueError(f"ops.image_u8: out must be a contiguous uint8 sheet of at least {need + (C,)} on {x.device}, got "
                             f"{out.dtype} {tuple(out.shape)} on {out.device}")
        pitch = out.shape[1] * C
    if bad is not None and (bad.dtype != torch.int32 or bad.numel() < B or not bad.is_contiguous()):
        raise ValueError(f"ops.image_u8: bad must be a contiguous int32 [{B}], got {bad.dtype} {tuple(bad.shape)}")
    image_kernels().image_u8(x, out, bad, B, H, W, C, bool(denormalize), pitch, cols, pad)
    return out


def denoise_kernels():
    """who runs denoise_prepare / mse_fwd / mse_bwd (comat_denoise_prepare, comat_mse_fwd, comat_mse_bwd): the installed backend
    where it has the entry points (the simulator of tests/denoise_sim.py), else the binding's module functions - as image_kernels()"""
    from . import _hip
    k = kernels()
    return k if hasattr(k, "denoise_prepare") else _hip


class DenoiseTables:
    """the three per-timestep tables comat_denoise_prepare reads, on the device, built once by the host: sab [T, 2] (the
    scheduler's add-noise coefficients rounded to fp32), sinus [T, C0] (row t: the timestep embedding of t), wtab [T] (loss weights)"""

    def __init__(self, sab, sinus, wtab, device):
        f = lambda a: torch.as_tensor(a, dtype=torch.float32).contiguous().to(device)
        self.sab, self.sinus, self.wtab = f(sab), f(sinus), f(wtab)
        self.T, self.C0 = self.sinus.shape
        if self.sab.shape != (self.T, 2) or self.wtab.shape != (self.T,):
            raise ValueError(f"ops.DenoiseTables: sab {tuple(self.sab.shape)}, sinus {tuple(self.sinus.shape)}, wtab "
                             f"{tuple(self.wtab.shape)} do not describe the same T timesteps")


def denoise_prepare(tab: DenoiseTables, t, noise, dtype, *, moments=None, z=None, latents=None, scaling=1.0, want_x0=False,
                    oob=None):
    """the UNet input of a noise-prediction step in ONE launch (include/comat_hip.h: comat_denoise_prepare).  Source: `moments`
    [B * P, 2 C] of the VAE encoder (sampled with z, the mean without) times `scaling`, or `latents` fp32 [B * P, C] as given.
    t int32 [B] and noise fp32 [B * P, C] live on the device.  No autograd (nothing in front of the UNet is trained).
    -> (xin [B * P, C] in `dtype`, temb fp32 [B, C0], w fp32 [B], x0 fp32 or None)"""
    B = t.numel()
    noise = _c(noise.detach())
    n, C = noise.shape
    if (moments is None) == (latents is None):
        raise ValueError("ops.denoise_prepare: exactly one of moments and latents")
    if n % B:
        raise ValueError(f"ops.denoise_prepare: noise {tuple(noise.shape)} does not divide into {B} samples")
    src = moments if latents is None else latents
    if src.dim() != 2 or src.shape != (n, 2 * C if latents is None else C) or (z is not None and z.shape != noise.shape):
        raise ValueError(f"ops.denoise_prepare: source {tuple(src.shape)} / z do not fit noise {tuple(noise.shape)}")
    dev = noise.device
    xin = torch.empty((n, C), dtype=dtype, device=dev)
    temb = torch.empty((B, tab.C0), dtype=torch.float32, device=dev)
    w = torch.empty(B, dtype=torch.float32, device=dev)
    x0 = torch.empty((n, C), dtype=torch.float32, device=dev) if want_x0 else None
    det = lambda a: None if a is None else _c(a.detach())
    denoise_kernels().denoise_prepare(det(moments), det(z), det(latents), noise, _c(t), tab.sab, tab.sinus, tab.wtab, xin, x0, temb, w,
                                      oob, float(scaling), tab.T, B, n // B, C, tab.C0)
    return xin, temb, w, x0


class _MseLoss(Function):
    """mean over the batch of w_b times the per-sample mean squared error (comat_mse_fwd / comat_mse_bwd); the gradient arriving
    at the loss is read by the kernel from the device, the target and the weights carry none"""

    @staticmethod
    def forward(ctx, pred, target, w, B):
        pred, target = _c(pred), _c(target)
        n = pred.numel() // B
        per_sample = torch.empty(B, dtype=torch.float32, device=pred.device)
        loss = torch.empty(1, dtype=torch.float32, device=pred.device)
        denoise_kernels().mse_fwd(pred, target, w, per_sample, loss, B, n)
        ctx.save_for_backward(pred, target, w)
        ctx.geo = (B, n)
        ctx.mark_non_differentiable(per_sample)
        return loss, per_sample

    @staticmethod
    def backward(ctx, g, _):
        pred, target, w = ctx.saved_tensors
        B, n = ctx.geo
        dpred = torch.empty_like(pred)
        denoise_kernels().mse_bwd(pred, target, w, _c(g.float()).reshape(1), dpred, B, n)
        return dpred, None, None, None


def mse_loss(pred, target, B, w=None):
    """(loss [1], per_sample [B]) of F.mse_loss(pred.float(), target) with per-sample weights w [B] (None: 1); pred fp32 or bf16
    [B * P, C] (any shape of B equal samples), target fp32 of the same shape"""
    if pred.shape != target.shape or pred.numel() % B or target.dtype != torch.float32:
        raise ValueError(f"ops.mse_loss: pred {tuple(pred.shape)} {pred.dtype} and target {tuple(target.shape)} {target.dtype} do not "
                         f"fit {B} samples (target is fp32)")
    return _MseLoss.apply(pred, target.detach(), None if w is None else _c(w.detach()), B)


class TrainableEmbedding:
    """The two tables of a text tower that is trained in full (`--tune_text_encoder`): `tok` [vocab, dim] and `pos` [max_pos, dim]
    are views of the owner's fp32 MASTER (the forward reads them and rounds once: no compute-dtype copy of the 38 M-element token
    table, nothing to refresh), `tok_grad` / `pos_grad` fp32 views of its flat gradient, `gate` the owner's gate."""

    trainable = True

    def __init__(self, tok, tok_grad, pos, pos_grad):
        self.tok, self.tok_grad, self.pos, self.pos_grad = tok, tok_grad, pos, pos_grad
        self.requires_grad = True
        self._pos_ids = {}

    def pos_ids(self, n, L):
        """i mod L for i < n as a device tensor, built once per (n, L): the ids of the position table's gradient launch"""
        t = self._pos_ids.get((n, L))
        if t is None:
            t = self._pos_ids[(n, L)] = (torch.arange(n, dtype=torch.int64) % L).to(self.tok.device)
        return t


class _TrainedEmbedding(Function):
    """out[i] = cast(tok[ids[i]] + pos[i mod L]) in one launch; backward: the two tables' gradients, one comat_embed_grad launch
    each over the same dy, accumulated into the owner's flat gradient.  The ids carry no gradient: the node runs in the backward
    pass through the owner's gate (gate_of), as every trained node whose data input carries none."""

    @staticmethod
    def forward(ctx, ids, emb, L, dtype, gate=None):
        n, (vocab, dim) = ids.numel(), emb.tok.shape
        out = torch.empty((n, dim), dtype=dtype, device=ids.device)
        table_kernels().embed_fwd(ids, emb.tok, emb.pos, out, n, L, dim, vocab)
        ctx.emb, ctx.L = emb, L
        ctx.wg = trains(emb, ctx)
        if ctx.wg:
            ctx.save_for_backward(ids)
        return out

    @staticmethod
    def backward(ctx, g):
        if ctx.wg:
            g, emb, (ids,) = _c(g), ctx.emb, ctx.saved_tensors
            n, dim, k = ids.numel(), emb.tok.shape[1], table_kernels()
            pos_ids = emb.pos_ids(n, ctx.L)
            for a in range(0, n, EMBED_GRAD_MAX_N):  # one launch takes that many ids: more (bs > 26 at 77 tokens) go in slices,
                b = min(n, a + EMBED_GRAD_MAX_N)     # each slice's sum added to the row in turn - still one fixed order
                k.embed_grad(ids[a:b], g[a:b], emb.tok_grad, b - a, dim, emb.tok.shape[0])
                k.embed_grad(pos_ids[a:b], g[a:b], emb.pos_grad, b - a, dim, emb.pos.shape[0])
        return None, None, None, None, None


def trained_embedding(ids, emb: TrainableEmbedding, L, dtype):
    """token + position embedding of ids [B * L] (int64) from trained fp32 tables -> [B * L, dim] of `dtype`"""
    if L > emb.pos.shape[0]:
        raise ValueError(f"{L} tokens, the position table has {emb.pos.shape[0]}")
    return _TrainedEmbedding.apply(_c(ids.reshape(-1)), emb, L, dtype, gate_of(emb))


class _Permute(Function):
    @staticmethod
    def forward(ctx, x, B, Cc, H, W, to_nhwc, out_dtype):
        x = _c(x)
        y = torch.empty(((B * H * W, Cc) if to_nhwc else (B, Cc, H, W)), dtype=out_dtype, device=x.device)
        kernels().permute_nchw_nhwc(x, y, B, Cc, H, W, to_nhwc)
        ctx.cfg = (B, Cc, H, W, to_nhwc, x.dtype)
        return y

    @staticmethod
    def backward(ctx, g):
        B, Cc, H, W, to_nhwc, xdt = ctx.cfg
        g = _c(g)
        dx = torch.empty(((B, Cc, H, W) if to_nhwc else (B * H * W, Cc)), dtype=xdt, device=g.device)
        kernels().permute_nchw_nhwc(g, dx, B, Cc, H, W, not to_nhwc)
        return dx, None, None, None, None, None, None


def nchw_to_tokens(x, out_dtype=None):
    B, Cc, H, W = x.shape
    return _Permute.apply(x, B, Cc, H, W, True, out_dtype or x.dtype)


def tokens_to_nchw(x, B, H, W, out_dtype=None):
    return _Permute.apply(x, B, x.shape[1], H, W, False, out_dtype or x.dtype)


# ----------------------------------------------------------------------------------------------------------------
# losses
# ----------------------------------------------------------------------------------------------------------------
class _CrossEntropy(Function):
    @staticmethod
    def forward(ctx, logits, labels, ignore_index, ls):
        logits = _c(logits)
        T, V = logits.shape
        dev = logits.device
        logp = torch.empty((T,), dtype=torch.float32, device=dev)
        lse = torch.empty((T,), dtype=torch.float32, device=dev)
        acc = torch.empty((2,), dtype=torch.float32, device=dev)
        kernels().cross_entropy_fwd(logits, labels, logp, lse, acc, T, V, V, ignore_index, ls)
        ctx.save_for_backward(logits, labels, lse, acc)
        ctx.cfg = (ignore_index, ls)
        ctx.mark_non_differentiable(logp)
        # (a batch without a valid row: loss 0, like the backward kernel's max(count, 1), not 0 / 0)
        return acc[0] / acc[1].clamp(min=1.0), logp

    @staticmethod
    def backward(ctx, g, _):
        logits, labels, lse, acc = ctx.saved_tensors
        ignore_index, ls = ctx.cfg
        T, V = logits.shape
        dl = torch.empty_like(logits)
        g_up = _c(g.reshape(1).to(torch.float32))  # device scalar: no host sync in the middle of backward
        kernels().cross_entropy_bwd(logits, labels, lse, dl, T, V, V, ignore_index, ls, g_up, acc)
        return dl, None, None, None


def cross_entropy(logits, labels, ignore_index=-100, label_smoothing=0.0):
    """mean token CE over labels != ignore_index.  Returns (loss, per-token log-prob of the label)."""
    return _CrossEntropy.apply(logits, labels, int(ignore_index), float(label_smoothing))


class _DiscHead(Function):
    @staticmethod
    def forward(ctx, x, w, b, target, pix_per_sample):
        x = _c(x)
        P = x.shape[0]
        assert x.shape[1] == 4
        loss = torch.empty((1,), dtype=torch.float32, device=x.device)
        kernels().disc_head_fwd(x, w, b, target, loss, P, pix_per_sample)
        ctx.save_for_backward(x, w, b, target)
        ctx.pps = pix_per_sample
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        x, w, b, target = ctx.saved_tensors
        P = x.shape[0]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dwb = dw = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dwb = torch.zeros((5,), dtype=torch.float32, device=x.device)
            dw, db = dwb[:4], dwb[4:]
        kernels().disc_head_bwd(x, w, b, target, _c(g.reshape(1).to(torch.float32)), dx, dwb, P, ctx.pps)
        return dx, dw, db, None, None


def disc_head_loss(x, w, b, target, pix_per_sample):
    """mean BCE-with-logits of Linear(4,1)(x) against target[pixel // pix_per_sample] (gan_sdxl.py:83-88)."""
    return _DiscHead.apply(x, w, b, target, int(pix_per_sample))


class _DiscConvHead(Function):
    @staticmethod
    def forward(ctx, x, w, b, target, B, H, W):
        x = _c(x)
        P, Cc = x.shape
        assert P == B * H * W and tuple(w.shape) == (9, Cc), (tuple(x.shape), tuple(w.shape), B, H, W)
        z = torch.empty((P,), dtype=torch.float32, device=x.device)
        loss = torch.empty((1,), dtype=torch.float32, device=x.device)
        kernels().disc_convhead_fwd(x, w, b, target, z, loss, B, H, W, Cc)
        ctx.save_for_backward(x, w, z, target)
        ctx.cfg = (B, H, W)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        x, w, z, target = ctx.saved_tensors
        B, H, W = ctx.cfg
        Cc = x.shape[1]
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dwb = dw = db = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dwb = torch.zeros((9 * Cc + 1,), dtype=torch.float32, device=x.device)
            dw, db = dwb[:9 * Cc].view(9, Cc), dwb[9 * Cc:]
        if dx is not None or dwb is not None:
            kernels().disc_convhead_bwd(x, w, z, target, _c(g.reshape(1).to(torch.float32)), dx, dwb, B, H, W, Cc)
        return dx, dw, db, None, None, None, None


def disc_convhead_loss(x, w9c, b, target, B, H, W):
    """mean BCE-with-logits of Conv2d(C, 1, 3, padding=1)(x) against target[sample] (gan_sdxl.py:27-30,81-88 with
    --gan_unet_lastlayer_cls).  x: [B*H*W, C] tokens; w9c: fp32 [9, C], the Conv2d weight [1, C, 3, 3] tap-major
    (conv_weight_to_taps); b fp32 [1]; target fp32 [B]."""
    return _DiscConvHead.apply(x, w9c, b, target, int(B), int(H), int(W))


def conv_weight_to_taps(w):
    """Conv2d weight [1, C, 3, 3] -> tap-major [9, C] (tap = ky * 3 + kx), the layout of comat_disc_convhead_*"""
    assert w.dim() == 4 and w.shape[0] == 1 and tuple(w.shape[2:]) == (3, 3), tuple(w.shape)
    return w[0].permute(1, 2, 0).reshape(9, w.shape[1]).contiguous()


def taps_to_conv_weight(w9c):
    """tap-major [9, C] -> Conv2d weight [1, C, 3, 3]"""
    return w9c.reshape(3, 3, -1).permute(2, 0, 1).unsqueeze(0).contiguous()


class _AttnMapGather(Function):
    @staticmethod
    def forward(ctx, amap, mask, tok_idx, tok_obj):
        amap = _c(amap)
        H, npix, L = amap.shape
        n_tok = tok_idx.numel()
        dev = amap.device
        num = torch.zeros((H, n_tok), dtype=torch.float32, device=dev)
        den = torch.zeros((H, n_tok), dtype=torch.float32, device=dev)
        avg = torch.zeros((n_tok, npix), dtype=torch.float32, device=dev)
        kernels().attnmap_gather_fwd(amap, mask, tok_idx, tok_obj, num, den, avg, H, npix, L, n_tok)
        ctx.save_for_backward(mask, tok_idx, tok_obj)
        ctx.cfg = (H, npix, L, n_tok, amap.dtype)
        return num, den, avg

    @staticmethod
    def backward(ctx, g_num, g_den, g_avg):
        mask, tok_idx, tok_obj = ctx.saved_tensors
        H, npix, L, n_tok, adt = ctx.cfg
        dev = mask.device
        z = lambda t, shape: torch.zeros(shape, dtype=torch.float32, device=dev) if t is None else _c(t)
        g_num, g_den = z(g_num, (H, n_tok)), z(g_den, (H, n_tok))
        g_avg = None if g_avg is None else _c(g_avg)
        damap = torch.empty((H, npix, L), dtype=adt, device=dev)  # the kernel writes every element
        kernels().attnmap_gather_bwd(g_num, g_den, g_avg, mask, tok_idx, tok_obj, damap, H, npix, L, n_tok)
        return damap, None, None, None


def attnmap_gather(amap, mask, tok_idx, tok_obj):
    """amap [heads, npix, L] -> (num [heads, n_tok], den [heads, n_tok], avg [n_tok, npix])."""
    return _AttnMapGather.apply(amap, mask, tok_idx, tok_obj)


def attrcon_kernels():
    """who runs mask_resize_any / attrcon_* (comat_mask_resize_any, comat_attrcon_*): the installed backend where it has them (the
    simulator of tests/attrcon_sim.py), else the binding's module functions - which refuse anything that is not in HBM"""
    from . import _hip
    k = kernels()
    return k if hasattr(k, "attrcon_loss") else _hip


class AttrconTables:
    """The ragged per-sample tables of one step's attribute-concentration loss, in device memory (include/comat_hip.h):
    n_obj, n_tok int32 [bs]; tok_idx, tok_obj int32 [bs, TOK]; inv_len fp32 [bs, TOK]; OBJ, TOK the batch's maxima"""

    def __init__(self, n_obj, n_tok, tok_idx, tok_obj, inv_len, bs, OBJ, TOK):
        self.n_obj, self.n_tok, self.tok_idx, self.tok_obj, self.inv_len = n_obj, n_tok, tok_idx, tok_obj, inv_len
        self.bs, self.OBJ, self.TOK = bs, OBJ, TOK


class _AttrconLayerLoss(Function):
    """The M captured maps [bs * heads, npix, L] of one (timestep, layer) -> (token loss, pixel loss) of the batch, both already
    divided by bs: M comat_attrcon_gather_fwd calls and one comat_attrcon_loss, which also leaves the derivatives of the two
    scalars; the backward is one comat_attrcon_gather_bwd per map, scaled by the two upstream gradients on the device."""

    @staticmethod
    def forward(ctx, tab, masks_res, *maps):
        k = attrcon_kernels()
        maps = [_c(m) for m in maps]
        M, (BH, npix, L), dev = len(maps), maps[0].shape, maps[0].device
        bs, OBJ, TOK = tab.bs, tab.OBJ, tab.TOK
        heads = BH // bs
        nd, av = bs * heads * TOK, bs * TOK * npix
        nws = k.attrcon_workspace_floats(M, bs, heads, npix, TOK)
        # one zero-filled buffer: num, den, g_num, g_den [M, bs, heads, TOK] | avg, g_avg [bs, TOK, npix] | out [2] | workspace
        buf = torch.zeros(4 * M * nd + 2 * av + 2 + nws, dtype=torch.float32, device=dev)
        num, den, g_num, g_den = (buf[i * M * nd:(i + 1) * M * nd].view(M, bs, heads, TOK) for i in range(4))
        o = 4 * M * nd
        avg, g_avg = buf[o:o + av].view(bs, TOK, npix), buf[o + av:o + 2 * av].view(bs, TOK, npix)
        out, ws = buf[o + 2 * av:o + 2 * av + 2], buf[o + 2 * av + 2:]
        for m, a in enumerate(maps):
            k.attrcon_gather_fwd(a, masks_res, tab.n_obj, tab.n_tok, tab.tok_idx, tab.tok_obj, num[m], den[m], avg, ws, bs, heads,
                                 npix, L, OBJ, TOK)
        k.attrcon_loss(num, den, avg, masks_res, tab.n_obj, tab.n_tok, tab.tok_obj, tab.inv_len, g_num, g_den, g_avg, out, ws, M,
                       bs, heads, npix, OBJ, TOK)
        ctx.tab, ctx.cfg = tab, (M, bs, heads, npix, L, maps[0].dtype)
        ctx.save_for_backward(masks_res, g_num, g_den, g_avg)
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_tl, g_pl):
        k, tab = attrcon_kernels(), ctx.tab
        masks_res, g_num, g_den, g_avg = ctx.saved_tensors
        M, bs, heads, npix, L, adt = ctx.cfg
        z = lambda t: torch.zeros((), dtype=torch.float32, device=masks_res.device) if t is None else t.float()
        go = torch.stack([z(g_tl), z(g_pl)])
        grads = []
        for m in range(M):
            damap = torch.empty((bs * heads, npix, L), dtype=adt, device=masks_res.device)  # the kernel writes every element
            k.attrcon_gather_bwd(g_num[m], g_den[m], g_avg, masks_res, tab.n_obj, tab.n_tok, tab.tok_idx, tab.tok_obj, go, damap,
                                 bs, heads, npix, L, tab.OBJ, tab.TOK)
            grads.append(damap)
        return (None, None, *grads)


def attrcon_layer_loss(tab: AttrconTables, masks_res, maps):
    """maps: the captured [bs * heads, npix, L] maps of one (timestep, layer); masks_res fp32 [bs, OBJ, npix] -> (token, pixel)"""
    return _AttrconLayerLoss.apply(tab, masks_res, *maps)
