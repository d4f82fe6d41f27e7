"""CPU simulator of the libcomat_hip C ABI — TEST INFRASTRUCTURE ONLY.

It implements, with plain torch CPU ops, the documented semantics of every entry point in include/comat_hip.h
(same argument lists as comat_amd._hip.HipKernels).  tests/ plug it in through
`comat_amd.ops.set_kernel_backend(SimKernels())` to exercise the host logic (operator wiring, model assembly,
gradient gating, the step graph, the 2-rank gloo path) on machines without a GPU.  The product never imports it.

The methods are grouped by the part of the header they restate.  Where the header lists COMAT_EINVAL cases the simulator refuses
them as `_hip._check` does: a RuntimeError that names the entry point (`_refuse`).  tests/test_abi.py holds the argument lists to
those of HipKernels.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import fp8 as OF

ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2
UN_COPY, UN_SILU, UN_GELU, UN_AFFINE = 0, 1, 2, 3
CONSTANT, CONSTANT_WITH_WARMUP, LINEAR, COSINE, COSINE_WITH_RESTARTS, POLYNOMIAL = range(6)  # comat_lr_schedule::kind
TINY = 2.0 ** -100


def _v(t, sizes, strides):
    return torch.as_strided(t, sizes, strides, t.storage_offset())


def _sub(flat, shape, ld, off):
    """the [rows, cols] matrix at element `off` of a flat tensor, row pitch ld"""
    return torch.as_strided(flat, shape, (ld, 1), flat.storage_offset() + off)


def _refuse(name, cond, msg):
    if not cond:
        raise RuntimeError(f"{name} failed (rc=-1): {name}: {msg}")


def _check_schedule(name, s):
    _refuse(name, CONSTANT <= s.kind <= POLYNOMIAL, f"unknown schedule kind {s.kind}")
    _refuse(name, s.stride >= 1 and s.warmup >= 0, f"stride must be >= 1 and warmup >= 0 (got {s.stride}, {s.warmup})")
    _refuse(name, s.kind < LINEAR or s.total >= 1, f"this kind needs total >= 1 (got {s.total})")
    _refuse(name, s.kind != POLYNOMIAL or s.base_lr > s.lr_end, "polynomial needs base_lr > lr_end")


def lr_at(s, applied):
    """the rate after `applied` updates: (float32)(base_lr * multiplier(stride * applied)), the multiplier in doubles"""
    c, W, T = s.stride * int(applied), s.warmup, s.total
    lam = 1.0
    if s.kind != CONSTANT:
        span = float(max(1, T - W))
        if c < W:
            lam = float(c) / float(max(1, W))
        elif s.kind == LINEAR:
            lam = max(0.0, float(T - c) / span)
        elif s.kind == COSINE:
            lam = max(0.0, 0.5 * (1.0 + math.cos(math.pi * s.num_cycles * 2.0 * (float(c - W) / span))))
        elif s.kind == COSINE_WITH_RESTARTS:
            progress = float(c - W) / span
            lam = 0.0 if progress >= 1.0 else max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((s.num_cycles * progress) % 1.0))))
        elif s.kind == POLYNOMIAL:
            if c > T:
                lam = s.lr_end / s.base_lr
            else:
                pct = 1.0 - float(c - W) / float(T - W) if T != W else float("nan")  # 0 / 0 at c == T == W, as on the device
                lam = ((s.base_lr - s.lr_end) * pct ** s.power + s.lr_end) / s.base_lr
    return float(np.float32(s.base_lr * lam))


def _f(t, scale=None):
    """operand -> fp32 values; uint8 tensors hold fp8 e4m3 bytes (value = scale * fp8)"""
    if t.dtype == torch.uint8:
        return t.view(torch.float8_e4m3fn).float() * scale.float()
    return t.float()


def _lse(s):
    """m + log(sum exp(s - m)) over the last axis, as the kernels evaluate it: a +Inf entry gives NaN (inf - inf), where
    torch.logsumexp answers +Inf - the log-sum-exp CARRIES a non-finite score (include/comat_hip.h, non-finite values)"""
    m = s.max(-1, keepdim=True).values
    return (m + torch.log(torch.exp(s - m).sum(-1, keepdim=True)))[..., 0]


def _act(x, act):
    if act == ACT_SILU:
        return F.silu(x)
    if act == ACT_GELU:
        return F.gelu(x)
    return x


class SimKernels:
    name = "sim"

    # ---- contraction ---------------------------------------------------------------------------------------
    def gemm(self, A, B, Cout, M, N, K, lda, ldb, ldc, transA=False, transB=False, batch=(1, 1), sA=(0, 0),
             sB=(0, 0), sC=(0, 0), bias=None, bias2=None, rows_per_bias2=0, R=None, ldr=0, sR=(0, 0), alpha=1.0,
             beta=0.0, act=ACT_NONE, scales=None, geglu=None, tail=None, ktail=None, q8=None):
        b1, b2 = batch
        if tail is not None:  # comat_gemm_params::epi2 = 4: the last n2 columns are alpha2 * A B2^T into C2, the rest as usual
            B2, C2t, n2, ldc2, sB2t, sC2t, alpha2 = tail
            assert geglu is None and not transA and not transB and b2 == 1 and 0 < n2 < N
            self.gemm(A, B, Cout, M, N - n2, K, lda, ldb, ldc, batch=batch, sA=sA, sB=sB, sC=sC, bias=bias, bias2=bias2,
                      rows_per_bias2=rows_per_bias2, R=R, ldr=ldr, sR=sR, alpha=alpha, beta=beta, act=act, scales=scales)
            self.gemm(A, B2, C2t, M, n2, K, lda, ldb, ldc2, batch=batch, sA=sA, sB=(sB2t, 0), sC=(sC2t, 0), alpha=alpha2,
                      scales=scales)
            return
        assert (scales is not None) == (A.dtype == torch.uint8)
        if scales is not None:
            assert not transA and not transB and K % 64 == 0 and lda % 16 == 0 and ldb % 16 == 0 and b2 == 1
        sa, sb = scales[:2] if scales is not None else (None, None)
        if scales is not None and len(scales) > 2 and scales[2] and b1 > 1:  # per-batch scale of B (comat_gemm_params::s_scale_b)
            sb = torch.as_strided(sb, (b1, 1, 1, 1), (scales[2], 0, 0, 0), sb.storage_offset())
        Av = _v(A, (b1, b2, M, K), (sA[0], sA[1], 1, lda) if transA else (sA[0], sA[1], lda, 1))
        Bv = _v(B, (b1, b2, N, K), (sB[0], sB[1], 1, ldb) if transB else (sB[0], sB[1], ldb, 1))
        prod = _f(Av, sa) @ _f(Bv, sb).transpose(-1, -2)
        if ktail is not None:  # comat_gemm_params::A2k: bf16 k-tail on top of the scaled fp8 product
            A2, B2, K2, lda2, ldb2, sA2, sB2 = ktail
            assert scales is not None and K2 % 16 == 0 and geglu is None and b2 == 1
            prod = prod + _v(A2, (b1, b2, M, K2), (sA2, 0, lda2, 1)).float() @ _v(B2, (b1, b2, N, K2), (sB2, 0, ldb2, 1)).float().transpose(-1, -2)
        acc = alpha * prod
        if bias is not None:
            acc = acc + bias.float()
        if bias2 is not None:
            acc = acc + bias2.float().repeat_interleave(rows_per_bias2, 0)[:M]
        acc = _act(acc, act)
        if R is not None and beta != 0:  # beta == 0: R is not read
            acc = acc + beta * _v(R, (b1, b2, M, N), (sR[0], sR[1], ldr, 1)).float()
        if geglu is not None and geglu[1] == "bwd":  # epi2 = 3: dF (rounded) -> gradient of the interleaved pre-activations
            pre = geglu[0]
            assert b1 == b2 == 1 and N % 16 == 0 and R is None and act == ACT_NONE and bias is None and bias2 is None
            dF = acc.reshape(M, N).to(pre.dtype)
            self.geglu_il_bwd(dF, pre, Cout, M, N)
            return
        if geglu is not None:  # comat_gemm_params::epi2: value / gate columns interleaved in sixteens, both rounded first
            y, keep = geglu
            assert b1 == b2 == 1 and N % 32 == 0 and R is None and act == ACT_NONE and bias2 is None
            assert y is not None or q8 is not None
            pre = acc.reshape(M, N).to(torch.bfloat16 if y is None else y.dtype)
            if keep:
                _v(Cout, (M, N), (ldc, 1)).copy_(pre)
            t = pre.float().reshape(M, N // 32, 2, 16)
            out = (t[:, :, 0] * F.gelu(t[:, :, 1])).reshape(M, N // 2).to(pre.dtype)
            if y is not None:
                y.copy_(out)
            if q8 is not None:  # comat_gemm_params::q8: the e4m3 bytes of the rounded product + its abs-max
                self._quantize_scaled(out, q8[1], q8[2], out=q8[0])
            return
        _v(Cout, (b1, b2, M, N), (sC[0], sC[1], ldc, 1)).copy_(acc.to(Cout.dtype))

    @staticmethod
    def geglu_gemm_ok(x, w, M, N, K):
        return N % 32 == 0 and M >= 1

    def geglu_il_fwd(self, x, y, M, D):
        t = x.float().reshape(M, D // 16, 2, 16)
        y.copy_((t[:, :, 0] * F.gelu(t[:, :, 1])).reshape(M, D).to(y.dtype))

    def geglu_il_bwd(self, dy, x, dx, M, D):
        t = x.float().detach().reshape(M, D // 16, 2, 16).requires_grad_(True)
        with torch.enable_grad():
            out = (t[:, :, 0] * F.gelu(t[:, :, 1])).reshape(M, D)
            (g,) = torch.autograd.grad(out, t, dy.float())
        dx.copy_(g.reshape(M, 2 * D).to(dx.dtype))

    def gemm_segments(self, segs, Cout, M, N, ldc, bias=None, R=None, ldr=0, alpha=1.0, beta=0.0, batch=1, sC=0, sR=0):
        acc = torch.zeros((batch, M, N), dtype=torch.float32)
        for sg in segs:
            A, B, K, lda, ldb = sg[:5]
            sA, sB = (sg[5], sg[6]) if len(sg) > 5 else (0, 0)
            acc = acc + _v(A, (batch, M, K), (sA, lda, 1)).float() @ _v(B, (batch, N, K), (sB, ldb, 1)).float().transpose(1, 2)
        acc = alpha * acc
        if bias is not None:
            acc = acc + bias.float().reshape(batch, 1, N)
        if R is not None and beta != 0:  # beta == 0: R is not read
            acc = acc + beta * _v(R, (batch, M, N), (sR, ldr, 1)).float()
        _v(Cout, (batch, M, N), (sC, ldc, 1)).copy_(acc.to(Cout.dtype))

    @staticmethod
    def tt_group_ok(A, B, Cacc, M, N, K, lda, ldb, ldc):
        return (A.dtype == torch.bfloat16 and B.dtype == torch.bfloat16 and Cacc.dtype == torch.float32
                and M >= 8 and N >= 8 and K >= 1 and M % 8 == 0 and N % 8 == 0 and lda % 8 == 0 and ldb % 8 == 0
                and ldc % 4 == 0)

    def gemm_tt_grouped(self, problems):
        ptrs = [p[2].data_ptr() for p in problems]
        assert len(set(ptrs)) == len(ptrs), "comat_gemm_tt_grouped: the outputs of one call must not overlap"
        for A, B, Cacc, M, N, K, lda, ldb, ldc in problems:
            assert self.tt_group_ok(A, B, Cacc, M, N, K, lda, ldb, ldc)
            Cv = _v(Cacc, (M, N), (ldc, 1))
            Cv.add_(_v(A, (M, K), (1, lda)).float() @ _v(B, (K, N), (ldb, 1)).float())

    def transpose_cast_tiles(self, src, dst, tiles):
        sf, df = src.reshape(-1), dst.reshape(-1)
        for so, do, rows, cols, r0, c0 in tiles.tolist():
            r1, c1 = min(r0 + 32, rows), min(c0 + 32, cols)
            blk = sf[so:so + rows * cols].view(rows, cols)[r0:r1, c0:c1]
            df[do:do + rows * cols].view(cols, rows)[c0:c1, r0:r1] = blk.t().to(dst.dtype)

    def conv2d(self, X, W, Y, B, Hin, Win, Cin, Hout, Wout, Cout, KH, KW, stride, pad, mode=0, ups=1, bias=None,
               bias2=None, R=None, alpha=1.0, beta=0.0, act=ACT_NONE, scales=None):
        assert (scales is not None) == (X.dtype == torch.uint8)
        if scales is not None:
            assert mode == 0 and Cin % 64 == 0
        sa, sb = scales if scales is not None else (None, None)
        x = _f(_v(X, (B, Hin, Win, Cin), (Hin * Win * Cin, Win * Cin, Cin, 1)), sa).permute(0, 3, 1, 2)
        w = _f(_v(W, (Cout, KH, KW, Cin), (KH * KW * Cin, KW * Cin, Cin, 1)), sb).permute(0, 3, 1, 2)
        if mode == 0:
            if ups == 2:
                x = F.interpolate(x, scale_factor=2, mode="nearest")
            y = F.conv2d(x, w, stride=stride, padding=pad)
        else:
            # transposed gather: src = (dst + k - pad)/stride when divisible
            xz = torch.zeros((B, Cin, (Hin - 1) * stride + 1, (Win - 1) * stride + 1))
            xz[:, :, ::stride, ::stride] = x
            pb = Hout + KH - 1 - pad - xz.shape[2]
            pr = Wout + KW - 1 - pad - xz.shape[3]
            xz = F.pad(xz, (pad, max(pr, 0), pad, max(pb, 0)))
            y = F.conv2d(xz, w)[:, :, :Hout, :Wout]
        assert y.shape == (B, Cout, Hout, Wout), (y.shape, (B, Cout, Hout, Wout))
        acc = alpha * y.permute(0, 2, 3, 1).reshape(B * Hout * Wout, Cout)
        if bias is not None:
            acc = acc + bias.float()
        if bias2 is not None:
            acc = acc + bias2.float().repeat_interleave(Hout * Wout, 0)
        acc = _act(acc, act)
        if R is not None and beta != 0:  # beta == 0: R is not read
            acc = acc + beta * _v(R, (B * Hout * Wout, Cout), (Cout, 1)).float()
        _v(Y, (B * Hout * Wout, Cout), (Cout, 1)).copy_(acc.to(Y.dtype))

    def conv2d_wgrad(self, X, dY, dW, B, Hin, Win, Cin, Hout, Wout, Cout, KH, KW, stride, pad, ups=1):
        name = "comat_conv2d_wgrad"
        _refuse(name, X is not None and dY is not None and dW is not None, "null operand")
        _refuse(name, X.dtype == dY.dtype and X.dtype in (torch.float32, torch.bfloat16) and dW.dtype == torch.float32,
                "operands must be bf16 or fp32, dW fp32")
        _refuse(name, KH == KW and KH in (1, 3), f"KH == KW in {{1, 3}} (got {KH} x {KW})")
        _refuse(name, stride in (1, 2), f"stride in {{1, 2}} (got {stride})")
        _refuse(name, ups == 1 or (ups == 2 and stride == 1), f"ups in {{1, 2}}, ups == 2 only with stride 1 (got ups {ups}, stride {stride})")
        _refuse(name, min(B, Hin, Win, Cin, Cout, Hout, Wout) >= 1 and pad >= 0, "sizes must be positive")
        _refuse(name, Hin * ups + 2 * pad >= KH and Win * ups + 2 * pad >= KW
                and Hout == (Hin * ups + 2 * pad - KH) // stride + 1 and Wout == (Win * ups + 2 * pad - KW) // stride + 1,
                f"Hout x Wout = {Hout} x {Wout} is not the output of this convolution")
        x = _v(X, (B, Hin, Win, Cin), (Hin * Win * Cin, Win * Cin, Cin, 1)).float().permute(0, 3, 1, 2)
        g = _v(dY, (B, Hout, Wout, Cout), (Hout * Wout * Cout, Wout * Cout, Cout, 1)).float().permute(0, 3, 1, 2)
        if ups == 2:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        gw = torch.nn.grad.conv2d_weight(x, (Cout, Cin, KH, KW), g, stride=stride, padding=pad)
        _v(dW, (Cout, KH, KW, Cin), (KH * KW * Cin, KW * Cin, Cin, 1)).add_(gw.permute(0, 2, 3, 1))

    def conv2d_wgrad_workspace_bytes(self, X, dY, dW, B, Hin, Win, Cin, Hout, Wout, Cout, KH, KW, stride, pad, ups=1):
        return 0

    def colsum(self, x, out, M, Cc, ld):
        name = "comat_colsum"
        _refuse(name, x is not None and out is not None, "null operand")
        _refuse(name, x.dtype in (torch.float32, torch.bfloat16) and out.dtype == torch.float32, "x must be bf16 or fp32, out fp32")
        _refuse(name, M >= 1 and Cc >= 1 and ld >= Cc, f"M, C >= 1 and ld >= C (got M {M}, C {Cc}, ld {ld})")
        out.reshape(-1)[:Cc].add_(_v(x, (M, Cc), (ld, 1)).float().sum(0))

    def colsum_batched(self, x, out, B, M, Cc, ld):
        name = "comat_colsum_batched"
        _refuse(name, x is not None and out is not None, "null operand")
        _refuse(name, x.dtype in (torch.float32, torch.bfloat16) and out.dtype == torch.float32, "x must be bf16 or fp32, out fp32")
        _refuse(name, 1 <= B <= 65535 and M >= 1 and Cc >= 1 and ld >= Cc,
                f"1 <= B <= 65535, M, C >= 1 and ld >= C (got B {B}, M {M}, C {Cc}, ld {ld})")
        out.reshape(-1)[:B * Cc].copy_(_v(x, (B, M, Cc), (M * ld, ld, 1)).float().sum(1).reshape(-1))

    # ---- fp8 operands ---------------------------------------------------------------------------------------
    @staticmethod
    def _track(amax, m):
        """amax [1] int32 holds float bits; non-negative floats order like their bits"""
        cur = amax.view(torch.float32)
        cur.copy_(torch.maximum(cur, m.reshape(1).float()))

    def fp8_quantize_scaled(self, x, scale, amax, out=None):
        return self._quantize_scaled(x, scale, amax, out)

    def _quantize_scaled(self, x, scale, amax, out=None):
        xf = x.float()
        q = (xf * (1.0 / scale.float())).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
        self._track(amax, xf.abs().max())
        if out is None:
            out = torch.empty(x.shape, dtype=torch.uint8)
        out.copy_(q)
        return out

    def fp8_scales_update(self, amax, scale, n):
        a = amax[:n].view(torch.float32)
        seen = (amax[:n] != 0) & torch.isfinite(a)  # a non-finite abs-max: the site is treated as having seen no tensor
        scale[:n].copy_(torch.where(seen, torch.clamp(a, min=2.0 ** -100) / 448.0, scale[:n]))
        amax[:n].zero_()

    def fp8_scales_update_hist(self, amax, scale, hist, count, clip_steps, worst, clip_now, n, hist_len, margin, account):
        """header text, site by site in vector form; every value fp32, operations in the header's order"""
        n, hist_len = int(n), int(hist_len)
        acc = (clip_steps, worst, clip_now)
        if amax is None or scale is None or hist is None or count is None or n <= 0:
            raise RuntimeError("comat_fp8_scales_update_hist failed (rc=-1): null argument or no sites")
        if not 1 <= hist_len <= 16:
            raise RuntimeError("comat_fp8_scales_update_hist failed (rc=-1): hist_len must be in [1, 16]")
        if not (margin >= 1.0 and math.isfinite(margin)):
            raise RuntimeError("comat_fp8_scales_update_hist failed (rc=-1): margin must be finite and >= 1")
        if any(t is None for t in acc) != all(t is None for t in acc):
            raise RuntimeError("comat_fp8_scales_update_hist failed (rc=-1): clip_steps / worst / clip_now: all or none")
        f32 = lambda v: torch.tensor(v, dtype=torch.float32)
        a = amax[:n].view(torch.float32).clone()
        seen = (amax[:n] != 0) & torch.isfinite(a)  # a non-finite abs-max: the site is treated as having seen no tensor
        a = torch.where(seen, a, torch.zeros_like(a))
        s_a = torch.clamp(a, min=TINY) / f32(448.0)
        if clip_now is not None:
            s = scale[:n].clone()
            clipped = seen & (s > 0) & (s_a > s) if account else torch.zeros(n, dtype=torch.bool)
            clip_steps[:n] += clipped.to(torch.int32)
            ratio = s_a / torch.where(clipped, s, torch.ones_like(s))
            worst[:n].copy_(torch.where(clipped, torch.maximum(worst[:n], ratio), worst[:n]))
            clip_now[:n].copy_(clipped.to(torch.int32))
        h = hist.reshape(-1)[: n * hist_len].view(n, hist_len)  # the table is used as [n, hist_len]
        slot = (count[:n] % hist_len).long()
        rows = torch.arange(n)
        h[rows[seen], slot[seen]] = a[seen]
        count[:n] += seen.to(torch.int32)
        filled = torch.clamp(count[:n], max=hist_len)
        live = torch.arange(hist_len).reshape(1, -1) < filled.reshape(-1, 1)
        m = torch.where(live, h, torch.zeros_like(h)).max(dim=1).values
        new = torch.clamp(m, min=TINY) * f32(margin) / f32(448.0)
        scale[:n].copy_(torch.where(seen, new, scale[:n]))
        amax[:n].zero_()

    def layernorm_fwd_q_ok(self, x):
        return x.shape[1] % 8 == 0

    def layernorm_fwd_q(self, x, gamma, beta, y, stats, M, Cc, eps, q8, scale, amax):
        self.layernorm_fwd(x, gamma, beta, y, stats, M, Cc, eps)
        self._quantize_scaled(y, scale, amax, out=q8)

    def groupnorm_fwd_q_ok(self, x, B, HW, Cc, G):
        return Cc % 8 == 0 and HW > 256

    def groupnorm_fwd_q(self, x, gamma, beta, y, stats, B, HW, Cc, G, eps, silu, q8, scale, amax):
        self.groupnorm_fwd(x, gamma, beta, y, stats, B, HW, Cc, G, eps, silu)
        self._quantize_scaled(y, scale, amax, out=q8)

    def fp8_quantize(self, x, out=None, scale=None, amax=None):
        """include/comat_hip.h: scale = max(amax, 2^-100) / 448, bytes = e4m3fn(x * (1 / scale)) (RNE, saturating)"""
        xf = x.float()
        if amax is not None:
            self._track(amax, xf.abs().max())
        sc = torch.clamp(xf.abs().max(), min=2.0 ** -100) / 448.0
        q = (xf * (1.0 / sc)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
        if scale is None:
            scale = torch.empty(1, dtype=torch.float32)
        scale.copy_(sc.reshape(1))
        if out is None:
            out = torch.empty(x.shape, dtype=torch.uint8)
        out.copy_(q)
        return out, scale

    # ---- normalisation -------------------------------------------------------------------------------------
    @staticmethod
    def _gn(xf, gamma, beta, B, HW, Cc, G, eps, silu):
        xg = xf.reshape(B, HW, G, Cc // G)
        mean = xg.mean(dim=(1, 3), keepdim=True)
        var = xg.var(dim=(1, 3), unbiased=False, keepdim=True)
        rstd = (var + eps).rsqrt()
        y = ((xg - mean) * rstd).reshape(B * HW, Cc) * gamma + beta
        if silu:
            y = F.silu(y)
        return y, mean.reshape(B, G), rstd.reshape(B, G)

    def groupnorm_fwd(self, x, gamma, beta, y, stats, B, HW, Cc, G, eps, silu):
        yy, mean, rstd = self._gn(x.float(), gamma, beta, B, HW, Cc, G, eps, silu)
        y.copy_(yy.to(y.dtype))
        stats.copy_(torch.stack([mean, rstd], dim=-1))

    def groupnorm_bwd(self, dy, x, gamma, beta, stats, dx, B, HW, Cc, G, silu, add=None):
        mean = stats[..., 0].reshape(B, 1, G, 1)
        rstd = stats[..., 1].reshape(B, 1, G, 1)
        xf = x.float()
        xh = ((xf.reshape(B, HW, G, Cc // G) - mean) * rstd).reshape(B * HW, Cc)
        g = dy.float()
        if silu:
            yhat = xh * gamma + beta
            s = torch.sigmoid(yhat)
            g = g * (s * (1 + yhat * (1 - s)))
        g = g * gamma
        gg = g.reshape(B, HW, G, Cc // G)
        xhg = xh.reshape(B, HW, G, Cc // G)
        s1 = gg.mean(dim=(1, 3), keepdim=True)
        s2 = (gg * xhg).mean(dim=(1, 3), keepdim=True)
        out = (rstd * (gg - s1 - xhg * s2)).reshape(B * HW, Cc)
        if add is not None:
            out = out + add.float()
        dx.copy_(out.to(dx.dtype))

    def groupnorm_bwd_affine(self, dy, x, gamma, beta, stats, dgamma, dbeta, B, HW, Cc, G, silu):
        name = "comat_groupnorm_bwd_affine"
        _refuse(name, all(t is not None for t in (dy, x, gamma, beta, stats, dgamma, dbeta)), "null operand")
        _refuse(name, B >= 1 and HW >= 1 and Cc >= 1 and G >= 1 and Cc % G == 0, "B, HW >= 1 and G must divide C")
        mean = stats[..., 0].reshape(B, 1, G, 1)
        rstd = stats[..., 1].reshape(B, 1, G, 1)
        xh = ((x.float().reshape(B, HW, G, Cc // G) - mean) * rstd).reshape(B * HW, Cc)
        dz = dy.float().reshape(B * HW, Cc)
        if silu:
            z = xh * gamma + beta
            s = torch.sigmoid(z)
            dz = dz * (s * (1 + z * (1 - s)))
        dgamma.reshape(-1)[:Cc].add_((dz * xh).sum(0))
        dbeta.reshape(-1)[:Cc].add_(dz.sum(0))

    def layernorm_fwd(self, x, gamma, beta, y, stats, M, Cc, eps):
        xf = x.float()
        mean = xf.mean(-1, keepdim=True)
        rstd = (xf.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
        y.copy_((((xf - mean) * rstd) * gamma + beta).to(y.dtype))
        stats.copy_(torch.cat([mean, rstd], dim=-1))

    def layernorm_bwd(self, dy, x, gamma, stats, dx, M, Cc, add=None):
        mean, rstd = stats[:, :1], stats[:, 1:]
        xh = (x.float() - mean) * rstd
        g = dy.float() * gamma
        s1 = g.mean(-1, keepdim=True)
        s2 = (g * xh).mean(-1, keepdim=True)
        d = rstd * (g - s1 - xh * s2)
        if add is not None:
            d = d + add.float()
        dx.copy_(d.to(dx.dtype))

    def layernorm_bwd_affine(self, dy, x, stats, dgamma, dbeta, M, Cc, scratch=True):
        name = "comat_layernorm_bwd_affine"
        _refuse(name, all(t is not None for t in (dy, x, stats, dgamma, dbeta)), "null operand")
        _refuse(name, M >= 1 and Cc >= 1, f"M, C >= 1 (got M {M}, C {Cc})")
        st = stats.reshape(M, 2)
        xh = (x.float().reshape(M, Cc) - st[:, :1]) * st[:, 1:]
        d = dy.float().reshape(M, Cc)
        dgamma.reshape(-1)[:Cc].add_((d * xh).sum(0))
        dbeta.reshape(-1)[:Cc].add_(d.sum(0))

    # ---- softmax -------------------------------------------------------------------------------------------
    def softmax_fwd(self, S, P, rows, cols, q_len=0, causal=False, causal_offset=0, key_mask=None, rows_per_mask=0):
        s = S.reshape(rows, cols).float().clone()
        hidden = torch.zeros(rows, cols, dtype=torch.bool)
        if causal:
            q = torch.arange(rows) % q_len
            j = torch.arange(cols)
            hidden |= j[None, :] > (q[:, None] + causal_offset)
        if key_mask is not None:
            km = key_mask.reshape(-1, cols).bool().repeat_interleave(rows_per_mask, 0)[:rows]
            hidden |= ~km
        p = torch.softmax(s.masked_fill(hidden, float("-inf")), dim=-1)
        # a masked key has probability 0 whatever the row holds (a row without a visible key: all zeros); a NaN among the
        # visible scores is carried into every visible probability
        p = torch.where(hidden, torch.zeros_like(p), p)
        P.reshape(rows, cols).copy_(p.to(P.dtype))

    def softmax_bwd(self, P, dP, dS, rows, cols, scale):
        p = P.reshape(rows, cols).float()
        g = dP.reshape(rows, cols).float()
        dS.reshape(rows, cols).copy_((scale * p * (g - (g * p).sum(-1, keepdim=True))).to(dS.dtype))

    @staticmethod
    def _heads(t, B, N, H, d, ld):
        return _v(t, (B, H, N, d), (N * ld, d, ld, 1)).float()

    def flash_attn_fwd(self, q, k, v, o, lse, B, H, Nq, Nk, d, ldq, ldk, ldv, ldo, scale, q8=None):
        qh, kh, vh = self._heads(q, B, Nq, H, d, ldq), self._heads(k, B, Nk, H, d, ldk), self._heads(v, B, Nk, H, d, ldv)
        s = qh @ kh.transpose(-1, -2) * scale
        lse.copy_(_lse(s))
        _v(o, (B, H, Nq, d), (Nq * ldo, d, ldo, 1)).copy_((torch.softmax(s, -1) @ vh).to(o.dtype))
        if q8 is not None:  # comat_flash_attn_fwd_q: the e4m3 bytes of the rounded output + its abs-max; q8 [B*Nq, ldq8], layout of O
            self._quantize_scaled(_v(o, (B * Nq, H * d), (ldo, 1)), q8[1], q8[2], out=q8[0][:, :H * d])

    def flash_attn_bwd(self, q, k, v, o, do, lse, dbuf, dq, dk, dv, B, H, Nq, Nk, d, ldq, ldk, ldv, ldo, scale):
        qh, kh, vh = self._heads(q, B, Nq, H, d, ldq), self._heads(k, B, Nk, H, d, ldk), self._heads(v, B, Nk, H, d, ldv)
        oh, gh = self._heads(o, B, Nq, H, d, ldo), self._heads(do, B, Nq, H, d, ldo)
        p = torch.exp(qh @ kh.transpose(-1, -2) * scale - lse[..., None])
        D = (oh * gh).sum(-1)
        dbuf.copy_(D)
        dp = gh @ vh.transpose(-1, -2)
        ds = p * (dp - D[..., None]) * scale
        _v(dv, (B, H, Nk, d), (Nk * ldv, d, ldv, 1)).copy_((p.transpose(-1, -2) @ gh).to(dv.dtype))
        _v(dq, (B, H, Nq, d), (Nq * ldq, d, ldq, 1)).copy_((ds @ kh).to(dq.dtype))
        _v(dk, (B, H, Nk, d), (Nk * ldk, d, ldk, 1)).copy_((ds.transpose(-1, -2) @ qh).to(dk.dtype))

    # ---- elementwise ---------------------------------------------------------------------------------------
    def unary(self, op, x, y, n, p0=0.0, p1=0.0):
        v = x.reshape(-1)[:n].float()
        if op == UN_SILU:
            v = F.silu(v)
        elif op == UN_GELU:
            v = F.gelu(v)
        elif op == UN_AFFINE:
            v = p0 * v + p1
        y.reshape(-1)[:n].copy_(v.to(y.dtype))

    def unary_bwd(self, op, dy, x, dx, n):
        v = x.reshape(-1)[:n].float().detach().requires_grad_(True)
        with torch.enable_grad():
            out = F.silu(v) if op == UN_SILU else F.gelu(v)
            (g,) = torch.autograd.grad(out, v, dy.reshape(-1)[:n].float())
        dx.reshape(-1)[:n].copy_(g.to(dx.dtype))

    def axpby(self, a, x, b, y, out, n):
        v = a * x.reshape(-1)[:n].float()
        if y is not None:
            v = v + b * y.reshape(-1)[:n].float()
        out.reshape(-1)[:n].copy_(v.to(out.dtype))

    def geglu_fwd(self, x, y, M, D):
        xf = x.float()
        y.copy_((xf[:, :D] * F.gelu(xf[:, D:])).to(y.dtype))

    def geglu_bwd(self, dy, x, dx, M, D):
        xf = x.float().detach().requires_grad_(True)
        with torch.enable_grad():
            out = xf[:, :D] * F.gelu(xf[:, D:])
            (g,) = torch.autograd.grad(out, xf, dy.float())
        dx.copy_(g.to(dx.dtype))

    def copy2d(self, src, ld_src, dst, ld_dst, rows, cols):
        _v(dst, (rows, cols), (ld_dst, 1)).copy_(_v(src, (rows, cols), (ld_src, 1)).to(dst.dtype))

    @staticmethod
    def copy2d_pair_ok(items):
        return True

    def copy2d_pair(self, items, rows):
        for src, ld_src, dst, ld_dst, cols in items:
            self.copy2d(src, ld_src, dst, ld_dst, rows, cols)

    def add_rowvec(self, x, v, out, rows, cols):
        out.copy_((x.float() + v.float().reshape(1, cols)).to(out.dtype))

    def sumpool2x2(self, x, y, B, H, W, Cc):
        xv = x.reshape(B, H, 2, W, 2, Cc).float()
        y.copy_(xv.sum(dim=(2, 4)).reshape(B * H * W, Cc).to(y.dtype))

    def weights_refresh(self, master, w, wt, problems, tiles):
        name = "comat_weights_refresh"
        _refuse(name, all(t is not None for t in (master, wt, problems, tiles)), "null operand")
        _refuse(name, wt.dtype in (torch.float32, torch.bfloat16), "the compute dtype must be bf16 or fp32")
        _refuse(name, wt.dtype == torch.float32 or w is not None, "bf16 mode needs the forward copy w")
        _refuse(name, tiles.shape[0] >= 1, f"n_tiles must be in [1, 2^31) (got {tiles.shape[0]})")
        rows = problems.tolist()
        mf, tf = master.reshape(-1), wt.reshape(-1)
        for pi, r0, c0 in tiles.tolist():  # tile by tile, as the launch: a wrong table shows here too
            src, ow, owt, R, Cc, lds, ldw, ldt = rows[pi]
            r, c = min(64, R - r0), min(64, Cc - c0)
            v = _sub(mf, (r, c), lds, src + r0 * lds + c0).to(wt.dtype)  # ONE rounding
            if wt.dtype != torch.float32:
                _sub(w.reshape(-1), (r, c), ldw, ow + r0 * ldw + c0).copy_(v)
            _sub(tf, (c, r), ldt, owt + c0 * ldt + r0).copy_(v.t())

    def weights_refresh_q8(self, master, w, wt, q8, scales, amax, problems, slots, tiles):  # the bytes: oracle/fp8.py's
        name = "comat_weights_refresh_q8"
        _refuse(name, all(t is not None for t in (master, wt, q8, scales, amax, problems, slots, tiles)), "null operand")
        _refuse(name, wt.dtype in (torch.float32, torch.bfloat16), "the compute dtype must be bf16 or fp32")
        _refuse(name, wt.dtype == torch.float32 or w is not None, "bf16 mode needs the forward copy w")
        _refuse(name, 1 <= tiles.shape[0] < 2 ** 31, f"n_tiles must be in [1, 2^31) (got {tiles.shape[0]})")
        n_slots = scales.numel()
        _refuse(name, n_slots >= 1, f"n_slots must be >= 1 (got {n_slots})")
        self.weights_refresh(master, w, wt, problems, tiles)  # the copies: exactly those of comat_weights_refresh
        rows, sl, tl = problems.tolist(), slots.tolist(), tiles.tolist()
        fwd = (master if wt.dtype == torch.float32 else w).reshape(-1)
        at = lambda pi, r0, c0: (rows[pi][0] if wt.dtype == torch.float32 else rows[pi][1], rows[pi][5] if wt.dtype == torch.float32
                                 else rows[pi][6], min(64, rows[pi][3] - r0), min(64, rows[pi][4] - c0))
        amax.zero_()  # the call starts its maxima from zero ...
        am = amax.view(torch.float32)
        for pi, r0, c0 in tl:  # ... folds them tile by tile over the rounded values ...
            if sl[pi] >= 0:
                off, ld, r, c = at(pi, r0, c0)
                am[sl[pi]] = torch.maximum(am[sl[pi]], _sub(fwd, (r, c), ld, off + r0 * ld + c0).float().abs().max())
        used = sorted({s for s in sl if s >= 0})
        for s in used:
            scales[s] = torch.clamp(am[s], min=2.0 ** -100) / OF.FP8_MAX
        qf = q8.reshape(-1)
        for pi, r0, c0 in tl:  # ... and a second pass over the same table writes the bytes at the forward copy's offsets
            if sl[pi] >= 0:
                off, ld, r, c = at(pi, r0, c0)
                ldw = rows[pi][6]
                v = _sub(fwd, (r, c), ld, off + r0 * ld + c0)
                _sub(qf, (r, c), ldw, rows[pi][1] + r0 * ldw + c0).copy_(OF.quantize_with_scale(v, scales[sl[pi]]))

    def permute_nchw_nhwc(self, x, y, B, Cc, H, W, to_nhwc):
        if to_nhwc:
            y.reshape(B, H, W, Cc).copy_(x.reshape(B, Cc, H, W).permute(0, 2, 3, 1).to(y.dtype))
        else:
            y.reshape(B, Cc, H, W).copy_(x.reshape(B, H, W, Cc).permute(0, 3, 1, 2).to(y.dtype))

    # ---- guidance + scheduler step -------------------------------------------------------------------------
    def cfg_ddpm_fwd(self, x, eps2, z, x_prev, n, s, cx, ce, sigma):
        e = eps2.reshape(2, n).float()
        eps = e[0] + s * (e[1] - e[0])
        v = cx * x.reshape(-1) + ce * eps
        if z is not None:
            v = v + sigma * z.reshape(-1)
        x_prev.reshape(-1).copy_(v)

    def cfg_ddpm_bwd(self, g, dx, deps2, n, s, cx, ce):
        gf = g.reshape(-1).float()
        if dx is not None:
            dx.reshape(-1).copy_(cx * gf)
        d = deps2.reshape(2, n)
        d[0].copy_((ce * (1 - s) * gf).to(deps2.dtype))
        d[1].copy_((ce * s * gf).to(deps2.dtype))

    def cfg_rescale_ddpm_fwd(self, x, eps2, z, x_prev, n, s, cx, ce, sigma, phi, batch, per_sample, stats):
        assert batch * per_sample == n and stats.dtype == torch.float32
        e2 = eps2.reshape(2, batch, per_sample).float()
        eu, ec = e2[0], e2[1]
        e = eu + s * (ec - eu)
        mu_t, mu_c = ec.mean(1, keepdim=True), e.mean(1, keepdim=True)
        V_t, V_c = ((ec - mu_t) ** 2).sum(1, keepdim=True), ((e - mu_c) ** 2).sum(1, keepdim=True)
        stats.reshape(-1)[: 4 * batch].copy_(torch.cat([mu_t, V_t, mu_c, V_c], 1).reshape(-1))
        k = phi * torch.sqrt(V_t / V_c) + (1.0 - phi)
        v = cx * x.reshape(batch, per_sample) + ce * (k * e)
        if z is not None:
            v = v + sigma * z.reshape(batch, per_sample)
        x_prev.reshape(-1).copy_(v.reshape(-1))

    def cfg_rescale_ddpm_bwd(self, g, eps2, stats, dx, deps2, n, s, cx, ce, phi, batch, per_sample):
        assert batch * per_sample == n
        e2 = eps2.reshape(2, batch, per_sample).float()
        eu, ec = e2[0], e2[1]
        e = eu + s * (ec - eu)
        st = stats.reshape(-1)[: 4 * batch].reshape(batch, 4)
        mu_t, V_t, mu_c, V_c = (st[:, i:i + 1] for i in range(4))
        r = torch.sqrt(V_t / V_c)
        k = phi * r + (1.0 - phi)
        gf = g.reshape(batch, per_sample).float()
        d = ce * gf
        D = (d * e).sum(1, keepdim=True)
        de = k * d - D * phi * r * (e - mu_c) / V_c
        dec = D * phi * r * (ec - mu_t) / V_t
        if dx is not None:
            dx.reshape(-1).copy_((cx * gf).reshape(-1))
        out = deps2.reshape(2, n)
        out[0].copy_(((1.0 - s) * de).reshape(-1).to(deps2.dtype))
        out[1].copy_((s * de + dec).reshape(-1).to(deps2.dtype))

    @staticmethod
    def _guided(eps, halves, batch, per_sample, s):
        e2 = eps.reshape(halves, batch, per_sample).float()
        if halves == 1:
            return e2[0], None
        return e2[0] + s * (e2[1] - e2[0]), e2[1]

    def ddpm_step2_fwd(self, x, eps, z, x_prev, x0, n, halves, s, cx, ce, sigma, px, pe, phi, batch, per_sample, stats):
        assert batch * per_sample == n and halves in (1, 2) and (halves == 2 or phi == 0) and per_sample % 4 == 0
        assert x_prev is not None or x0 is not None
        e, ec = self._guided(eps, halves, batch, per_sample, s)
        k = 1.0
        if phi > 0:
            mu_t, mu_c = ec.mean(1, keepdim=True), e.mean(1, keepdim=True)
            V_t, V_c = ((ec - mu_t) ** 2).sum(1, keepdim=True), ((e - mu_c) ** 2).sum(1, keepdim=True)
            stats.reshape(-1)[: 4 * batch].copy_(torch.cat([mu_t, V_t, mu_c, V_c], 1).reshape(-1))
            k = phi * torch.sqrt(V_t / V_c) + (1.0 - phi)
        xs = x.reshape(batch, per_sample)
        if x_prev is not None:
            v = cx * xs + ce * (k * e)
            if z is not None:
                v = v + sigma * z.reshape(batch, per_sample)
            x_prev.reshape(-1).copy_(v.reshape(-1))
        if x0 is not None:
            x0.reshape(-1).copy_((px * xs + pe * (k * e)).reshape(-1))

    def ddpm_step2_bwd(self, g_prev, g_x0, eps, stats, dx, deps, n, halves, s, cx, ce, px, pe, phi, batch, per_sample,
                       eps_dtype=None):
        assert batch * per_sample == n and (g_prev is not None or g_x0 is not None) and (dx is not None or deps is not None)
        zero = torch.zeros(batch, per_sample)
        gp = zero if g_prev is None else g_prev.reshape(batch, per_sample).float()
        gx = zero if g_x0 is None else g_x0.reshape(batch, per_sample).float()
        d = ce * gp + pe * gx
        if dx is not None:
            dx.reshape(-1).copy_((cx * gp + px * gx).reshape(-1))
        if deps is None:
            return
        if halves == 1:
            deps.reshape(-1).copy_(d.reshape(-1).to(deps.dtype))
            return
        de, dec = d, 0.0
        if phi > 0:
            e, ec = self._guided(eps, halves, batch, per_sample, s)
            st = stats.reshape(-1)[: 4 * batch].reshape(batch, 4)
            mu_t, V_t, mu_c, V_c = (st[:, i:i + 1] for i in range(4))
            r = torch.sqrt(V_t / V_c)
            k = phi * r + (1.0 - phi)
            D = (d * e).sum(1, keepdim=True)
            de = k * d - D * phi * r * (e - mu_c) / V_c
            dec = D * phi * r * (ec - mu_t) / V_t
        out = deps.reshape(2, n)
        out[0].copy_(((1.0 - s) * de).reshape(-1).to(deps.dtype))
        out[1].copy_((s * de + dec).reshape(-1).to(deps.dtype))

    def add_noise_fwd(self, x, noise, noisy, xin, n, sa, sb, copies):
        assert copies in (1, 2) and xin.numel() == copies * n
        v = sa * x.reshape(-1).float() + sb * noise.reshape(-1).float()
        noisy.reshape(-1).copy_(v)
        xin.reshape(copies, n).copy_(v.to(xin.dtype).expand(copies, n))

    # ---- image path ----------------------------------------------------------------------------------------
    def resample2d(self, src, out, B, Hin, Win, Hout, Wout, Cc, ystart, ywt, xstart, xwt, KT, scale, shift):
        def gather(x, dim, start, wt, n_out, n_in):
            """sum over the KT window positions of weight * x along `dim`; a position of weight 0 or outside the image is no tap
            (the kernel skips it: not 0 * NaN)"""
            wt = wt.reshape(n_out, KT).float().cpu()
            idx = start.long().cpu()[:, None] + torch.arange(KT)[None, :]
            live = (idx >= 0) & (idx < n_in) & (wt != 0)
            idx = idx.clamp(0, n_in - 1)
            shape = [1] * x.dim()
            shape[dim] = n_out
            acc = 0.0
            for t in range(KT):
                term = wt[:, t].reshape(shape) * x.index_select(dim, idx[:, t])
                acc = acc + torch.where(live[:, t].reshape(shape), term, torch.zeros_like(term))
            return acc
        x = src.reshape(B, Hin, Win, Cc).float()
        y = gather(gather(x, 2, xstart, xwt, Wout, Win), 1, ystart, ywt, Hout, Hin)  # rows of x first, as the kernel
        if scale is not None:
            y = y * scale
        if shift is not None:
            y = y + shift
        out.reshape(B, Hout, Wout, Cc).copy_(y.to(out.dtype))

    def patchify(self, img, patches, B, H, W, Cc, P, inverse):
        nH, nW = H // P, W // P
        if not inverse:
            v = img.reshape(B, nH, P, nW, P, Cc).permute(0, 1, 3, 2, 4, 5).reshape(B * nH * nW, P * P * Cc)
            patches.copy_(v)
        else:
            v = patches.reshape(B, nH, nW, P, P, Cc).permute(0, 1, 3, 2, 4, 5).reshape(B * H * W, Cc)
            img.copy_(v)

    def embedding(self, ids, table, out, n, dim, vocab):
        out.copy_(table[ids.clamp(0, vocab - 1)])

    # ---- losses --------------------------------------------------------------------------------------------
    def cross_entropy_fwd(self, logits, labels, logp, row_lse, loss_sum_cnt, T, V, ld, ignore_index, ls):
        z = logits.float()
        lse = _lse(z)
        row_lse.copy_(lse)
        valid = (labels != ignore_index) & (labels >= 0) & (labels < V)
        y = labels.clamp(0, V - 1)
        lp = z.gather(1, y[:, None])[:, 0] - lse
        logp.copy_(torch.where(valid, lp, torch.zeros_like(lp)))
        loss = (1 - ls) * (-lp) + ls * (lse - z.mean(-1))
        loss_sum_cnt[0] = loss[valid].sum()
        loss_sum_cnt[1] = valid.sum().float()

    def cross_entropy_bwd(self, logits, labels, row_lse, dlogits, T, V, ld, ignore_index, ls, g_up, loss_sum_cnt):
        gscale = float(g_up[0]) / max(float(loss_sum_cnt[1]), 1.0)
        z = logits.float()
        valid = (labels != ignore_index) & (labels >= 0) & (labels < V)
        g = torch.exp(z - row_lse[:, None]) - ls / V
        y = labels.clamp(0, V - 1)
        g[torch.arange(T), y] -= (1 - ls)
        g = torch.where(valid[:, None], g * gscale, torch.zeros_like(g))  # an ignored row: gradient 0, its logits not read
        dlogits.copy_(g.to(dlogits.dtype))

    def disc_head_fwd(self, x, w, b, target, loss, P, pix_per_sample):
        z = x.float() @ w.float() + b.float()
        t = target.float().repeat_interleave(pix_per_sample)[:P]
        loss[0] = F.binary_cross_entropy_with_logits(z, t)

    def disc_head_bwd(self, x, w, b, target, g_up, dx, dwb, P, pix_per_sample):
        gscale = float(g_up[0])
        xf = x.float()
        z = xf @ w.float() + b.float()
        t = target.float().repeat_interleave(pix_per_sample)[:P]
        dz = gscale * (torch.sigmoid(z) - t) / P
        if dx is not None:
            dx.copy_((dz[:, None] * w.float()[None, :]).to(dx.dtype))
        if dwb is not None:
            dwb[:4] += dz @ xf
            dwb[4] += dz.sum()

    @staticmethod
    def _check_convhead(name, x, B, H, W, C):
        _refuse(name, B > 0 and H > 0 and W > 0, f"B, H, W must be positive (got {B}, {H}, {W})")
        _refuse(name, C >= 8 and C % 8 == 0 and C <= 1024, f"C must be a multiple of 8 in [8, 1024] (got {C})")
        assert x.shape == (B * H * W, C)

    @staticmethod
    def _conv_weight(w, C):
        return w.float().reshape(3, 3, C).permute(2, 0, 1).unsqueeze(0)  # tap-major [9, C] -> [1, C, 3, 3]

    def disc_convhead_fwd(self, x, w, b, target, z, loss, B, H, W, C):
        self._check_convhead("comat_disc_convhead_fwd", x, B, H, W, C)
        xi = x.float().reshape(B, H, W, C).permute(0, 3, 1, 2)
        zz = F.conv2d(xi, self._conv_weight(w, C), b.float(), padding=1).reshape(B, H * W)
        z.copy_(zz.reshape(-1))
        loss[0] = F.binary_cross_entropy_with_logits(zz, target.float()[:, None].expand(B, H * W))

    def disc_convhead_bwd(self, x, w, z, target, g_up, dx, dwb, B, H, W, C):
        _refuse("comat_disc_convhead_bwd", dx is not None or dwb is not None, "neither dx nor dwb is asked for")
        self._check_convhead("comat_disc_convhead_bwd", x, B, H, W, C)
        P = B * H * W
        dz = float(g_up[0]) / P * (torch.sigmoid(z.float().reshape(B, H * W)) - target.float()[:, None])
        dz = dz.reshape(B, 1, H, W)
        wc = self._conv_weight(w, C)
        if dx is not None:
            d = F.conv_transpose2d(dz, wc, padding=1)  # [B, C, H, W]
            dx.copy_(d.permute(0, 2, 3, 1).reshape(P, C).to(dx.dtype))
        if dwb is not None:
            xi = x.float().reshape(B, H, W, C).permute(0, 3, 1, 2)
            dw = torch.nn.grad.conv2d_weight(xi, wc.shape, dz, padding=1)  # [1, C, 3, 3]
            dwb[:9 * C] += dw[0].permute(1, 2, 0).reshape(-1)
            dwb[9 * C] += dz.sum()

    def attnmap_gather_fwd(self, amap, mask, tok_idx, tok_obj, num, den, avg, heads, npix, L, n_tok):
        a = amap.float()[:, :, tok_idx.long()]  # [h, npix, n_tok]
        m = mask[tok_obj.long()]  # [n_tok, npix]
        num += torch.einsum("hpt,tp->ht", a, m)
        den += a.sum(1)
        avg += a.mean(0).t()

    def attnmap_gather_bwd(self, g_num, g_den, g_avg, mask, tok_idx, tok_obj, damap, heads, npix, L, n_tok):
        m = mask[tok_obj.long()]  # [n_tok, npix]
        g = g_num[:, None, :] * m.t()[None] + g_den[:, None, :]
        if g_avg is not None:
            g = g + g_avg.t()[None] / heads
        d = torch.zeros(damap.shape, dtype=torch.float32)  # the kernel writes every element of dA
        for t in range(n_tok):
            d[:, :, int(tok_idx[t])] += g[:, :, t]
        damap.copy_(d.to(damap.dtype))

    # ---- optimizer -----------------------------------------------------------------------------------------
    def sumsq(self, x, n, out):
        out[0] += (x.reshape(-1)[:n].double() ** 2).sum().float()

    def grad_norm_scale(self, g, g_out, n, norm_out, target):
        gf = g.reshape(-1)[:n].float()
        norm = gf.double().pow(2).sum().sqrt().float()
        norm_out[0] = norm
        if target > 0:
            c = 0.0 if float(norm) == 0 else target / norm  # a zero gradient stays zero, a NaN norm is carried
            g_out.reshape(-1)[:n].copy_((gf * c).to(g_out.dtype))

    def adamw_tick(self, counters, gnorm_sq):
        counters[0 if math.isfinite(float(gnorm_sq[0])) else 1] += 1

    def adamw(self, p, g, m, v, n, lr, beta1, beta2, eps, wd, step, gnorm_sq, max_norm, step_dev=None, grad_scale=1.0):
        if step_dev is not None:
            step = int(step_dev[0]) + 1
        clip = grad_scale
        if gnorm_sq is not None and not math.isfinite(float(gnorm_sq[0])):
            return  # non-finite gradient norm: the update is skipped
        if gnorm_sq is not None and max_norm > 0:
            clip = grad_scale * min(1.0, max_norm / (math.sqrt(float(gnorm_sq[0])) * grad_scale + 1e-6))
        gg = g * clip
        m.mul_(beta1).add_(gg, alpha=1 - beta1)
        v.mul_(beta2).addcmul_(gg, gg, value=1 - beta2)
        bc1 = 1 - beta1 ** step
        bc2s = math.sqrt(1 - beta2 ** step)
        p.mul_(1 - lr * wd)
        p.addcdiv_(m, v.sqrt() / bc2s + eps, value=-lr / bc1)

    # ---- optimizer: learning-rate schedule on the device ---------------------------------------------------
    def lr_schedule_eval(self, sched, counters, lr_out):
        _check_schedule("comat_lr_schedule_eval", sched)
        lr_out[0] = lr_at(sched, counters[0])

    def adamw_tick_lr(self, counters, gnorm_sq, sched, lr_out):
        _check_schedule("comat_adamw_tick_lr", sched)
        if math.isfinite(float(gnorm_sq[0])):
            counters[0] += 1
            lr_out[0] = lr_at(sched, counters[0])
        else:
            counters[1] += 1

    def adamw_lr(self, p, g, m, v, n, lr_dev, beta1, beta2, eps, wd, step_dev, gnorm_sq, max_norm, grad_scale=1.0):
        _refuse("comat_adamw_lr", lr_dev is not None and step_dev is not None, "bad args (lr_dev and step_dev are required)")
        self.adamw(p, g, m, v, n, float(lr_dev[0]), beta1, beta2, eps, wd, 0, gnorm_sq, max_norm, step_dev=step_dev,
                   grad_scale=grad_scale)

    # ---- optimizer: gradient accumulation, the window on the device ----------------------------------------
    def accum_zero(self, g, n, window):
        _refuse("comat_accum_zero", g is not None and window is not None, "null pointer")
        _refuse("comat_accum_zero", n >= 1, f"n must be >= 1 (got {n})")
        if int(window[0]) == 0:
            g.reshape(-1)[:n].zero_()

    def adamw_window(self, p, g, m, v, n, lr_dev, beta1, beta2, eps, wd, step_dev, gnorm_sq, max_norm, window, accum_steps,
                     grad_scale=1.0):
        name = "comat_adamw_window"
        _refuse(name, all(x is not None for x in (p, g, m, v, lr_dev, step_dev, window)), "null pointer")
        _refuse(name, n >= 1 and grad_scale > 0, f"n must be >= 1 and grad_scale > 0 (got {n}, {grad_scale})")
        _refuse(name, accum_steps >= 1, f"accum_steps must be >= 1 (got {accum_steps})")
        if int(window[0]) == accum_steps - 1:
            self.adamw_lr(p, g, m, v, n, lr_dev, beta1, beta2, eps, wd, step_dev, gnorm_sq, max_norm, grad_scale=grad_scale)

    def window_tick(self, window, accum_steps, counters, gnorm_sq, sched, lr_out, step_loss=None, train_loss=None):
        name = "comat_window_tick"
        if sched is not None:
            _check_schedule(name, sched)
        _refuse(name, window is not None and counters is not None and gnorm_sq is not None
                and (sched is None or lr_out is not None), "null pointer")
        _refuse(name, accum_steps >= 1, f"accum_steps must be >= 1 (got {accum_steps})")
        _refuse(name, (step_loss is None) == (train_loss is None), "step_loss and train_loss go together")
        w = int(window[0])
        if train_loss is not None:  # fp32, in the stated order
            prev = np.float32(0.0) if w == 0 else np.float32(float(train_loss[0]))
            train_loss[0] = float(prev + np.float32(float(step_loss.reshape(-1)[0])) / np.float32(accum_steps))
        if w != accum_steps - 1:
            window[0] = w + 1
            return
        if math.isfinite(float(gnorm_sq[0])):
            counters[0] += 1
            if sched is not None:
                lr_out[0] = lr_at(sched, counters[0])
        else:
            counters[1] += 1
        if train_loss is not None:
            train_loss[1] = train_loss[0]
        window[0] = 0
