"""CPU simulator of the weight-gradient entry points of fully trained layers — TEST INFRASTRUCTURE ONLY.

`SimKernelsVae` adds, in plain torch, the documented semantics (include/comat_hip.h) of comat_conv2d_wgrad, comat_colsum and
comat_groupnorm_bwd_affine to `SimKernelsAccum`, with the argument lists of comat_amd._hip.HipKernels and the contract's
refusals (a RuntimeError that names the entry point, as `_hip._check` raises for COMAT_EINVAL).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from sim_backend import _v
from sim_backend_accum import SimKernelsAccum, _refuse, release, use_hip  # noqa: F401 - re-exported


class SimKernelsVae(SimKernelsAccum):
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

    def conv2d_wgrad_workspace_bytes(self, *a, **kw):
        return 0

    def colsum(self, x, out, M, Cc, ld):
        name = "comat_colsum"
        _refuse(name, x is not None and out is not None, "null operand")
        _refuse(name, x.dtype in (torch.float32, torch.bfloat16) and out.dtype == torch.float32, "x must be bf16 or fp32, out fp32")
        _refuse(name, M >= 1 and Cc >= 1 and ld >= Cc, f"M, C >= 1 and ld >= C (got M {M}, C {Cc}, ld {ld})")
        out.reshape(-1)[:Cc].add_(_v(x, (M, Cc), (ld, 1)).float().sum(0))

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


def use_sim_vae():
    from comat_amd import ops
    ops.set_kernel_backend(SimKernelsVae())
    return torch.device("cpu")
