"""CPU simulator of the discriminator conv head's entry points — TEST INFRASTRUCTURE ONLY.

`SimKernelsGan` adds, in plain torch, the documented semantics (include/comat_hip.h) of comat_disc_convhead_fwd / _bwd to
`SimKernelsModes`, with the argument lists of comat_amd._hip.HipKernels and the contract's refusals (a RuntimeError that names
the entry point, as `_hip._check` raises for COMAT_EINVAL).  `use_sim_gan`, `use_hip` and `release` are what the fixtures of
the test modules call.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from sim_backend_modes import SimKernelsModes, release, use_hip  # noqa: F401 - re-exported


def _refuse(name, cond, msg):
    if not cond:
        raise RuntimeError(f"{name} failed (rc=-1): {name}: {msg}")


class SimKernelsGan(SimKernelsModes):
    @staticmethod
    def _check(name, x, B, H, W, C):
        _refuse(name, B > 0 and H > 0 and W > 0, f"B, H, W must be positive (got {B}, {H}, {W})")
        _refuse(name, C >= 8 and C % 8 == 0 and C <= 1024, f"C must be a multiple of 8 in [8, 1024] (got {C})")
        assert x.shape == (B * H * W, C)

    @staticmethod
    def _conv_weight(w, C):
        return w.float().reshape(3, 3, C).permute(2, 0, 1).unsqueeze(0)  # tap-major [9, C] -> [1, C, 3, 3]

    def disc_convhead_fwd(self, x, w, b, target, z, loss, B, H, W, C):
        self._check("comat_disc_convhead_fwd", x, B, H, W, C)
        xi = x.float().reshape(B, H, W, C).permute(0, 3, 1, 2)
        zz = F.conv2d(xi, self._conv_weight(w, C), b.float(), padding=1).reshape(B, H * W)
        z.copy_(zz.reshape(-1))
        loss[0] = F.binary_cross_entropy_with_logits(zz, target.float()[:, None].expand(B, H * W))

    def disc_convhead_bwd(self, x, w, z, target, g_up, dx, dwb, B, H, W, C):
        _refuse("comat_disc_convhead_bwd", dx is not None or dwb is not None, "neither dx nor dwb is asked for")
        self._check("comat_disc_convhead_bwd", x, B, H, W, C)
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


def use_sim_gan():
    from comat_amd import ops
    ops.set_kernel_backend(SimKernelsGan())
    return torch.device("cpu")
