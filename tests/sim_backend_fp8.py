"""CPU simulator of comat_fp8_scales_update_hist — TEST INFRASTRUCTURE ONLY.

`SimKernelsFp8` adds to `SimKernelsExt`, in plain torch, what include/comat_hip.h documents for the recipe form of the
delayed-scaling update, with the argument list of comat_amd._hip.HipKernels.fp8_scales_update_hist.  The test modules of the fp8
recipe install it through fixtures of their own (`use_sim_fp8` below; `use_hip` / `release` are those of tests/sim_backend_ext.py).
"""
from __future__ import annotations

import math

import torch

from sim_backend_ext import SimKernelsExt, release, use_hip  # noqa: F401 - re-exported for the fixtures

TINY = 2.0 ** -100


class SimKernelsFp8(SimKernelsExt):
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
        seen = amax[:n] != 0
        a = amax[:n].view(torch.float32).clone()
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


def use_sim_fp8():
    from comat_amd import ops
    ops.set_kernel_backend(SimKernelsFp8())
    return torch.device("cpu")
