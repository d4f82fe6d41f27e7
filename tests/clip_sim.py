"""The ABI simulator with the quick-GELU op of the elementwise family (COMAT_UN_QUICK_GELU = 4, include/comat_hip.h) - TEST
INFRASTRUCTURE ONLY.  tests/sim_backend.py restates ops 0..3; the text-tower tests install this subclass over the `sim` leg of
conftest's `dev` fixture (`clip_dev` below).  The argument lists are those of SimKernels / HipKernels."""
from __future__ import annotations

import pytest
import torch

from sim_backend import SimKernels, _refuse

UN_QUICK_GELU = 4


class ClipSimKernels(SimKernels):
    def unary(self, op, x, y, n, p0=0.0, p1=0.0):
        if op != UN_QUICK_GELU:
            _refuse("comat_unary", 0 <= op <= 3, f"bad op {op}")
            return super().unary(op, x, y, n, p0, p1)
        v = x.reshape(-1)[:n].float()
        y.reshape(-1)[:n].copy_((v * torch.sigmoid(1.702 * v)).to(y.dtype))

    def unary_bwd(self, op, dy, x, dx, n):
        if op != UN_QUICK_GELU:
            _refuse("comat_unary_bwd", op in (1, 2), f"bad op {op}")
            return super().unary_bwd(op, dy, x, dx, n)
        v = x.reshape(-1)[:n].float()
        s = torch.sigmoid(1.702 * v)
        dx.reshape(-1)[:n].copy_((dy.reshape(-1)[:n].float() * (s + 1.702 * v * s * (1 - s))).to(dx.dtype))


@pytest.fixture
def clip_dev(dev):
    """conftest's `dev` with the simulator that knows op 4 on the sim leg; the hip leg is the real library"""
    from comat_amd import ops
    if dev.type == "cpu":
        ops.set_kernel_backend(ClipSimKernels())
    return dev
