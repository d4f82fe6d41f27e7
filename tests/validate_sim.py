"""The ABI simulator with the entry point of validation sampling's last operator (comat_image_u8, include/comat_hip.h) - TEST
INFRASTRUCTURE ONLY.  The binding keeps its wrapper as a module function (comat_amd._hip.image_u8, handed out by
ops.image_kernels()); this subclass of tests/masked_attn_sim.py's simulator carries the mirror under the same name and argument
list, and the tests of validation install it over the `sim` leg of conftest's `dev` fixture (`val_dev` below).

The mirror is written from the header's definition in numpy: per element, in fp32, v = denorm ? x * 0.5 + 0.5 : x, clamp to [0, 1]
(NaN to 0), times 255, rint (half to even); the placement formula byte for byte; bad[b] = 1 stored where image b holds a
non-finite element and nothing stored elsewhere.  Its operands are pointers, as the library's: `x` and `out` are read and written
through their storage from their first element on, whatever their shape."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from masked_attn_sim import MaskedAttnSimKernels
from sim_backend import _refuse


def bytes_of(x32, denorm):
    """the definition on a float32 numpy array -> uint8, and which elements were not finite"""
    x32 = np.asarray(x32, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (x32 * np.float32(0.5) + np.float32(0.5)).astype(np.float32) if denorm else x32
        v = np.where(v >= 0, v, np.float32(0)).astype(np.float32)  # negatives, -Inf and NaN
        v = np.where(v > 1, np.float32(1), v).astype(np.float32)
        return np.rint((v * np.float32(255)).astype(np.float32)).astype(np.uint8), ~np.isfinite(x32)


def _flat(t, n):
    """n elements of t's storage from its first element on (the pointer the library would get)"""
    return torch.as_strided(t, (n,), (1,), t.storage_offset())


class ValidateSimKernels(MaskedAttnSimKernels):
    def image_u8(self, x, out, bad, B, H, W, C, denorm, out_pitch, cols, pad):
        name = "comat_image_u8"
        _refuse(name, x is not None and out is not None, "null pointer")
        _refuse(name, B > 0 and H > 0 and W > 0, "bad shape (B, H, W must be positive)")
        _refuse(name, 1 <= C <= 4, f"C = {C}, 1 to 4 channels")
        _refuse(name, x.dtype in (torch.float32, torch.bfloat16), "bad dtype")
        _refuse(name, cols >= 1, f"cols = {cols}, at least one image a sheet row")
        _refuse(name, pad >= 0, f"pad = {pad} must not be negative")
        widest = (pad + (min(B, cols) - 1) * (W + pad) + W) * C
        _refuse(name, out_pitch >= widest, f"out_pitch = {out_pitch}, the widest row written has {widest} bytes")
        assert out.dtype == torch.uint8 and (bad is None or bad.dtype == torch.int32)
        src = _flat(x, B * H * W * C).float().numpy().reshape(B, H, W * C)
        u8, nonfinite = bytes_of(src, denorm)
        rows = pad + ((B - 1) // cols) * (H + pad) + H  # sheet rows down to the last one written
        sheet = _flat(out, (rows - 1) * out_pitch + widest).numpy()
        for b in range(B):
            for y in range(H):
                at = (pad + (b // cols) * (H + pad) + y) * out_pitch + (pad + (b % cols) * (W + pad)) * C
                sheet[at:at + W * C] = u8[b, y]
            if bad is not None and nonfinite[b].any():
                _flat(bad, B)[b] = 1


def sim_matches_binding():
    """(names, mismatches): the mirror above against the binding's module function, by argument list"""
    import inspect

    from comat_amd import _hip
    names = ("image_u8",)
    args = lambda f, skip: list(inspect.signature(f).parameters)[skip:]
    return names, [n for n in names if not hasattr(_hip, n) or args(getattr(_hip, n), 0) != args(getattr(ValidateSimKernels, n), 1)]


@pytest.fixture
def val_dev(dev):
    """conftest's `dev` with the simulator that knows comat_image_u8 on the sim leg; the hip leg is the real library.  The
    process-wide switch of the fused masked attention is off again when the test is over (as masked_dev)."""
    from comat_amd import ops
    if dev.type == "cpu":
        ops.set_kernel_backend(ValidateSimKernels())
    yield dev
    ops.set_fused_masked_attention(False)
