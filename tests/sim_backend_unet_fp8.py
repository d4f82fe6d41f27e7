"""CPU simulator of the fp8 forward of a fully trained UNet — TEST INFRASTRUCTURE ONLY.

`SimKernelsUnetFp8` joins `SimKernelsUnet` (the entry points of `--full_finetuning`) and `SimKernelsFp8` (the delayed-scaling
recipe) and adds, in plain torch, the documented semantics (include/comat_hip.h) of comat_weights_refresh_q8 with the argument list
of comat_amd._hip.HipKernels.weights_refresh_q8 and the contract's refusals (a RuntimeError that names the entry point, as
`_hip._check` raises for COMAT_EINVAL).  The bytes are those of the CPU oracle (oracle/fp8.py).
"""
from __future__ import annotations

import torch

from oracle import fp8 as OF
from sim_backend_fp8 import SimKernelsFp8
from sim_backend_unet import SimKernelsUnet, _refuse, _sub, release, use_hip  # noqa: F401 - re-exported


class SimKernelsUnetFp8(SimKernelsUnet, SimKernelsFp8):
    def weights_refresh_q8(self, master, w, wt, q8, scales, amax, problems, slots, tiles):
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


def use_sim_unet_fp8():
    from comat_amd import ops
    ops.set_kernel_backend(SimKernelsUnetFp8())
    return torch.device("cpu")
