"""CPU simulator of the entry points of a fully trained UNet (`--full_finetuning`) — TEST INFRASTRUCTURE ONLY.

`SimKernelsUnet` adds, in plain torch, the documented semantics (include/comat_hip.h) of comat_weights_refresh,
comat_layernorm_bwd_affine and comat_colsum_batched to `SimKernelsVae`, with the argument lists of comat_amd._hip.HipKernels and
the contract's refusals (a RuntimeError that names the entry point, as `_hip._check` raises for COMAT_EINVAL).
"""
from __future__ import annotations

import torch

from sim_backend import _v
from sim_backend_vae import SimKernelsVae, _refuse, release, use_hip  # noqa: F401 - re-exported


def _sub(flat, shape, ld, off):
    """the [rows, cols] matrix at element `off` of a flat tensor, row pitch ld"""
    return torch.as_strided(flat, shape, (ld, 1), flat.storage_offset() + off)


class SimKernelsUnet(SimKernelsVae):
    def colsum_batched(self, x, out, B, M, Cc, ld):
        name = "comat_colsum_batched"
        _refuse(name, x is not None and out is not None, "null operand")
        _refuse(name, x.dtype in (torch.float32, torch.bfloat16) and out.dtype == torch.float32, "x must be bf16 or fp32, out fp32")
        _refuse(name, 1 <= B <= 65535 and M >= 1 and Cc >= 1 and ld >= Cc,
                f"1 <= B <= 65535, M, C >= 1 and ld >= C (got B {B}, M {M}, C {Cc}, ld {ld})")
        out.reshape(-1)[:B * Cc].copy_(_v(x, (B, M, Cc), (M * ld, ld, 1)).float().sum(1).reshape(-1))

    def layernorm_bwd_affine(self, dy, x, stats, dgamma, dbeta, M, Cc, scratch=True):
        name = "comat_layernorm_bwd_affine"
        _refuse(name, all(t is not None for t in (dy, x, stats, dgamma, dbeta)), "null operand")
        _refuse(name, M >= 1 and Cc >= 1, f"M, C >= 1 (got M {M}, C {Cc})")
        st = stats.reshape(M, 2)
        xh = (x.float().reshape(M, Cc) - st[:, :1]) * st[:, 1:]
        d = dy.float().reshape(M, Cc)
        dgamma.reshape(-1)[:Cc].add_((d * xh).sum(0))
        dbeta.reshape(-1)[:Cc].add_(d.sum(0))

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


def use_sim_unet():
    from comat_amd import ops
    ops.set_kernel_backend(SimKernelsUnet())
    return torch.device("cpu")
