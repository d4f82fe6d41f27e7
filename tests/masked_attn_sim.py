"""The ABI simulator with the two entry points of the fused masked attention (comat_flash_attn_masked_fwd / _bwd,
include/comat_hip.h) - TEST INFRASTRUCTURE ONLY.  The binding keeps its wrappers as module functions
(comat_amd._hip.flash_attn_masked_fwd / _bwd, handed out by ops.masked_attn_kernels()); this subclass of tests/clip2_sim.py's
simulator carries the mirrors under the same names and argument lists, and the tests of the masked path install it over the `sim`
leg of conftest's `dev` fixture (`masked_dev` below).

The mirrors state the mask in torch's own words - key j is visible to query q of batch entry b iff (not causal or
j <= q + causal_offset) and (key_mask is None or key_mask[b, j] != 0) - compute in fp32 and round once to the storage type.  A
query without a visible key gets O = 0 and lse = +inf; the backward recomputes p = exp(s - lse) and selects 0 at masked entries."""
from __future__ import annotations

import pytest
import torch

from clip2_sim import Clip2SimKernels
from sim_backend import _refuse, _v


def visible(B, Nq, Nk, causal, causal_offset, key_mask):
    """bool [B, 1, Nq, Nk]"""
    vis = torch.ones(B, 1, Nq, Nk, dtype=torch.bool)
    if causal:
        vis &= (torch.arange(Nk)[None, :] <= torch.arange(Nq)[:, None] + causal_offset)[None, None]
    if key_mask is not None:
        vis &= (key_mask.reshape(-1)[:B * Nk].reshape(B, 1, 1, Nk) != 0)
    return vis


def _check_args(name, ptrs, B, H, Nq, Nk, d, lds, dtype):
    _refuse(name, all(t is not None for t in ptrs), "null pointer")
    _refuse(name, B > 0 and H > 0 and Nq > 0 and Nk > 0 and d > 0 and B * H <= 65535, "bad shape")
    _refuse(name, dtype in (torch.float32, torch.bfloat16), "bad dtype")
    kc = 8 if dtype == torch.bfloat16 else 4
    _refuse(name, d <= 160 and d % kc == 0, f"head dim {d} unsupported (<=160, multiple of {kc})")
    _refuse(name, all(ld % kc == 0 for ld in lds), "leading dims must be 16-byte multiples")


class MaskedAttnSimKernels(Clip2SimKernels):
    def __init__(self):
        super().__init__()
        self.masked_calls = {"fwd": 0, "bwd": 0}

    def flash_attn_masked_fwd(self, q, k, v, o, lse, B, H, Nq, Nk, d, ldq, ldk, ldv, ldo, scale, causal, causal_offset, key_mask):
        name = "comat_flash_attn_masked_fwd"
        _check_args(name, (q, k, v, o, lse), B, H, Nq, Nk, d, (ldq, ldk, ldv, ldo), None if q is None else q.dtype)
        self.masked_calls["fwd"] += 1
        qh, kh, vh = self._heads(q, B, Nq, H, d, ldq), self._heads(k, B, Nk, H, d, ldk), self._heads(v, B, Nk, H, d, ldv)
        vis = visible(B, Nq, Nk, causal, causal_offset, key_mask)
        s = (qh @ kh.transpose(-1, -2) * scale).masked_fill(~vis, float("-inf"))
        empty = ~vis.any(-1)  # [B, 1, Nq]
        m = torch.where(empty, torch.zeros(()), s.amax(-1))
        e = torch.where(vis, torch.exp(s - m[..., None]), torch.zeros(()))
        l = e.sum(-1)
        p = torch.where(vis, e / torch.where(empty, torch.ones(()), l)[..., None], torch.zeros(()))
        lse.copy_(torch.where(empty, torch.full((), float("inf")), m + torch.log(l)).expand(B, H, Nq))
        _v(o, (B, H, Nq, d), (Nq * ldo, d, ldo, 1)).copy_((p @ vh).to(o.dtype))

    def flash_attn_masked_bwd(self, q, k, v, o, do, lse, dbuf, dq, dk, dv, B, H, Nq, Nk, d, ldq, ldk, ldv, ldo, scale, causal,
                              causal_offset, key_mask):
        name = "comat_flash_attn_masked_bwd"
        _check_args(name, (q, k, v, o, do, lse, dbuf, dq, dk, dv), B, H, Nq, Nk, d, (ldq, ldk, ldv, ldo), None if q is None else q.dtype)
        self.masked_calls["bwd"] += 1
        qh, kh, vh = self._heads(q, B, Nq, H, d, ldq), self._heads(k, B, Nk, H, d, ldk), self._heads(v, B, Nk, H, d, ldv)
        oh, gh = self._heads(o, B, Nq, H, d, ldo), self._heads(do, B, Nq, H, d, ldo)
        vis = visible(B, Nq, Nk, causal, causal_offset, key_mask)
        p = torch.where(vis, torch.exp(qh @ kh.transpose(-1, -2) * scale - lse[..., None]), torch.zeros(()))
        D = (oh * gh).sum(-1)
        dbuf.copy_(D)
        dp = gh @ vh.transpose(-1, -2)
        ds = torch.where(vis, p * (dp - D[..., None]) * scale, torch.zeros(()))
        _v(dv, (B, H, Nk, d), (Nk * ldv, d, ldv, 1)).copy_((p.transpose(-1, -2) @ gh).to(dv.dtype))
        _v(dq, (B, H, Nq, d), (Nq * ldq, d, ldq, 1)).copy_((ds @ kh).to(dq.dtype))
        _v(dk, (B, H, Nk, d), (Nk * ldk, d, ldk, 1)).copy_((ds.transpose(-1, -2) @ qh).to(dk.dtype))


def sim_matches_binding():
    """(names, mismatches): the mirrors above against the binding's module functions, by argument list"""
    import inspect

    from comat_amd import _hip
    names = ("flash_attn_masked_fwd", "flash_attn_masked_bwd")
    args = lambda f, skip: list(inspect.signature(f).parameters)[skip:]
    return names, [n for n in names if not hasattr(_hip, n) or args(getattr(_hip, n), 0) != args(getattr(MaskedAttnSimKernels, n), 1)]


@pytest.fixture
def masked_dev(dev):
    """conftest's `dev` with the simulator that knows comat_flash_attn_masked_* on the sim leg; the hip leg is the real library.
    The process-wide switch of ops is off again when the test is over."""
    from comat_amd import ops
    if dev.type == "cpu":
        ops.set_kernel_backend(MaskedAttnSimKernels())
    yield dev
    if hasattr(ops, "set_fused_masked_attention"):
        ops.set_fused_masked_attention(False)
