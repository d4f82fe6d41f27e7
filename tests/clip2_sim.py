"""The ABI simulator with the entry point of the second text tower's pooled output (comat_eos_pool, include/comat_hip.h) - TEST
INFRASTRUCTURE ONLY.  The binding keeps its wrapper as a module function (comat_amd._hip.eos_pool, handed out by
ops.pool_kernels()); this subclass of tests/clip_tune_sim.py's simulator carries the mirror under the same name and argument list,
and the tests of SDXL's second tower install it over the `sim` leg of conftest's `dev` fixture (`clip2_dev` below).

The mirror states the position rule in torch's own words and normalises the gathered rows with the simulator's layernorm_fwd: on
the simulator, too, out[b] has the bits layernorm_fwd gives that row (its rows do not depend on one another)."""
from __future__ import annotations

import pytest
import torch

from clip_tune_sim import ClipTuneSimKernels
from sim_backend import _refuse


def eos_positions(ids, eos_id):
    """transformers' two rules (CLIPTextTransformer.forward), on the ids as given"""
    if eos_id == 2:
        return ids.argmax(-1)
    return (ids == eos_id).int().argmax(-1)


class Clip2SimKernels(ClipTuneSimKernels):
    def eos_pool(self, ids, h, gamma, beta, out, pos, B, L, C, eos_id, eps):
        name = "comat_eos_pool"
        _refuse(name, all(t is not None for t in (ids, h, gamma, beta, out)), "null pointer")
        _refuse(name, B > 0 and L > 0 and C > 0, "bad shape (B, L, C must be positive)")
        _refuse(name, eos_id >= 0, "eos_id must not be negative")
        _refuse(name, h.dtype in (torch.float32, torch.bfloat16), "bad dtype")
        assert ids.dtype == torch.int64 and gamma.dtype == torch.float32 and beta.dtype == torch.float32 and out.dtype == h.dtype
        p = eos_positions(ids.reshape(-1)[:B * L].reshape(B, L), eos_id)
        rows = h.reshape(-1)[:B * L * C].reshape(B * L, C)[torch.arange(B) * L + p]
        y, stats = torch.empty_like(rows), torch.empty((B, 2), dtype=torch.float32)
        self.layernorm_fwd(rows, gamma, beta, y, stats, B, C, eps)
        out.reshape(-1)[:B * C].copy_(y.reshape(-1))
        if pos is not None:
            pos.reshape(-1)[:B].copy_(p)


def sim_matches_binding():
    """(names, mismatches): the mirror above against the binding's module function, by argument list"""
    import inspect

    from comat_amd import _hip
    names = ("eos_pool",)
    args = lambda f, skip: list(inspect.signature(f).parameters)[skip:]
    return names, [n for n in names if args(getattr(_hip, n), 0) != args(getattr(Clip2SimKernels, n), 1)]


@pytest.fixture
def clip2_dev(dev):
    """conftest's `dev` with the simulator that knows comat_eos_pool on the sim leg; the hip leg is the real library"""
    from comat_amd import ops
    if dev.type == "cpu":
        ops.set_kernel_backend(Clip2SimKernels())
    return dev
