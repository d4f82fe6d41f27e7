"""The ABI simulator with the two entry points of the fully trained text tower (comat_embed_fwd / comat_embed_grad,
include/comat_hip.h) - TEST INFRASTRUCTURE ONLY.  The binding keeps their wrappers as module functions (comat_amd._hip.embed_fwd /
embed_grad, handed out by ops.table_kernels()); this subclass of tests/clip_sim.py's simulator carries their mirrors under the
same names and argument lists, and the tests of `--tune_text_encoder` install it over the `sim` leg of conftest's `dev` fixture
(`tune_dev` below)."""
from __future__ import annotations

import pytest
import torch

from clip_sim import ClipSimKernels
from sim_backend import _refuse

EMBED_GRAD_MAX_N = 4096  # COMAT_EMBED_GRAD_MAX_N


class ClipTuneSimKernels(ClipSimKernels):
    def embed_fwd(self, ids, tok, pos, out, n, L, dim, vocab):
        name = "comat_embed_fwd"
        _refuse(name, all(t is not None for t in (ids, tok, pos, out)), "null pointer")
        _refuse(name, n > 0 and dim > 0 and vocab > 0 and 0 < L <= pos.shape[0], "bad shape")
        _refuse(name, out.dtype in (torch.float32, torch.bfloat16), "bad dtype")
        assert ids.dtype == torch.int64 and tok.dtype == torch.float32 and pos.dtype == torch.float32
        rows = tok.reshape(-1, dim)[ids.reshape(-1)[:n].clamp(0, vocab - 1)]
        p = pos.reshape(-1, dim)[torch.arange(n, device=ids.device) % L]
        out.reshape(-1, dim)[:n].copy_((rows + p).to(out.dtype))  # one fp32 sum, one rounding

    def embed_grad(self, ids, dy, dtable, n, dim, vocab):
        """the kernel's order, restated: per id the rows are added to 0 in ascending i (fp32), that sum is added once to the row"""
        name = "comat_embed_grad"
        _refuse(name, all(t is not None for t in (ids, dy, dtable)), "null pointer")
        _refuse(name, n > 0 and dim > 0 and vocab > 0, "bad shape")
        _refuse(name, n <= EMBED_GRAD_MAX_N, f"n = {n}, at most {EMBED_GRAD_MAX_N} ids per launch")
        _refuse(name, dy.dtype in (torch.float32, torch.bfloat16), "bad dtype")
        assert ids.dtype == torch.int64 and dtable.dtype == torch.float32
        v = ids.reshape(-1)[:n].clamp(0, vocab - 1)
        g, table = dy.reshape(-1, dim)[:n].float(), dtable.reshape(-1, dim)
        for row in torch.unique(v).tolist():
            acc = torch.zeros(dim, dtype=torch.float32, device=g.device)
            for j in torch.nonzero(v == row).reshape(-1).tolist():  # ascending
                acc += g[j]
            table[row] += acc


def sim_matches_binding():
    """(names, mismatches): the mirrors above against the binding's module functions, by argument list"""
    import inspect

    from comat_amd import _hip
    names = ("embed_fwd", "embed_grad")
    args = lambda f, skip: list(inspect.signature(f).parameters)[skip:]
    return names, [n for n in names if args(getattr(_hip, n), 0) != args(getattr(ClipTuneSimKernels, n), 1)]


@pytest.fixture
def tune_dev(dev):
    """conftest's `dev` with the simulator that knows the two entry points on the sim leg; the hip leg is the real library"""
    from comat_amd import ops
    if dev.type == "cpu":
        ops.set_kernel_backend(ClipTuneSimKernels())
    return dev
