"""Shared helpers of the parity tests."""
import dataclasses

import pytest
import torch

from comat_amd import config, weights
from oracle import sd as O


def tol(dtype):
    return 2e-4 if dtype == torch.float32 else 3e-2


def check(got, ref, dtype, what="", factor=1.0):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    assert err / scale < tol(dtype) * factor, f"{what}: max err {err:.3e} vs scale {scale:.3e} ({dtype})"


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((got - ref).norm() / (ref.norm() + 1e-30))


def tok(t):
    """NCHW -> channels-last tokens"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def untok(t, B, H, W):
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


def oracle_cfgs(ucfg=config.TINY_UNET, vcfg=config.TINY_VAE):
    return O.UNetConfig(**dataclasses.asdict(ucfg)), O.VAEConfig(**dataclasses.asdict(vcfg))


def tiny_weights(dtype, ucfg=config.TINY_UNET):
    """Tiny-config weights rounded to `dtype` (so oracle and kernels see identical values)."""
    q = lambda d: {k: v.to(dtype).float() for k, v in d.items()}
    usd = q(weights.make_unet_weights(ucfg, perturb_norms=True))
    vsd = q(weights.make_vae_weights(config.TINY_VAE, perturb_norms=True))
    lsd = q(weights.make_lora_weights(ucfg))
    # make LoRA up factors big enough that their gradients are well conditioned in the tiny model
    lsd = {k: (v * 5 if k.endswith("up.weight") else v).to(dtype).float() for k, v in lsd.items()}
    return usd, vsd, lsd


# the library's defaults for the options whose default moved in round 4 (runtime.hip)
DEFAULT_OPTS = dict(flash_xcd=1, g2_order=2, gemm3=1, norm_fused=5)


def _set_opts(**kw):
    from comat_amd import _hip
    for k_, v_ in kw.items():
        _hip.set_option(k_, v_)


def restore_default_opts():
    _set_opts(gemm2=1, gemm2_tt=1, g2_cfg=0, g2_splits=0, force_splits=0, flash_trim=1, flash_tr=1, flash_kt=4, flash_merge=1, flash_xcd=DEFAULT_OPTS['flash_xcd'],
              g2_order=DEFAULT_OPTS['g2_order'], norm_fused=DEFAULT_OPTS['norm_fused'], gemm3=DEFAULT_OPTS['gemm3'], g3_cfg=0)


@pytest.fixture
def default_opts():
    """restore the library's kernel-selection options after a test that forces variants"""
    yield
    restore_default_opts()


_INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_BYTE_FILL = 0xA5  # fill of integer windows: no value a kernel under test writes by accident in a whole row


class Window:
    """A [rows, cols] operand at leading dimension `ld` (optionally `batch` of them, `gap` elements apart) embedded in ONE
    flat poisoned buffer: `lead` guard rows, a `left` element offset, the rows with their ld - cols pad columns, the gaps
    between batch entries, `trail` guard rows.  Float buffers are filled with NaN (an input window: whatever a kernel reads
    outside its operand poisons its result), integer buffers with a fixed byte pattern.  An output window is armed after the
    operand was written and checked bit for bit afterwards: every element outside the window must be what it was.
    `left` = 8 elements keeps the window 16-byte aligned; the scalar-path cases use left = 1 with an odd ld."""

    def __init__(self, rows, cols, ld=None, dtype=torch.float32, device="cpu", lead=2, trail=2, left=8, batch=1, gap=0):
        ld = cols if ld is None else ld
        assert ld >= cols and rows >= 1 and batch >= 1
        self.rows, self.cols, self.ld, self.batch = rows, cols, ld, batch
        self.stride = rows * ld + gap  # element stride between batch entries
        self.off = lead * ld + left
        n = self.off + batch * self.stride + trail * ld
        if dtype.is_floating_point:
            self.buf = torch.full((n,), float("nan"), dtype=dtype, device=device)
        else:
            self.buf = torch.empty(n, dtype=dtype, device=device)
            self.buf.view(torch.uint8).fill_(_BYTE_FILL)
        self._snap = None
        inside = torch.zeros(n, dtype=torch.bool)
        torch.as_strided(inside, (batch, rows, cols), (self.stride, ld, 1), self.off).fill_(True)
        self._outside = (~inside).to(device)

    def _strided(self, cols):
        if self.batch == 1:
            return torch.as_strided(self.buf, (self.rows, cols), (self.ld, 1), self.off)
        return torch.as_strided(self.buf, (self.batch, self.rows, cols), (self.stride, self.ld, 1), self.off)

    @property
    def view(self):
        """the strided [rows, cols] ([batch, rows, cols]) tensor; its data_ptr() is what the kernel gets"""
        return self._strided(self.cols)

    @property
    def padded(self):
        """[rows, ld] rows INCLUDING their pad columns, for the bindings that read a leading dimension off shape[1]"""
        assert self.batch == 1
        return torch.as_strided(self.buf, (self.rows, self.ld), (self.ld, 1), self.off)

    @property
    def flat(self):
        """the window as one vector (an operand without a leading dimension)"""
        assert self.batch == 1 and (self.ld == self.cols or self.rows == 1)
        return torch.as_strided(self.buf, (self.rows * self.cols,), (1,), self.off)

    def put(self, x):
        self.view.copy_(x.to(device=self.buf.device, dtype=self.buf.dtype).reshape(self.view.shape))
        return self

    def arm(self):
        """snapshot the whole buffer as raw integers (after put, before the call)"""
        self._snap = self.buf.view(_INT_OF[self.buf.element_size()]).clone()
        return self

    def get(self):
        return self.view.clone()

    def assert_guard_intact(self, what=""):
        assert self._snap is not None, "arm() the window before the call"
        now = self.buf.view(_INT_OF[self.buf.element_size()])
        bad = (now != self._snap) & self._outside
        n = int(bad.sum())
        if n:
            i = int(torch.nonzero(bad)[0])
            r, c = divmod(i - self.off, self.ld) if i >= self.off else (-1, i)
            raise AssertionError(f"{what}: {n} guard element(s) overwritten, first at flat index {i} "
                                 f"(row {r}, column {c} of a [{self.rows}, {self.cols}] window at ld {self.ld})")

    def assert_written(self, what=""):
        """every window element was written (float windows: no NaN left and none leaked in)"""
        assert torch.isfinite(self.view.float()).all(), f"{what}: non-finite values inside the window"
