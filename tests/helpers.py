"""Shared helpers of the parity tests."""
import contextlib
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


@contextlib.contextmanager
def fp8_state():
    """a test that sets the fp8 scaling mode or a recipe starts from none and leaves what it found.  A module builds its `dev` /
    `sim` / `hip` on the suite's with it - `def dev(dev): with fp8_state(): yield dev` - so the state is restored while the
    backend is still installed and the backend is released last."""
    from comat_amd import ops
    prev = (ops.fp8_scaling(), ops.fp8_recipe())
    ops.fp8_reset()
    ops.clear_fp8_recipe()
    try:
        yield
    finally:
        ops.set_fp8_scaling(prev[0])
        ops.clear_fp8_recipe()
        if prev[1] is not None:
            ops.set_fp8_recipe(**prev[1])
        ops.fp8_reset()


# ---- exact integer-operand parity (tests/test_exact_products.py) -------------------------------------------------------------
def ints(*shape, seed, hi=8):
    """float tensor of NON-ZERO integers drawn uniformly from +-{1 .. hi}: exact in bf16 (hi <= 256) and, up to 8, in e4m3; no
    dropped product can hide behind a zero factor"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.randint(1, hi + 1, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sign).float()


def assert_sums_exact(K, a, b, factor=1, extra=0.0):
    """every partial sum of K products a * b (times `factor`: 3 where alpha2 = 0.75 multiplies the sum; plus `extra`, the largest
    value accumulated into) is an integer below 2^24: no summation order can round in fp32"""
    amax, bmax = float(a.abs().max()), float(b.abs().max())
    assert bool((a == a.round()).all()) and bool((b == b.round()).all()), "operands must be integers"
    assert K * amax * bmax * factor + extra < 2 ** 24, f"partial sums may round: K {K}, max |a| {amax}, max |b| {bmax}, factor {factor}"


def _first_mismatch(bad, shape):
    i = int(torch.nonzero(bad.reshape(-1))[0])
    idx = []
    for n in reversed(shape):
        idx.append(i % n)
        i //= n
    return tuple(reversed(idx))


def assert_exact(got, ref64, out_dtype, what, alpha=1.0):
    """`got` equals the exact result bit for bit: ref64 (fp64) must itself be an fp32 number everywhere - then an fp32 accumulator
    of exact partial sums holds it whatever the summation order - and the stored value is its one round-to-nearest-even to
    out_dtype.  A failure names the first (batch, row, column) and the difference over alpha: the sum of the products that are
    missing or counted twice."""
    assert ref64.dtype == torch.float64
    assert torch.equal(ref64.float().double(), ref64), f"{what}: the reference is not exact in fp32 - the case proves nothing"
    want = ref64.float().to(out_dtype)
    got = got.detach().cpu()
    assert got.dtype == out_dtype and got.shape == want.shape, (what, got.dtype, out_dtype, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = (got != want) | torch.isnan(got)
    at = _first_mismatch(bad, got.shape)
    g, w = float(got[at]), float(want[at])
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {at}: got {g!r}, expected {w!r} "
                         f"(exact {float(ref64[at])!r}); difference / alpha = {(g - float(ref64[at])) / alpha!r}")


ACT_FP64 = {"none": lambda t: t, "silu": torch.nn.functional.silu, "gelu": torch.nn.functional.gelu}


def act_interval(ref64, out_dtype):
    """[lo, hi] per element for the result of an activation epilogue: the fp32 value within 2e-4 * max(1, |ref|) of the fp64
    activation - what the device activation code is held to in fp32 (test_value_ranges.assert_pointwise) - and, for a bf16 output,
    the ONE round-to-nearest-even of such a value: rounding is monotonic, so the stored number lies between the roundings of the
    two ends.  (A relative allowance for the final rounding would have to be 2^-8 |ref|, half an ulp just above a power of two;
    2^-9 |ref| is half an ulp only just BELOW one and refuses the correctly rounded exact result.  The interval needs neither.)"""
    lim = 2e-4 * torch.clamp(ref64.abs(), min=1.0)
    lo, hi = ref64 - lim, ref64 + lim
    if out_dtype == torch.bfloat16:
        lo, hi = lo.to(torch.bfloat16).double(), hi.to(torch.bfloat16).double()
    return lo, hi


def assert_act_exact_pre(got, pre64, act, out_dtype, what):
    """epilogues with an activation: the pre-activation pre64 is exact (an fp32 number), the activation is not.  `act` is a name
    of ACT_FP64 or a callable fp64 -> fp64 (GEGLU: it rounds value and gate to bf16 first, as the epilogue does); the result is
    held per element to act_interval of the fp64 activation of pre64."""
    assert pre64.dtype == torch.float64
    assert torch.equal(pre64.float().double(), pre64), f"{what}: the pre-activation is not exact in fp32 - the case proves nothing"
    ref = (ACT_FP64[act] if isinstance(act, str) else act)(pre64)
    got = got.detach().cpu()
    assert got.dtype == out_dtype and got.shape == ref.shape, (what, got.dtype, out_dtype, tuple(got.shape), tuple(ref.shape))
    lo, hi = act_interval(ref, out_dtype)
    g = got.double()
    bad = ~((g >= lo) & (g <= hi))  # (a NaN is bad)
    if bool(bad.any()):
        at = _first_mismatch(bad, got.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the bound, first at {at}: got {float(got[at])!r}, "
                             f"expected {float(ref[at])!r} (accepted: {float(lo[at])!r} .. {float(hi[at])!r})")


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
