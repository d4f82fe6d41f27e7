"""quick-GELU (COMAT_UN_QUICK_GELU = 4 of comat_unary / comat_unary_bwd) against x * sigmoid(1.702 x) in fp64, forward and
backward, on the simulator and on the real kernels.  Bound: the one tests/test_ops.py holds SiLU / GELU to - max error over the
output's scale below 2e-4 (fp32) / 2e-2 (bf16).  The hard values (+-0, +-20, +-88: 1.702 * 88 overflows exp in fp32) are in a
tensor of their own and held element by element as well, so that the scale of 88 cannot hide a wrong small value."""
import pytest
import torch

from clip_sim import clip_dev  # noqa: F401 - fixture
from comat_amd import ops

DTYPES = [torch.float32, torch.bfloat16]
HARD = [0.0, -0.0, 20.0, -20.0, 88.0, -88.0, 1.0, -1.0, 5.0, -5.0, 0.125, -0.125]
PAD = 3  # elements of NaN in front of and behind a window: 12 / 6 bytes, so the window starts off every vector boundary


def tol(dtype):
    return 2e-4 if dtype == torch.float32 else 2e-2


def ref_fwd_bwd(x, g):
    x, g = x.double(), g.double()
    s = torch.sigmoid(1.702 * x)
    return x * s, g * (s + 1.702 * x * s * (1 - s))


def values(n, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, generator=gen) * 3).to(dtype)
    g = torch.randn(n, generator=gen).to(dtype)
    return x, g


def window(t, dev):
    """t inside a buffer of NaN; (buffer, view of the window)"""
    buf = torch.full((t.numel() + 2 * PAD,), float("nan"), dtype=t.dtype)
    buf[PAD:PAD + t.numel()] = t
    buf = buf.to(dev)
    return buf, buf[PAD:PAD + t.numel()]


def halo_untouched(buf):
    return bool(torch.isnan(buf[:PAD]).all() and torch.isnan(buf[-PAD:]).all())


def run(dev, x, g, windowed):
    k = ops.kernels()
    n = x.numel()
    if windowed:
        xb, xd = window(x, dev)
        gb, gd = window(g, dev)
        yb, y = window(torch.zeros_like(x), dev)
        dxb, dx = window(torch.zeros_like(x), dev)
    else:
        xd, gd = x.to(dev), g.to(dev)
        y, dx = torch.empty_like(xd), torch.empty_like(xd)
    k.unary(ops.UN_QUICK_GELU, xd, y, n)
    k.unary_bwd(ops.UN_QUICK_GELU, gd, xd, dx, n)
    if windowed:
        assert halo_untouched(yb) and halo_untouched(dxb), "a store outside the window"
        assert halo_untouched(xb) and halo_untouched(gb)
    return y.cpu(), dx.cpu()


def held(got, ref, dtype, what):
    err = (got.double() - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    assert torch.isfinite(got).all(), what
    assert err / scale < tol(dtype), f"{what}: max err {err:.3e} vs scale {scale:.3e} ({dtype})"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 7, 8, 4099])
@pytest.mark.parametrize("windowed", [False, True])
def test_quick_gelu_forward_backward(clip_dev, dtype, n, windowed):
    x, g = values(n, dtype, seed=n)
    y, dx = run(clip_dev, x, g, windowed)
    ry, rdx = ref_fwd_bwd(x, g)
    held(y, ry, dtype, f"quick_gelu n={n}")
    held(dx, rdx, dtype, f"quick_gelu bwd n={n}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_quick_gelu_hard_values(clip_dev, dtype):
    x = torch.tensor(HARD).to(dtype)
    g = torch.linspace(-1.5, 2.0, len(HARD)).to(dtype)
    y, dx = run(clip_dev, x, g, windowed=True)
    ry, rdx = ref_fwd_bwd(x, g)
    held(y, ry, dtype, "hard values")
    held(dx, rdx, dtype, "hard values bwd")
    # element by element: the same relative bound, with a floor at the smallest normal fp32 (results below it may flush to 0)
    for got, ref, what in ((y, ry, "fwd"), (dx, rdx, "bwd")):
        bad = (got.double() - ref).abs() > tol(dtype) * ref.abs() + 1e-37
        assert not bad.any(), f"{what} at x = {x[bad].tolist()}: {got[bad].tolist()} vs {ref[bad].tolist()}"
    assert y[0].item() == 0.0 and y[1].item() == 0.0  # +-0 -> 0
    assert dx[0].item() == pytest.approx(0.5 * g[0].item()) and dx[1].item() == pytest.approx(0.5 * g[1].item())


def test_autograd_operator(clip_dev):
    x, g = values(300, torch.float32, seed=2)
    xd = x.to(clip_dev).requires_grad_(True)
    y = ops.quick_gelu(xd)
    y.backward(g.to(clip_dev))
    ry, rdx = ref_fwd_bwd(x, g)
    held(y.detach().cpu(), ry, torch.float32, "ops.quick_gelu")
    held(xd.grad.cpu(), rdx, torch.float32, "ops.quick_gelu bwd")


def test_unknown_op_is_refused(clip_dev):
    x = torch.zeros(8, device=clip_dev)
    with pytest.raises(RuntimeError, match="comat_unary"):
        ops.kernels().unary(99, x, torch.empty_like(x), 8)
    with pytest.raises(RuntimeError, match="comat_unary_bwd"):
        ops.kernels().unary_bwd(99, x, x, torch.empty_like(x), 8)
    with pytest.raises(RuntimeError, match="comat_unary_bwd"):  # COPY and AFFINE have no backward entry
        ops.kernels().unary_bwd(ops.UN_COPY, x, x, torch.empty_like(x), 8)


@pytest.mark.gpu
def test_library_returns_einval_for_op_99(hip):
    from comat_amd import _hip
    lib = _hip.load_library()
    assert lib.comat_unary(99, None, None, 0, 0.0, 0.0, 0, 0, None) == -1
    x = torch.zeros(8, device=hip)
    y = torch.empty_like(x)
    assert lib.comat_unary(99, x.data_ptr(), y.data_ptr(), 8, 0.0, 0.0, _hip.F32, _hip.F32, None) == -1
    assert lib.comat_unary_bwd(99, x.data_ptr(), x.data_ptr(), y.data_ptr(), 8, _hip.F32, None) == -1
