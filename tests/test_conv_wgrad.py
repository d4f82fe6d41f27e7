"""comat_conv2d_wgrad, comat_colsum, comat_groupnorm_bwd_affine (include/comat_hip.h): the weight gradients of layers that are
trained in full - the VAE decoder under `--tune_vae` (training_utils/pipeline.py:68,170-171).

Every case runs on the ABI simulator (tests/sim_backend.py) and, marked gpu, on the library.  Expected values are fp64:
torch.nn.grad.conv2d_weight on the same (bf16-rounded) operands with F.interpolate(mode="nearest") in front for ups = 2; fp64
column sums; fp64 autograd of F.group_norm (+ F.silu).  The bound is helpers.check(..., torch.float32) - 2e-4 of the result's
maximum, what test_gemm_tt_grouped holds this product class (bf16 operands, fp32 accumulation, fp32 result) to.

The (pixel, tap) -> source-row mapping of the gather is proven on the CPU first: test_decode_program builds
tests/conv_wgrad_decode_check.cpp with the host compiler and enumerates every pair of the geometries below.
"""
import functools
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

from helpers import Window, _set_opts, check, restore_default_opts

F32, BF16 = torch.float32, torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPELINED, GENERAL = 6, 7  # comat_last_gemm_kernel() ids of the two paths (comat_amd/csrc/common.h)

# (B, Hin, Win, Cin, Cout, k, stride, ups), dtype: the smallest shape that reaches one way of going wrong
GEOMS = [
    ((1, 5, 7, 8, 8, 3, 1, 1), BF16),       # K = 35 pixels: under one k-tile, zero-page k-rows, every border kind
    ((2, 9, 6, 24, 40, 3, 1, 1), BF16),     # an image boundary inside a k-tile, ragged channel tiles
    ((1, 4, 4, 16, 8, 3, 1, 2), BF16),      # the upsample mapping
    ((2, 8, 8, 16, 16, 3, 2, 1), BF16),     # stride 2
    ((1, 6, 6, 136, 264, 3, 1, 1), BF16),   # more than one 128-tile each way, ragged
    ((1, 64, 64, 8, 8, 3, 1, 1), BF16),     # K = 4 096: the in-launch split-K combine
    ((2, 5, 5, 16, 24, 1, 1, 1), BF16),     # 1 x 1
    ((1, 6, 5, 4, 32, 3, 1, 1), BF16),      # general path: narrow Cin
    ((1, 6, 5, 8, 3, 3, 1, 1), BF16),       # general path: narrow Cout
    ((2, 5, 7, 8, 16, 3, 1, 1), F32),       # general path: fp32 parity mode
]
IDS = ["-".join(map(str, g)) + ("-fp32" if d == F32 else "") for g, d in GEOMS]


def kernels():
    from comat_amd import ops
    return ops.kernels()


def out_hw(geom):
    B, Hin, Win, Cin, Cout, k, stride, ups = geom
    pad = k // 2
    return (Hin * ups + 2 * pad - k) // stride + 1, (Win * ups + 2 * pad - k) // stride + 1, pad


def expected_path(geom, dtype):
    return PIPELINED if dtype == BF16 and geom[3] % 8 == 0 and geom[4] % 8 == 0 else GENERAL


@functools.lru_cache(maxsize=None)
def data(geom, dtype):
    """X [B, Hin, Win, Cin], dY [B, Hout, Wout, Cout] rounded to dtype, and the fp64 weight gradient in the kernel layout
    [Cout, k, k, Cin]; computed once per geometry and shared (never written)"""
    B, Hin, Win, Cin, Cout, k, stride, ups = geom
    Ho, Wo, pad = out_hw(geom)
    g = torch.Generator().manual_seed(hash(geom) % (1 << 31))
    x = (torch.randn(B, Hin, Win, Cin, generator=g) * 0.5).to(dtype)
    dy = (torch.randn(B, Ho, Wo, Cout, generator=g) * 0.5).to(dtype)
    xn = x.double().permute(0, 3, 1, 2)
    if ups == 2:
        xn = F.interpolate(xn, scale_factor=2, mode="nearest")
    ref = torch.nn.grad.conv2d_weight(xn, (Cout, Cin, k, k), dy.double().permute(0, 3, 1, 2), stride=stride, padding=pad)
    return x, dy, ref.permute(0, 2, 3, 1).contiguous()


def call(geom, x, dy, dw):
    B, Hin, Win, Cin, Cout, k, stride, ups = geom
    Ho, Wo, pad = out_hw(geom)
    kernels().conv2d_wgrad(x, dy, dw, B, Hin, Win, Cin, Ho, Wo, Cout, k, k, stride, pad, ups)


def served_by(dev, want):
    if dev.type == "cuda":
        from comat_amd import _hip
        got = _hip.last_gemm_kernel()
        assert got == want, f"served by kernel {got} ({_hip.GEMM_KERNEL_NAMES.get(got)}), the case is about kernel {want}"


def run_geometry(dev, geom, dtype):
    x, dy, ref = data(geom, dtype)
    xd, dyd = x.to(dev), dy.to(dev)
    dw = torch.zeros(ref.shape, dtype=F32, device=dev)
    call(geom, xd, dyd, dw)
    served_by(dev, expected_path(geom, dtype))
    err = (dw.cpu().double() - ref).abs().max().item() / (ref.abs().max().item() + 1e-6)
    print(f"conv2d_wgrad {geom} {dtype}: max err / max |ref| = {err:.3e}")
    check(dw, ref, F32, f"conv2d_wgrad {geom}")
    first = dw.clone()
    call(geom, xd, dyd, dw)  # a second call accumulates
    check(dw, 2 * ref, F32, f"conv2d_wgrad {geom}, second call")
    if dev.type == "cuda":  # the same inputs give the same bits
        again = torch.zeros_like(first)
        call(geom, xd, dyd, again)
        assert torch.equal(again, first), f"conv2d_wgrad {geom}: two runs differ"


@pytest.mark.parametrize("geom,dtype", GEOMS, ids=IDS)
def test_conv_wgrad(dev, geom, dtype):
    run_geometry(dev, geom, dtype)


def test_conv_wgrad_forced_splits(dev):
    """the in-launch combine on the smallest problem: two slices of one k-tile each (option force_splits)"""
    if dev.type == "cuda":
        _set_opts(force_splits=2)
    try:
        run_geometry(dev, *GEOMS[0])
    finally:
        if dev.type == "cuda":
            restore_default_opts()


def test_conv_wgrad_halo(dev):
    """X and dY inside NaN halos (two guard rows each side keep an over-read inside the allocation, where it poisons the result
    instead of faulting), dW in an armed window that must stay bit-exact outside"""
    geom, dtype = GEOMS[1]
    B, Hin, Win, Cin, Cout, k, stride, ups = geom
    Ho, Wo, pad = out_hw(geom)
    x, dy, ref = data(geom, dtype)
    wx = Window(B * Hin * Win, Cin, None, dtype, dev).put(x.reshape(-1, Cin))
    wy = Window(B * Ho * Wo, Cout, None, dtype, dev).put(dy.reshape(-1, Cout))
    ww = Window(Cout, k * k * Cin, None, F32, dev).put(torch.zeros(Cout, k * k * Cin)).arm()
    call(geom, wx.view, wy.view, ww.view)
    served_by(dev, PIPELINED)
    ww.assert_guard_intact("conv2d_wgrad halo: dW")
    ww.assert_written("conv2d_wgrad halo: dW")
    check(ww.get(), ref.reshape(Cout, -1), F32, "conv2d_wgrad halo")


def test_conv_wgrad_refusals(dev):
    k = kernels()
    x = torch.zeros(1, 4, 4, 8, dtype=BF16, device=dev)
    dy3 = torch.zeros(1, 4, 4, 8, dtype=BF16, device=dev)
    dw = torch.zeros(8, 3, 3, 8, dtype=F32, device=dev)
    with pytest.raises(RuntimeError, match="comat_conv2d_wgrad"):  # KH = 2
        k.conv2d_wgrad(x, torch.zeros(1, 3, 3, 8, dtype=BF16, device=dev), torch.zeros(8, 2, 2, 8, dtype=F32, device=dev),
                       1, 4, 4, 8, 3, 3, 8, 2, 2, 1, 0, 1)
    with pytest.raises(RuntimeError, match="comat_conv2d_wgrad"):  # ups = 2 with stride 2
        k.conv2d_wgrad(x, dy3, dw, 1, 4, 4, 8, 4, 4, 8, 3, 3, 2, 1, 2)
    for nul in range(3):  # a null pointer
        ops_ = [x, dy3, dw]
        ops_[nul] = None
        with pytest.raises(RuntimeError, match="comat_conv2d_wgrad"):
            k.conv2d_wgrad(*ops_, 1, 4, 4, 8, 4, 4, 8, 3, 3, 1, 1, 1)
    assert float(dw.abs().max()) == 0.0  # nothing was launched


# ---- comat_colsum ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(4100, 24, 32), (7, 3, 3), (1, 8, 8)], ids=["4100x24-ld32", "7x3", "1x8"])
def test_colsum(dev, shape, dtype):
    M, C, ld = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randn(M, ld, generator=g).to(dtype)
    out0 = torch.randn(C, generator=g)
    ref = out0.double() + x[:, :C].double().sum(0)
    xd, out = x.to(dev), out0.clone().to(dev)
    kernels().colsum(xd, out, M, C, ld)
    check(out, ref, F32, f"colsum {shape}")
    if dev.type == "cuda":
        again = out0.to(dev)
        kernels().colsum(xd, again, M, C, ld)
        assert torch.equal(again, out)


# ---- comat_groupnorm_bwd_affine --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("shape", [(2, 35, 16, 8), (1, 4096, 8, 8), (2, 9, 24, 4)], ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_bwd_affine(dev, shape, silu, dtype):
    B, HW, C, G = shape
    eps = 1e-6
    g = torch.Generator().manual_seed(13)
    x = (torch.randn(B, HW, C, generator=g) * 1.5 + 0.3).to(dtype)
    dy = torch.randn(B, HW, C, generator=g).to(dtype)
    gamma, beta = torch.randn(C, generator=g) * 0.5 + 1.0, torch.randn(C, generator=g) * 0.3
    xn = x.double().permute(0, 2, 1).contiguous()  # [B, C, HW]
    gm, bt = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.group_norm(xn, G, gm, bt, eps)
    if silu:
        y = F.silu(y)
    dgm, dbt = torch.autograd.grad(y, (gm, bt), dy.double().permute(0, 2, 1))
    xg = xn.reshape(B, G, -1)
    stats = torch.stack([xg.mean(-1), (xg.var(-1, unbiased=False) + eps).rsqrt()], dim=-1).float()  # [B, G, 2], what fwd saves
    d0, b0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    dgamma, dbeta = d0.clone().to(dev), b0.clone().to(dev)
    args = (dy.reshape(-1, C).to(dev), x.reshape(-1, C).to(dev), gamma.to(dev), beta.to(dev), stats.to(dev))
    kernels().groupnorm_bwd_affine(*args, dgamma, dbeta, B, HW, C, G, silu)
    check(dgamma, d0.double() + dgm, dtype, f"groupnorm_bwd_affine {shape} dgamma")
    check(dbeta, b0.double() + dbt, dtype, f"groupnorm_bwd_affine {shape} dbeta")
    if dev.type == "cuda":
        dg2, db2 = d0.to(dev), b0.to(dev)
        kernels().groupnorm_bwd_affine(*args, dg2, db2, B, HW, C, G, silu)
        assert torch.equal(dg2, dgamma) and torch.equal(db2, dbeta)


# ---- the decode, on the CPU ------------------------------------------------------------------------------------------------
def test_decode_program(tmp_path):
    """tests/conv_wgrad_decode_check.cpp, built with the host compiler: every (pixel, tap) of every geometry above maps inside
    X or to the zero page, and to what the definition of comat_conv2d_wgrad says"""
    cxx = shutil.which("g++")
    assert cxx, "the decode check needs a host C++ compiler (g++)"
    exe = str(tmp_path / "conv_wgrad_decode_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "conv_wgrad_decode_check.cpp"), "-o", exe],
                   check=True)
    args = [str(v) for geom, _ in GEOMS for v in geom]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(": ok") == len(GEOMS)
