"""comat_image_u8 (include/comat_hip.h): decoded image tokens to bytes, dense or placed on a contact sheet - on the simulator
(tests/validate_sim.py) and on the real kernel.

There is no tolerance in this file.  Every byte is held to `expected` below - np.rint(np.clip(x * 0.5 + 0.5, 0, 1) * 255) in
fp32, the arithmetic of diffusers' VaeImageProcessor.postprocess + numpy_to_pil - computed HERE, not by the simulator; non-finite
inputs to the header's rule (NaN 0, +Inf 255, -Inf 0).  Sources are windowed (helpers.Window): NaN all around them, so a read
outside the operand raises `bad`; destinations sit in armed byte windows checked bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from comat_amd import _hip, ops
from helpers import Window
from validate_sim import ValidateSimKernels, sim_matches_binding, val_dev  # noqa: F401 - fixture

f32 = np.float32
FILL = 0xA5  # helpers.Window's fill of integer buffers


def expected(x32, denorm=True):
    """the definition, fp32 step by step, on FINITE values"""
    x32 = np.asarray(x32, dtype=f32)
    v = (x32 * f32(0.5) + f32(0.5)).astype(f32) if denorm else x32
    return np.rint(np.clip(v, 0, 1).astype(f32) * f32(255)).astype(np.uint8)


def expected_any(x32, denorm=True):
    """`expected`, and the header's rule where x is not finite"""
    x32 = np.asarray(x32, dtype=f32)
    fin = np.isfinite(x32)
    out = expected(np.where(fin, x32, f32(0)), denorm)
    out[np.isposinf(x32)] = 255
    out[np.isneginf(x32) | np.isnan(x32)] = 0
    return out


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def run_dense(dev, x, B, H, W, Cn, denorm=True, src_off=0, dst_off=0, want_bad=True):
    """x: torch [B * H * W * Cn] of the storage dtype.  The call on a source window `src_off` elements and a destination window
    `dst_off` bytes off their 16-byte aligned places.  -> (bytes uint8 numpy [B, H, W, Cn], bad list)"""
    xw = Window(B * H * W, Cn, dtype=x.dtype, device=dev, lead=0, left=8 + src_off).put(x.reshape(B * H * W, Cn))
    ow = Window(B * H, W * Cn, dtype=torch.uint8, device=dev, lead=0, left=8 + dst_off).arm()
    bw = Window(1, B, dtype=torch.int32, device=dev)
    bw.flat.zero_()
    bw.arm()
    if dev.type == "cuda":
        assert xw.view.data_ptr() % 16 == (src_off * x.element_size()) % 16 and ow.view.data_ptr() % 8 == dst_off % 8
    ops.image_kernels().image_u8(xw.view, ow.view, bw.flat if want_bad else None, B, H, W, Cn, denorm, W * Cn, 1, 0)
    sync(dev)
    ow.assert_guard_intact("out")
    bw.assert_guard_intact("bad")
    return ow.get().cpu().numpy().reshape(B, H, W, Cn), bw.flat.cpu().tolist()


# ---- 1. values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("denorm", [True, False])
def test_every_bf16_bit_pattern(val_dev, denorm):
    """all 65 536 patterns as one image: the 65 280 finite ones against the definition (they tell truncation apart - 29 313 bytes -
    but neither half-up rounding nor the fused form: the fp32 sweep below binds there), the others against the header's rule"""
    x = torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16).copy()).view(torch.bfloat16)
    x32 = x.float().numpy()
    assert int(np.isfinite(x32).sum()) == 65280
    want = expected_any(x32, denorm)
    if denorm:
        fin = np.isfinite(x32)
        trunc = np.floor(np.clip(x32[fin] * f32(0.5) + f32(0.5), 0, 1).astype(f32) * f32(255)).astype(np.uint8)
        assert int((trunc != want[fin]).sum()) == 29313
    got, bad = run_dense(val_dev, x, 1, 128, 128, 4, denorm)
    diff = got.reshape(-1) != want
    assert not diff.any(), f"{int(diff.sum())} patterns differ, first 0x{int(np.nonzero(diff)[0][0]):04x}"
    assert bad == [1]


def boundary_values():
    """x_k = fp32(2 (k + 0.5) / 255 - 1), k = 0 .. 254 - where x / 2 + 0.5 times 255 meets k + 0.5 - with 64 fp32 neighbours a side"""
    x = (2.0 * (np.arange(255, dtype=np.float64) + 0.5) / 255.0 - 1.0).astype(f32)
    cols = [x]
    lo = hi = x
    for _ in range(64):
        lo, hi = np.nextafter(lo, f32(-2)), np.nextafter(hi, f32(2))
        cols += [lo, hi]
    return np.stack(cols, axis=1).reshape(-1)


def test_fp32_boundary_sweep(val_dev):
    x32 = boundary_values()
    assert x32.size == 32895 == 3 * 85 * 129 and np.unique(x32).size == 32895
    want = expected(x32)
    v = np.clip((x32 * f32(0.5) + f32(0.5)).astype(f32), 0, 1).astype(f32)
    half_up = np.floor((v * f32(255)).astype(f32).astype(np.float64) + 0.5).astype(np.uint8)
    fused = np.rint(np.clip((x32.astype(np.float64) * 127.5 + 127.5).astype(f32), 0, 255)).astype(np.uint8)  # fma: one rounding
    n_half, n_fused = int((half_up != want).sum()), int((fused != want).sum())
    print(f"boundary sweep: half-up differs at {n_half} values, fma(x, 127.5, 127.5) at {n_fused}")
    assert n_half > 0 and n_fused > 0, "the sweep does not tell the definition from half-up rounding / the fused form"
    got, bad = run_dense(val_dev, torch.from_numpy(x32), 1, 85, 129, 3)
    diff = got.reshape(-1) != want
    assert not diff.any(), (f"{int(diff.sum())} values differ ({int((got.reshape(-1) == half_up)[diff].sum())} of them as half-up, "
                            f"{int((got.reshape(-1) == fused)[diff].sum())} as the fused form), first x = {x32[np.nonzero(diff)[0][0]]!r}")
    assert bad == [0]


# ---- 2. shapes and alignments --------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1, 3), (2, 3, 5, 3), (3, 8, 8, 3), (2, 4, 16, 3), (1, 7, 33, 4), (5, 2, 21, 1), (2, 2, 40, 2)]


def draw(n, dtype, seed):
    """values over [-1.6, 1.6] (both clamps act) with every 7th on a rounding boundary"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, generator=g) * 3.2 - 1.6)
    b = torch.from_numpy(boundary_values())
    x[::7] = b[torch.randint(0, b.numel(), (x[::7].numel(),), generator=g)]
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dst_off", [0, 1, 3])
@pytest.mark.parametrize("src_off", [0, 1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_and_offsets(val_dev, shape, src_off, dst_off, dtype):
    """rows shorter than a chunk, heads and tails, several rows and images; source and destination 0, 1 and 3 elements / bytes off:
    equal offsets keep the chunked path (with a head), unequal ones take the element path - the same bytes either way"""
    B, H, W, Cn = shape
    for denorm in (True, False):
        x = draw(B * H * W * Cn, dtype, seed=sum(shape) + src_off * 10 + dst_off)
        got, bad = run_dense(val_dev, x, B, H, W, Cn, denorm, src_off, dst_off)
        want = expected(x.float().numpy(), denorm).reshape(B, H, W, Cn)
        assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
        assert bad == [0] * B, "a clean image was flagged: something outside the operand was read"


# ---- 3. placement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("pad", [0, 1, 2])
@pytest.mark.parametrize("cols", [1, 2, 3])
def test_sheet_placement(val_dev, cols, pad, dtype):
    """B = 5: a last sheet row that is not full.  The sheet is 0xA5 everywhere first, its pitch wider than the rows written"""
    dev = val_dev
    B, H, W, Cn = 5, 6, 10, 3
    x = draw(B * H * W * Cn, dtype, seed=cols * 10 + pad)
    Hs, Ws = ops.sheet_shape(B, H, W, cols, pad)
    assert Hs == pad + -(-B // cols) * (H + pad) and Ws == pad + min(B, cols) * (W + pad)
    pitch = Ws * Cn + 5
    sw = Window(Hs, Ws * Cn, ld=pitch, dtype=torch.uint8, device=dev).arm()
    assert bool((sw.buf == FILL).all())
    xw = Window(B * H * W, Cn, dtype=dtype, device=dev).put(x.reshape(-1, Cn))
    ops.image_kernels().image_u8(xw.view, sw.view, None, B, H, W, Cn, True, pitch, cols, pad)
    sync(dev)
    sw.assert_guard_intact("sheet")
    want = np.full((Hs, Ws * Cn), FILL, dtype=np.uint8)
    img = expected(x.float().numpy()).reshape(B, H, W * Cn)
    for b in range(B):
        y0, x0 = pad + (b // cols) * (H + pad), (pad + (b % cols) * (W + pad)) * Cn
        want[y0:y0 + H, x0:x0 + W * Cn] = img[b]
    got = sw.get().cpu().numpy()
    assert np.array_equal(got, want), f"{int((got != want).sum())} sheet bytes differ"
    assert int((want == FILL).sum()) >= Hs * Ws * Cn - B * H * W * Cn  # (the background survived where no image lies)


def test_the_operator(val_dev):
    dev = val_dev
    B, H, W = 3, 4, 6
    x = draw(B * H * W * 3, torch.float32, seed=1).reshape(-1, 3)
    want = expected(x.numpy()).reshape(B, H, W, 3)
    got = ops.image_u8(x.to(dev).requires_grad_(True), B, H, W)
    assert got.dtype == torch.uint8 and got.shape == (B, H, W, 3) and not got.requires_grad
    assert np.array_equal(got.cpu().numpy(), want)
    got01 = ops.image_u8((x * 0.5 + 0.5).to(dev), B, H, W, denormalize=False)
    assert np.array_equal(got01.cpu().numpy(), want)
    sheet = torch.full(ops.sheet_shape(B, H, W, 2, 1) + (3,), 7, dtype=torch.uint8, device=dev)
    bad = torch.zeros(B, dtype=torch.int32, device=dev)
    assert ops.image_u8(x.to(dev), B, H, W, out=sheet, cols=2, pad=1, bad=bad) is sheet
    s = sheet.cpu().numpy()
    assert np.array_equal(s[1:1 + H, 1 + (W + 1):1 + (W + 1) + W], want[1]) and np.array_equal(s[2 + H:2 + 2 * H, 1:1 + W], want[2])
    assert (s[0] == 7).all() and (s[:, 0] == 7).all() and (s[2 + H:, 2 + W:] == 7).all() and bad.tolist() == [0, 0, 0]
    for kw, words in ((dict(cols=2), "pass it as `out`"), (dict(out=sheet[:3]), "at least"), (dict(out=sheet.float()), "uint8"),
                      (dict(out=sheet, cols=0), "cols"), (dict(out=sheet, pad=-1), "pad"),
                      (dict(bad=torch.zeros(B, device=dev)), "int32")):
        with pytest.raises(ValueError, match=words):
            ops.image_u8(x.to(dev), B, H, W, **kw)
    with pytest.raises(ValueError, match="do not fit"):
        ops.image_u8(x.to(dev)[:-1], B, H, W)


# ---- 4. non-finite values ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_nonfinite_values_and_the_bad_flags(val_dev, dtype):
    B, H, W, Cn = 3, 5, 9, 3
    x = draw(B * H * W * Cn, dtype, seed=4)
    clean, bad = run_dense(val_dev, x, B, H, W, Cn)
    assert bad == [0, 0, 0]
    n = H * W * Cn
    at = {n + 1: float("nan"), n + 40: float("inf"), 2 * n - 1: float("-inf")}  # head, middle and last element of image 1
    y = x.clone()
    for i, v in at.items():
        y[i] = v
    got, bad = run_dense(val_dev, y, B, H, W, Cn)
    assert bad == [0, 1, 0]
    flat = got.reshape(-1)
    assert [int(flat[i]) for i in at] == [0, 255, 0]
    keep = np.ones(B * n, dtype=bool)
    keep[list(at)] = False
    assert np.array_equal(flat[keep], clean.reshape(-1)[keep]), "a non-finite element changed other bytes"
    got2, none = run_dense(val_dev, y, B, H, W, Cn, want_bad=False)  # bad = NULL is taken, and nothing is stored there
    assert np.array_equal(got2, got) and none == [0, 0, 0]


# ---- 5. refusals, the seam --------------------------------------------------------------------------------------------------------
BAD_ARGS = [(dict(x=None), "null pointer"), (dict(out=None), "null pointer"), (dict(B=0), "bad shape"), (dict(H=0), "bad shape"),
            (dict(W=-1), "bad shape"), (dict(C=0), "channels"), (dict(C=5), "channels"), (dict(cols=0), "cols"), (dict(pad=-1), "pad"),
            (dict(out_pitch=11), "out_pitch"), (dict(cols=2, out_pitch=12), "out_pitch"), (dict(pad=1, out_pitch=14), "out_pitch")]


def test_bad_arguments_are_refused_by_name(val_dev):
    dev = val_dev
    B, H, W, Cn = 2, 3, 4, 3
    x = draw(B * H * W * Cn, torch.float32, seed=2).reshape(-1, Cn).to(dev)
    out = torch.full((B * H + 8, 2 * W * Cn + 8), FILL, dtype=torch.uint8, device=dev)
    call = ops.image_kernels().image_u8
    good = dict(x=x, out=out, bad=None, B=B, H=H, W=W, C=Cn, denorm=True, out_pitch=W * Cn, cols=1, pad=0)
    for change, words in BAD_ARGS + [(dict(x=x.half()), "bad dtype")]:
        with pytest.raises(RuntimeError, match=f"comat_image_u8.*{words}"):
            call(**{**good, **change})
    sync(dev)
    assert bool((out == FILL).all()), "a refused call wrote"
    call(**good)
    call(**{**good, "cols": 2, "out_pitch": 2 * W * Cn})  # exactly the widest row
    sync(dev)


def test_library_refuses_without_launching():
    """the cross-compiled library's own checks, without a GPU (as tests/test_abi.py does for other entry points)"""
    lib = _hip.load_library()
    src, dst = C.create_string_buffer(64), C.create_string_buffer(64)
    good = dict(x=C.addressof(src), out=C.addressof(dst), bad=None, B=2, H=3, W=4, C=3, dtype=_hip.F32, denorm=1, out_pitch=12, cols=1,
                pad=0, stream=None)
    for change, words in BAD_ARGS + [(dict(dtype=_hip.FP8), "bad dtype"), (dict(dtype=-1), "bad dtype")]:
        assert lib.comat_image_u8(*{**good, **change}.values()) == -1, change
        msg = lib.comat_last_error().decode()
        assert "comat_image_u8" in msg and words in msg, (change, msg)
    assert dst.raw == bytes(64)


def test_simulator_mirror_has_the_bindings_argument_list():
    names, differ = sim_matches_binding()
    assert names == ("image_u8",) and not differ
    assert "comat_image_u8" in _hip.SIGNATURES and _hip.ABI_VERSION == 8


def test_image_kernels_hands_out_the_installed_backend(sim):
    assert ops.image_kernels() is _hip  # the plain simulator lacks the entry point: the binding answers (and refuses CPU tensors)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.image_u8(torch.zeros(4, 3), 1, 2, 2)
    k = ValidateSimKernels()
    ops.set_kernel_backend(k)
    assert ops.image_kernels() is k
