"""8-bit blockwise AdamW state (`--use_8bit_adam`, training_script.py:216-223) without a GPU: the two code books and the library's
literals of them, the float64 restatement the GPU tests check against (tests/optim8_reference.py), the configuration field, and the
refusals - of the optimizer under a backend without the kernels, and of the cross-compiled library's entry points."""
import ctypes as C

import pytest
import torch

import optim8_reference as R
from comat_amd import _hip, optim8
from comat_amd.step import StepConfig

F32 = torch.float32


# ---- code books ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
def test_dynamic_map(signed):
    t = optim8.dynamic_map(signed)
    assert t.dtype == F32 and t.shape == (256,)
    assert bool((t[1:] > t[:-1]).all()), "256 distinct ascending values"
    assert float(t[-1]) == 1.0 and float(t.abs().max()) == 1.0
    zero = optim8.zero_code(signed)
    assert zero == (127 if signed else 0) and float(t[zero]) == 0.0 and int((t == 0).sum()) == 1
    gaps = (t[1:].double() - t[:-1].double())
    if signed:
        assert float(t[0]) > -1.0
        assert t[126].item() == -t[128].item() == -torch.tensor(5.5e-7, dtype=torch.float64).float().item()
        assert float(gaps.max()) == pytest.approx(0.9 / 64, rel=1e-5)
        assert torch.equal(t[:127], -t[128:255].flip(0)), "symmetric apart from +1.0"
    else:
        assert float(t[0]) == 0.0 and t[1].item() == torch.tensor(3.25e-7, dtype=torch.float64).float().item()
        assert float(gaps.max()) == pytest.approx(0.9 / 128, rel=1e-5)


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
def test_library_carries_the_same_bits(signed):
    """comat_q8_map copies the literals of csrc/q8_maps.inc to host memory: the float64 construction, bit for bit"""
    got = optim8.q8_map(signed)
    assert torch.equal(got.view(torch.int32), optim8.dynamic_map(signed).view(torch.int32))


def test_literal_file_is_what_the_module_prints():
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(optim8.__file__)), "csrc", "q8_maps.inc")
    assert open(path).read() == optim8.maps_inc_text()


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def hard_values(signed, seed=0):
    """blocks of 256: all zero, one 1e30 among 1e-30s, denormals, negative only, exact table entries, Gaussian; then a partial block"""
    gen = torch.Generator().manual_seed(seed)
    t = optim8.dynamic_map(signed)
    big = torch.full((256,), 1e-30)
    big[77] = 1e30
    blocks = [torch.zeros(256), big, torch.rand(256, generator=gen) * 1e-39, -torch.rand(256, generator=gen) - 0.01,
              t[torch.randperm(256, generator=gen)] * 0.5, torch.randn(256, generator=gen), torch.randn(37, generator=gen) * 1e-3]
    x = torch.cat(blocks).float()
    return x if signed else torch.cat([x[:768], x[768:1024], x[1024:].abs()])  # (the negative block stays: it quantises to zero)


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
def test_restatement_round_trip(signed):
    x = hard_values(signed)
    codes, absmax = R.quantize(x, signed)
    assert codes.dtype == torch.uint8 and absmax.dtype == F32 and absmax.numel() == 7
    assert torch.equal(absmax, R.block_max(x)) and float(absmax[0]) == 0.0 and float(absmax[1]) == float(torch.tensor(1e30))
    assert bool((codes[:256] == optim8.zero_code(signed)).all()), "an all-zero block gets the zero code"
    back = R.dequantize(codes, absmax, signed)
    assert back.dtype == F32 and bool(torch.isfinite(back).all())
    a = R.per_element(absmax, x.numel()).double()
    gap = 0.9 / 64 if signed else 0.9 / 128
    inside = torch.ones_like(x, dtype=torch.bool) if signed else x >= 0  # the unsigned table holds nothing below zero
    # half the largest gap of the table (the nominal 0.9 / count: the entries are its fp32 roundings, 2^-25 each at most), plus
    # the rounding of the one fp32 product (2^-24 of the scale; below the normal range half a denormal step)
    assert bool(((back.double() - x.double()).abs() <= gap / 2 * a + a * 2.0 ** -23 + 1e-45)[inside].all())
    assert bool((back[~inside] == 0).all())
    R.assert_nearest_or_tied(x, codes, absmax, signed, 0.0, "the restatement's own codes")
    exact = slice(1024, 1280)  # values on table entries come back as they were
    assert torch.equal(back[exact], x[exact])


def test_restatement_update_is_adamw():
    gen = torch.Generator().manual_seed(3)
    p, g = torch.randn(300, generator=gen), torch.randn(300, generator=gen)
    q = torch.nn.Parameter(p.clone().double())
    q.grad = g.clone().double()
    opt = torch.optim.AdamW([q], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    m = v = torch.zeros(300, dtype=torch.float64)
    pp = p
    for t in (1, 2):
        opt.step()
        pp, m, v = R.adamw(pp, g, m, v, 1e-2, 0.9, 0.999, 1e-8, 1e-2, t, 1.0)
    assert torch.allclose(pp, q.detach(), rtol=1e-12, atol=1e-14)
    assert R.clip_factor(4.0, 0.1, 0.5) == pytest.approx(0.1 / (2.0 * 0.5 + 1e-6) * 0.5) and R.clip_factor(1e-6, 0.1, 1.0) == 1.0


# ---- configuration and refusals -------------------------------------------------------------------------------------------------
def test_config_field():
    assert StepConfig().use_8bit_adam is False and StepConfig.sdxl().use_8bit_adam is False
    assert StepConfig(use_8bit_adam=True).use_8bit_adam is True


def test_no_cpu_path(sim):
    p, g = torch.zeros(8192), torch.zeros(8192)
    with pytest.raises(RuntimeError, match="use_8bit_adam"):
        optim8.FlatAdamW8bit([(p, g)], 1e-2, (0.9, 0.999), 1e-8, 1e-2, 0.1)


def test_library_refuses_without_launching():
    """null pointers and misaligned pointers come back as -1 with the entry point's name, without a launch (no GPU here)"""
    lib = _hip.load_library()
    A = 1 << 20  # an aligned address that is never dereferenced: every case below is refused before the launch
    adamw8 = lambda p=A, g=A, m8=A, v8=A, am=A, av=A, n=8, lr=A, step=A, gs=1.0, accum=1: lib.comat_adamw8_window(
        p, g, m8, v8, am, av, n, lr, 0.9, 0.999, 1e-8, 0.0, step, None, 0.1, gs, None, accum, None)
    cases = [("comat_q8_map", lambda: lib.comat_q8_map(1, None)),
             ("comat_q8_map", lambda: lib.comat_q8_map(2, (C.c_float * 256)())),
             ("comat_q8_quantize_blockwise", lambda: lib.comat_q8_quantize_blockwise(None, A, A, 8, 1, None)),
             ("comat_q8_quantize_blockwise", lambda: lib.comat_q8_quantize_blockwise(A, None, A, 8, 1, None)),
             ("comat_q8_quantize_blockwise", lambda: lib.comat_q8_quantize_blockwise(A, A, None, 8, 1, None)),
             ("comat_q8_quantize_blockwise", lambda: lib.comat_q8_quantize_blockwise(A, A, A, 0, 1, None)),
             ("comat_q8_quantize_blockwise", lambda: lib.comat_q8_quantize_blockwise(A, A, A, 8, 2, None)),
             ("comat_q8_quantize_blockwise", lambda: lib.comat_q8_quantize_blockwise(A + 4, A, A, 8, 1, None)),
             ("comat_q8_quantize_blockwise", lambda: lib.comat_q8_quantize_blockwise(A, A + 2, A, 8, 1, None)),
             ("comat_q8_quantize_blockwise", lambda: lib.comat_q8_quantize_blockwise(A, A, A + 8, 8, 1, None)),
             ("comat_q8_dequantize_blockwise", lambda: lib.comat_q8_dequantize_blockwise(None, A, A, 8, 0, None)),
             ("comat_q8_dequantize_blockwise", lambda: lib.comat_q8_dequantize_blockwise(A, None, A, 8, 0, None)),
             ("comat_q8_dequantize_blockwise", lambda: lib.comat_q8_dequantize_blockwise(A, A, None, 8, 0, None)),
             ("comat_q8_dequantize_blockwise", lambda: lib.comat_q8_dequantize_blockwise(A + 1, A, A, 8, 0, None)),
             ("comat_q8_dequantize_blockwise", lambda: lib.comat_q8_dequantize_blockwise(A, A + 4, A, 8, 0, None)),
             ("comat_q8_dequantize_blockwise", lambda: lib.comat_q8_dequantize_blockwise(A, A, A + 12, 8, 0, None)),
             ("comat_q8_dequantize_blockwise", lambda: lib.comat_q8_dequantize_blockwise(A, A, A, -3, 0, None))]
    cases += [("comat_adamw8_window", lambda kw=kw: adamw8(**kw)) for kw in (
        dict(p=None), dict(g=None), dict(m8=None), dict(v8=None), dict(am=None), dict(av=None), dict(lr=None), dict(step=None),
        dict(n=0), dict(gs=0.0), dict(accum=0), dict(p=A + 4), dict(g=A + 8), dict(m8=A + 1), dict(v8=A + 2), dict(am=A + 4),
        dict(av=A + 12))]
    for name, call in cases:
        lib.comat_last_error.restype = C.c_char_p
        assert call() == -1, name
        assert name.encode() + b":" in lib.comat_last_error(), (name, lib.comat_last_error())
    out = (C.c_float * 256)()
    assert lib.comat_q8_map(0, out) == 0 and out[0] == 0.0 and out[255] == 1.0
