"""The kernels of the sampler's other modes: comat_ddpm_step2_fwd / _bwd (guidance on or off, x_prev and / or the scheduler's
pred_original_sample, rescaled or not; ops.ddpm_step) and comat_add_noise_fwd (ops.add_noise).  Reference: the header's
formulas evaluated by torch autograd in fp64 on the dtype-rounded inputs.  Tolerance: helpers.check (2e-4 fp32, 3e-2 bf16 of the
reference's maximum), the bound tests/test_cfg_rescale.py holds the same quantities to.  Every operand sits in a
helpers.Window: NaN halos around the inputs, guard bands around the outputs that are compared bit for bit.
Shapes: per_sample 4 (one vector), 80 (the sampler fixture's sample), 4096 (exactly one pass of a 1 024-lane block), 4100 (one
lane into a second pass); 1 and 3 samples."""
import ctypes as C
import functools

import pytest
import torch

from comat_amd import ops
from helpers import Window, check

DTYPES = [torch.float32, torch.bfloat16]
F32 = torch.float32
S, CX, CE, SG, PX, PE = 7.5, 0.93, -0.21, 0.05, 1.9, -1.6
PS = [4, 80, 4096, 4100]
VARIANTS = [(1, 0.0), (2, 0.0), (2, 0.7)]  # (halves, phi)


def rnd(*shape, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype).float()


def flat(x, dtype, dev):
    """a vector between 64 NaN guard elements on either side (16-byte aligned for every dtype)"""
    x = x.reshape(1, -1)
    return Window(1, x.shape[1], x.shape[1] + 64, dtype, dev, lead=0, trail=0, left=64).put(x)


def flat_out(n, dtype, dev):
    return Window(1, n, n + 64, dtype, dev, lead=0, trail=0, left=64).arm()


def settle(w, ref, dtype, what):
    w.assert_guard_intact(what)
    w.assert_written(what)
    check(w.get(), ref.reshape(w.view.shape), dtype, what)


@functools.lru_cache(maxsize=None)
def data(batch, P, halves, dtype):
    n = batch * P
    return rnd(n, seed=1), rnd(n, seed=2), rnd(halves * n, dtype=dtype, seed=3), rnd(n, seed=4), rnd(n, seed=5)


@functools.lru_cache(maxsize=None)
def reference(batch, P, halves, phi, dtype, with_z, use_gp, use_gx):
    """the header's formulas by fp64 autograd -> x_prev, x0, dx, deps (computed once per case, shared, never modified)"""
    x, z, e, gp, gx = data(batch, P, halves, dtype)
    n = batch * P
    xr, er = x.double().requires_grad_(True), e.double().requires_grad_(True)
    if halves == 2:
        eu, ec = er[:n].reshape(batch, P), er[n:].reshape(batch, P)
        eg = eu + S * (ec - eu)
    else:
        eg = ec = er.reshape(batch, P)
    k = phi * (ec.std(1, keepdim=True) / eg.std(1, keepdim=True)) + (1 - phi) if phi > 0 else 1.0
    ke = (k * eg).reshape(-1)
    xp = CX * xr + CE * ke + (SG * z.double() if with_z else 0.0)
    x0 = PX * xr + PE * ke
    loss = (xp * gp.double()).sum() * float(use_gp) + (x0 * gx.double()).sum() * float(use_gx)
    loss.backward()
    return xp.detach(), x0.detach(), xr.grad, er.grad


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("halves,phi", VARIANTS)
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("P", PS)
def test_step2_against_fp64_autograd(dev, dtype, halves, phi, batch, P):
    k = ops.kernels()
    n = batch * P
    x, z, e, gp, gx = data(batch, P, halves, dtype)
    xw, zw, ew, gpw, gxw = flat(x, F32, dev), flat(z, F32, dev), flat(e, dtype, dev), flat(gp, F32, dev), flat(gx, F32, dev)
    tag = f"P={P} B={batch} halves={halves} phi={phi} {dtype}"
    stw = flat_out(4 * batch, F32, dev)
    # forward: x_prev only, x0 only, both; z present and NULL
    for with_z in (True, False):
        rxp, rx0, _, _ = reference(batch, P, halves, phi, dtype, with_z, True, True)
        for want_prev, want_x0 in ((True, False), (False, True), (True, True)):
            pw, ow = flat_out(n, F32, dev), flat_out(n, F32, dev)
            stw.arm()
            k.ddpm_step2_fwd(xw.flat, ew.flat, zw.flat if with_z else None, pw.flat if want_prev else None,
                             ow.flat if want_x0 else None, n, halves, S, CX, CE, SG, PX, PE, phi, batch, P,
                             stw.flat if phi > 0 else None)
            stw.assert_guard_intact(f"stats {tag}")
            for w, want, ref, name in ((pw, want_prev, rxp, "x_prev"), (ow, want_x0, rx0, "x0")):
                if want:
                    settle(w, ref, F32, f"{name} {tag} z={with_z}")
                else:  # an output that was not asked for is not touched at all
                    w.assert_guard_intact(f"{name} (null) {tag}")
                    assert torch.isnan(w.get()).all()
    if phi > 0:
        stw.assert_written(f"stats {tag}")
    # backward: g_prev only, g_x0 only, both; dx NULL; deps NULL (an untrained step)
    for use_gp, use_gx in ((True, False), (False, True), (True, True)):
        _, _, rdx, rde = reference(batch, P, halves, phi, dtype, True, use_gp, use_gx)
        for want_dx, want_de in ((True, True), (False, True), (True, False)):
            dxw, dew = flat_out(n, F32, dev), flat_out(halves * n, dtype, dev)
            stw.arm()
            k.ddpm_step2_bwd(gpw.flat if use_gp else None, gxw.flat if use_gx else None, ew.flat, stw.flat if phi > 0 else None,
                             dxw.flat if want_dx else None, dew.flat if want_de else None, n, halves, S, CX, CE, PX, PE, phi,
                             batch, P, eps_dtype=dtype)
            stw.assert_guard_intact(f"stats (read by bwd) {tag}")
            what = f"{tag} g_prev={use_gp} g_x0={use_gx}"
            if want_dx:
                settle(dxw, rdx, F32, f"dx {what}")
            else:
                dxw.assert_guard_intact(f"dx (null) {what}")
                assert torch.isnan(dxw.get()).all()
            if want_de:
                settle(dew, rde, dtype, f"deps {what}")
            else:
                dew.assert_guard_intact(f"deps (null) {what}")
                assert torch.isnan(dew.get().float()).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("P", PS)
def test_x_prev_has_the_bits_of_the_existing_steps_and_of_a_second_run(hip, dtype, batch, P):
    """x_prev against comat_cfg_ddpm_fwd (phi = 0) and comat_cfg_rescale_ddpm_fwd (phi = 0.7) on the same operands, alone and
    next to x0; two runs of forward and backward give the same bits"""
    k = ops.kernels()
    n = batch * P
    x, z, e, gp, gx = (t.to(hip, dt_) for t, dt_ in zip(data(batch, P, 2, dtype), (F32, F32, dtype, F32, F32)))
    stats, stats2 = (torch.empty((batch, 4), dtype=F32, device=hip) for _ in range(2))
    for phi in (0.0, 0.7):
        for zz in (z, None):
            want = torch.empty_like(x)
            if phi == 0.0:
                k.cfg_ddpm_fwd(x, e, zz, want, n, S, CX, CE, SG)
            else:
                k.cfg_rescale_ddpm_fwd(x, e, zz, want, n, S, CX, CE, SG, phi, batch, P, stats)
            alone, beside, x0a, x0b = (torch.empty_like(x) for _ in range(4))
            k.ddpm_step2_fwd(x, e, zz, alone, None, n, 2, S, CX, CE, SG, PX, PE, phi, batch, P, stats2)
            k.ddpm_step2_fwd(x, e, zz, beside, x0a, n, 2, S, CX, CE, SG, PX, PE, phi, batch, P, stats2)
            k.ddpm_step2_fwd(x, e, zz, None, x0b, n, 2, S, CX, CE, SG, PX, PE, phi, batch, P, stats2)
            what = f"phi={phi} z {'given' if zz is not None else 'null'}"
            assert torch.equal(bits(want), bits(alone)), f"x_prev bits differ ({what})"
            assert torch.equal(bits(want), bits(beside)), f"x_prev bits differ next to x0 ({what})"
            assert torch.equal(bits(x0a), bits(x0b)), f"x0 bits differ with and without x_prev ({what})"
            if phi > 0:
                assert torch.equal(bits(stats), bits(stats2)), "statistics differ from the rescaled kernel's"
        runs = []
        for _ in range(2):
            dx, de = torch.empty_like(x), torch.empty_like(e)
            k.ddpm_step2_bwd(gp, gx, e, stats2, dx, de, n, 2, S, CX, CE, PX, PE, phi, batch, P)
            runs.append((dx, de))
        assert torch.equal(bits(runs[0][0]), bits(runs[1][0])) and torch.equal(bits(runs[0][1]), bits(runs[1][1]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("halves,phi", VARIANTS)
def test_ops_ddpm_step_through_autograd(dev, dtype, halves, phi):
    """ops.ddpm_step as one autograd Function: both outputs used, then an untrained step (eps takes no gradient: only dx)"""
    batch, P = 3, 80
    x, z, e, gp, gx = data(batch, P, halves, dtype)
    rxp, rx0, rdx, rde = reference(batch, P, halves, phi, dtype, True, True, True)
    to = lambda t, dt_=F32: t.to(dev, dt_).clone()  # (a copy: the shared inputs stay as they are)
    xd, ed = to(x).requires_grad_(True), to(e, dtype).requires_grad_(True)
    xp, x0 = ops.ddpm_step(xd, ed, to(z), S, CX, CE, SG, halves=halves, x0_coef=(PX, PE), rescale=phi, batch=batch)
    torch.autograd.backward((xp, x0), (to(gp), to(gx)))
    check(xp, rxp, F32, "x_prev")
    check(x0, rx0, F32, "x0")
    check(xd.grad, rdx, F32, "dx")
    check(ed.grad, rde, dtype, "deps")
    assert ed.grad.dtype == dtype
    _, _, rdx0, _ = reference(batch, P, halves, phi, dtype, True, False, True)
    xd = to(x).requires_grad_(True)
    none, x0 = ops.ddpm_step(xd, to(e, dtype), None, S, CX, CE, SG, halves=halves, x0_coef=(PX, PE), want_prev=False,
                             rescale=phi, batch=batch)
    assert none is None and x0.grad_fn.saved_tensors == ()
    x0.backward(to(gx))
    check(x0, rx0, F32, "x0 alone")
    check(xd.grad, rdx0, F32, "dx of an untrained x0-only step")


def test_ops_ddpm_step_refuses_what_the_kernel_refuses(dev):
    x, e = torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    with pytest.raises(ValueError, match="rescale"):
        ops.ddpm_step(x, e, None, S, CX, CE, SG, halves=1, rescale=0.5, batch=1)
    with pytest.raises(ValueError, match="neither"):
        ops.ddpm_step(x, e, None, S, CX, CE, SG, halves=1, want_prev=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [4, 80, 1023, 4100])
def test_add_noise(dev, dtype, n):
    k = ops.kernels()
    sa, sb = 0.83, 0.56
    x, noise = rnd(n, seed=1), rnd(n, seed=2)
    ref = sa * x.double() + sb * noise.double()
    xw, nw = flat(x, F32, dev), flat(noise, F32, dev)
    for copies in (1, 2):
        yw, iw = flat_out(n, F32, dev), flat_out(copies * n, dtype, dev)
        k.add_noise_fwd(xw.flat, nw.flat, yw.flat, iw.flat, n, sa, sb, copies)
        settle(yw, ref, F32, f"noisy n={n}")
        settle(iw, ref.repeat(copies), dtype, f"xin n={n} copies={copies}")
        cast = yw.get().reshape(-1).to(dtype)
        got = iw.get().reshape(copies, n)
        for c in range(copies):  # every copy is the cast of `noisy`, bit for bit
            assert torch.equal(bits(got[c].contiguous()), bits(cast)), f"copy {c} of {copies}"
    noisy, xin = ops.add_noise(x.to(dev).reshape(-1, 1), noise.to(dev).reshape(-1, 1), sa, sb, 2, dtype)
    assert noisy.shape == (n, 1) and xin.shape == (2 * n, 1) and xin.dtype == dtype and not xin.requires_grad
    check(noisy, ref.reshape(-1, 1), F32, "ops.add_noise")


def test_library_exports_and_validates_the_new_entry_points():
    """no GPU needed: contract violations come back as -1 + a message, nothing is launched"""
    from comat_amd import _hip
    lib = _hip.load_library()
    for name in ("comat_ddpm_step2_fwd", "comat_ddpm_step2_bwd", "comat_add_noise_fwd"):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    fwd = lambda xp, x0, halves, phi, batch, P, stats: lib.comat_ddpm_step2_fwd(
        p, p, None, xp, x0, batch * P, halves, 7.5, 1.0, 1.0, 0.0, 1.0, 1.0, phi, batch, P, stats, 0, None)
    bwd = lambda gp, gx, dx, de, halves, phi, batch, P, stats: lib.comat_ddpm_step2_bwd(
        gp, gx, p, stats, dx, de, batch * P, halves, 7.5, 1.0, 1.0, 1.0, 1.0, phi, batch, P, 0, None)
    # guidance off takes no rescale
    assert fwd(p, None, 1, 0.7, 2, 8, p) == -1 and b"halves = 1" in lib.comat_last_error()
    assert bwd(p, None, p, p, 1, 0.7, 2, 8, p) == -1 and b"halves = 1" in lib.comat_last_error()
    # both outputs / both gradients null
    assert fwd(None, None, 2, 0.0, 2, 8, None) == -1 and b"both outputs" in lib.comat_last_error()
    assert bwd(None, None, p, p, 2, 0.0, 2, 8, None) == -1 and b"both gradients" in lib.comat_last_error()
    assert bwd(p, p, None, None, 2, 0.0, 2, 8, None) == -1 and b"both outputs" in lib.comat_last_error()
    # per_sample no multiple of 4
    assert fwd(p, p, 2, 0.0, 2, 6, None) == -1 and b"multiple of 4" in lib.comat_last_error()
    assert bwd(p, p, p, p, 2, 0.0, 2, 6, None) == -1 and b"multiple of 4" in lib.comat_last_error()
    # rescale without statistics, halves out of range, batch * per_sample != n
    assert fwd(p, None, 2, 0.7, 2, 8, None) == -1 and b"statistics" in lib.comat_last_error()
    assert fwd(p, None, 3, 0.0, 2, 8, None) == -1 and b"halves" in lib.comat_last_error()
    assert lib.comat_ddpm_step2_fwd(p, p, None, p, None, 32, 2, 7.5, 1.0, 1.0, 0.0, 1.0, 1.0, 0.0, 3, 8, None, 0, None) == -1
    assert b"per_sample" in lib.comat_last_error()
    assert lib.comat_add_noise_fwd(p, p, p, p, 16, 1.0, 1.0, 3, 0, None) == -1 and b"copies" in lib.comat_last_error()
    assert lib.comat_add_noise_fwd(p, p, None, p, 16, 1.0, 1.0, 1, 0, None) == -1
    assert lib.comat_abi_version() == 8
