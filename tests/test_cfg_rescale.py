"""Rescaled classifier-free guidance fused with the DDPM step (comat_cfg_rescale_ddpm_fwd / _bwd, ops.cfg_ddpm_step(...,
rescale=phi, batch=B)): `rescale_noise_cfg` of the reference's denoise loop (TrainableSDPipeline.py:155-161) followed by the
scheduler step.  Reference of the parity cases: the formula evaluated by torch autograd in fp64 on the dtype-rounded inputs.
Tolerance: helpers.check (2e-4 fp32, 3e-2 bf16 of the reference's maximum), the bound of the unrescaled op."""
import ctypes as C

import pytest
import torch

from comat_amd import ops
from helpers import check

DTYPES = [torch.float32, torch.bfloat16]
S, CX, CE, SG = 7.5, 0.93, -0.21, 0.05


def rnd(*shape, dtype=torch.float32, seed=0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) + offset).to(dtype).float()


def dv(x, dev, dtype=None, grad=False):
    t = x.detach().to(device=dev, dtype=dtype or x.dtype).contiguous()
    return t.clone().requires_grad_(True) if grad else t


def inputs(batch, P, dtype, offset=0.0):
    n = batch * P
    return rnd(n, seed=1), rnd(n, seed=2), rnd(2 * n, dtype=dtype, seed=3, offset=offset), rnd(n, seed=4)


def reference(x, e2, z, g, batch, P, phi, s=S):
    """the issue's formula by fp64 autograd: -> x', dx, deps2"""
    n = batch * P
    xr, er = x.double().requires_grad_(True), e2.double().requires_grad_(True)
    eu, ec = er[:n].reshape(batch, P), er[n:].reshape(batch, P)
    e = eu + s * (ec - eu)
    k = phi * (ec.std(1, keepdim=True) / e.std(1, keepdim=True)) + (1 - phi)
    out = CX * xr + CE * (k * e).reshape(-1) + SG * z.double()
    out.backward(g.double())
    return out.detach(), xr.grad, er.grad


def run(dev, x, e2, z, g, batch, dtype, phi, eps_grad=True):
    xd, ed = dv(x, dev, grad=True), dv(e2, dev, dtype, grad=eps_grad)
    out = ops.cfg_ddpm_step(xd, ed, dv(z, dev), S, CX, CE, SG, rescale=phi, batch=batch)
    out.backward(dv(g, dev))
    return out.detach(), xd.grad, ed.grad


CASES = [(2, 256, 0.0, 0.7), (3, 1024, 3.0, 0.7), (1, 16384, 0.0, 0.7), (4, 16384, 0.0, 0.7), (1, 65536, 0.0, 0.7),
         (4, 16384, 0.0, 1.0)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("batch,P,offset,phi", CASES)
def test_rescaled_step_against_fp64_autograd(dev, dtype, batch, P, offset, phi):
    x, z, e2, g = inputs(batch, P, dtype, offset)
    ref, rdx, rde = reference(x, e2, z, g, batch, P, phi)
    out, dx, de = run(dev, x, e2, z, g, batch, dtype, phi)
    for name, got, want, dt_ in (("fwd", out, ref, torch.float32), ("dx", dx, rdx, torch.float32), ("deps2", de, rde, dtype)):
        err = (got.double().cpu() - want).abs().max().item() / (want.abs().max().item() + 1e-6)
        print(f"rescale {name} B={batch} P={P} {dtype}: max err / max ref = {err:.3e}")
    check(out, ref, torch.float32, "rescale fwd")
    check(dx, rdx, torch.float32, "rescale dx")
    check(de, rde, dtype, "rescale deps2")
    assert de.dtype == dtype


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("batch,P", [(2, 256), (4, 16384), (1, 65536)])
def test_phi_zero_gives_the_bits_of_the_plain_step(hip, dtype, batch, P):
    k = ops.kernels()
    n = batch * P
    x, z, e2, g = (dv(t, hip, dt_) for t, dt_ in zip(inputs(batch, P, dtype), (None, None, dtype, None)))
    a, b = torch.empty_like(x), torch.empty_like(x)
    stats = torch.empty((batch, 4), dtype=torch.float32, device=hip)
    for zz in (z, None):
        k.cfg_ddpm_fwd(x, e2, zz, a, n, S, CX, CE, SG)
        k.cfg_rescale_ddpm_fwd(x, e2, zz, b, n, S, CX, CE, SG, 0.0, batch, P, stats)
        assert torch.equal(a, b), f"forward bits differ (z {'given' if zz is not None else 'null'})"
    da, db = torch.empty_like(e2), torch.empty_like(e2)
    dxa, dxb = torch.empty_like(x), torch.empty_like(x)
    k.cfg_ddpm_bwd(g, dxa, da, n, S, CX, CE)
    k.cfg_rescale_ddpm_bwd(g, e2, stats, dxb, db, n, S, CX, CE, 0.0, batch, P)
    assert torch.equal(dxa, dxb) and torch.equal(da.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                                                 db.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
    k.cfg_rescale_ddpm_bwd(g, e2, stats, None, db, n, S, CX, CE, 0.0, batch, P)  # dx may be null
    assert torch.equal(da, db)


@pytest.mark.parametrize("dtype", DTYPES)
def test_phi_one_matches_the_std_of_the_text_prediction(dev, dtype):
    batch, P = 3, 4096
    x, z, e2, g = inputs(batch, P, dtype, 1.5)
    out, _, _ = run(dev, x, e2, z, g, batch, dtype, 1.0)
    eps = ((out.cpu().double() - CX * x.double() - SG * z.double()) / CE).reshape(batch, P)
    want = e2[batch * P:].double().reshape(batch, P).std(1)
    check(eps.std(1), want, torch.float32, "std of the rescaled noise")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_same_bits_on_every_run_and_in_a_graph_replay(hip, dtype):
    batch, P = 4, 16384
    x, z, e2, g = inputs(batch, P, dtype)
    first = run(hip, x, e2, z, g, batch, dtype, 0.7)
    second = run(hip, x, e2, z, g, batch, dtype, 0.7)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    # forward + backward captured on the package's capture stream (its workspaces exist before the capture begins)
    xs, es, zs, gs = dv(x, hip, grad=True), dv(e2, hip, dtype, grad=True), dv(z, hip), dv(g, hip)
    cap = ops.capture_stream(hip)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with ops.graph_capture(graph, stream=cap):
        out = ops.cfg_ddpm_step(xs, es, zs, S, CX, CE, SG, rescale=0.7, batch=batch)
        dx, de = torch.autograd.grad(out, (xs, es), gs)
    for _ in range(2):
        out.zero_(), dx.zero_(), de.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(first, (out, dx, de)):
            assert torch.equal(a, b.detach())


def test_untrained_step_keeps_nothing_for_backward(dev):
    batch, P, dtype = 2, 1024, torch.float32
    x, z, e2, g = inputs(batch, P, dtype)
    calls = []
    k = ops.kernels()
    bwd = k.cfg_rescale_ddpm_bwd
    k.cfg_rescale_ddpm_bwd = lambda *a, **kw: (calls.append(1), bwd(*a, **kw))
    xd = dv(x, dev, grad=True)
    out = ops.cfg_ddpm_step(xd, dv(e2, dev), dv(z, dev), S, CX, CE, SG, rescale=0.7, batch=batch)
    assert out.grad_fn.saved_tensors == ()
    out.backward(dv(g, dev))
    assert not calls, "the rescaled backward kernel ran for a step whose eps2 takes no gradient"
    assert torch.equal(xd.grad.cpu(), (CX * g))
    ref, _, _ = reference(x, e2, z, g, batch, P, 0.7)
    check(out, ref, torch.float32, "untrained fwd")
    with torch.no_grad():
        o2 = ops.cfg_ddpm_step(dv(x, dev), dv(e2, dev), dv(z, dev), S, CX, CE, SG, rescale=0.7, batch=batch)
    assert torch.equal(o2, out.detach())


def test_rescale_needs_the_batch(sim):
    with pytest.raises(ValueError, match="batch"):
        ops.cfg_ddpm_step(torch.zeros(8), torch.zeros(16), None, S, CX, CE, SG, rescale=0.5)


def test_library_exports_and_validates_the_new_entry_points():
    """no GPU needed: argument errors come back as -1 + a message, nothing is launched"""
    from comat_amd import _hip
    lib = _hip.load_library()
    for name in ("comat_cfg_rescale_ddpm_fwd", "comat_cfg_rescale_ddpm_bwd", "comat_grad_norm_scale"):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    # per_sample * batch != n
    assert lib.comat_cfg_rescale_ddpm_fwd(p, p, None, p, 32, 7.5, 1.0, 1.0, 0.0, 0.7, 3, 8, p, 0, None) == -1
    assert b"per_sample" in lib.comat_last_error()
    assert lib.comat_cfg_rescale_ddpm_bwd(p, p, p, None, p, 32, 7.5, 1.0, 1.0, 0.7, 3, 8, 0, None) == -1
    assert b"per_sample" in lib.comat_last_error()
    # null statistics
    assert lib.comat_cfg_rescale_ddpm_fwd(p, p, None, p, 32, 7.5, 1.0, 1.0, 0.0, 0.7, 4, 8, None, 0, None) == -1
    assert b"statistics" in lib.comat_last_error()
    assert lib.comat_cfg_rescale_ddpm_bwd(p, p, None, None, p, 32, 7.5, 1.0, 1.0, 0.7, 4, 8, 0, None) == -1
    assert b"statistics" in lib.comat_last_error()
    assert lib.comat_grad_norm_scale(None, None, 0, 0, None, 0.0, None, None) == -1
    assert lib.comat_grad_norm_scale(p, None, 16, 0, p, 1e4, p, None) == -1  # target > 0 without an output
    assert b"g_out" in lib.comat_last_error()
    assert lib.comat_abi_version() == 8
