"""CPU simulator of the entry points added after tests/sim_backend.py was written — TEST INFRASTRUCTURE ONLY.

`SimKernelsExt` adds, in plain torch, the documented semantics (include/comat_hip.h) of comat_cfg_rescale_ddpm_fwd / _bwd and
comat_grad_norm_scale to `SimKernels`, with the argument lists of comat_amd._hip.HipKernels.  The test modules that need them
install it through fixtures of their own (`use_sim_ext`, `use_hip`, `release` below are what those fixtures call).
"""
from __future__ import annotations

import pytest
import torch

from sim_backend import SimKernels


class SimKernelsExt(SimKernels):
    def cfg_rescale_ddpm_fwd(self, x, eps2, z, x_prev, n, s, cx, ce, sigma, phi, batch, per_sample, stats):
        assert batch * per_sample == n and stats.dtype == torch.float32
        e2 = eps2.reshape(2, batch, per_sample).float()
        eu, ec = e2[0], e2[1]
        e = eu + s * (ec - eu)
        mu_t, mu_c = ec.mean(1, keepdim=True), e.mean(1, keepdim=True)
        V_t, V_c = ((ec - mu_t) ** 2).sum(1, keepdim=True), ((e - mu_c) ** 2).sum(1, keepdim=True)
        stats.reshape(-1)[: 4 * batch].copy_(torch.cat([mu_t, V_t, mu_c, V_c], 1).reshape(-1))
        k = phi * torch.sqrt(V_t / V_c) + (1.0 - phi)
        v = cx * x.reshape(batch, per_sample) + ce * (k * e)
        if z is not None:
            v = v + sigma * z.reshape(batch, per_sample)
        x_prev.reshape(-1).copy_(v.reshape(-1))

    def cfg_rescale_ddpm_bwd(self, g, eps2, stats, dx, deps2, n, s, cx, ce, phi, batch, per_sample):
        assert batch * per_sample == n
        e2 = eps2.reshape(2, batch, per_sample).float()
        eu, ec = e2[0], e2[1]
        e = eu + s * (ec - eu)
        st = stats.reshape(-1)[: 4 * batch].reshape(batch, 4)
        mu_t, V_t, mu_c, V_c = (st[:, i:i + 1] for i in range(4))
        r = torch.sqrt(V_t / V_c)
        k = phi * r + (1.0 - phi)
        gf = g.reshape(batch, per_sample).float()
        d = ce * gf
        D = (d * e).sum(1, keepdim=True)
        de = k * d - D * phi * r * (e - mu_c) / V_c
        dec = D * phi * r * (ec - mu_t) / V_t
        if dx is not None:
            dx.reshape(-1).copy_((cx * gf).reshape(-1))
        out = deps2.reshape(2, n)
        out[0].copy_(((1.0 - s) * de).reshape(-1).to(deps2.dtype))
        out[1].copy_((s * de + dec).reshape(-1).to(deps2.dtype))

    def grad_norm_scale(self, g, g_out, n, norm_out, target):
        gf = g.reshape(-1)[:n].float()
        norm = gf.double().pow(2).sum().sqrt().float()
        norm_out[0] = norm
        if target > 0:
            c = target / norm if float(norm) > 0 else 0.0  # a zero gradient stays zero
            g_out.reshape(-1)[:n].copy_((gf * c).to(g_out.dtype))


def use_sim_ext():
    from comat_amd import ops
    ops.set_kernel_backend(SimKernelsExt())
    return torch.device("cpu")


def use_hip():
    from comat_amd import _hip, ops
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    ops.set_kernel_backend(_hip.HipKernels())  # raises if the .so is missing: no silent fallback
    return torch.device("cuda:0")


def release():
    """the teardown of tests/conftest.py: a test owns its backend instance and with it every per-stream workspace"""
    from comat_amd import ops
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except Exception:  # noqa: BLE001 - a pending error of the test that just failed
            pass
        ops.reset_capture_stream(torch.device("cuda:0"))
    ops.drop_side_stream_state()
    ops.set_kernel_backend(None)
