"""CPU simulator of the entry points of the sampler's other modes — TEST INFRASTRUCTURE ONLY.

`SimKernelsModes` adds, in plain torch, the documented semantics (include/comat_hip.h) of comat_ddpm_step2_fwd / _bwd and
comat_add_noise_fwd to `SimKernelsExt`, with the argument lists of comat_amd._hip.HipKernels.  `use_sim_modes`, `use_hip` and
`release` are what the fixtures of the test modules call.
"""
from __future__ import annotations

import torch

from sim_backend_ext import SimKernelsExt, release, use_hip  # noqa: F401 - re-exported


class SimKernelsModes(SimKernelsExt):
    @staticmethod
    def _guided(eps, halves, batch, per_sample, s):
        e2 = eps.reshape(halves, batch, per_sample).float()
        if halves == 1:
            return e2[0], None
        return e2[0] + s * (e2[1] - e2[0]), e2[1]

    def ddpm_step2_fwd(self, x, eps, z, x_prev, x0, n, halves, s, cx, ce, sigma, px, pe, phi, batch, per_sample, stats):
        assert batch * per_sample == n and halves in (1, 2) and (halves == 2 or phi == 0) and per_sample % 4 == 0
        assert x_prev is not None or x0 is not None
        e, ec = self._guided(eps, halves, batch, per_sample, s)
        k = 1.0
        if phi > 0:
            mu_t, mu_c = ec.mean(1, keepdim=True), e.mean(1, keepdim=True)
            V_t, V_c = ((ec - mu_t) ** 2).sum(1, keepdim=True), ((e - mu_c) ** 2).sum(1, keepdim=True)
            stats.reshape(-1)[: 4 * batch].copy_(torch.cat([mu_t, V_t, mu_c, V_c], 1).reshape(-1))
            k = phi * torch.sqrt(V_t / V_c) + (1.0 - phi)
        xs = x.reshape(batch, per_sample)
        if x_prev is not None:
            v = cx * xs + ce * (k * e)
            if z is not None:
                v = v + sigma * z.reshape(batch, per_sample)
            x_prev.reshape(-1).copy_(v.reshape(-1))
        if x0 is not None:
            x0.reshape(-1).copy_((px * xs + pe * (k * e)).reshape(-1))

    def ddpm_step2_bwd(self, g_prev, g_x0, eps, stats, dx, deps, n, halves, s, cx, ce, px, pe, phi, batch, per_sample,
                       eps_dtype=None):
        assert batch * per_sample == n and (g_prev is not None or g_x0 is not None) and (dx is not None or deps is not None)
        zero = torch.zeros(batch, per_sample)
        gp = zero if g_prev is None else g_prev.reshape(batch, per_sample).float()
        gx = zero if g_x0 is None else g_x0.reshape(batch, per_sample).float()
        d = ce * gp + pe * gx
        if dx is not None:
            dx.reshape(-1).copy_((cx * gp + px * gx).reshape(-1))
        if deps is None:
            return
        if halves == 1:
            deps.reshape(-1).copy_(d.reshape(-1).to(deps.dtype))
            return
        de, dec = d, 0.0
        if phi > 0:
            e, ec = self._guided(eps, halves, batch, per_sample, s)
            st = stats.reshape(-1)[: 4 * batch].reshape(batch, 4)
            mu_t, V_t, mu_c, V_c = (st[:, i:i + 1] for i in range(4))
            r = torch.sqrt(V_t / V_c)
            k = phi * r + (1.0 - phi)
            D = (d * e).sum(1, keepdim=True)
            de = k * d - D * phi * r * (e - mu_c) / V_c
            dec = D * phi * r * (ec - mu_t) / V_t
        out = deps.reshape(2, n)
        out[0].copy_(((1.0 - s) * de).reshape(-1).to(deps.dtype))
        out[1].copy_((s * de + dec).reshape(-1).to(deps.dtype))

    def add_noise_fwd(self, x, noise, noisy, xin, n, sa, sb, copies):
        assert copies in (1, 2) and xin.numel() == copies * n
        v = sa * x.reshape(-1).float() + sb * noise.reshape(-1).float()
        noisy.reshape(-1).copy_(v)
        xin.reshape(copies, n).copy_(v.to(xin.dtype).expand(copies, n))


def use_sim_modes():
    from comat_amd import ops
    ops.set_kernel_backend(SimKernelsModes())
    return torch.device("cpu")
