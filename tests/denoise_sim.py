"""The ABI simulator with the three entry points of the denoising fine-tune (comat_denoise_prepare, comat_mse_fwd, comat_mse_bwd,
include/comat_hip.h) - TEST INFRASTRUCTURE ONLY.  The binding keeps their wrappers as module functions (comat_amd._hip.denoise_prepare,
mse_fwd, mse_bwd, handed out by ops.denoise_kernels()); this subclass of tests/validate_sim.py's simulator carries the mirrors under
the same names and argument lists, and the tests install it over the `sim` leg of conftest's `dev` fixture (`denoise_dev` below).

The mirrors are written from the header's definitions in numpy, fp32 step by step in the stated order:
  * prepare: x0 = scaling * (mean + exp(0.5 * clamp(logvar, -30, 20)) * z) with np.exp on float32 (the library's expf may differ from
    it in the last bits: the posterior path is held to float64 under a bound, not to these bits); the noising is the SIMULATOR's
    comat_add_noise_fwd arithmetic - sa * x0 and sb * noise rounded, then their sum - where the kernel reproduces the fused form of
    the library's comat_add_noise_fwd: each leg's prepare is compared with its own leg's add_noise_fwd;
  * mse_fwd: every term (pred - target)^2 from float64 rounded once, the lanes / butterfly / wave order of the header, so that its
    bits are the kernel's; mse_bwd: the coefficient from float64 rounded once, difference and product in fp32.
`launches` logs (entry point, kernel launches it stands for) per call.  Operands are pointers: read and written through their
storage from their first element on."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from sim_backend import _refuse
from validate_sim import ValidateSimKernels, _flat

f32 = np.float32
RT = 1024  # lanes of the per-sample block of comat_mse_fwd


def _np(t, n):
    return _flat(t, n).float().numpy()


def _ok(t):
    return t is not None and t.dtype in (torch.float32, torch.bfloat16)


def sq_sum_in_kernel_order(d64):
    """sum of the fp32-rounded squares of d64 [n] (float64) in comat_mse_fwd's order -> float32"""
    with np.errstate(over="ignore", invalid="ignore"):
        term = (d64 * d64).astype(f32)
        n = term.size
        K = -(-n // (4 * RT))
        pad = np.zeros(K * 4 * RT, dtype=f32)
        pad[:n] = term
        pad = pad.reshape(K, RT, 4)
        acc = np.zeros(RT, dtype=f32)
        for k in range(K):  # a lane adds its terms in ascending i
            for j in range(4):
                acc = (acc + pad[k, :, j]).astype(f32)
        v = acc.reshape(RT // 64, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):  # the xor butterfly inside a wave
            v = (v + v[:, lane ^ o]).astype(f32)
        s = f32(0)
        for wv in range(RT // 64):
            s = f32(s + v[wv, 0])
        return s


class DenoiseSimKernels(ValidateSimKernels):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.launches = []

    def denoise_prepare(self, moments, z, latents, noise, t, sab, sinus, wtab, xin, x0, temb, w, oob, scaling, T, B, P, C, C0):
        name = "comat_denoise_prepare"
        _refuse(name, (moments is not None) != (latents is not None),
                f"exactly one of moments and latents (got {'both' if moments is not None else 'neither'})")
        _refuse(name, not (latents is not None and z is not None), "z goes with moments, not with latents")
        _refuse(name, all(a is not None for a in (noise, t, sab, sinus, wtab, xin, temb, w)), "null pointer")
        _refuse(name, B > 0 and P > 0 and C > 0 and C0 > 0 and T > 0, "bad shape (B, P, C, C0, T must be positive)")
        _refuse(name, B <= 65535, f"B = {B}, at most 65535 samples a launch")
        _refuse(name, P * C <= 2 ** 31 - 1, "bad shape (P * C beyond 2^31 - 1)")
        _refuse(name, _ok(xin) and (moments is None or _ok(moments)), "bad dtype")
        assert t.dtype == torch.int32 and (oob is None or oob.dtype == torch.int32)
        self.launches.append((name, 1))
        n = P * C
        tb = _flat(t, B).numpy().astype(np.int64)
        tc = np.clip(tb, 0, T - 1)
        sabn = _np(sab, 2 * T).reshape(T, 2)
        with np.errstate(over="ignore", invalid="ignore"):
            if moments is not None:
                m = _np(moments, B * P * 2 * C).reshape(B * P, 2 * C)
                mean, lv = m[:, :C], m[:, C:]
                if z is None:
                    x = (f32(scaling) * mean).astype(f32)
                else:
                    lvc = np.where(lv < f32(-30), f32(-30), np.where(lv > f32(20), f32(20), lv)).astype(f32)  # keeps a NaN
                    sd = np.exp((f32(0.5) * lvc).astype(f32)).astype(f32)
                    x = (f32(scaling) * (mean + (sd * _np(z, B * n).reshape(B * P, C)).astype(f32)).astype(f32)).astype(f32)
            else:
                x = _np(latents, B * n).reshape(B * P, C).copy()
            x = x.reshape(B, n)
            nz = _np(noise, B * n).reshape(B, n)
            sa, sb = sabn[tc, 0][:, None], sabn[tc, 1][:, None]
            noisy = ((sa * x).astype(f32) + (sb * nz).astype(f32)).astype(f32)
        _flat(xin, B * n).copy_(torch.from_numpy(noisy.reshape(-1)).to(xin.dtype))
        if x0 is not None:
            _flat(x0, B * n).copy_(torch.from_numpy(x.reshape(-1)))
        _flat(temb, B * C0).copy_(torch.from_numpy(_np(sinus, T * C0).reshape(T, C0)[tc].reshape(-1)))
        _flat(w, B).copy_(torch.from_numpy(_np(wtab, T)[tc]))
        if oob is not None and (tb != tc).any():
            _flat(oob, 1)[0] = 1

    def mse_fwd(self, pred, target, w, per_sample, loss, B, n):
        name = "comat_mse_fwd"
        _refuse(name, all(a is not None for a in (pred, target, per_sample, loss)), "null pointer")
        _refuse(name, B > 0 and n > 0, "bad shape (B, n must be positive)")
        _refuse(name, B <= 65535, f"B = {B}, at most 65535 samples a launch")
        _refuse(name, _ok(pred), "bad dtype")
        self.launches.append((name, 2))
        p, q = _np(pred, B * n).reshape(B, n), _np(target, B * n).reshape(B, n)
        with np.errstate(over="ignore", invalid="ignore"):
            ps = np.array([sq_sum_in_kernel_order(p[b].astype(np.float64) - q[b].astype(np.float64)) / f32(n) for b in range(B)],
                          dtype=f32)
            wn = None if w is None else _np(w, B)
            s = f32(0)
            for b in range(B):
                s = f32(s + (ps[b] if wn is None else f32(wn[b] * ps[b])))
            total = f32(s / f32(B))
        _flat(per_sample, B).copy_(torch.from_numpy(ps))
        _flat(loss, 1)[0] = float(total)

    def mse_bwd(self, pred, target, w, g, dpred, B, n):
        name = "comat_mse_bwd"
        _refuse(name, all(a is not None for a in (pred, target, dpred)), "null pointer")
        _refuse(name, B > 0 and n > 0, "bad shape (B, n must be positive)")
        _refuse(name, B <= 65535, f"B = {B}, at most 65535 samples a launch")
        _refuse(name, _ok(pred), "bad dtype")
        assert dpred.dtype == pred.dtype
        self.launches.append((name, 1))
        p, q = _np(pred, B * n).reshape(B, n), _np(target, B * n).reshape(B, n)
        gv = np.float64(1.0 if g is None else _np(g, 1)[0])
        wv = np.ones(B, dtype=np.float64) if w is None else _np(w, B).astype(np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            c = (((gv * wv) * 2.0) / (np.float64(B) * np.float64(n))).astype(f32)[:, None]
            d = (c * (p - q).astype(f32)).astype(f32)
        _flat(dpred, B * n).copy_(torch.from_numpy(d.reshape(-1)).to(dpred.dtype))


NAMES = ("denoise_prepare", "mse_fwd", "mse_bwd")


def sim_matches_binding():
    """(names, mismatches): the mirrors above against the binding's module functions, by argument list"""
    import inspect

    from comat_amd import _hip
    args = lambda f, skip: list(inspect.signature(f).parameters)[skip:]
    return NAMES, [n for n in NAMES if not hasattr(_hip, n) or args(getattr(_hip, n), 0) != args(getattr(DenoiseSimKernels, n), 1)]


@pytest.fixture
def denoise_dev(dev):
    """conftest's `dev` with the simulator that knows the denoising entry points on the sim leg; the hip leg is the real library.
    The process-wide switch of the fused masked attention is off again when the test is over (as val_dev)."""
    from comat_amd import ops
    if dev.type == "cpu":
        ops.set_kernel_backend(DenoiseSimKernels())
    yield dev
    ops.set_fused_masked_attention(False)
