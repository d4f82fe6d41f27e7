"""CPU simulator of the learning-rate schedule's entry points — TEST INFRASTRUCTURE ONLY.

`SimKernelsLr` adds, in plain Python doubles and torch, the documented semantics (include/comat_hip.h) of
comat_lr_schedule_eval, comat_adamw_tick_lr and comat_adamw_lr to `SimKernelsGan`, with the argument lists of
comat_amd._hip.HipKernels and the contract's refusals (a RuntimeError that names the entry point, as `_hip._check` raises for
COMAT_EINVAL).  `use_sim_lr`, `use_hip` and `release` are what the fixtures of the test modules call.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from sim_backend_gan import SimKernelsGan, release, use_hip  # noqa: F401 - re-exported

CONSTANT, CONSTANT_WITH_WARMUP, LINEAR, COSINE, COSINE_WITH_RESTARTS, POLYNOMIAL = range(6)


def _refuse(name, cond, msg):
    if not cond:
        raise RuntimeError(f"{name} failed (rc=-1): {name}: {msg}")


def _check(name, s):
    _refuse(name, CONSTANT <= s.kind <= POLYNOMIAL, f"unknown schedule kind {s.kind}")
    _refuse(name, s.stride >= 1 and s.warmup >= 0, f"stride must be >= 1 and warmup >= 0 (got {s.stride}, {s.warmup})")
    _refuse(name, s.kind < LINEAR or s.total >= 1, f"this kind needs total >= 1 (got {s.total})")
    _refuse(name, s.kind != POLYNOMIAL or s.base_lr > s.lr_end, "polynomial needs base_lr > lr_end")


def lr_at(s, applied):
    """the rate after `applied` updates: (float32)(base_lr * multiplier(stride * applied)), the multiplier in doubles"""
    c, W, T = s.stride * int(applied), s.warmup, s.total
    lam = 1.0
    if s.kind != CONSTANT:
        span = float(max(1, T - W))
        if c < W:
            lam = float(c) / float(max(1, W))
        elif s.kind == LINEAR:
            lam = max(0.0, float(T - c) / span)
        elif s.kind == COSINE:
            lam = max(0.0, 0.5 * (1.0 + math.cos(math.pi * s.num_cycles * 2.0 * (float(c - W) / span))))
        elif s.kind == COSINE_WITH_RESTARTS:
            progress = float(c - W) / span
            lam = 0.0 if progress >= 1.0 else max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((s.num_cycles * progress) % 1.0))))
        elif s.kind == POLYNOMIAL:
            if c > T:
                lam = s.lr_end / s.base_lr
            else:
                pct = 1.0 - float(c - W) / float(T - W) if T != W else float("nan")  # 0 / 0 at c == T == W, as on the device
                lam = ((s.base_lr - s.lr_end) * pct ** s.power + s.lr_end) / s.base_lr
    return float(np.float32(s.base_lr * lam))


class SimKernelsLr(SimKernelsGan):
    def lr_schedule_eval(self, sched, counters, lr_out):
        _check("comat_lr_schedule_eval", sched)
        lr_out[0] = lr_at(sched, counters[0])

    def adamw_tick_lr(self, counters, gnorm_sq, sched, lr_out):
        _check("comat_adamw_tick_lr", sched)
        if math.isfinite(float(gnorm_sq[0])):
            counters[0] += 1
            lr_out[0] = lr_at(sched, counters[0])
        else:
            counters[1] += 1

    def adamw_lr(self, p, g, m, v, n, lr_dev, beta1, beta2, eps, wd, step_dev, gnorm_sq, max_norm, grad_scale=1.0):
        _refuse("comat_adamw_lr", lr_dev is not None and step_dev is not None, "bad args (lr_dev and step_dev are required)")
        self.adamw(p, g, m, v, n, float(lr_dev[0]), beta1, beta2, eps, wd, 0, gnorm_sq, max_norm, step_dev=step_dev,
                   grad_scale=grad_scale)


def use_sim_lr():
    from comat_amd import ops
    ops.set_kernel_backend(SimKernelsLr())
    return torch.device("cpu")
