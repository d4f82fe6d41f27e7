"""CPU simulator of the gradient-accumulation entry points — TEST INFRASTRUCTURE ONLY.

`SimKernelsAccum` adds, in plain Python and torch, the documented semantics (include/comat_hip.h) of comat_accum_zero,
comat_adamw_window and comat_window_tick to `SimKernelsLr`, with the argument lists of comat_amd._hip.HipKernels and the
contract's refusals (a RuntimeError that names the entry point, as `_hip._check` raises for COMAT_EINVAL).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from sim_backend_lr import SimKernelsLr, _check, _refuse, lr_at, release, use_hip  # noqa: F401 - re-exported


class SimKernelsAccum(SimKernelsLr):
    def accum_zero(self, g, n, window):
        _refuse("comat_accum_zero", g is not None and window is not None, "null pointer")
        _refuse("comat_accum_zero", n >= 1, f"n must be >= 1 (got {n})")
        if int(window[0]) == 0:
            g.reshape(-1)[:n].zero_()

    def adamw_window(self, p, g, m, v, n, lr_dev, beta1, beta2, eps, wd, step_dev, gnorm_sq, max_norm, window, accum_steps,
                     grad_scale=1.0):
        name = "comat_adamw_window"
        _refuse(name, all(x is not None for x in (p, g, m, v, lr_dev, step_dev, window)), "null pointer")
        _refuse(name, n >= 1 and grad_scale > 0, f"n must be >= 1 and grad_scale > 0 (got {n}, {grad_scale})")
        _refuse(name, accum_steps >= 1, f"accum_steps must be >= 1 (got {accum_steps})")
        if int(window[0]) == accum_steps - 1:
            self.adamw_lr(p, g, m, v, n, lr_dev, beta1, beta2, eps, wd, step_dev, gnorm_sq, max_norm, grad_scale=grad_scale)

    def window_tick(self, window, accum_steps, counters, gnorm_sq, sched, lr_out, step_loss=None, train_loss=None):
        name = "comat_window_tick"
        if sched is not None:
            _check(name, sched)
        _refuse(name, window is not None and counters is not None and gnorm_sq is not None
                and (sched is None or lr_out is not None), "null pointer")
        _refuse(name, accum_steps >= 1, f"accum_steps must be >= 1 (got {accum_steps})")
        _refuse(name, (step_loss is None) == (train_loss is None), "step_loss and train_loss go together")
        w = int(window[0])
        if train_loss is not None:  # fp32, in the stated order
            prev = np.float32(0.0) if w == 0 else np.float32(float(train_loss[0]))
            train_loss[0] = float(prev + np.float32(float(step_loss.reshape(-1)[0])) / np.float32(accum_steps))
        if w != accum_steps - 1:
            window[0] = w + 1
            return
        if math.isfinite(float(gnorm_sq[0])):
            counters[0] += 1
            if sched is not None:
                lr_out[0] = lr_at(sched, counters[0])
        else:
            counters[1] += 1
        if train_loss is not None:
            train_loss[1] = train_loss[0]
        window[0] = 0


def use_sim_accum():
    from comat_amd import ops
    ops.set_kernel_backend(SimKernelsAccum())
    return torch.device("cpu")
