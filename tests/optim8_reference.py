"""Pure-torch restatement of the 8-bit blockwise optimizer state (comat_amd/optim8.py, csrc/optim8.hip) on float64 intermediates: the
checker of tests/test_optim8_kernels.py and tests/test_optim8_step.py.  Nothing here calls the library."""
import torch

from comat_amd.optim8 import BLOCK, dynamic_map, zero_code

F64 = torch.float64


def table(signed):
    return dynamic_map(signed).double()


def per_element(absmax, n):
    """the scale of each of n elements"""
    return absmax.detach().cpu().repeat_interleave(BLOCK)[:n]


def block_max(x):
    """max |x| over blocks of 256 (the last may be partial), in x's dtype: a maximum rounds nothing"""
    x = x.detach().cpu().abs()
    pad = (-x.numel()) % BLOCK
    return torch.cat([x, x.new_zeros(pad)]).reshape(-1, BLOCK).max(dim=1).values


def quantize(x, signed):
    """fp32 [n] -> (codes uint8 [n], absmax fp32 [ceil(n / 256)]): the nearest table entry to x / absmax in float64 (a value at the
    midpoint of two entries takes the lower), the zero code in an all-zero block"""
    x = x.detach().cpu().float()
    absmax = block_max(x)
    a = per_element(absmax, x.numel()).double()
    y = torch.where(a > 0, x.double() / torch.where(a > 0, a, torch.ones_like(a)), torch.zeros_like(a))
    t = table(signed)
    codes = torch.searchsorted((t[1:] + t[:-1]) / 2, y)
    codes = torch.where(a > 0, codes, torch.full_like(codes, zero_code(signed)))
    return codes.to(torch.uint8), absmax


def dequantize(codes, absmax, signed):
    """table[code] * absmax, one fp32 product"""
    codes = codes.detach().cpu()
    return dynamic_map(signed)[codes.long()] * per_element(absmax.float(), codes.numel())


def code_errors(x, codes, absmax, signed):
    """(|table[c] absmax - x| of the given codes, the smallest such error over all 256 codes, the scale per element), float64; x may
    be fp32 or float64"""
    x = x.detach().cpu().double()
    a = per_element(absmax.float(), x.numel()).double()
    t = table(signed)
    err = (t[codes.detach().cpu().long()] * a - x).abs()
    best = (t[None, :] * a[:, None] - x[:, None]).abs().min(dim=1).values
    return err, best, a


def assert_nearest_or_tied(x, codes, absmax, signed, slack, what):
    """every code's error is within `slack` x the block's scale of the best any code reaches"""
    err, best, a = code_errors(x, codes, absmax, signed)
    bad = ~(err <= best + a * slack)  # (a NaN is bad)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} codes are not nearest, first at {i}: x {float(x[i])!r}, code "
                             f"{int(codes[i])}, scale {float(a[i])!r}, error {float(err[i])!r} against {float(best[i])!r}")


def clip_factor(gnorm_sq, max_norm, grad_scale):
    """the factor adamw_lr_kernel multiplies the gradient by (float64)"""
    if not max_norm > 0:
        return grad_scale
    c = max_norm / (gnorm_sq ** 0.5 * grad_scale + 1e-6)
    return c * grad_scale if c < 1.0 else grad_scale


def adamw(p, g, m, v, lr, b1, b2, eps, wd, t, clip):
    """one AdamW update in float64 (t: the 1-based count of this update) -> p', m', v'"""
    p, g, m, v = (x.detach().cpu().double() for x in (p, g, m, v))
    gi = g * clip
    m = b1 * m + (1 - b1) * gi
    v = b2 * v + (1 - b2) * gi * gi
    bc1, bc2s = 1 - b1 ** t, (1 - b2 ** t) ** 0.5
    p = p * (1 - lr * wd) - (lr / bc1) * m / (v.sqrt() / bc2s + eps)
    return p, m, v
