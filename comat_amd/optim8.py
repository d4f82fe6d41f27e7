"""8-bit blockwise AdamW state (`--use_8bit_adam`; training_script.py:216-223 makes bnb.optim.AdamW8bit the optimizer class of the
generator, :258-264, and of the discriminator, :269-275).

The two moments of every large segment are kept as one code byte per element plus one fp32 scale (the block's abs-max) per 256
consecutive elements of the flat buffer: 2 + 8/256 bytes per parameter where fp32 AdamW holds 8.  A code indexes one of two
256-entry tables in [-1, 1] (`dynamic_map`: signed for the first moment, unsigned for the second).  One kernel per segment
(comat_adamw8_window) dequantises, runs the AdamW element of the fp32 kernels, takes the new block maxima and stores the nearest
codes; the parameters are updated from the fresh fp32 moments, never from the requantised ones.

bitsandbytes is not a dependency and no file of its format is read or written: the tables are this module's float64 construction
(restated from the published `create_dynamic_map(signed, 7, 8)`), carried by the library as literals (csrc/q8_maps.inc).  The
deviations from that library are listed in INTEGRATION.md.  There is no CPU path: under a backend that is not `HipKernels` the
optimizer raises."""
from __future__ import annotations

import ctypes as C

import torch

from . import _hip, ops
from ._hip import _check, _ptr, _stream
from .step import FlatAdamW, lr_schedule

BLOCK = 256          # elements per scale
MIN_8BIT_SIZE = 4096  # a smaller segment keeps fp32 moments (bitsandbytes' min_8bit_size, here per segment)


def dynamic_map(signed: bool) -> torch.Tensor:
    """256 ascending fp32 values: 0, 1 and, for decade i = 0..6, 10^(i-6) * (0.1 + 0.9 (j + 1/2) / count), j < count = 2^i (signed:
    with their negatives) or 2^(i+1); evaluated in float64 and rounded once.  Signed: zero is code 127; unsigned: code 0."""
    vals = [0.0, 1.0]
    for i in range(7):
        count = 2 ** i if signed else 2 ** (i + 1)
        for j in range(count):
            x = float(f"1e{i - 6}") * (0.1 + 0.9 * (j + 0.5) / count)
            vals += [x, -x] if signed else [x]
    out = torch.tensor(sorted(vals), dtype=torch.float64).float()
    assert out.numel() == 256
    return out


def zero_code(signed: bool) -> int:
    return 127 if signed else 0


def maps_inc_text() -> str:
    """the text of csrc/q8_maps.inc: two brace-enclosed rows of 256 literals, the unsigned table first (row index = is_signed)"""
    rows = []
    for signed in (False, True):
        vals = [s + ("f" if "." in s or "e" in s else ".0f") for s in (f"{v:.9g}" for v in dynamic_map(signed).tolist())]
        lines = ["    " + ", ".join(vals[i:i + 8]) + "," for i in range(0, 256, 8)]
        rows.append("{  // " + ("signed" if signed else "unsigned") + "\n" + "\n".join(lines) + "\n},")
    return ("// q8_maps.inc - the two code books of the 8-bit optimizer state as fp32 literals: comat_amd/optim8.py dynamic_map(False),\n"
            "// dynamic_map(True), printed by optim8.maps_inc_text(); tests/test_optim8_host.py holds them to that construction bit for bit.\n"
            + "\n".join(rows) + "\n")


def _lib():
    return _hip.load_library()


def q8_map(signed: bool) -> torch.Tensor:
    """the library's copy of a table (host memory; needs no GPU)"""
    out = (C.c_float * 256)()
    _check(_lib().comat_q8_map(int(bool(signed)), out), "comat_q8_map")
    return torch.tensor(list(out), dtype=torch.float32)


def _require_hip(what):
    if not isinstance(ops.kernels(), _hip.HipKernels):
        raise RuntimeError(f"{what}: use_8bit_adam runs on the HIP kernels only (comat_adamw8_window, comat_q8_*); the installed "
                           f"backend is {type(ops.kernels()).__name__} and there is no CPU path")


def n_blocks(n: int) -> int:
    return (n + BLOCK - 1) // BLOCK


def quantize_blockwise(x, codes, absmax, n, signed):
    """codes[i] = index of a table entry nearest to x[i] / absmax[i // 256], absmax[b] = max |x| over block b (0: the zero code)"""
    assert x.dtype == torch.float32 and codes.dtype == torch.uint8 and absmax.dtype == torch.float32
    _check(_lib().comat_q8_quantize_blockwise(_ptr(x), _ptr(codes), _ptr(absmax), n, int(bool(signed)), _stream()),
           "comat_q8_quantize_blockwise")


def dequantize_blockwise(codes, absmax, x, n, signed):
    """x[i] = table[codes[i]] * absmax[i // 256]"""
    assert x.dtype == torch.float32 and codes.dtype == torch.uint8 and absmax.dtype == torch.float32
    _check(_lib().comat_q8_dequantize_blockwise(_ptr(codes), _ptr(absmax), _ptr(x), n, int(bool(signed)), _stream()),
           "comat_q8_dequantize_blockwise")


def adamw8_window(p, g, m8, v8, absmax_m, absmax_v, n, lr_dev, beta1, beta2, eps, wd, step_dev, gnorm_sq, max_norm, window=None,
                  accum_steps=1, grad_scale=1.0):
    """comat_adamw_window on 8-bit state; window None: every launch closes (the form comat_adamw_lr has)"""
    assert m8.dtype == torch.uint8 and v8.dtype == torch.uint8
    _check(_lib().comat_adamw8_window(_ptr(p), _ptr(g), _ptr(m8), _ptr(v8), _ptr(absmax_m), _ptr(absmax_v), n, _ptr(lr_dev), beta1,
                                      beta2, eps, wd, _ptr(step_dev), _ptr(gnorm_sq), max_norm, grad_scale, _ptr(window),
                                      accum_steps, _stream()), "comat_adamw8_window")


def dequantized_state(sd, device):
    """an 8-bit state dict as the 32-bit one a plain FlatAdamW loads: m, v of every 8-bit segment dequantised on `device`"""
    _require_hip("loading 8-bit optimizer state")
    out = {k: v for k, v in sd.items() if k not in ("state_bits", "seg8", "m8", "v8", "absmax_m", "absmax_v")}
    small_m, small_v = iter(sd["m"]), iter(sd["v"])
    big = zip(sd["m8"], sd["v8"], sd["absmax_m"], sd["absmax_v"])
    out["m"], out["v"] = [], []
    for is8 in sd["seg8"]:
        if not is8:
            out["m"].append(next(small_m))
            out["v"].append(next(small_v))
            continue
        m8, v8, am, av = (t.to(device).contiguous() for t in next(big))
        n = m8.numel()
        m, v = torch.empty(n, dtype=torch.float32, device=device), torch.empty(n, dtype=torch.float32, device=device)
        dequantize_blockwise(m8, am, m, n, True)
        dequantize_blockwise(v8, av, v, n, False)
        out["m"].append(m)
        out["v"].append(v)
    return out


class FlatAdamW8bit(FlatAdamW):
    """FlatAdamW whose moments are 8-bit blockwise for every segment of at least MIN_8BIT_SIZE elements: `m8`, `v8` (uint8 [n]) and
    `absmax_m`, `absmax_v` (fp32 [ceil(n / 256)]) where the parent has `m`, `v` (those entries are None).  A smaller segment (the
    discriminator's head) keeps fp32 moments and the fp32 kernel.  The optimizer always owns `lr_now` (a constant schedule is
    evaluated into it once), so one launch form serves every schedule and every accum_steps: sumsq per segment, comat_adamw8_window
    or adamw_window / adamw_lr per segment, then adamw_tick_lr or window_tick.  Every buffer is allocated here, before any capture."""

    def __init__(self, segments, lr, betas, eps, weight_decay, max_norm, schedule=None, accum_steps=1):
        _require_hip("FlatAdamW8bit")
        super().__init__(segments, lr, betas, eps, weight_decay, max_norm, schedule=schedule, accum_steps=accum_steps)
        # what the tick evaluates when the parent keeps no schedule (constant at one scheduler step per update)
        self._tick_schedule = self.schedule if self.schedule is not None else lr_schedule("constant", lr)
        if self.lr_now is None:
            self.lr_now = torch.zeros(1, dtype=torch.float32, device=self.counters.device)
            ops.kernels().lr_schedule_eval(self._tick_schedule, self.counters, self.lr_now)

    def _alloc_moments(self):
        self.seg8 = [p.numel() >= MIN_8BIT_SIZE for p, _ in self.segments]
        codes = lambda p, is8, signed: torch.full((p.numel(),), zero_code(signed), dtype=torch.uint8, device=p.device) if is8 else None
        scales = lambda p, is8: torch.zeros(n_blocks(p.numel()), dtype=torch.float32, device=p.device) if is8 else None
        self.m8 = [codes(p, is8, True) for (p, _), is8 in zip(self.segments, self.seg8)]
        self.v8 = [codes(p, is8, False) for (p, _), is8 in zip(self.segments, self.seg8)]
        self.absmax_m = [scales(p, is8) for (p, _), is8 in zip(self.segments, self.seg8)]
        self.absmax_v = [scales(p, is8) for (p, _), is8 in zip(self.segments, self.seg8)]
        fp32 = lambda: [None if is8 else torch.zeros_like(p) for (p, _), is8 in zip(self.segments, self.seg8)]
        return fp32(), fp32()

    def _state_tensors(self):
        return [t for ts in (self.m, self.v, self.m8, self.v8, self.absmax_m, self.absmax_v) for t in ts if t is not None]

    def state_bytes(self):
        """bytes of optimizer state held: codes and scales, the fp32 moments of the small segments"""
        return sum(t.numel() * t.element_size() for t in self._state_tensors())

    def step(self, grad_scale=1.0, step_loss=None):
        k = ops.kernels()
        b1, b2 = self.betas
        self.gnorm_sq.zero_()
        for _, g in self.segments:
            k.sumsq(g, g.numel(), self.gnorm_sq)
        for i, (p, g) in enumerate(self.segments):
            if self.seg8[i]:
                adamw8_window(p, g, self.m8[i], self.v8[i], self.absmax_m[i], self.absmax_v[i], p.numel(), self.lr_now, b1, b2,
                              self.eps, self.wd, self.counters, self.gnorm_sq, self.max_norm, self.window, self.accum_steps,
                              grad_scale=grad_scale)
            elif self.window is not None:
                k.adamw_window(p, g, self.m[i], self.v[i], p.numel(), self.lr_now, b1, b2, self.eps, self.wd, self.counters,
                               self.gnorm_sq, self.max_norm, self.window, self.accum_steps, grad_scale=grad_scale)
            else:
                k.adamw_lr(p, g, self.m[i], self.v[i], p.numel(), self.lr_now, b1, b2, self.eps, self.wd, self.counters,
                           self.gnorm_sq, self.max_norm, grad_scale=grad_scale)
        if self.window is None:
            k.adamw_tick_lr(self.counters, self.gnorm_sq, self._tick_schedule, self.lr_now)
            return
        if step_loss is not None and step_loss.dtype != torch.float32:
            step_loss = step_loss.float()
        k.window_tick(self.window, self.accum_steps, self.counters, self.gnorm_sq, self.schedule, self.lr_now, step_loss,
                      None if step_loss is None else self.train_loss)
        if not self._capturing():
            self.advance()

    def _moments_state(self):
        pick = lambda ts: [t.detach().clone() for t in ts if t is not None]
        return dict(state_bits=8, seg8=tuple(self.seg8), m=pick(self.m), v=pick(self.v), m8=pick(self.m8), v8=pick(self.v8),
                    absmax_m=pick(self.absmax_m), absmax_v=pick(self.absmax_v))

    def _load_moments(self, sd):
        """8-bit state is copied into the buffers; 32-bit state (a file without `state_bits`) is quantised into them"""
        bits = sd.get("state_bits", 32)
        if bits == 32:
            if len(sd["m"]) != len(self.segments) or len(sd["v"]) != len(self.segments) or \
                    any(a.shape != p.shape for a, (p, _) in zip(sd["m"] + sd["v"], self.segments * 2)):
                raise ValueError("optimizer state does not match this optimizer's segments")
            for i, is8 in enumerate(self.seg8):
                if not is8:
                    self.m[i].copy_(sd["m"][i])
                    self.v[i].copy_(sd["v"][i])
                    continue
                dev = self.m8[i].device
                for src, codes, scales, signed in ((sd["m"][i], self.m8[i], self.absmax_m[i], True),
                                                   (sd["v"][i], self.v8[i], self.absmax_v[i], False)):
                    x = src.to(device=dev, dtype=torch.float32).contiguous()
                    quantize_blockwise(x, codes, scales, x.numel(), signed)
            return
        if bits != 8:
            raise ValueError(f"optimizer state has state_bits = {bits}: 8 and 32 are the formats")
        mine = self._moments_state()
        names = ("m", "v", "m8", "v8", "absmax_m", "absmax_v")
        if list(sd["seg8"]) != self.seg8 or any(len(sd[k]) != len(mine[k]) or any(a.shape != b.shape for a, b in zip(sd[k], mine[k]))
                                                for k in names):
            raise ValueError("optimizer state does not match this optimizer's segments")
        pick = lambda ts: [t for t in ts if t is not None]
        for k, dst in zip(names, (self.m, self.v, self.m8, self.v8, self.absmax_m, self.absmax_v)):
            for d, s in zip(pick(dst), sd[k]):
                d.copy_(s)
