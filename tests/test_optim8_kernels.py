"""The kernels of the 8-bit blockwise optimizer state on the GPU (csrc/optim8.hip: comat_q8_quantize_blockwise,
comat_q8_dequantize_blockwise, comat_adamw8_window) against the float64 restatement of tests/optim8_reference.py.  Every operand
lives in a helpers.Window: the guard bands beyond n elements, and beyond ceil(n / 256) scales, are checked bit for bit.

Bounds.  A scale is the exact maximum of values the test also holds: bit-equal.  A code must be nearest or tied: its error
|table[c] absmax - x| may exceed the best code's by absmax 2^-22 - the fp32 roundings of one division and one product, no tuned
tolerance.  After an update the moments are known to the test only through float64 arithmetic on the same inputs: the new scales are
held to 2^-22 relative, the codes to a slack of absmax 2^-21, the parameters to the bound of test_adamw_with_clip."""
import numpy as np
import pytest
import torch

import optim8_reference as R
from comat_amd import optim8
from helpers import Window, check

pytestmark = pytest.mark.gpu

F32, U8, I32 = torch.float32, torch.uint8, torch.int32
# a partial block alone, almost a block, an exact block, a one-element last block, a tail that is no multiple of 4, a bank-style multiple of 8
SIZES = [1, 255, 256, 257, 1027, 4104]
f32 = lambda x: float(np.float32(x))
HP = dict(beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8), wd=f32(1e-2))
LR, MAX_NORM, GRAD_SCALE = f32(5e-3), f32(0.1), 0.5


def kernels():
    from comat_amd import ops
    return ops.kernels()


def win(n, dev, dtype=F32):
    """n elements in a poisoned buffer, 2 n guard elements on either side, the first element 16-byte (codes: 4-byte) aligned"""
    w = Window(1, n, dtype=dtype, device=dev, lead=2, trail=2, left=8 + (-2 * n) % 4)
    assert w.flat.data_ptr() % (16 if dtype == F32 else 4) == 0
    return w


def word(v, dev, dtype=I32):
    return torch.tensor([v], dtype=dtype, device=dev)


def hard_values(n, signed):
    """blocks of 256 - all zero, one 1e30 among 1e-30s, denormals, negative only, exact table entries (at a power-of-two scale),
    Gaussians of several scales - in an order that depends on n, so that the short sizes see different ones; cut to n"""
    gen = torch.Generator().manual_seed(n)
    big = torch.full((256,), 1e-30)
    big[77] = 1e30
    perm = torch.randperm(256, generator=gen)
    blocks = [torch.zeros(256), big, torch.rand(256, generator=gen) * 1e-39, -torch.rand(256, generator=gen) - 0.01,
              optim8.dynamic_map(signed)[perm] * 0.5]
    blocks = blocks[n % 5:] + blocks[:n % 5]
    while sum(b.numel() for b in blocks) < n:
        blocks.append(torch.randn(256, generator=gen) * 10.0 ** float(torch.randint(-6, 3, (1,), generator=gen)))
    x = torch.cat(blocks)[:n].float()
    exact_at = 256 * ((4 - n % 5) % 5)  # where the table-entry block starts
    return x, perm, exact_at


# ---- quantise -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
@pytest.mark.parametrize("n", SIZES)
def test_quantize(hip, n, signed):
    x, perm, exact_at = hard_values(n, signed)
    nb = optim8.n_blocks(n)
    xw, cw, aw = win(n, hip).put(x), win(n, hip, U8).arm(), win(nb, hip).arm()
    optim8.quantize_blockwise(xw.flat, cw.flat, aw.flat, n, signed)
    torch.cuda.synchronize()
    what = f"quantize n={n} signed={signed}"
    cw.assert_guard_intact(what + " codes")
    aw.assert_guard_intact(what + " scales")
    codes, absmax = cw.get().cpu().reshape(-1), aw.get().cpu().reshape(-1)
    assert torch.equal(absmax.view(I32), R.block_max(x).view(I32)), f"{what}: a scale is not the exact block maximum"
    R.assert_nearest_or_tied(x, codes, absmax, signed, 2.0 ** -22, what)
    zero = (R.per_element(absmax, n) == 0)
    assert bool((codes[zero] == optim8.zero_code(signed)).all()), f"{what}: an all-zero block must get the zero code"
    if exact_at + 256 <= n:  # values on table entries get exactly those entries
        assert torch.equal(codes[exact_at:exact_at + 256].long(), perm), f"{what}: values on table entries"


# ---- dequantise ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
@pytest.mark.parametrize("n", SIZES)
def test_dequantize(hip, n, signed):
    """bit-equal to table[c] * absmax in fp32 on the host; from 256 elements on, one block holds all 256 codes"""
    gen = torch.Generator().manual_seed(50 + n)
    nb = optim8.n_blocks(n)
    codes = torch.cat([torch.randperm(256, generator=gen), torch.randint(0, 256, (max(n, 256),), generator=gen)])[:n].to(U8)
    absmax = torch.rand(nb, generator=gen) * 10.0 ** torch.randint(-30, 30, (nb,), generator=gen).float()
    cw, aw, xw = win(n, hip, U8).put(codes), win(nb, hip).put(absmax), win(n, hip).arm()
    optim8.dequantize_blockwise(cw.flat, aw.flat, xw.flat, n, signed)
    torch.cuda.synchronize()
    xw.assert_guard_intact(f"dequantize n={n}")
    assert torch.equal(xw.get().cpu().reshape(-1).view(I32), R.dequantize(codes, absmax, signed).view(I32))


# ---- the update ---------------------------------------------------------------------------------------------------------------
class State:
    """p, g and the 8-bit moments of n elements in windows; zero state: zero codes and zero scales"""

    def __init__(self, n, dev, p, g):
        self.n, self.nb, self.dev = n, optim8.n_blocks(n), dev
        self.p, self.g = win(n, dev).put(p), win(n, dev).put(g)
        self.m8 = win(n, dev, U8).put(torch.full((n,), 127, dtype=U8))
        self.v8 = win(n, dev, U8).put(torch.zeros(n, dtype=U8))
        self.am, self.av = win(self.nb, dev).put(torch.zeros(self.nb)), win(self.nb, dev).put(torch.zeros(self.nb))
        self.lr, self.nsq = word(LR, dev, F32), torch.zeros(1, dtype=F32, device=dev)
        self.counters = torch.zeros(2, dtype=I32, device=dev)

    def outputs(self):
        return dict(p=self.p, m8=self.m8, v8=self.v8, absmax_m=self.am, absmax_v=self.av)

    def arm(self):
        for w in self.outputs().values():
            w.arm()
        return self

    def copy_from(self, other):
        for a, b in zip(self.outputs().values(), other.outputs().values()):
            a.put(b.get())
        self.g.put(other.g.get())
        self.counters.copy_(other.counters)
        return self

    def norm(self):
        self.nsq.zero_()
        kernels().sumsq(self.g.flat, self.n, self.nsq)
        return float(self.nsq[0])

    def step(self, nsq=None, window=None, accum_steps=1, max_norm=MAX_NORM, wd=HP["wd"]):
        optim8.adamw8_window(self.p.flat, self.g.flat, self.m8.flat, self.v8.flat, self.am.flat, self.av.flat, self.n, self.lr,
                             HP["beta1"], HP["beta2"], HP["eps"], wd, self.counters, self.nsq if nsq is None else nsq, max_norm,
                             window, accum_steps, grad_scale=GRAD_SCALE)
        torch.cuda.synchronize()

    def untouched(self, what):
        for name, w in self.outputs().items():
            assert torch.equal(w.buf.view(w._snap.dtype), w._snap), f"{what}: {name} was written"

    def guards(self, what):
        for name, w in self.outputs().items():
            w.assert_guard_intact(f"{what}: {name}")

    def bits(self):
        return [w.get().cpu() for w in self.outputs().values()]

    def moments(self):
        """(m, v) dequantised on the host in fp32, and the raw codes and scales"""
        m8, v8, am, av = (w.get().cpu().reshape(-1) for w in (self.m8, self.v8, self.am, self.av))
        return R.dequantize(m8, am, True), R.dequantize(v8, av, False), (m8, v8, am, av)


def inputs(n, seed):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = (torch.rand(n, generator=gen) + 0.5) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)  # |g|_2 >= 0.5 sqrt(n): the clip acts
    return p, g * 10.0 ** torch.randint(0, 3, (n,), generator=gen).float()


def clip32(nsq):
    """the clip factor as adamw_lr_kernel's fp32 statements give it (the fused multiply-add through float64: one rounding)"""
    d = np.float32(np.float64(np.sqrt(np.float32(nsq))) * GRAD_SCALE + np.float64(np.float32(1e-6)))
    c = np.float32(MAX_NORM) / d
    return float(c * np.float32(GRAD_SCALE)) if c < 1 else GRAD_SCALE


@pytest.mark.parametrize("n", SIZES)
def test_update_steps(hip, n):
    """step 1 from the zero state: p bit-identical to comat_adamw_lr's on copies (clip active, grad_scale 0.5, weight decay on), codes
    and scales against that kernel's own m, v; steps 2..5 from the state the kernel left, against the float64 restatement.

    The gradients of steps 2..5 keep every element's sign and, within 10 %, its size.  The bound on the scales, 2^-22 = four fp32
    roundings, is what adamw_element's arithmetic can be held to only where nothing cancels: m' = fma(b1, m, (1 - b1) g') has three
    roundings (g', the product, the sum) when b1 m and g' share a sign, and v' = b2 v + ((1 - b2) g') g' has 4 w + (1 - w) + 1 of
    them, w the new term's share of v' - at most 0.6 here.  Where the two terms of m' have opposite signs the relative error of their
    fp32 sum is that of fp32 AdamW itself and has no bound (measured with independent signs at n = 1, where the clip makes every
    |g'| equal and the terms cancel to a tenth: 5.2e-7).  Codes and parameters are checked on every element either way."""
    k = kernels()
    p0, g0 = inputs(n, 300 + n)
    s = State(n, hip, p0, g0).arm()
    nsq = s.norm()
    assert nsq * GRAD_SCALE ** 2 > MAX_NORM ** 2
    A = [win(n, hip).put(x) for x in (p0, torch.zeros(n), torch.zeros(n))]
    k.adamw_lr(A[0].flat, s.g.flat, A[1].flat, A[2].flat, n, s.lr, HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], s.counters, s.nsq,
               MAX_NORM, grad_scale=GRAD_SCALE)
    s.step()
    s.guards(f"adamw8 n={n} step 1")
    pa, ma, va = (w.get().cpu().reshape(-1) for w in A)
    assert torch.equal(s.p.get().cpu().reshape(-1).view(I32), pa.view(I32)), "step 1: p differs from comat_adamw_lr's"
    assert not torch.equal(pa, p0)
    _, _, (m8, v8, am, av) = s.moments()
    assert torch.equal(am.view(I32), R.block_max(ma).view(I32)) and torch.equal(av.view(I32), R.block_max(va).view(I32))
    R.assert_nearest_or_tied(ma, m8, am, True, 2.0 ** -22, f"n={n} step 1, first moment")
    R.assert_nearest_or_tied(va, v8, av, False, 2.0 ** -22, f"n={n} step 1, second moment")
    for t in (2, 3, 4, 5):
        m, v, _ = s.moments()
        p = s.p.get().cpu().reshape(-1)
        g = g0 * (0.9 + 0.1 * torch.rand(n, generator=torch.Generator().manual_seed(300 + n + 1000 * t)))
        s.g.put(g)
        s.counters.copy_(torch.tensor([t - 1, 0], dtype=I32))
        s.arm()
        clip = clip32(s.norm())
        assert clip < GRAD_SCALE
        pe, me, ve = R.adamw(p, g, m, v, LR, HP["beta1"], HP["beta2"], HP["eps"], HP["wd"], t, clip)
        s.step()
        what = f"adamw8 n={n} step {t}"
        s.guards(what)
        _, _, (m8, v8, am, av) = s.moments()
        for got, want, name in ((am, R.block_max(me), "first"), (av, R.block_max(ve), "second")):
            rel = ((got.double() - want) / want).abs().max().item()
            print(f"{what}: {name}-moment scales off by {rel:.3e} relative (limit {2.0 ** -22:.3e})")
            assert rel <= 2.0 ** -22, f"{what}: {name}-moment scales"
        R.assert_nearest_or_tied(me, m8, am, True, 2.0 ** -21, what + ", first moment")
        R.assert_nearest_or_tied(ve, v8, av, False, 2.0 ** -21, what + ", second moment")
        check(s.p.get().reshape(-1), pe.float(), F32, what + " parameters", factor=0.5)


@pytest.mark.parametrize("n", SIZES)
def test_nothing_written_when_the_update_does_not_apply(hip, n):
    """a window that is not closing, and a non-finite squared norm (closing window or none): p, codes and scales bit-equal"""
    p0, g0 = inputs(n, 400 + n)
    s = State(n, hip, p0, g0)
    s.norm()
    s.step()  # some state
    s.arm()
    for idx, N in ((0, 2), (1, 3), (0, 3), (2, 2)):
        s.step(window=word(idx, hip), accum_steps=N)
        s.untouched(f"n={n} window {idx} of {N}")
    for bad in (float("inf"), float("-inf"), float("nan")):
        s.step(nsq=word(bad, hip, F32))
        s.step(nsq=word(bad, hip, F32), window=word(1, hip), accum_steps=2)
        s.untouched(f"n={n} squared norm {bad}")
    s.step(window=word(1, hip), accum_steps=2)  # and a closing window updates
    assert not torch.equal(s.p.buf.view(I32), s.p._snap) and not torch.equal(s.am.buf.view(I32), s.am._snap)
    s.guards(f"n={n} closing window")


@pytest.mark.parametrize("n", SIZES)
def test_two_runs_give_the_same_bits(hip, n):
    p0, g0 = inputs(n, 500 + n)
    a = State(n, hip, p0, g0)
    a.norm()
    a.step()
    _, g1 = inputs(n, 501 + n)
    a.g.put(g1)
    a.counters.copy_(torch.tensor([1, 0], dtype=I32))
    b = State(n, hip, p0, g0).copy_from(a)
    a.norm(), b.norm()
    a.step(), b.step()
    for x, y, name in zip(a.bits(), b.bits(), a.outputs()):
        assert torch.equal(x.view(I32) if x.dtype == F32 else x, y.view(I32) if y.dtype == F32 else y), f"n={n}: {name} differs"


@pytest.mark.parametrize("n", SIZES)
def test_pads_stay_zero(hip, n):
    """zero gradient on zero state, weight decay on: p (zero, as the banks' pad elements are) and the codes stay what they were"""
    s = State(n, hip, torch.zeros(n), torch.zeros(n)).arm()
    s.norm()
    for t in range(2):
        s.counters.copy_(torch.tensor([t, 0], dtype=I32))
        s.step()
        for name, w in s.outputs().items():
            assert torch.equal(w.buf.view(w._snap.dtype), w._snap), f"n={n}: {name} changed"
    # and a parameter that is not zero, without weight decay, keeps its bits too
    p0, _ = inputs(n, 600 + n)
    s = State(n, hip, p0, torch.zeros(n)).arm()
    s.norm()
    s.step(wd=0.0)
    s.untouched(f"n={n} zero gradient, no decay")
