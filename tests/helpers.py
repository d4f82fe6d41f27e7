"""Shared helpers of the parity tests."""
import contextlib
import dataclasses
import math

import pytest
import torch

from comat_amd import config, weights
from oracle import sd as O


def tol(dtype):
    return 2e-4 if dtype == torch.float32 else 3e-2


def check(got, ref, dtype, what="", factor=1.0):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    assert err / scale < tol(dtype) * factor, f"{what}: max err {err:.3e} vs scale {scale:.3e} ({dtype})"


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((got - ref).norm() / (ref.norm() + 1e-30))


def tok(t):
    """NCHW -> channels-last tokens"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def untok(t, B, H, W):
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


def oracle_cfgs(ucfg=config.TINY_UNET, vcfg=config.TINY_VAE):
    return O.UNetConfig(**dataclasses.asdict(ucfg)), O.VAEConfig(**dataclasses.asdict(vcfg))


def tiny_weights(dtype, ucfg=config.TINY_UNET):
    """Tiny-config weights rounded to `dtype` (so oracle and kernels see identical values)."""
    q = lambda d: {k: v.to(dtype).float() for k, v in d.items()}
    usd = q(weights.make_unet_weights(ucfg, perturb_norms=True))
    vsd = q(weights.make_vae_weights(config.TINY_VAE, perturb_norms=True))
    lsd = q(weights.make_lora_weights(ucfg))
    # make LoRA up factors big enough that their gradients are well conditioned in the tiny model
    lsd = {k: (v * 5 if k.endswith("up.weight") else v).to(dtype).float() for k, v in lsd.items()}
    return usd, vsd, lsd


# the library's defaults for the options whose default moved in round 4 (runtime.hip)
DEFAULT_OPTS = dict(flash_xcd=1, g2_order=2, gemm3=1, norm_fused=5)


def _set_opts(**kw):
    from comat_amd import _hip
    for k_, v_ in kw.items():
        _hip.set_option(k_, v_)


def restore_default_opts():
    _set_opts(gemm2=1, gemm2_tt=1, g2_cfg=0, g2_splits=0, force_splits=0, flash_trim=1, flash_tr=1, flash_kt=4, flash_merge=1, flash_xcd=DEFAULT_OPTS['flash_xcd'],
              g2_order=DEFAULT_OPTS['g2_order'], norm_fused=DEFAULT_OPTS['norm_fused'], gemm3=DEFAULT_OPTS['gemm3'], g3_cfg=0)


@pytest.fixture
def default_opts():
    """restore the library's kernel-selection options after a test that forces variants"""
    yield
    restore_default_opts()


@contextlib.contextmanager
def fp8_state():
    """a test that sets the fp8 scaling mode or a recipe starts from none and leaves what it found.  A module builds its `dev` /
    `sim` / `hip` on the suite's with it - `def dev(dev): with fp8_state(): yield dev` - so the state is restored while the
    backend is still installed and the backend is released last."""
    from comat_amd import ops
    prev = (ops.fp8_scaling(), ops.fp8_recipe())
    ops.fp8_reset()
    ops.clear_fp8_recipe()
    try:
        yield
    finally:
        ops.set_fp8_scaling(prev[0])
        ops.clear_fp8_recipe()
        if prev[1] is not None:
            ops.set_fp8_recipe(**prev[1])
        ops.fp8_reset()


# ---- exact integer-operand parity (tests/test_exact_products.py) -------------------------------------------------------------
def ints(*shape, seed, hi=8):
    """float tensor of NON-ZERO integers drawn uniformly from +-{1 .. hi}: exact in bf16 (hi <= 256) and, up to 8, in e4m3; no
    dropped product can hide behind a zero factor"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.randint(1, hi + 1, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sign).float()


def assert_sums_exact(K, a, b, factor=1, extra=0.0):
    """every partial sum of K products a * b (times `factor`: 3 where alpha2 = 0.75 multiplies the sum; plus `extra`, the largest
    value accumulated into) is an integer below 2^24: no summation order can round in fp32"""
    amax, bmax = float(a.abs().max()), float(b.abs().max())
    assert bool((a == a.round()).all()) and bool((b == b.round()).all()), "operands must be integers"
    assert K * amax * bmax * factor + extra < 2 ** 24, f"partial sums may round: K {K}, max |a| {amax}, max |b| {bmax}, factor {factor}"


def _first_mismatch(bad, shape):
    i = int(torch.nonzero(bad.reshape(-1))[0])
    idx = []
    for n in reversed(shape):
        idx.append(i % n)
        i //= n
    return tuple(reversed(idx))


def assert_exact(got, ref64, out_dtype, what, alpha=1.0):
    """`got` equals the exact result bit for bit: ref64 (fp64) must itself be an fp32 number everywhere - then an fp32 accumulator
    of exact partial sums holds it whatever the summation order - and the stored value is its one round-to-nearest-even to
    out_dtype.  A failure names the first (batch, row, column) and the difference over alpha: the sum of the products that are
    missing or counted twice."""
    assert ref64.dtype == torch.float64
    assert torch.equal(ref64.float().double(), ref64), f"{what}: the reference is not exact in fp32 - the case proves nothing"
    want = ref64.float().to(out_dtype)
    got = got.detach().cpu()
    assert got.dtype == out_dtype and got.shape == want.shape, (what, got.dtype, out_dtype, tuple(got.shape), tuple(want.shape))
    if torch.equal(got, want):
        return
    bad = (got != want) | torch.isnan(got)
    at = _first_mismatch(bad, got.shape)
    g, w = float(got[at]), float(want[at])
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {at}: got {g!r}, expected {w!r} "
                         f"(exact {float(ref64[at])!r}); difference / alpha = {(g - float(ref64[at])) / alpha!r}")


ACT_FP64 = {"none": lambda t: t, "silu": torch.nn.functional.silu, "gelu": torch.nn.functional.gelu}


def act_interval(ref64, out_dtype):
    """[lo, hi] per element for the result of an activation epilogue: the fp32 value within 2e-4 * max(1, |ref|) of the fp64
    activation - what the device activation code is held to in fp32 (test_value_ranges.assert_pointwise) - and, for a bf16 output,
    the ONE round-to-nearest-even of such a value: rounding is monotonic, so the stored number lies between the roundings of the
    two ends.  (A relative allowance for the final rounding would have to be 2^-8 |ref|, half an ulp just above a power of two;
    2^-9 |ref| is half an ulp only just BELOW one and refuses the correctly rounded exact result.  The interval needs neither.)"""
    lim = 2e-4 * torch.clamp(ref64.abs(), min=1.0)
    lo, hi = ref64 - lim, ref64 + lim
    if out_dtype == torch.bfloat16:
        lo, hi = lo.to(torch.bfloat16).double(), hi.to(torch.bfloat16).double()
    return lo, hi


def assert_act_exact_pre(got, pre64, act, out_dtype, what):
    """epilogues with an activation: the pre-activation pre64 is exact (an fp32 number), the activation is not.  `act` is a name
    of ACT_FP64 or a callable fp64 -> fp64 (GEGLU: it rounds value and gate to bf16 first, as the epilogue does); the result is
    held per element to act_interval of the fp64 activation of pre64."""
    assert pre64.dtype == torch.float64
    assert torch.equal(pre64.float().double(), pre64), f"{what}: the pre-activation is not exact in fp32 - the case proves nothing"
    ref = (ACT_FP64[act] if isinstance(act, str) else act)(pre64)
    got = got.detach().cpu()
    assert got.dtype == out_dtype and got.shape == ref.shape, (what, got.dtype, out_dtype, tuple(got.shape), tuple(ref.shape))
    lo, hi = act_interval(ref, out_dtype)
    g = got.double()
    bad = ~((g >= lo) & (g <= hi))  # (a NaN is bad)
    if bool(bad.any()):
        at = _first_mismatch(bad, got.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the bound, first at {at}: got {float(got[at])!r}, "
                             f"expected {float(ref[at])!r} (accepted: {float(lo[at])!r} .. {float(hi[at])!r})")


_INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_BYTE_FILL = 0xA5  # fill of integer windows: no value a kernel under test writes by accident in a whole row


class Window:
    """A [rows, cols] operand at leading dimension `ld` (optionally `batch` of them, `gap` elements apart) embedded in ONE
    flat poisoned buffer: `lead` guard rows, a `left` element offset, the rows with their ld - cols pad columns, the gaps
    between batch entries, `trail` guard rows.  Float buffers are filled with NaN (an input window: whatever a kernel reads
    outside its operand poisons its result), integer buffers with a fixed byte pattern.  An output window is armed after the
    operand was written and checked bit for bit afterwards: every element outside the window must be what it was.
    `left` = 8 elements keeps the window 16-byte aligned; the scalar-path cases use left = 1 with an odd ld."""

    def __init__(self, rows, cols, ld=None, dtype=torch.float32, device="cpu", lead=2, trail=2, left=8, batch=1, gap=0):
        ld = cols if ld is None else ld
        assert ld >= cols and rows >= 1 and batch >= 1
        self.rows, self.cols, self.ld, self.batch = rows, cols, ld, batch
        self.stride = rows * ld + gap  # element stride between batch entries
        self.off = lead * ld + left
        n = self.off + batch * self.stride + trail * ld
        if dtype.is_floating_point:
            self.buf = torch.full((n,), float("nan"), dtype=dtype, device=device)
        else:
            self.buf = torch.empty(n, dtype=dtype, device=device)
            self.buf.view(torch.uint8).fill_(_BYTE_FILL)
        self._snap = None
        inside = torch.zeros(n, dtype=torch.bool)
        torch.as_strided(inside, (batch, rows, cols), (self.stride, ld, 1), self.off).fill_(True)
        self._outside = (~inside).to(device)

    def _strided(self, cols):
        if self.batch == 1:
            return torch.as_strided(self.buf, (self.rows, cols), (self.ld, 1), self.off)
        return torch.as_strided(self.buf, (self.batch, self.rows, cols), (self.stride, self.ld, 1), self.off)

    @property
    def view(self):
        """the strided [rows, cols] ([batch, rows, cols]) tensor; its data_ptr() is what the kernel gets"""
        return self._strided(self.cols)

    @property
    def padded(self):
        """[rows, ld] rows INCLUDING their pad columns, for the bindings that read a leading dimension off shape[1]"""
        assert self.batch == 1
        return torch.as_strided(self.buf, (self.rows, self.ld), (self.ld, 1), self.off)

    @property
    def flat(self):
        """the window as one vector (an operand without a leading dimension)"""
        assert self.batch == 1 and (self.ld == self.cols or self.rows == 1)
        return torch.as_strided(self.buf, (self.rows * self.cols,), (1,), self.off)

    def put(self, x):
        self.view.copy_(x.to(device=self.buf.device, dtype=self.buf.dtype).reshape(self.view.shape))
        return self

    def arm(self):
        """snapshot the whole buffer as raw integers (after put, before the call)"""
        self._snap = self.buf.view(_INT_OF[self.buf.element_size()]).clone()
        return self

    def get(self):
        return self.view.clone()

    def assert_guard_intact(self, what=""):
        assert self._snap is not None, "arm() the window before the call"
        now = self.buf.view(_INT_OF[self.buf.element_size()])
        bad = (now != self._snap) & self._outside
        n = int(bad.sum())
        if n:
            i = int(torch.nonzero(bad)[0])
            r, c = divmod(i - self.off, self.ld) if i >= self.off else (-1, i)
            raise AssertionError(f"{what}: {n} guard element(s) overwritten, first at flat index {i} "
                                 f"(row {r}, column {c} of a [{self.rows}, {self.cols}] window at ld {self.ld})")

    def assert_written(self, what=""):
        """every window element was written (float windows: no NaN left and none leaked in)"""
        assert torch.isfinite(self.view.float()).all(), f"{what}: non-finite values inside the window"


# ---- exact attention operands (tests/test_exact_attention.py) ----------------------------------------------------------------
# Every query attends a SET of keys whose raw scores are all equal (c^2, with c^2 * scale = 128); every other key scores 0, at
# least 104 / scale lower, so that its un-normalised probability is exactly 0 in fp32.  The closed form - P = indicator / |S| -
# is the reference; with integer V and dO and power-of-two |S| every partial sum of every kernel is an fp32 number.
ATTN_SIZES = (1, 2, 4, 8, 16, 32)
ATTN_GAP = 128.0  # c^2 * scale
ATTN_ORDERS = ("strided", "ascending", "tail")


def attn_group_sizes(Nk):
    """sizes that cover Nk keys: one of each power of two up to 32 while they fit, then 32s, then AT MOST ONE remainder group
    below 32 (which may or may not be a power of two)"""
    sizes, left = [], Nk
    for s in ATTN_SIZES:
        if left >= s:
            sizes.append(s)
            left -= s
    while left >= 32:
        sizes.append(32)
        left -= 32
    if left:
        sizes.append(left)
    assert sum(sizes) == Nk and sum(1 for s in sizes if s & (s - 1)) <= 1
    return sizes


def _is_pow2(n):
    return (n > 0) & ((n & (n - 1)) == 0)


def exact_attention_operands(B, H, Nq, Nk, d, order="strided", layout=0, scale=0.125, seed=0, uniform=False):
    """fp64 Q [B, H, Nq, d], K, V [B, H, Nk, d], dO dense / sparse [B, H, Nq, d] and the key -> group map of every head.
    Head dims are of three disjoint kinds: G code dims (column 0 and column d - 1 among them) carry c in key j at its group's
    dim and in query i at its target's; K-noise dims hold +-{1..4} in K and 0 in Q, Q-noise dims the reverse (`layout` swaps
    the two), so that raw scores are exactly c^2 or 0 while dQ and dK are not trivially zero.  `order`: 'strided' spreads every
    group over all key tiles, 'ascending' lays the groups out one after the other, 'tail' does so with the groups a head's
    queries attend LAST (earlier tiles accumulate keys the moving maximum later zeroes).  Query i of head (b, h) targets group
    (i + rot[b, h]) % G.  uniform: Q = 0 - every key counts once."""
    c = (ATTN_GAP / scale) ** 0.5
    assert c == int(c) and math.frexp(scale)[0] == 0.5, "scale: a power of two with an integer c"
    sizes = attn_group_sizes(Nk)
    G = len(sizes)
    assert G <= d // 2, f"{G} groups need {2 * G} head dims, d = {d}"
    pos = [0] if G == 1 else [(p * (d - 1)) // (G - 1) for p in range(G)]
    assert len(set(pos)) == G and pos[0] == 0 and pos[-1] >= d - 8
    rest = [x for x in range(d) if x not in pos]
    qn, kn = (rest[0::2], rest[1::2]) if layout == 0 else (rest[1::2], rest[0::2])
    pos_t, sizes_t = torch.tensor(pos), torch.tensor(sizes)
    Q, K = torch.zeros(B, H, Nq, d, dtype=torch.float64), torch.zeros(B, H, Nk, d, dtype=torch.float64)
    kg = torch.empty(B, H, Nk, dtype=torch.long)
    rot = torch.empty(B, H, dtype=torch.long)
    frac = torch.cat([(torch.arange(s) + 0.5) / s for s in sizes])  # position of a key inside its group, as a fraction
    gid = torch.repeat_interleave(torch.arange(G), sizes_t)
    for b in range(B):
        for h in range(H):
            r = (3 * (b * H + h) + 1) % G
            rot[b, h] = r
            if order == "strided":
                kg[b, h] = gid[torch.argsort(frac + gid * 1e-6, stable=True)]
            elif order == "ascending":
                kg[b, h] = gid
            else:
                assert order == "tail"
                seq = (torch.arange(G) + r + min(Nq, G)) % G  # the attended groups r .. r + min(Nq, G) - 1 come last
                kg[b, h] = torch.repeat_interleave(seq, sizes_t[seq])
            K[b, h, torch.arange(Nk), pos_t[kg[b, h]]] = c
            if not uniform:
                Q[b, h, torch.arange(Nq), pos_t[(torch.arange(Nq) + r) % G]] = c
    if not uniform:
        Q[..., qn] = ints(B, H, Nq, len(qn), seed=seed + 1, hi=4).double()
    K[..., kn] = ints(B, H, Nk, len(kn), seed=seed + 2, hi=4).double()
    V = ints(B, H, Nk, d, seed=seed + 3, hi=4).double()
    dO = ints(B, H, Nq, d, seed=seed + 4, hi=4).double()
    g = torch.Generator().manual_seed(seed + 5)
    sp = torch.zeros(B, H, Nq, d, dtype=torch.float64)
    col = (torch.arange(Nq)[None, None, :] * 7 + 3 + torch.arange(B * H).reshape(B, H, 1)) % d  # walks over all d columns
    sp.scatter_(-1, col[..., None], (torch.randint(0, 2, (B, H, Nq, 1), generator=g) * 2 - 1).double())
    return dict(Q=Q, K=K, V=V, dO_dense=dO, dO_sparse=sp, kg=kg, rot=rot, sizes=sizes, scale=scale, code_dims=pos)


def exact_attention_forward(Q, K, V, scale, allowed=None):
    """closed form in fp64 (NOT a softmax, which leaves 1e-57 in the unattended entries): the attended set of a row is where its
    raw score is the row's maximum over the allowed keys; P = indicator / |S|, O = P V, lse = max * scale + ln |S|.  Asserts the
    preconditions of the forward on these inputs."""
    S = Q @ K.transpose(-1, -2)
    assert float(S.abs().max()) < 2 ** 24 and torch.equal(S, S.round()), "raw scores must be exact in fp32"
    Sm = S if allowed is None else S.masked_fill(~allowed, float("-inf"))
    top = Sm.max(-1, keepdim=True).values
    assert bool(torch.isfinite(top).all()), "a row without an allowed key"
    M = Sm == top
    other = torch.isfinite(Sm) & ~M
    if bool(other.any()):
        gap = float((top - Sm)[other].min())
        assert gap >= 104.0 / scale, f"an unattended key scores only {gap * scale} below the attended ones: exp(-104) is the first fp32 zero"
    n = M.sum(-1)
    P = M.double() / n[..., None]
    O = (M.double() @ V) / n[..., None]  # (the sum is exact; P @ V would leave 1e-16 where a sum over a set of 3 is zero)
    # every partial sum of un-normalised P V - the keys a moving maximum later zeroes included - is an integer below 2^24
    assert torch.equal(V, V.round()) and V.shape[-2] * float(V.abs().max()) < 2 ** 24
    return dict(M=M, n=n, P=P, O=O, A_O=P @ V.abs(), lse=top[..., 0] * scale + torch.log(n.double()), row_pow2=_is_pow2(n) & (n <= 32))


def bf16_number(x64):
    return x64.float().to(torch.bfloat16).double() == x64


def exact_attention_backward(Q, K, V, scale, fwd, dO, gP=None, exact_dS=True):
    """dV = P^T dO, D = rowsum(P . dP) (= rowsum(dO . O) without a gradient on P), dS = P (dP - D), dQ = scale dS K,
    dK = scale dS^T Q, each with the same formula on absolute values (A_*: the scale of the fp32 bound).  key_pow2: keys every
    attending row of which has a power-of-two set.  Asserts the preconditions: (exact_dS) scale * dS of the power-of-two rows is
    a bf16 number - the kernels pack it - and every partial sum is a multiple of `unit` below 2^24 units."""
    P, M, rp2 = fwd["P"], fwd["M"], fwd["row_pow2"]
    Vt = V.transpose(-1, -2)
    dP = dO @ Vt
    aP = dO.abs() @ Vt.abs()
    if gP is not None:
        dP, aP = dP + gP, aP + gP.abs()
    D = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - D)
    aS = P * (aP + (P * aP).sum(-1, keepdim=True))
    out = dict(dV=P.transpose(-1, -2) @ dO, A_dV=P.transpose(-1, -2) @ dO.abs(), dS=dS,
               dQ=scale * (dS @ K), A_dQ=scale * (aS @ K.abs()), dK=scale * (dS.transpose(-1, -2) @ Q),
               A_dK=scale * (aS.transpose(-1, -2) @ Q.abs()))
    out["key_pow2"] = ~((M & ~rp2[..., None]).any(-2))
    unit = scale / 1024.0  # P in multiples of 1/32, dS of 1/32^2
    rows, keys = rp2[..., None], out["key_pow2"][..., None]
    assert torch.equal(dO, dO.round()) and float(out["A_dV"].max()) < 2 ** 24 / 32
    if exact_dS:
        sdS = (scale * dS)[rp2]
        assert bool(bf16_number(sdS).all()), "scale * dS of a power-of-two row is not a bf16 number: the pack would round it"
        assert torch.equal(sdS / unit, (sdS / unit).round())
        assert float((out["A_dQ"] * rows).max()) < 2 ** 24 * unit and float((out["A_dK"] * keys).max()) < 2 ** 24 * unit
    return out


def _at(bad):
    return _first_mismatch(bad, bad.shape)


def attn_bits_error(got, exact64, sel, what, explain=None):
    """None, or what is wrong: on the rows `sel` [B, H, N] `got` (bf16 [B, H, N, d]) must be the ONE round-to-nearest-even of the
    exact value, bit for bit.  explain(b, h, row, got_row) -> the nearest single-key explanation."""
    assert got.dtype == torch.bfloat16 and got.shape == exact64.shape, (what, got.dtype, tuple(got.shape), tuple(exact64.shape))
    pick = sel[..., None].expand_as(exact64)
    assert torch.equal(exact64.float().double()[pick], exact64[pick]), f"{what}: the reference is not exact in fp32 - the case proves nothing"
    want = exact64.float().to(torch.bfloat16)
    bad = ((got != want) | torch.isnan(got)) & pick
    if not bool(bad.any()):
        return None
    at = _at(bad)
    msg = (f"{what}: {int(bad.sum())} of {int(pick.sum())} elements differ, first at (batch, head, row, column) = {at}: got {float(got[at])!r}, "
           f"expected {float(want[at])!r} (exact {float(exact64[at])!r})")
    if explain is not None:
        msg += "; " + explain(at[0], at[1], at[2], got[at[:3]])
    return msg


def attn_lse_error(lse, ref64, what, ulps=16):
    """None, or what is wrong: |lse - ref| <= 16 fp32 ulps of |ref| (2.4e-4 at 130: covers m * scale + log l, the residual of
    the fused multiply-add and the base-2 detour; a miscounted key moves lse by at least ln(33 / 32) = 0.031)"""
    lse = lse.double()
    lim = ulps * torch.exp2(torch.floor(torch.log2(ref64.abs().clamp(min=1e-30))) - 23)
    bad = ~((lse - ref64).abs() <= lim)
    if not bool(bad.any()):
        return None
    at = _at(bad)
    return (f"{what}: {int(bad.sum())} of {bad.numel()} rows beyond {ulps} ulps, first at (batch, head, row) = {at}: got {float(lse[at])!r}, expected "
            f"{float(ref64[at])!r}: |S| is off by a factor {float(torch.exp(lse[at] - ref64[at]))!r}")


def attn_close_error(got, exact64, A64, what, dtype=torch.float32, explain=None):
    """None, or what is wrong: per element |got - exact| <= tol(dtype) * A, A the same formula on absolute values"""
    g = got.double()
    bad = ~((g - exact64).abs() <= tol(dtype) * A64)
    if not bool(bad.any()):
        return None
    at = _at(bad)
    return (f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond {tol(dtype)} * A, first at {at}: got {float(g[at])!r}, exact {float(exact64[at])!r}, "
            f"A {float(A64[at])!r}" + ("; " + explain(at[0], at[1], at[2], got[at[:3]]) if explain is not None else ""))


def attn_rounded_error(got, exact64, A64, what, sel=None, explain=None):
    """None, or what is wrong: a bf16 result of fp32 arithmetic on UN-snapped probabilities (the simulator keeps P in fp32).
    Its value before the store is within tol(float32) * A of the exact one - the bound of the fp32 legs, A the same formula on
    absolute values - and the store is one round-to-nearest-even, which is monotonic: the stored number lies between the
    roundings of the two ends (act_interval's argument).  Where the terms do not cancel (A ~ |exact|) that is the exact value
    itself if it is a bf16 number and one of its two bf16 neighbours otherwise; where they do - a sum of +-v / 3 that is exactly
    zero, dQ in a code column - fp32 leaves a residual of 1e-8 that no relative bound around an exact zero admits."""
    g = got.double()
    e = tol(torch.float32) * A64
    lo, hi = (exact64 - e).float().to(torch.bfloat16).double(), (exact64 + e).float().to(torch.bfloat16).double()
    bad = ~((g >= lo) & (g <= hi))
    if sel is not None:  # rows [B, H, N] to hold
        bad = bad & sel[..., None]
    if not bool(bad.any()):
        return None
    at = _at(bad)
    return (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {at}: got {float(g[at])!r}, exact {float(exact64[at])!r} "
            f"(accepted: {float(lo[at])!r} .. {float(hi[at])!r})" + ("; " + explain(at[0], at[1], at[2], got[at[:3]]) if explain is not None else ""))


def single_term_explanation(got_row, cands, noun):
    """cands: {label: fp64 [n, d]} - row k of a label is the value of this output row had term k been treated that way.  Names
    the first (label, k) whose bf16 rounding is `got_row` in every column (an fp32 row: that lies within 2e-4 of the row's
    largest value of it), else the nearest one."""
    best = None
    g = got_row.double()
    for label, c in cands.items():
        if c.numel() == 0:
            continue
        if got_row.dtype == torch.bfloat16:
            hit = (c.float().to(torch.bfloat16).double() == g).all(-1)
        else:
            hit = (c - g).abs().amax(-1) <= 2e-4 * float(g.abs().max())
        if bool(hit.any()):
            return f"reproduced by {noun} {int(torch.nonzero(hit)[0])} {label}"
        err = (c - g).abs().amax(-1)
        k = int(err.argmin())
        if best is None or float(err[k]) < best[0]:
            best = (float(err[k]), label, k)
    return f"no single {noun} reproduces the row; nearest: {noun} {best[2]} {best[1]} (max |difference| {best[0]:.3g})" if best else f"no {noun} to explain it"


def explain_O_row(V_bh, M_row):
    """candidates for one output row: every key of the set dropped, every key counted once more, with and without the
    normaliser following"""
    n = int(M_row.sum())
    tot = (V_bh * M_row[:, None]).sum(0)
    m = M_row[:, None]
    inf = torch.full_like(V_bh, float("inf"))
    drop = torch.where(m, tot - V_bh, inf)  # only a key of the set can be dropped
    return {"dropped (normaliser too)": drop / max(n - 1, 1), "dropped (normaliser kept)": drop / n,
            "counted once more (normaliser too)": (tot + V_bh) / (n + 1), "counted once more (normaliser kept)": (tot + V_bh) / n}
