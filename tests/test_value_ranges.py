"""Value ranges: the kernels that reduce and then subtract, exponentiate or divide, on the inputs that separate a right
implementation from a subtly wrong one.  The other parity modules draw every operand from `rnd()` (unit-variance noise):
flat softmax rows, group means of ~0, logits within +-4, AdamW steps of 0.1 % of the parameter.  Here the shapes are the
smallest that reach each code path and the VALUES are the hard part.

Common rules
  * reference: the plain fp64 evaluation of the operation on the dtype-rounded inputs;
  * bound: the one the sibling test of test_ops.py uses for that quantity, `tol(dtype) * factor` through `check` - applied per
    statistical unit (group, row, block of queries) wherever the case gives the units different scales, so that a unit with
    small outputs cannot hide behind a large one;
  * precondition (`headroom`): the same formula evaluated in torch fp32 on the CPU stays within a tenth of that bound.  It is
    a condition on the inputs - the ladder asks nothing that plain fp32 arithmetic cannot give - not a measurement of a kernel.

1. GroupNorm / LayerNorm conditioning (siblings: test_groupnorm, test_groupnorm_two_launch_forms, test_layernorm)
   ladder, one rung per group or row: mean / deviation in {0, 10, 100} (the offset's sign alternates), scale in {1e-3, 1, 1e3},
   one exactly constant unit, one unit constant but for a single element.  Bounds: y `tol(dtype)`, dx `tol(dtype) * 2` per unit;
   rstd against fp64 at `tol(float32)` for both storage types (the statistics are fp32 either way), the mean likewise in units
   of the deviation; the constant unit has rstd = 1 / sqrt(eps) to fp32 rounding, y = silu?(beta) and a finite gradient.  On
   the hip leg every `norm_fused` mode 0..5 runs.  Precondition: two-pass fp32 statistics, a tenth of each bound.
2. fused attention on peaked and ordered scores (siblings: test_flash_attention, test_attention)
   q_i = b_i u + noise, k_j = a_j u + noise, a_j a ramp: scaled scores span ~ +-25; keys ascending (the running maximum moves
   on every tile), descending (never after tile 0), shuffled; one dominant key per row (p_max > 0.999); half of the queries
   scaled by 0.01 (flat and peaked rows in one wave).  Bounds: O `tol`, dQ / dK / dV `tol * 3`, log-sum-exp against fp64
   `tol(float32) * max(1, |lse|)`; the three key orders agree with each other to the same bounds.  The unfused path (causal
   and key mask) on the same scores: P and O `tol`, row sums as test_attention, gradients `tol * 3`.  Precondition: torch fp32
   attention, a tenth of each bound - which the dominant-key case meets for O, dV and the log-sum-exp only: dS = P (dP - D)
   cancels there, plain fp32 leaves dQ and dK 3e-4 .. 5e-2 from fp64 against their own (vanishing) maximum, so those two are
   only required to be finite in that case.  The mixed case checks O and dQ per unit (flat rows / peaked rows).
3. masked softmax edges (sibling: test_attention's probability check, `tol(dtype)` per row)
   a fully masked row (all-zero P and dS, never NaN), a row that sees exactly one key (exactly 1.0), equal visible scores,
   scores at +-80; cols in {1, 65, 77}.  Precondition: torch fp32 softmax, a tenth of the bound.
4. cross entropy (sibling: test_cross_entropy: loss and token log-probabilities `tol(float32) * 5`, gradient `tol(dtype)`)
   a confident row (loss exactly 0: it must count as a valid row), logits scaled by 20, an all-equal row, a row shifted by
   +1000 (fp32) / +64 (bf16), a label on the minimum logit -80, an ignored row; and a batch of ignored rows only (loss 0,
   gradient 0).  Precondition: torch fp32 log-softmax, a tenth of each bound.
5. optimizer tail (siblings: test_adamw_with_clip: `tol(float32)` on the checked quantity, sumsq `tol(float32) * 5`)
   |p| <= 0.05, |g| from 1e-6 to 1e2 in one buffer, one g = 0; steps 1, 2 and 1000, clip active and idle; the UPDATE
   p_after - p_before, m and v against an fp64 AdamW, each against its own maximum.  sumsq / grad_norm_scale: all-ones buffers
   sum to n exactly; 1e-3 next to 1e3; a zero gradient stays zero.  Precondition: fp32 AdamW, a tenth of the bound.
6. BCE heads and activations (siblings: test_disc_head, test_convhead_matches_conv2d_bce, test_elementwise)
   logits at +-100 and 0 reached through the weights; SiLU, GELU and GEGLU at x in {+-0, +-1e-6, +-5, +-20, +-90, +-1e4}, per
   element |err| <= tol * max(1, |ref|), finite everywhere.  Precondition: torch fp32, a tenth of the bound (GEGLU pairs every
   value with every gate but 1e4 * gelu(-5), which the precondition rules out).

Found by these tests and fixed with them: GroupNorm's fp32 sums of x and x^2 (rstd up to 4.6e-3 off, y up to 5.4e-3 of its
scale at mean / deviation 100: now shifted sums where a group needs them, norm.hip), 0 * (target / 0) = NaN in
comat_grad_norm_scale, and the 0 / 0 loss of ops.cross_entropy on a batch without a valid row.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from comat_amd import ops
from helpers import _set_opts, default_opts, restore_default_opts  # noqa: F401 - default_opts is a fixture
from test_ops import check, rnd, tol

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DTYPES = [F32, BF16]


def dv(x, dev, dtype=None):
    return x.detach().to(device=dev, dtype=dtype or x.dtype).contiguous().clone()


def unit_err(got, ref):
    """max over the units (rows of [units, -1]) of max |got - ref| / (max |ref| + 1e-6): the quantity `check` bounds"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    got, ref = got.reshape(got.shape[0], -1), ref.reshape(ref.shape[0], -1)
    return float(((got - ref).abs().amax(1) / (ref.abs().amax(1) + 1e-6)).max())


def headroom(ref32, ref64, dtype, what, factor=1.0):
    """the precondition: fp32 evaluation of the reference formula within a tenth of the bound, per unit"""
    e = unit_err(ref32, ref64)
    assert e < tol(dtype) * factor / 10, f"{what}: plain fp32 is {e:.2e} from fp64 - the inputs ask more than the bound / 10"


def check_units(got, ref, dtype, what, factor=1.0):
    """`check` per unit: got / ref are [units, ...]"""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    for u in range(got.shape[0]):
        check(got[u], ref[u], dtype, f"{what} [unit {u}]", factor=factor)


# ================================================================================================================
# 1. GroupNorm / LayerNorm conditioning
# ================================================================================================================
CONST, ONE_OFF = "const", "one-off"
# (mean / deviation, scale) per unit, the hard rungs first so that the smallest shape has them
RUNGS = [(100, 1.0), (100, 1e3), (100, 1e-3), CONST, ONE_OFF, (10, 1.0), (10, 1e-3), (10, 1e3), (0, 1.0), (0, 1e-3), (0, 1e3)]
CONST_VALUE = 3.5  # dyadic: sums of it are exact in fp32, so the fp32 precondition holds with var = 0


def ladder(units, per_unit, dtype, seed):
    """[units, per_unit] values representable in `dtype`, unit u on rung RUNGS[u % 11]"""
    x = rnd(units, per_unit, seed=seed)
    for u in range(units):
        rung = RUNGS[u % len(RUNGS)]
        if rung == CONST:
            x[u] = CONST_VALUE
        elif rung == ONE_OFF:
            x[u] = CONST_VALUE
            x[u, per_unit // 2] = CONST_VALUE + 1.0
        else:
            ratio, scale = rung
            x[u] = (x[u] + (ratio if u % 2 == 0 else -ratio)) * scale
    return x.to(dtype).float()


def norm_reference(xu, gamma_u, beta_u, gyu, eps, silu, dt):
    """units are rows of xu [U, n]; gamma_u / beta_u [U, n] already laid out per element.  Two-pass statistics in `dt`."""
    x = xu.to(dt).requires_grad_(True)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = (var + torch.tensor(eps, dtype=F32).to(dt)).rsqrt()
    y = (x - mean) * rstd * gamma_u.to(dt) + beta_u.to(dt)
    if silu:
        y = F.silu(y)
    (dx,) = torch.autograd.grad(y, x, gyu.to(dt))
    return y.detach(), dx, mean.detach()[:, 0], rstd.detach()[:, 0]


def assert_norm(got, ref64, ref32, xu, beta_u, dtype, silu, eps, what):
    y, dx, mean, rstd = got
    y64, dx64, mean64, rstd64 = ref64
    headroom(ref32[0], y64, dtype, what + " y")
    headroom(ref32[1], dx64, dtype, what + " dx", factor=2)
    assert float(((ref32[3].double() - rstd64) / rstd64).abs().max()) < tol(F32) / 10, what + ": fp32 rstd"
    assert float(((ref32[2].double() - mean64) * rstd64).abs().max()) < tol(F32) / 10, what + ": fp32 mean"
    check_units(y, y64, dtype, what + " y")
    check_units(dx, dx64, dtype, what + " dx", factor=2)
    e_r = ((rstd.double().cpu() - rstd64) / rstd64).abs()
    assert float(e_r.max()) < tol(F32), f"{what}: rstd off by {float(e_r.max()):.2e} relative (unit {int(e_r.argmax())})"
    e_m = ((mean.double().cpu() - mean64) * rstd64).abs()
    assert float(e_m.max()) < tol(F32), f"{what}: mean off by {float(e_m.max()):.2e} deviations (unit {int(e_m.argmax())})"
    for u in range(xu.shape[0]):
        if RUNGS[u % len(RUNGS)] != CONST:
            continue
        want = 1.0 / math.sqrt(float(torch.tensor(eps, dtype=F32)))
        assert abs(float(rstd[u]) - want) <= want * 2.0 ** -21, f"{what}: constant unit {u}: rstd {float(rstd[u])} != {want}"
        yb = beta_u[u].to(dtype).float()
        if silu:
            check(y[u], F.silu(beta_u[u].double()), dtype, f"{what}: constant unit {u}: y != silu(beta)")
        else:
            assert torch.equal(y[u].float().cpu(), yb), f"{what}: constant unit {u}: y != beta"
        assert torch.isfinite(dx[u].float()).all(), f"{what}: constant unit {u}: non-finite gradient"


def gn_units(t, B, HW, C, G):
    """[B*HW, C] -> [B*G, HW * C/G]"""
    return t.reshape(B, HW, G, C // G).permute(0, 2, 1, 3).reshape(B * G, HW * (C // G))


def gn_tokens(t, B, HW, C, G):
    return t.reshape(B, G, HW, C // G).permute(0, 2, 1, 3).reshape(B * HW, C)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("shape", [(2, 50, 32, 8), (1, 130, 320, 32), (2, 256, 64, 8), (1, 1024, 128, 32)])
def test_groupnorm_conditioning(dev, dtype, silu, shape, default_opts):
    B, HW, C, G = shape
    eps, cpg = 1e-5, C // G
    xu = ladder(B * G, HW * cpg, dtype, seed=1)
    gamma, beta = rnd(C, seed=2) * 0.5 + 1, rnd(C, seed=3) * 0.3
    gyu = rnd(B * G, HW * cpg, dtype=dtype, seed=4)
    per_el = lambda v: gn_units(v.reshape(1, C).expand(B * HW, C), B, HW, C, G)
    gamma_u, beta_u = per_el(gamma), per_el(beta)
    ref64 = norm_reference(xu, gamma_u, beta_u, gyu, eps, silu, F64)
    ref32 = norm_reference(xu, gamma_u, beta_u, gyu, eps, silu, F32)
    k = ops.kernels()
    x, gy = dv(gn_tokens(xu, B, HW, C, G), dev, dtype), dv(gn_tokens(gyu, B, HW, C, G), dev, dtype)
    gd, bd = dv(gamma, dev), dv(beta, dev)
    # every multi-launch form needs whole 16-byte channel vectors; these shapes all have them, so every mode accepts them
    assert C % (4 if dtype == F32 else 8) == 0
    for mode in (range(6) if dev.type == "cuda" else (None,)):
        if mode is not None:
            _set_opts(norm_fused=mode)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        stats = torch.full((B, G, 2), float("nan"), dtype=F32, device=dev)
        k.groupnorm_fwd(x, gd, bd, y, stats, B, HW, C, G, eps, silu)
        k.groupnorm_bwd(gy, x, gd, bd, stats, dx, B, HW, C, G, silu)
        st = stats.cpu().reshape(B * G, 2)
        got = (gn_units(y.float().cpu(), B, HW, C, G), gn_units(dx.float().cpu(), B, HW, C, G), st[:, 0], st[:, 1])
        assert_norm(got, ref64, ref32, xu, beta_u, dtype, silu, eps, f"gn {shape} norm_fused={mode}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(5, 70), (37, 96), (8, 1280)])
def test_layernorm_conditioning(dev, dtype, shape):
    M, C = shape
    eps = 1e-5
    x = ladder(M, C, dtype, seed=1)
    gamma, beta = rnd(C, seed=2) * 0.5 + 1, rnd(C, seed=3) * 0.3
    gy = rnd(M, C, dtype=dtype, seed=4)
    gamma_u, beta_u = gamma.reshape(1, C).expand(M, C), beta.reshape(1, C).expand(M, C)
    ref64 = norm_reference(x, gamma_u, beta_u, gy, eps, False, F64)
    ref32 = norm_reference(x, gamma_u, beta_u, gy, eps, False, F32)
    k = ops.kernels()
    xd, gd = dv(x, dev, dtype), dv(gy, dev, dtype)
    y, dx = torch.empty_like(xd), torch.empty_like(xd)
    stats = torch.full((M, 2), float("nan"), dtype=F32, device=dev)
    k.layernorm_fwd(xd, dv(gamma, dev), dv(beta, dev), y, stats, M, C, eps)
    k.layernorm_bwd(gd, xd, dv(gamma, dev), stats, dx, M, C)
    st = stats.cpu()
    assert_norm((y.float().cpu(), dx.float().cpu(), st[:, 0], st[:, 1]), ref64, ref32, x, beta_u, dtype, False, eps, f"ln {shape}")


# ================================================================================================================
# 3. masked softmax edges
# ================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", [1, 65, 77])
def test_softmax_edges(dev, dtype, cols):
    k = ops.kernels()
    g = torch.Generator().manual_seed(cols)
    R = 6
    S = torch.randn(R, cols, generator=g) * 10
    mask = torch.ones(R, cols, dtype=torch.int8)
    mask[0] = 0                                    # row 0: fully masked
    mask[1] = 0
    mask[1, cols // 2] = 1                         # row 1: exactly one visible key
    S[2] = 7.25                                    # row 2: equal visible scores, a third of the keys masked
    mask[2, 1::3] = 0
    S[3] = torch.where(torch.arange(cols) % 2 == 0, 80.0, -80.0)  # row 3: scores at +-80
    S[4, cols // 3] = 80.0                         # row 4: noise with one score at +80, masked keys at the row's end
    mask[4, cols - cols // 4:] = 0
    # row 5: plain noise of deviation 10
    causal_rows = 4                                # and a causal call: row q sees keys 0..q, row 0 exactly one
    Sc = torch.where(torch.arange(cols)[None, :] % 2 == 0, 80.0, -80.0) + torch.randn(causal_rows, cols, generator=g)

    def reference(s, visible, dt):
        p = torch.softmax(s.to(dt).masked_fill(~visible, float("-inf")), -1)
        return torch.nan_to_num(p, nan=0.0)  # the behaviour the kernel defines for a row without a visible key
    vis = mask.bool()
    vis_c = torch.arange(cols)[None, :] <= torch.arange(causal_rows)[:, None]
    for s, visible, kw, what in ((S, vis, dict(key_mask=dv(mask, dev), rows_per_mask=1), "key mask"),
                                 (Sc, vis_c, dict(q_len=causal_rows, causal=True, causal_offset=0), "causal")):
        rows = s.shape[0]
        p64 = reference(s, visible, F64)
        headroom(reference(s, visible, F32), p64, dtype, f"softmax {what}")
        P = torch.full((rows, cols), float("nan"), dtype=dtype, device=dev)
        k.softmax_fwd(dv(s, dev), P, rows, cols, **kw)
        check_units(P, p64, dtype, f"softmax {what} cols={cols}")
        Pc = P.float().cpu()
        assert torch.equal(Pc[~visible], torch.zeros_like(Pc[~visible])), f"softmax {what}: a masked key has weight"
        one = visible.sum(1) == 1
        assert one.any() and torch.equal(Pc[one][visible[one]], torch.ones(int(one.sum()))), \
            f"softmax {what}: one visible key is not exactly 1.0"
        # backward from the kernel's own P (its dtype-rounded input)
        dP = torch.randn(rows, cols, generator=g) * 3
        bwd = lambda dt: 0.37 * Pc.to(dt) * (dP.to(dt) - (dP.to(dt) * Pc.to(dt)).sum(-1, keepdim=True))
        live = visible.sum(1) > 1  # (one visible key: dS = p (g - g p) is 0 up to rounding - nothing to scale an error by)
        if live.any():
            headroom(bwd(F32)[live], bwd(F64)[live], dtype, f"softmax bwd {what}")
        dS = torch.full((rows, cols), float("nan"), dtype=dtype, device=dev)
        k.softmax_bwd(P, dv(dP, dev), dS, rows, cols, 0.37)
        dSc = dS.float().cpu()
        assert torch.isfinite(dSc).all(), f"softmax bwd {what}: non-finite values"
        if live.any():
            check_units(dSc[live], bwd(F64)[live], dtype, f"softmax bwd {what} cols={cols}")
        assert torch.equal(dSc[~live], torch.zeros_like(dSc[~live])), f"softmax bwd {what}: a row with <= 1 visible key has a gradient"


# ================================================================================================================
# 4. cross entropy
# ================================================================================================================
def ce_problem(V, dtype, seed):
    T = 6
    z = rnd(T, V, seed=seed) * 3
    labels = torch.randint(0, V, (T,), generator=torch.Generator().manual_seed(seed + 1))
    z[0] = -60.0
    z[0, labels[0]] = 60.0                       # confident: loss exactly 0
    z[1] = z[1] * 20 / 3                         # logits of deviation 20
    z[2] = 1.5                                   # all equal
    z[3] = z[3] / 3 + (1000.0 if dtype == F32 else 64.0)  # shifted
    z[4, labels[4]] = -80.0                      # the label holds the minimum
    labels[5] = -100                             # ignored
    return z.to(dtype).float(), labels


def ce_reference(z, labels, ls, dt):
    zr = z.to(dt).requires_grad_(True)
    valid = labels != -100
    lsm = torch.log_softmax(zr, -1)
    lp = lsm.gather(1, labels.clamp(min=0)[:, None])[:, 0]
    rows = (1 - ls) * (-lp) + ls * (-lsm.mean(-1))
    loss = (rows * valid).sum() / max(int(valid.sum()), 1)
    (dz,) = torch.autograd.grad(2.5 * loss, zr)
    return loss.detach().reshape(1), (lp * valid).detach(), dz


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ls", [0.0, 0.1])
@pytest.mark.parametrize("V", [70, 257])
def test_cross_entropy_hard_rows(dev, dtype, ls, V):
    z, labels = ce_problem(V, dtype, seed=V)
    T = z.shape[0]
    loss64, lp64, dz64 = ce_reference(z, labels, ls, F64)
    loss32, lp32, dz32 = ce_reference(z, labels, ls, F32)
    headroom(loss32[None], loss64[None], F32, "ce loss", factor=5)
    headroom(lp32[:, None], lp64[:, None], F32, "ce log-probs", factor=5)
    headroom(dz32, dz64, dtype, "ce gradient")
    if ls == 0.0:
        assert float(lp64[0]) == 0.0 and float(lp32[0]) == 0.0  # the confident row sits exactly on the sentinel's edge
    zd = dv(z, dev, dtype).requires_grad_(True)
    loss, logp = ops.cross_entropy(zd, labels.to(dev), -100, ls)
    (2.5 * loss).backward()
    check(loss.reshape(1), loss64, F32, "ce loss", factor=5)
    check_units(logp[:, None], lp64[:, None], F32, "ce token log-probs", factor=5)
    check_units(zd.grad, dz64, dtype, "ce gradient")
    assert torch.equal(zd.grad[5].float().cpu(), torch.zeros(V)), "the ignored row has a gradient"
    # the kernel's own count of valid rows: the confident row (loss 0) is one of them
    k = ops.kernels()
    acc = torch.full((2,), float("nan"), dtype=F32, device=dev)
    k.cross_entropy_fwd(zd.detach(), labels.to(dev), torch.empty(T, device=dev), torch.empty(T, device=dev), acc, T, V, V, -100, ls)
    assert float(acc[1]) == 5.0, f"{float(acc[1])} valid rows counted, 5 expected"
    check((acc[0] / acc[1]).reshape(1), loss64, F32, "ce loss sum / count", factor=5)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_entropy_all_rows_ignored(dev, dtype):
    z, _ = ce_problem(70, dtype, seed=3)
    labels = torch.full((z.shape[0],), -100, dtype=torch.int64)
    zd = dv(z, dev, dtype).requires_grad_(True)
    loss, logp = ops.cross_entropy(zd, labels.to(dev), -100, 0.1)
    (2.5 * loss).backward()
    assert float(loss.detach()) == 0.0, f"loss {float(loss.detach())} of a batch without a valid row"
    assert torch.equal(logp.cpu(), torch.zeros(z.shape[0]))
    assert torch.equal(zd.grad.float().cpu(), torch.zeros_like(z)), "gradient of a batch without a valid row"


# ================================================================================================================
# 5. optimizer tail
# ================================================================================================================
HP = dict(lr=5e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.1)


def adamw_problem(n, step, seed):
    gen = torch.Generator().manual_seed(seed)
    p = (torch.rand(n, generator=gen) - 0.5) * 0.1                       # |p| <= 0.05
    sign = torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1
    g = sign * 10.0 ** torch.linspace(-6, 2, n)                          # 1e-6 .. 1e2 in one buffer
    g[n // 2] = 0.0
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:  # a state as earlier steps on gradients of this size leave it
        m = g * (torch.rand(n, generator=gen) - 0.3)
        v = g * g * (0.5 + torch.rand(n, generator=gen))
    return p, g, m, v


def adamw_reference(p, g, m, v, step, nsq, max_norm, dt):
    """(update p' - p, m', v') of one decoupled-weight-decay Adam step in `dt`; the clip as clip_grad_norm_ (+1e-6)"""
    p, g, m, v = (t.to(dt) for t in (p, g, m, v))
    lr, b1, b2, eps, wd = (torch.tensor(HP[x], dtype=F32).to(dt) for x in ("lr", "b1", "b2", "eps", "wd"))
    clip = torch.clamp(max_norm / (torch.tensor(nsq, dtype=F32).to(dt).sqrt() + 1e-6), max=1.0) if max_norm > 0 else 1.0
    gg = g * clip
    m2 = b1 * m + (1 - b1) * gg
    v2 = b2 * v + (1 - b2) * gg * gg
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p2 = p * (1 - lr * wd) - lr / bc1 * m2 / (v2.sqrt() / bc2.sqrt() + eps)
    return p2 - p, m2, v2


@pytest.mark.parametrize("entry", ["adamw", "adamw_step_dev", "adamw_lr", "adamw_window"])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("n", [5, 1027, 5000])
def test_adamw_update_and_moments(dev, entry, clip, step, n):
    p0, g, m0, v0 = adamw_problem(n, step, seed=n + step)
    nsq = float((g.double() ** 2).sum().float())
    max_norm = 0.1 if clip else 1e6  # |g|_2 > 1e2: 0.1 clips by ~1e-3 (eps then matters: sqrt(v) ~ 1e-9), 1e6 leaves g alone
    assert (math.sqrt(nsq) > max_norm) == clip
    ref64 = adamw_reference(p0, g, m0, v0, step, nsq, max_norm, F64)
    ref32 = adamw_reference(p0, g, m0, v0, step, nsq, max_norm, F32)
    for a, b, name in zip(ref32, ref64, ("update", "m", "v")):
        headroom(a[None], b[None], F32, f"adamw {name}")
    k = ops.kernels()
    p, gd, m, v = (dv(t, dev) for t in (p0, g, m0, v0))
    nd = torch.tensor([nsq], dtype=F32, device=dev)
    counters = torch.tensor([step - 1, 0], dtype=torch.int32, device=dev)
    lr_dev = torch.tensor([HP["lr"]], dtype=F32, device=dev)
    hp = (HP["b1"], HP["b2"], HP["eps"], HP["wd"])
    if entry == "adamw":
        k.adamw(p, gd, m, v, n, HP["lr"], *hp, step, nd, max_norm)
    elif entry == "adamw_step_dev":
        k.adamw(p, gd, m, v, n, HP["lr"], *hp, 1, nd, max_norm, step_dev=counters)
    elif entry == "adamw_lr":
        k.adamw_lr(p, gd, m, v, n, lr_dev, *hp, counters, nd, max_norm)
    else:  # the closing micro-step of a window of two
        k.adamw_window(p, gd, m, v, n, lr_dev, *hp, counters, nd, max_norm, torch.tensor([1], dtype=torch.int32, device=dev), 2)
    upd = p.double().cpu() - p0.double()
    what = f"{entry} n={n} step={step} clip={clip}"
    check(upd, ref64[0], F32, what + ": update")
    check(m, ref64[1], F32, what + ": m")
    check(v, ref64[2], F32, what + ": v")
    if step == 1:  # g = 0 from a zero state: the moments stay 0 and only the decay moves p
        assert float(m[n // 2]) == 0.0 and float(v[n // 2]) == 0.0


@pytest.mark.parametrize("n", [1, 255, 2 ** 20 + 3])
def test_sumsq_of_ones_is_exact(dev, n):
    """every partial sum is an integer below 2^24: whatever the summation order the result is n, unless an element is
    dropped or taken twice"""
    k = ops.kernels()
    x = torch.ones(n, dtype=F32, device=dev)
    out = torch.zeros(1, dtype=F32, device=dev)
    k.sumsq(x, n, out)
    assert float(out[0]) == float(n)
    for dtype in DTYPES:
        norm = torch.full((1,), float("nan"), dtype=F32, device=dev)
        xs, o = x.to(dtype), torch.full((n,), float("nan"), dtype=dtype, device=dev)
        k.grad_norm_scale(xs, o, n, norm, 3.0)
        want = math.sqrt(n)
        assert abs(float(norm[0]) - want) <= want * 2.0 ** -22, f"|ones({n})|_2 = {float(norm[0])}"
        check(o, torch.full((n,), 3.0 / want, dtype=F64), dtype, f"ones({n}) * 3 / norm")
        k.grad_norm_scale(xs, None, n, norm, 0.0)
        assert abs(float(norm[0]) - want) <= want * 2.0 ** -22


def test_sumsq_mixed_magnitudes(dev):
    k = ops.kernels()
    x = torch.full((5003,), 1e-3)
    x[[7, 2500, 5002]] = 1e3
    x64 = x.double()
    out = torch.zeros(1, dtype=F32, device=dev)
    k.sumsq(dv(x, dev), 5003, out)
    check(out, (x64 ** 2).sum().reshape(1), F32, "sumsq", factor=5)
    norm = torch.zeros(1, dtype=F32, device=dev)
    o = torch.empty(5003, dtype=F32, device=dev)
    k.grad_norm_scale(dv(x, dev), o, 5003, norm, 1e4)
    check(norm, x64.norm().reshape(1), F32, "norm", factor=5)
    big = x > 1
    ref = x64 * 1e4 / x64.norm()
    check(o.cpu()[big], ref[big], F32, "scaled gradient, large elements")
    check(o.cpu()[~big], ref[~big], F32, "scaled gradient, small elements")


@pytest.mark.parametrize("dtype", DTYPES)
def test_grad_norm_scale_of_a_zero_gradient(dev, dtype):
    """|g| = 0: the norm is 0 and the gradient stays 0 - not 0 * (target / 0) = NaN, which the step would hand on to every
    LoRA gradient behind it"""
    k = ops.kernels()
    n = 300
    gz = torch.zeros(n, dtype=dtype, device=dev)
    o = torch.full((n,), float("nan"), dtype=dtype, device=dev)
    norm = torch.full((1,), float("nan"), dtype=F32, device=dev)
    k.grad_norm_scale(gz, o, n, norm, 1e4)
    assert float(norm[0]) == 0.0
    assert torch.equal(o.float().cpu(), torch.zeros(n)), "a zero gradient did not stay zero"


# ================================================================================================================
# 6. BCE heads and activations
# ================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
def test_disc_head_saturated_logits(dev, dtype):
    bs, pps = 2, 8 * 8
    P = bs * pps
    w, b = torch.tensor([100.0, -100.0, 0.5, -0.25]), torch.tensor([0.0])
    rows = torch.tensor([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 0, 0], [0.5, 0.5, 1.0, 2.0], [0.01, 0, 1.0, 0], [1.0, 2.0, 0, 0]])
    x = rows[torch.arange(P) % 6].to(dtype).float()  # logits +100, -100, 0, 0, 1.5, -100 under both targets
    target = torch.tensor([0.0, 1.0])

    def reference(dt):
        xr, wr, br = (t.to(dt).requires_grad_(True) for t in (x, w, b))
        loss = F.binary_cross_entropy_with_logits(xr @ wr + br, target.to(dt).repeat_interleave(pps))
        (1.7 * loss).backward()
        return loss.detach().reshape(1), xr.grad, wr.grad, br.grad
    r64, r32 = reference(F64), reference(F32)
    for a, b_, dt, f, name in zip(r32, r64, (F32, dtype, F32, F32), (5, 1, 20, 20), ("loss", "dx", "dw", "db")):
        headroom(a[None], b_[None], dt, "bce " + name, factor=f)
    xd = dv(x, dev, dtype).requires_grad_(True)
    wd, bd = dv(w, dev).requires_grad_(True), dv(b, dev).requires_grad_(True)
    loss = ops.disc_head_loss(xd, wd, bd, dv(target, dev), pps)
    (1.7 * loss).backward()
    check(loss.reshape(1), r64[0], F32, "bce", factor=5)
    check(xd.grad, r64[1], dtype, "bce dx")
    check(wd.grad, r64[2], F32, "bce dw", factor=20)
    check(bd.grad, r64[3], F32, "bce db", factor=20)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 5, 6, 32), (2, 3, 1, 64)])
def test_disc_convhead_saturated_logits(dev, dtype, shape):
    """channels 0 and 1 are 1.0 at one corner pixel each and carry the weights +100 and -100 in every tap: the pixels whose 3x3
    window holds the corner have logits of +-100 (under both targets), the others stay near 0"""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(C)
    x = torch.zeros(B, H, W, C)
    x[0, 0, 0, 0] = x[1, H - 1, W - 1, 0] = 1.0      # +100 around a corner
    x[0, H - 1, W - 1, 1] = x[1, H // 2, W // 2, 1] = 1.0  # -100 around another pixel (not the mirror image: db must not cancel)
    x[..., 2:] = (torch.randn(B, H, W, C - 2, generator=g) * 0.5).to(dtype).float()
    w4 = torch.randn(1, C, 3, 3, generator=g) * 0.02
    w4[0, 0], w4[0, 1] = 100.0, -100.0
    b = torch.tensor([0.0])
    target = torch.tensor([0.0, 1.0])
    xt = x.reshape(B * H * W, C)

    def reference(dt):
        xr, wr, br = (t.to(dt).requires_grad_(True) for t in (xt, w4, b))
        z = F.conv2d(xr.reshape(B, H, W, C).permute(0, 3, 1, 2), wr, br, padding=1)
        loss = F.binary_cross_entropy_with_logits(z, target.to(dt).reshape(B, 1, 1, 1).expand(B, 1, H, W))
        (1.7 * loss).backward()
        return loss.detach().reshape(1), z.detach().reshape(-1), xr.grad, wr.grad, br.grad
    r64, r32 = reference(F64), reference(F32)
    assert float(r64[1].max()) > 99 and float(r64[1].min()) < -99 and float(r64[1].abs().min()) < 2
    for a, b_, dt, f, name in zip(r32, r64, (F32, F32, dtype, F32, F32), (5, 5, 1, 20, 20), ("loss", "z", "dx", "dw", "db")):
        headroom(a[None], b_[None], dt, "convhead " + name, factor=f)
    xd = dv(xt, dev, dtype).requires_grad_(True)
    wd, bd = dv(ops.conv_weight_to_taps(w4), dev).requires_grad_(True), dv(b, dev).requires_grad_(True)
    loss = ops.disc_convhead_loss(xd, wd, bd, dv(target, dev), B, H, W)
    z = loss.grad_fn.saved_tensors[2]
    (1.7 * loss).backward()
    check(loss.reshape(1), r64[0], F32, "convhead loss", factor=5)
    check(z, r64[1], F32, "convhead z", factor=5)
    check(xd.grad, r64[2], dtype, "convhead dx")
    check(ops.taps_to_conv_weight(wd.grad), r64[3], F32, "convhead dw", factor=20)
    check(bd.grad, r64[4], F32, "convhead db", factor=20)


ACT_POINTS = [0.0, 1e-6, 5.0, 20.0, 90.0, 1e4]


def assert_pointwise(got, ref64, ref32, dtype, what):
    """per element: |err| <= tol * max(1, |ref|), finite; the fp32 evaluation within a tenth of that"""
    got, ref64 = got.detach().double().cpu().reshape(-1), ref64.reshape(-1)
    lim = tol(dtype) * torch.clamp(ref64.abs(), min=1.0)
    e32 = (ref32.double().reshape(-1) - ref64).abs()
    assert bool((e32 <= lim / 10).all()), f"{what}: plain fp32 misses a tenth of the bound by {float((e32 / lim).max()):.2e}"
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    e = (got - ref64).abs()
    i = int((e / lim).argmax())
    assert bool((e <= lim).all()), f"{what}: element {i}: got {float(got[i])}, expected {float(ref64[i])}"


@pytest.mark.parametrize("dtype", DTYPES)
def test_activations_at_the_ends_of_their_range(dev, dtype):
    k = ops.kernels()
    pts = torch.tensor([s * v for v in ACT_POINTS for s in (1.0, -1.0)])  # +0 and -0 included
    x = pts.to(dtype).float()
    n = x.numel()
    gy = torch.linspace(-2, 2, n).to(dtype).float() + 0.25
    for name, op, fn in (("silu", ops.UN_SILU, F.silu), ("gelu", ops.UN_GELU, F.gelu)):
        def reference(dt):
            xr = x.to(dt).requires_grad_(True)
            y = fn(xr)
            (dx,) = torch.autograd.grad(y, xr, gy.to(dt))
            return y.detach(), dx
        r64, r32 = reference(F64), reference(F32)
        xd = dv(x, dev, dtype)
        y, dx = torch.full_like(xd, float("nan")), torch.full_like(xd, float("nan"))
        k.unary(op, xd, y, n)
        k.unary_bwd(op, dv(gy, dev, dtype), xd, dx, n)
        assert_pointwise(y, r64[0], r32[0], dtype, name)
        assert_pointwise(dx, r64[1], r32[1], dtype, name + " bwd")
    # geglu: every (value, gate) pair of the points
    D = n
    a, gate = x.reshape(n, 1).expand(n, D).clone(), x.reshape(1, D).expand(n, D)
    # (but 1e4 * gelu(-5): 1 + erf(-3.54) keeps ~3 digits in fp32 and the factor 1e4 lifts that above a tenth of the bound -
    # the precondition rules the pair out; the value becomes 90 there)
    a[(a.abs() == 1e4) & (gate == -5.0)] = 90.0
    xx = torch.cat([a, gate], 1).contiguous()
    gg = (torch.linspace(-1, 1, n * D).reshape(n, D) + 0.125).to(dtype).float()

    def reference(dt):
        xr = xx.to(dt).requires_grad_(True)
        y = xr[:, :D] * F.gelu(xr[:, D:])
        (dx,) = torch.autograd.grad(y, xr, gg.to(dt))
        return y.detach(), dx
    r64, r32 = reference(F64), reference(F32)
    xd = dv(xx, dev, dtype)
    y, dx = torch.full((n, D), float("nan"), dtype=dtype, device=dev), torch.full_like(xd, float("nan"))
    k.geglu_fwd(xd, y, n, D)
    k.geglu_bwd(dv(gg, dev, dtype), xd, dx, n, D)
    assert_pointwise(y, r64[0], r32[0], dtype, "geglu")
    assert_pointwise(dx, r64[1], r32[1], dtype, "geglu bwd")


# ================================================================================================================
# 2. fused attention on peaked and ordered scores
# ================================================================================================================
ATTN_GEOS = [(1, 70, 130, 2, 40), (1, 33, 577, 1, 64), (2, 16, 37, 2, 16), (1, 300, 77, 8, 80)]
FLASH_FWD_VARIANTS = [dict(flash_kt=1), dict(flash_kt=5), dict(flash_trim=0), dict(flash_xcd=0)]  # next to the defaults


def attn_problem(geo, dtype, case="ramp"):
    """q_i = b_i A u + noise, k_j = a_j u + noise with |u| = 1 and A = 25 sqrt(d): the scaled score of (i, j) is 25 b_i a_j plus
    noise of ~0.5.  ramp: a_j rises from -1 to 1, b_i from 0.5 to 1.  dominant: every a_j in [-1, -0.5] but one key at +1.
    mixed: the ramp with every other query scaled by 0.01 (a flat row next to a peaked one)."""
    B, Nq, Nk, H, d = geo
    u = torch.ones(d) / math.sqrt(d)
    b = torch.linspace(0.5, 1.0, Nq)
    a = torch.linspace(-1.0, 1.0, Nk)
    if case == "dominant":
        a = torch.linspace(-1.0, -0.5, Nk)
        a[Nk // 3] = 1.0
    q = (b * 25.0 * math.sqrt(d)).reshape(1, Nq, 1, 1) * u + 0.5 * rnd(B, Nq, H, d, seed=1)
    k = a.reshape(1, Nk, 1, 1) * u + 0.02 * rnd(B, Nk, H, d, seed=2)
    if case == "mixed":
        q[:, 1::2] *= 0.01
    v, go = rnd(B * Nk, H * d, dtype=dtype, seed=3), rnd(B * Nq, H * d, dtype=dtype, seed=4)
    return q.reshape(B * Nq, H * d).to(dtype).float(), k.reshape(B * Nk, H * d).to(dtype).float(), v, go


def attn_reference(q, k, v, go, geo, dt, causal=False, key_mask=None, gp=None):
    B, Nq, Nk, H, d = geo
    qr, kr, vr = (t.to(dt).requires_grad_(True) for t in (q, k, v))
    heads = lambda t, n: t.reshape(B, n, H, d).permute(0, 2, 1, 3)
    s = (heads(qr, Nq) @ heads(kr, Nk).transpose(-1, -2)) * torch.tensor(d ** -0.5, dtype=F32).to(dt)
    if causal:
        s = s.masked_fill(~torch.ones(Nq, Nk, dtype=torch.bool).tril(diagonal=Nk - Nq), float("-inf"))
    if key_mask is not None:
        s = s.masked_fill(~key_mask.bool()[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    o = (p @ heads(vr, Nk)).permute(0, 2, 1, 3).reshape(B * Nq, H * d)
    loss = (o * go.to(dt)).sum() + (0 if gp is None else (p * gp.to(dt)).sum())
    dq, dk, dvv = torch.autograd.grad(loss, (qr, kr, vr))
    return dict(O=o.detach(), lse=torch.logsumexp(s, -1).detach(), P=p.detach(), dQ=dq, dK=dk, dV=dvv)


ATTN_FACTOR = dict(O=1, P=1, dQ=3, dK=3, dV=3)


def lse_close(got, ref64, what):
    lim = tol(F32) * torch.clamp(ref64.abs(), min=1.0)
    e = (got.detach().double().cpu() - ref64).abs()
    assert bool((e <= lim).all()), f"{what}: log-sum-exp off by {float(e.max()):.2e} (limit {float(lim.min()):.2e} ..)"


def attn_headroom(r32, r64, dtype, names, what, units=None):
    for name in names:
        split = units if units is not None and name in ("O", "dQ") else (lambda t: [t])
        for a, b in zip(split(r32[name]), split(r64[name])):
            headroom(a[None], b[None], dtype, f"{what} {name}", factor=ATTN_FACTOR[name])
    e = (r32["lse"].double() - r64["lse"]).abs() / torch.clamp(r64["lse"].abs(), min=1.0)
    assert float(e.max()) < tol(F32) / 10, f"{what}: fp32 log-sum-exp {float(e.max()):.2e}"


def run_flash(q, k, v, go, geo, dev, dtype):
    B, Nq, Nk, H, d = geo
    qd, kd, vd = (dv(t, dev, dtype).requires_grad_(True) for t in (q, k, v))
    o, p = ops.attention(qd, kd, vd, B, Nq, Nk, H, d, need_probs=False)
    assert p is None
    o.backward(dv(go, dev, dtype))
    return dict(O=o.detach().float().cpu(), dQ=qd.grad.float().cpu(), dK=kd.grad.float().cpu(), dV=vd.grad.float().cpu())


def run_flash_fwd(q, k, v, geo, dev, dtype):
    B, Nq, Nk, H, d = geo
    HD = H * d
    qd, kd, vd = (dv(t, dev, dtype) for t in (q, k, v))
    o = torch.full_like(qd, float("nan"))
    lse = torch.full((B, H, Nq), float("nan"), dtype=F32, device=dev)
    ops.kernels().flash_attn_fwd(qd, kd, vd, o, lse, B, H, Nq, Nk, d, HD, HD, HD, HD, d ** -0.5)
    return o.float().cpu(), lse.cpu()


def permute_keys(t, perm, geo):
    B, _, Nk, H, d = geo
    return t.reshape(B, Nk, H * d)[:, perm].reshape(B * Nk, H * d)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geo", ATTN_GEOS)
def test_flash_attention_key_orders(dev, dtype, geo, default_opts):
    """ascending keys: the running maximum moves on every tile; descending: never after the first; shuffled.  One fp64
    reference (of the ascending order) serves all three: a permutation of the keys permutes dK and dV and nothing else."""
    B, Nq, Nk, H, d = geo
    q, k, v, go = attn_problem(geo, dtype)
    r64, r32 = attn_reference(q, k, v, go, geo, F64), attn_reference(q, k, v, go, geo, F32)
    assert float(r64["lse"].max()) > 25 and float(r64["lse"].max() - r64["lse"].min()) > 10  # top scores ~ 25 b_i, b_i from 0.5 to 1
    attn_headroom(r32, r64, dtype, ("O", "dQ", "dK", "dV"), f"attention {geo}")
    orders = dict(ascending=torch.arange(Nk), descending=torch.arange(Nk).flip(0),
                  shuffled=torch.randperm(Nk, generator=torch.Generator().manual_seed(Nk)))
    res = {}
    for name, perm in orders.items():
        inv = torch.argsort(perm)
        kp, vp = permute_keys(k, perm, geo), permute_keys(v, perm, geo)
        got = run_flash(q, kp, vp, go, geo, dev, dtype)
        got["dK"], got["dV"] = permute_keys(got["dK"], inv, geo), permute_keys(got["dV"], inv, geo)
        for x in ("O", "dQ", "dK", "dV"):
            check(got[x], r64[x], dtype, f"flash {geo} keys {name}: {x}", factor=ATTN_FACTOR[x])
        variants = [{}] + (FLASH_FWD_VARIANTS if dev.type == "cuda" else [])
        for opts in variants:
            _set_opts(**opts)
            o, lse = run_flash_fwd(q, kp, vp, geo, dev, dtype)
            check(o, r64["O"], dtype, f"flash fwd {geo} keys {name} {opts}: O")
            lse_close(lse, r64["lse"], f"flash fwd {geo} keys {name} {opts}")
            if opts:
                restore_default_opts()
        res[name] = got
    for other in ("descending", "shuffled"):
        for x in ("O", "dQ", "dK", "dV"):
            check(res[other][x], res["ascending"][x], dtype, f"flash {geo}: {x} with {other} keys against ascending keys",
                  factor=ATTN_FACTOR[x])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["dominant", "mixed"])
@pytest.mark.parametrize("geo", ATTN_GEOS)
def test_flash_attention_peaked_rows(dev, dtype, geo, case):
    B, Nq, Nk, H, d = geo
    q, k, v, go = attn_problem(geo, dtype, case)
    r64, r32 = attn_reference(q, k, v, go, geo, F64), attn_reference(q, k, v, go, geo, F32)
    pmax = r64["P"].amax(-1)  # [B, H, Nq]
    units, names = None, ("O", "dQ", "dK", "dV")
    if case == "dominant":
        # dS = P (dP - D) of a row with p_max -> 1 is a difference of nearly equal numbers: against their own (vanishing) maximum
        # plain fp32 leaves dQ and dK 3e-4 .. 5e-2 from fp64 at p_max > 0.999, so the precondition admits O, dV and the
        # log-sum-exp only; dQ and dK must be finite
        assert float(pmax.min()) > 0.999
        names = ("O", "dV")
    else:  # flat rows (the scaled-down queries) and peaked rows are two units: their dQ differ in scale
        assert float(pmax[..., 0::2].min()) > 10 * float(pmax[..., 1::2].max())
        units = lambda t: [t.reshape(B, Nq, H * d)[:, 0::2], t.reshape(B, Nq, H * d)[:, 1::2]]
    attn_headroom(r32, r64, dtype, names, f"attention {geo} {case}", units)
    got = run_flash(q, k, v, go, geo, dev, dtype)
    assert all(bool(torch.isfinite(t).all()) for t in got.values()), f"flash {geo} {case}: non-finite values"
    for x in names:
        split = units if units is not None and x in ("O", "dQ") else (lambda t: [t])
        for u, (a, b) in enumerate(zip(split(got[x]), split(r64[x]))):
            check(a, b, dtype, f"flash {geo} {case}: {x} [unit {u}]", factor=ATTN_FACTOR[x])
    o, lse = run_flash_fwd(q, k, v, geo, dev, dtype)
    check(o, r64["O"], dtype, f"flash fwd {geo} {case}: O")
    lse_close(lse, r64["lse"], f"flash fwd {geo} {case}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("masking", ["causal", "key_mask"])
@pytest.mark.parametrize("geo", [(1, 70, 130, 2, 40), (2, 16, 37, 2, 16)])
def test_unfused_attention_peaked_scores(dev, dtype, geo, masking):
    """the materialised path (softmax kernel between two GEMMs) on the ramp scores, under a causal mask and under a key
    mask that hides the highest-scoring keys of one sample"""
    B, Nq, Nk, H, d = geo
    q, k, v, go = attn_problem(geo, dtype)
    gp = rnd(B, H, Nq, Nk, dtype=dtype, seed=5) * 0.1
    km = None
    if masking == "key_mask":
        km = torch.ones(B, Nk, dtype=torch.int8)
        km[0, Nk - 5:] = 0
        km[B - 1, Nk // 2] = 0
    kw = dict(causal=masking == "causal", key_mask=km)
    r64, r32 = attn_reference(q, k, v, go, geo, F64, gp=gp, **kw), attn_reference(q, k, v, go, geo, F32, gp=gp, **kw)
    rows = lambda t: t.reshape(B * H * Nq, Nk)
    attn_headroom(r32, r64, dtype, ("O", "dQ", "dK", "dV"), f"attention {geo} {masking}")
    headroom(rows(r32["P"]), rows(r64["P"]), dtype, "attention probabilities")
    qd, kd, vd = (dv(t, dev, dtype).requires_grad_(True) for t in (q, k, v))
    o, p = ops.attention(qd, kd, vd, B, Nq, Nk, H, d, causal=kw["causal"], key_mask=None if km is None else km.to(dev))
    ((o.float() * dv(go, dev)).sum() + (p.float() * dv(gp, dev)).sum()).backward()
    check(o, r64["O"], dtype, f"attention {masking}: O")
    check_units(rows(p), rows(r64["P"]), dtype, f"attention {masking}: P")
    assert torch.allclose(p.float().sum(-1).cpu(), torch.ones(B, H, Nq), atol=2e-2 if dtype == BF16 else 1e-5)
    check(qd.grad, r64["dQ"], dtype, f"attention {masking}: dQ", factor=3)
    check(kd.grad, r64["dK"], dtype, f"attention {masking}: dK", factor=3)
    check(vd.grad, r64["dV"], dtype, f"attention {masking}: dV", factor=3)
