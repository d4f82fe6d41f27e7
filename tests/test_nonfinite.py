"""NaN and Inf: what a kernel does with a non-finite INPUT.  The optimizer tail skips an update whose gradient norm is not
finite (comat_sumsq -> comat_adamw*), and the step tests plant their Inf in the flat gradient itself.  That protection is worth
what the kernels in front of the gradient buffer carry: a NaN that a reduction drops, a clamp that turns it into a finite byte,
a guard that sends it to the "empty row" branch - each leaves a finite loss, a finite norm and an applied update.  Here one
non-finite value is planted in an operand and four rules are applied to the result.

The reference is always the plain torch fp64 evaluation (fp32 where torch has no fp64 kernel) of the operation's definition on
the dtype-rounded, poisoned inputs.

1. CARRY.  An output element whose reference is non-finite is non-finite in the kernel.  Only finiteness is compared (NaN against
   Inf is not).  An e4m3 output holds the byte 0x7F or 0xFF there, never a finite code; a scale or abs-max word derived from a
   poisoned tensor is non-finite.
2. CONTAIN.  An output element whose reference is finite is finite and within the bound of the sibling test of test_ops.py
   (`check(..., dtype, factor)` with the factor test_windows.py uses for the quantity), evaluated over the finite elements only.
   Integer-operand products (helpers.ints) are bit-equal there (`assert_exact`).  Units: a LayerNorm row, a GroupNorm (sample,
   group), a softmax row, an attention (batch, head) and query row, a GEMM row / column, a cross-entropy row, a
   comat_weights_refresh_q8 slot.
3. EXCLUDED MEANS UNREAD.  Where the header excludes an element - a key under `key_mask` or the causal mask, a row with
   `ignore_index`, R when beta == 0, a site that saw no tensor - its value does not matter: a NaN there gives the bits of the
   call with a 0 there.
4. NO RESIDUE.  After a poisoned call, the same call with clean inputs on the same backend instance (the same per-stream
   workspaces, tickets, partial slabs) gives exactly the bits of the clean call made before the poison.

Plants: one NaN, one +Inf, one -Inf, as separate runs and one plant per run, so that the dependent set is known: it is asserted
on the CPU reference (`depends`) before a kernel is compared, and the clean call is held to the sibling bound first - a case
that fails there is a broken case, not a finding.  Positions: the first element, the last element of the vectorised body, an
element of the scalar tail / k-tail / last ragged tile.  Softmax scores get a -Inf only where the row keeps a finite score (a
row of -Inf only is the masked row of test_value_ranges.py, section 3).  Shapes are the smallest of test_windows.py's lists
that reach each path.

Sections: A fp8 quantisers (flat, LayerNorm / GroupNorm / attention / GEGLU producers, comat_weights_refresh_q8), B the two
delayed-scaling updates (a site whose abs-max is non-finite is treated as having seen no tensor), C products - one case per
kernel family comat_last_gemm_kernel names (0 general, 1 pipelined, 2 k-major, 3 fp8, 4 grouped k-major, 5 lean, 6 / 7 the
two weight-gradient paths), comat_gemm_segments, comat_lora_merge, comat_conv2d forward and data-gradient, split-K forced with
g2_splits and with force_splits, D softmax, fused attention (every option set of test_exact_attention.py on the library leg)
and cross entropy, E norms (every norm_fused mode on the library leg), their affine gradients and the column reductions,
F sumsq, the gradient norm, the elementwise kernels, GEGLU, the sampler's kernels, the image path and the loss heads, G the step.
Rule 3 has a case for: a masked softmax key, an ignored cross-entropy row, R with beta == 0 (comat_gemm on four families,
comat_gemm_segments, comat_conv2d), a tap outside the image (NaN halos round the image), a resample window position of weight
0 and a pixel outside the crop, a pad column of comat_colsum, an embedding row and an attention-map column that no index
names, a slot -1 problem of comat_weights_refresh_q8, a site that saw no tensor, eps and stats of comat_ddpm_step2_bwd
without deps.

Found by these tests and fixed with them - each case named failed on the library built from the parent commit:
  * rule 1, abs-max: fp8_scale_kernel, fp8_quantize_scaled_kernel (fp8.hip), the tile pass of comat_weights_refresh_q8
    (refresh.hip), the _q epilogues of GroupNorm and LayerNorm (norm.hip), of the fused attention (attention.hip) and of the GEGLU
    product (gemm_shared.h): `fmaxf(m, |v|)` drops a NaN operand, and `fmaxf(amax, 2^-100) / 448` drops a NaN maximum - the
    site's word and scale were those of the tensor without its NaN;
  * rule 1, bytes: fp8_sat (common.h) - v_med3_f32 answers a NaN with -448, the finite byte 0xFE - in every quantiser above;
  * contract B: fp8_scales_update_kernel and fp8_scales_update_hist_kernel turned an Inf abs-max into scale = inf (for up to
    hist_len steps) and would have kept a NaN in the history for good; the simulator did the same;
  * rule 1: softmax_fwd_kernel (`sum > 0 ? 1 / sum : 0` sends a NaN row sum to the empty-row branch: every probability of the row
    but the planted one came out 0; the simulator's nan_to_num zeroed all of them), gnorm_scale_kernel of comat_grad_norm_scale
    (`norm > 0 ? target / norm : 0`: a NaN gradient left as zeros next to one NaN) and ce_final_kernel of
    comat_cross_entropy_fwd (`row_loss >= 0` skipped a valid row whose loss is NaN: a finite loss over one row fewer);
  * rule 3: every product epilogue added beta * R with beta == 0 (0 * NaN): the residual pointer now reaches no kernel then.
The simulator followed the kernels where it differed: a masked key weighs 0 in a poisoned softmax row, the log-sum-exp of the
fused attention and of the cross entropy is m + log(sum exp(s - m)) (NaN, not +Inf, on a +Inf score), an ignored row's gradient
is 0 and not 0 * NaN, a resample window position of weight 0 is skipped.
  * the step (section G): losses.grounding_loss_by_layer called torch's binary_cross_entropy, which checks 0 <= p <= 1 - a
    RuntimeError on the CPU, a device-side assertion on the GPU - so a step with a NaN in it died before it reached the
    optimizer's skip: spelled out in operators that carry the NaN.  And a skipped step still advanced the scale, history and count
    of the fp8 sites in FRONT of the NaN (the text projections of the prompt): fp8_end_of_step(gnorm_sq) now clears every
    running maximum on the device when the gradient norm is not finite.
    A site without a scale that met a NaN in its first step kept a NaN scale for good: a skipped step now leaves such a site its
    maximum, and the next finite one replaces the scale.
No kernel of section F's second half failed.  Of the further product families one thing showed: the pipelined path of
comat_conv2d_wgrad forms the product of a non-finite dY element with the zero page of a padding tap (0 * NaN), the general
path does not; torch's own conv2d_weight does either, by algorithm - the header now leaves those taps open (test_conv2d_wgrad).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from comat_amd import ops
from helpers import Window, _set_opts, assert_exact, default_opts, ints  # noqa: F401 - default_opts is a fixture
from oracle import fp8 as OF
from test_ops import check, rnd, tol  # noqa: F401 - tol: the bound `check` applies

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DTYPES = [F32, BF16]
NAN, INF = float("nan"), float("inf")
PLANTS = {"nan": NAN, "+inf": INF, "-inf": -INF}
plants = pytest.mark.parametrize("plant", list(PLANTS))
dtypes = pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


# ---- the four rules -----------------------------------------------------------------------------------------------------------
def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(_INT[t.element_size()]) if t.dtype.is_floating_point else t


def same_bits(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, (what, tuple(a.shape), tuple(b.shape))
    n = int((a != b).sum())
    assert n == 0, f"{what}: {n} of {a.numel()} elements differ in their bits"


def nonfinite(t):
    return ~torch.isfinite(t.detach().float().cpu())


def put(x, value, *idx):
    """a copy of x with `value` at idx"""
    x = x.clone()
    x[idx] = value
    return x


def depends(ref64, expected, what):
    """CPU precondition: the reference is non-finite exactly on `expected` (bool mask, or None: nowhere)"""
    nf = ~torch.isfinite(ref64)
    if expected is None:
        assert not bool(nf.any()), f"{what}: the clean reference is not finite - a broken case"
    else:
        expected = expected.expand_as(nf)
        assert torch.equal(nf, expected), (f"{what}: the reference's non-finite set ({int(nf.sum())} elements) is not the "
                                           f"dependent set the case states ({int(expected.sum())}) - a broken case")


def carried_contained(got, ref64, dtype, what, factor=1.0, exact_dtype=None):
    """rules 1 and 2 of one output against its fp64 reference; exact_dtype: bit-equal (integer operands) instead of the bound"""
    got = got.detach().cpu()
    assert got.shape == ref64.shape, (what, tuple(got.shape), tuple(ref64.shape))
    nf, g_nf = ~torch.isfinite(ref64), nonfinite(got)
    lost = nf & ~g_nf
    assert not bool(lost.any()), (f"{what}: rule 1 - {int(lost.sum())} of {int(nf.sum())} elements whose reference is non-finite are "
                                  f"finite, first at {tuple(torch.nonzero(lost)[0].tolist())}: {float(got[lost][0])!r}")
    leak = g_nf & ~nf
    assert not bool(leak.any()), (f"{what}: rule 2 - {int(leak.sum())} elements whose reference is finite are not, first at "
                                  f"{tuple(torch.nonzero(leak)[0].tolist())}")
    if bool((~nf).any()):
        if exact_dtype is not None:
            assert_exact(got[~nf], ref64[~nf], exact_dtype, what + " (finite elements)")
        else:
            check(got.float()[~nf], ref64[~nf], dtype, what + " (finite elements)", factor)


def nan_byte(q):
    return (q.cpu() & 0x7F) == 0x7F


def bytes_follow(got_q, want_q, what):
    """e4m3 bytes against the oracle's: a NaN byte where the oracle has one (rule 1), its bits everywhere else (rule 2)"""
    got_q, want_q = got_q.cpu(), want_q.cpu()
    assert got_q.shape == want_q.shape, (what, tuple(got_q.shape), tuple(want_q.shape))
    nf = nan_byte(want_q)
    lost = nf & ~nan_byte(got_q)
    assert not bool(lost.any()), (f"{what}: rule 1 - {int(lost.sum())} of {int(nf.sum())} bytes that must be NaN (0x7F / 0xFF) are finite "
                                  f"codes, first 0x{int(got_q[lost][0]):02X}")
    bad = (got_q != want_q) & ~nf
    assert not bool(bad.any()), f"{what}: rule 2 - {int(bad.sum())} of {int((~nf).sum())} finite bytes differ from the oracle's"


def word_nonfinite(w, what):
    assert not bool(torch.isfinite(bits(w).view(F32)).any()), f"{what}: rule 1 - the word {bits(w).view(F32).tolist()} is finite"


def drive(call, ref, clean, poisoned, dep, dtype, what, factors=None, exact=None):
    """The common course of a case.  call(inputs) -> {name: output tensor}; ref(inputs) -> {name: fp64 reference}; `dep`:
    {name: bool mask of the reference's non-finite set under the plant}.  Clean call (sibling bound), poisoned call (rules 1
    and 2), clean call again (rule 4) -> the poisoned call's outputs."""
    factors, exact = factors or {}, exact or {}
    r0, r1 = ref(clean), ref(poisoned)
    for name in r0:
        depends(r0[name], None, f"{what}: {name}")
        depends(r1[name], dep[name], f"{what}: {name}")
    o0 = call(clean)
    for name in r0:
        carried_contained(o0[name], r0[name], dtype, f"{what}: clean {name}", factors.get(name, 1.0), exact.get(name))
    o1 = call(poisoned)
    for name in r0:
        carried_contained(o1[name], r1[name], dtype, f"{what}: {name}", factors.get(name, 1.0), exact.get(name))
    o2 = call(clean)
    for name in o0:
        same_bits(o2[name], o0[name], f"{what}: rule 4 - {name} of a clean call after the poisoned one")
    return o1


def dv(x, dev, dtype=None):
    return x.detach().to(device=dev, dtype=dtype or x.dtype).contiguous().clone()


def zero_word(dev):
    return torch.zeros(1, dtype=torch.int32, device=dev)


def row_mask(shape, *idx):
    m = torch.zeros(shape, dtype=torch.bool)
    m[idx] = True
    return m


# ================================================================================================================
# A. fp8 quantisers
# ================================================================================================================
def flat_positions(n):
    """first element, last element of the 8-wide body, last element of the scalar tail"""
    pos = [0, n // 8 * 8 - 1] + ([n - 1] if n % 8 else [])
    return sorted(set(pos))


FLAT = [(n, p) for n in (8, 13, 4099) for p in flat_positions(n)]
flat = pytest.mark.parametrize("n,pos", FLAT, ids=[f"n{n}-at{p}" for n, p in FLAT])


@plants
@flat
@dtypes
def test_jit_quantiser(dev, dtype, n, pos, plant):
    """comat_fp8_scale + comat_fp8_quantize: a NaN gives a NaN scale and NaN bytes throughout; an Inf gives scale = inf, the
    planted byte NaN (inf * 0) and every other byte 0 - the oracle, bit for bit; the calibration word carries the plant"""
    k = ops.kernels()
    x0 = (rnd(n, seed=n) * 3).to(dtype)
    x1 = put(x0, PLANTS[plant], pos)
    q_ref, s_ref = OF.quantize(x1)
    assert not bool(torch.isfinite(s_ref)) and bool(nan_byte(q_ref)[pos])  # CPU precondition: what the oracle does today
    assert bool(nan_byte(q_ref).all()) if plant == "nan" else int(nan_byte(q_ref).sum()) == 1 and int((put(q_ref, 0, pos) & 0x7F).sum()) == 0

    def call(x):
        amax = zero_word(dev)
        q, s = k.fp8_quantize(dv(x, dev), amax=amax)
        return dict(q=q.cpu(), scale=s.cpu(), amax=amax.cpu())
    o0 = call(x0)
    q0, s0 = OF.quantize(x0)
    assert torch.equal(o0["q"], q0) and torch.equal(bits(o0["scale"].reshape(())), bits(s0)), "the clean call differs from the oracle"
    o1 = call(x1)
    what = f"fp8_quantize n={n} {plant} at {pos}"
    word_nonfinite(o1["scale"], what + ": scale")
    word_nonfinite(o1["amax"], what + ": abs-max word")
    bytes_follow(o1["q"], q_ref, what)
    o2 = call(x0)
    for name in o0:
        same_bits(o2[name], o0[name], f"{what}: rule 4 - {name}")


@plants
@flat
@dtypes
def test_scaled_quantiser(dev, dtype, n, pos, plant):
    """comat_fp8_quantize_scaled under a finite scale that saturates the tensor's tail: +-Inf saturate like every value beyond
    448 * scale, a NaN is the NaN byte; every other byte is the clean call's; the site's running maximum carries the plant and
    the scale word is not written"""
    k = ops.kernels()
    x0 = (rnd(n, seed=n) * 3).to(dtype)
    x1 = put(x0, PLANTS[plant], pos)
    s = OF.scale_of(x0) * 0.37
    q_ref = OF.quantize_with_scale(x1, s)
    assert bool(nan_byte(q_ref)[pos]) == (plant == "nan") and int(nan_byte(q_ref).sum()) == int(plant == "nan")
    assert torch.equal(put(q_ref, 0, pos), put(OF.quantize_with_scale(x0, s), 0, pos))

    def call(x):
        scale, amax = s.reshape(1).to(dev), zero_word(dev)
        q = k.fp8_quantize_scaled(dv(x, dev), scale, amax)
        return dict(q=q.cpu(), scale=scale.cpu(), amax=amax.cpu())
    o0 = call(x0)
    assert torch.equal(o0["q"], OF.quantize_with_scale(x0, s)), "the clean call differs from the oracle"
    o1 = call(x1)
    what = f"fp8_quantize_scaled n={n} {plant} at {pos}"
    bytes_follow(o1["q"], q_ref, what)
    word_nonfinite(o1["amax"], what + ": abs-max word")
    same_bits(o1["scale"], o0["scale"], what + ": the scale word")
    o2 = call(x0)
    for name in o0:
        same_bits(o2[name], o0[name], f"{what}: rule 4 - {name}")


def _producer(dev, what, y_ref, y_dep, dtype, call, x0, x1, factor=1.0, untouched=None):
    """a kernel that emits the e4m3 bytes of its own output: y by rules 1 and 2 against fp64, the bytes against the oracle's
    quantiser on the kernel's own y (as the sibling tests of test_fp8.py do), the site's word non-finite, the scale word kept;
    `untouched`: the elements whose bytes are those of the clean call (default: everything outside the dependent set)"""
    r0, r1 = y_ref(x0), y_ref(x1)
    depends(r0, None, what)
    depends(r1, y_dep, what)
    o0 = call(x0)
    carried_contained(o0["y"], r0, dtype, what + ": clean y", factor)
    assert torch.equal(o0["q"], OF.quantize_with_scale(o0["y"], o0["scale"][0])), what + ": clean bytes differ from the oracle's"
    o1 = call(x1)
    carried_contained(o1["y"], r1, dtype, what + ": y", factor)
    bytes_follow(o1["q"], OF.quantize_with_scale(o1["y"], o0["scale"][0]), what + ": bytes")
    keep = ~y_dep.expand_as(r1) if untouched is None else untouched
    same_bits(o1["q"][keep], o0["q"][keep], what + ": rule 2 - bytes outside the poisoned unit")
    word_nonfinite(o1["amax"], what + ": abs-max word")
    same_bits(o1["scale"], o0["scale"], what + ": the scale word")
    o2 = call(x0)
    for name in o0:
        same_bits(o2[name], o0[name], f"{what}: rule 4 - {name}")
    return o0, o1


@plants
@dtypes
@pytest.mark.parametrize("at", ["first", "last"])
def test_layernorm_producer(dev, dtype, at, plant):
    """comat_layernorm_fwd_q: the poisoned row's y, statistics and bytes are non-finite, every other row keeps its bytes"""
    k = ops.kernels()
    M, C = 37, 64
    x0 = rnd(M, C, dtype=dtype, seed=1) * 1.5 - 0.4
    gamma, beta = rnd(C, seed=2) * 0.5 + 1, rnd(C, seed=3) * 0.3
    r, c = (0, 0) if at == "first" else (M - 1, C - 1)
    x1 = put(x0, PLANTS[plant], r, c)
    y_ref = lambda x: F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), eps=1e-5)
    s = (OF.scale_of(y_ref(x0)) * 0.8).reshape(1)

    def call(x):
        xd = dv(x, dev, dtype)
        assert k.layernorm_fwd_q_ok(xd)
        y, st = torch.empty_like(xd), torch.empty((M, 2), device=dev)
        q8, scale, amax = torch.empty((M, C), dtype=torch.uint8, device=dev), s.to(dev), zero_word(dev)
        k.layernorm_fwd_q(xd, dv(gamma, dev), dv(beta, dev), y, st, M, C, 1e-5, q8, scale, amax)
        return dict(y=y.cpu(), stats=st.cpu(), q=q8.cpu(), scale=scale.cpu(), amax=amax.cpu())
    o0, o1 = _producer(dev, f"layernorm_fwd_q {plant} at {(r, c)}", y_ref, row_mask((M, 1), r), dtype, call, x0, x1)
    rows = row_mask((M,), r)
    assert bool(nonfinite(o1["stats"])[rows].any()), "rule 1: the poisoned row's statistics are finite"
    same_bits(o1["stats"][~rows], o0["stats"][~rows], "rule 2: statistics of the other rows")


@plants
@dtypes
@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_producer(dev, dtype, silu, plant):
    """comat_groupnorm_fwd_q: one (sample, group) is poisoned"""
    k = ops.kernels()
    B_, HW, C, G = 2, 300, 32, 8
    x0 = rnd(B_, HW, C, dtype=dtype, seed=1) * 2 + 0.7
    gamma, beta = rnd(C, seed=2) * 0.5 + 1, rnd(C, seed=3) * 0.3
    b, p, c = 1, HW - 1, C - 1
    x1 = put(x0, PLANTS[plant], b, p, c)

    def y_ref(x):
        y = F.group_norm(x.double().permute(0, 2, 1), G, gamma.double(), beta.double(), eps=1e-5).permute(0, 2, 1)
        return (F.silu(y) if silu else y).reshape(B_ * HW, C)
    s = (OF.scale_of(y_ref(x0)) * 0.8).reshape(1)
    unit = torch.zeros(B_, HW, G, C // G, dtype=torch.bool)
    unit[b, :, c // (C // G)] = True

    def call(x):
        xd = dv(x.reshape(B_ * HW, C), dev, dtype)
        assert k.groupnorm_fwd_q_ok(xd, B_, HW, C, G)
        y, st = torch.empty_like(xd), torch.empty((B_, G, 2), device=dev)
        q8, scale, amax = torch.empty(xd.shape, dtype=torch.uint8, device=dev), s.to(dev), zero_word(dev)
        k.groupnorm_fwd_q(xd, dv(gamma, dev), dv(beta, dev), y, st, B_, HW, C, G, 1e-5, silu, q8, scale, amax)
        return dict(y=y.cpu(), stats=st.cpu(), q=q8.cpu(), scale=scale.cpu(), amax=amax.cpu())
    o0, o1 = _producer(dev, f"groupnorm_fwd_q silu={silu} {plant}", y_ref, unit.reshape(B_ * HW, C), dtype, call, x0, x1)
    g = row_mask((B_, G), b, c // (C // G))
    assert bool(nonfinite(o1["stats"])[g].any()), "rule 1: the poisoned group's statistics are finite"
    same_bits(o1["stats"][~g], o0["stats"][~g], "rule 2: statistics of the other groups")


def _attn_ref(q, kk, v, B_, H, Nq, Nk, d, scale):
    """fp64 O [B * Nq, H * d] and lse [B, H, Nq] of operands stored [B * N, H * d]"""
    heads = lambda t, n: t.double().reshape(B_, n, H, d).permute(0, 2, 1, 3)
    s = heads(q, Nq) @ heads(kk, Nk).transpose(-1, -2) * scale
    o = torch.softmax(s, -1) @ heads(v, Nk)
    return o.permute(0, 2, 1, 3).reshape(B_ * Nq, H * d), torch.logsumexp(s, -1)


def _head_rows(B_, H, N, d, b, h, row=None):
    """mask [B * N, H * d] of the head-h columns of sample b (of one row of it)"""
    m = torch.zeros(B_, N, H, d, dtype=torch.bool)
    if row is None:
        m[b, :, h] = True
    else:
        m[b, row, h] = True
    return m.reshape(B_ * N, H * d)


@plants
@pytest.mark.parametrize("where", ["q", "k"])
def test_attention_producer(dev, where, plant):
    """comat_flash_attn_fwd_q: a plant in one query row poisons that row of its head, one in a key the queries of its (batch,
    head) that give it a score of NaN or +Inf"""
    k = ops.kernels()
    B_, H, Nq, Nk, d = 1, 8, 130, 77, 64
    HD, T = H * d, BF16
    q0, k0, v0 = (rnd(B_ * n_, HD, dtype=T, seed=s_) for n_, s_ in ((Nq, 1), (Nk, 2), (Nk, 3)))
    h = H - 1
    if where == "q":
        x0, x1 = (q0, k0, v0), (put(q0, PLANTS[plant], Nq - 1, h * d + d - 1), k0, v0)
        unit = _head_rows(B_, H, Nq, d, 0, h, Nq - 1)
    else:
        x0, x1 = (q0, k0, v0), (q0, put(k0, PLANTS[plant], Nk - 1, h * d), v0)
        # the key's score is q_i[c] * plant: NaN poisons every query of the head; +-Inf those whose product is +Inf (or 0 * Inf) -
        # where it is -Inf the key has weight 0 and the row keeps its finite scores
        hit = torch.ones(Nq, dtype=torch.bool) if plant == "nan" else ~(q0[:, h * d] * PLANTS[plant] == -INF)
        assert 0 < int(hit.sum()) and (plant == "nan" or int(hit.sum()) < Nq)
        unit = _head_rows(B_, H, Nq, d, 0, h) & hit[:, None]
    y_ref = lambda x: _attn_ref(*x, B_, H, Nq, Nk, d, d ** -0.5)[0]
    s = (OF.scale_of(y_ref(x0)) * 0.7).reshape(1)

    def call(x):
        qd, kd, vd = (dv(t, dev, T) for t in x)
        o, lse = torch.empty_like(qd), torch.empty(B_, H, Nq, device=dev)
        q8, scale, amax = torch.empty((B_ * Nq, HD), dtype=torch.uint8, device=dev), s.to(dev), zero_word(dev)
        k.flash_attn_fwd(qd, kd, vd, o, lse, B_, H, Nq, Nk, d, HD, HD, HD, HD, d ** -0.5, q8=(q8, scale, amax))
        return dict(y=o.cpu(), lse=lse.cpu(), q=q8.cpu(), scale=scale.cpu(), amax=amax.cpu())
    _producer(dev, f"flash_attn_fwd_q {plant} in {where}", y_ref, unit, T, call, x0, x1, untouched=~_head_rows(B_, H, Nq, d, 0, h))


@plants
@pytest.mark.parametrize("keep", [True, False], ids=["epi2=1", "epi2=2"])
def test_geglu_producer(dev, keep, plant, default_opts):
    """the GEGLU epilogue's q8 output (comat_gemm_params::epi2 1 / 2 with q8): integer operands, a plant in the k-tail of one
    row of A - that row of the product, of its bytes and the site's word carry it, every other row is the clean call's"""
    k = ops.kernels()
    if dev.type == "cuda":
        _set_opts(gemm2=1, gemm3=0, g2_cfg=0, g2_splits=0)
    M, N, K = 37, 64, 64
    D = N // 2
    x0, w, b = ints(M, K, seed=1, hi=4), ints(N, K, seed=2, hi=2) / 64, ints(N, seed=3, hi=2) / 8
    r = M - 1
    x1 = put(x0, PLANTS[plant], r, K - 1)

    def y_ref(x):
        pre = (x.double() @ w.double().t() + b.double()).float().to(BF16).double()  # both halves rounded first
        t = pre.reshape(M, N // 32, 2, 16)
        return (t[:, :, 0] * F.gelu(t[:, :, 1])).reshape(M, D)
    s = (OF.scale_of(y_ref(x0).float().to(BF16)) * 0.8).reshape(1)

    def call(x):
        xd, wd, bd = dv(x, dev, BF16), dv(w, dev, BF16), dv(b, dev)
        pre = torch.empty((M, N), dtype=BF16, device=dev) if keep else None
        y, q8 = torch.empty((M, D), dtype=BF16, device=dev), torch.empty((M, D), dtype=torch.uint8, device=dev)
        scale, amax = s.to(dev), zero_word(dev)
        k.gemm(xd, wd, pre, M, N, K, K, K, N, bias=bd, geglu=(y, keep), q8=(q8, scale, amax))
        return dict(y=y.cpu(), q=q8.cpu(), scale=scale.cpu(), amax=amax.cpu())
    _producer(dev, f"geglu epilogue keep_pre={keep} {plant}", y_ref, row_mask((M, 1), r), BF16, call, x0, x1)


@plants
@dtypes
@pytest.mark.parametrize("layer", [("lin", 65, 63), ("conv", 32, 3, 96)], ids=["lin65x63", "conv32x3x96"])
def test_refresh_q8_slot(dev, dtype, layer, plant):
    """comat_weights_refresh_q8: a plant in the last element of one slot's master (the last ragged tile; the last tap's second
    column tile) - that slot's scale and bytes are the oracle's (non-finite scale; NaN: every byte NaN, Inf: the planted byte
    NaN and the others 0), every other slot keeps its scale and bytes, the copies carry the plant in its own element"""
    import test_full_finetune_fp8_kernels as RQ
    place, n, _, _ = RQ.table()
    m0 = RQ.base_master()
    off, cnt = RQ.offset_of(layer), RQ.count(layer)
    doff = next(d for L, _, d in place if L == layer)
    m1 = put(m0, PLANTS[plant], off + cnt - 1)
    want_q, want_s = OF.quantize(m1[off:off + cnt].to(dtype))
    assert not bool(torch.isfinite(want_s)) and bool(nan_byte(want_q)[-1])
    st = RQ.run(dev, dtype, m0)  # fresh poisoned buffers and a plan; the later calls reuse them
    RQ.check_against_oracle(st, dtype, m0, what="clean: ")

    def again(master):
        md = master.to(dev)
        st["plan"].run(md, st["w"], st["wt"], st["q8"], st["scales"], st["amax"])
        same_bits(md, master, "the master was written")
        return {key: st[key].cpu().clone() for key in ("w", "wt", "q8", "scales") if st[key] is not None}
    o0, o1 = again(m0), again(m1)
    what = f"weights_refresh_q8 {layer} {plant}"
    slot = RQ.SLOT[layer]
    word_nonfinite(o1["scales"][slot:slot + 1], what + ": the slot's scale")
    bytes_follow(o1["q8"][doff:doff + cnt], want_q, what + ": the slot's bytes")
    others = torch.ones(RQ.N_SLOTS, dtype=torch.bool)
    others[slot] = False
    same_bits(o1["scales"][others], o0["scales"][others], what + ": rule 2 - the other slots' scales")
    outside = torch.ones(n, dtype=torch.bool)
    outside[doff:doff + cnt] = False
    same_bits(o1["q8"][outside], o0["q8"][outside], what + ": rule 2 - bytes of the other slots")
    for name in ("w", "wt"):
        if name in o1:
            changed = bits(o1[name]) != bits(o0[name])
            assert int(changed.sum()) == 1 and bool(nonfinite(o1[name])[changed].all()), f"{what}: {name} beyond the planted element"
    o2 = again(m0)
    for name in o0:
        same_bits(o2[name], o0[name], f"{what}: rule 4 - {name}")
    free = ("conv", 24, 1, 40)  # rule 3: a problem with slot -1 is not quantised - a plant in its master reaches no byte and no scale
    assert RQ.SLOT[free] == -1
    o3 = again(put(m0, PLANTS[plant], RQ.offset_of(free)))
    same_bits(o3["q8"], o0["q8"], what + ": rule 3 - bytes with the plant in a slot -1 problem")
    same_bits(o3["scales"], o0["scales"], what + ": rule 3 - scales with the plant in a slot -1 problem")
    again(m0)


# ================================================================================================================
# B. the delayed-scaling updates: a non-finite abs-max is a site that saw no tensor
# ================================================================================================================
N_SITES = 300  # two blocks of 256
POISONED = {0: INF, 255: NAN, 256: INF, 299: NAN}  # first and last lane of the first block, the second block's ends


def _site_words(step):
    """ordinary abs-maxima that grow from update to update (so that a site clips each time), every third site unseen"""
    g = torch.Generator().manual_seed(step)
    a = (torch.rand(N_SITES, generator=g) + 0.5) * 2.0 ** step
    a[1::3] = 0.0
    for i in POISONED:
        a[i] = 1.5 * 2.0 ** step  # the sites poisoned later are ordinary, seen sites before
    return a.to(F32).view(torch.int32).clone()


def _poisoned_words(step):
    w = _site_words(step).view(F32).clone()
    for i, v in POISONED.items():
        w[i] = v
    return w.view(torch.int32).clone()


@pytest.mark.parametrize("account", [True, False], ids=["account", "no-account"])
@pytest.mark.parametrize("hist_len,ring", [(1, 0), (4, 0), (4, 3)], ids=["h1", "h4-ring0", "h4-ring3"])
def test_hist_update_treats_a_nonfinite_site_as_unseen(dev, hist_len, ring, account):
    """comat_fp8_scales_update_hist with +Inf and NaN words next to ordinary and zero ones: scale, hist, count, clip_steps and
    worst of such a site are untouched, clip_now is 0 and the running maximum is cleared - the tables are those of the header's
    update (test_fp8_recipe._ref_update) with a ZERO word at those sites, bit for bit; after it a clean update gives the bits
    of a twin that never saw the poisoned step"""
    from test_fp8_recipe import _launch, _ref_update, _tables
    k = ops.kernels()
    pre = hist_len + ring  # count % hist_len == ring, the window full
    pre += hist_len if pre < 2 else 0  # (hist_len = 1: a second update, so that the clip flag to be cleared is set there too)
    keys = ("scale", "hist", "count", "clip_steps", "worst", "clip_now", "amax")
    got, ref, twin = _tables(N_SITES, hist_len, dev), _tables(N_SITES, hist_len, "cpu"), _tables(N_SITES, hist_len, "cpu")
    for step in range(pre):
        for t in (got, ref, twin):
            t["amax"].copy_(_site_words(step))
        _launch(k, got, N_SITES, hist_len, 1.25, account)
        _ref_update(ref, hist_len, 1.25, account)
        _ref_update(twin, hist_len, 1.25, account)
    sites = torch.tensor(sorted(POISONED))
    assert bool((ref["count"][sites] % hist_len == ring).all()) and bool((ref["count"][sites] >= hist_len).all())
    assert pre >= 2
    if account:
        assert bool((ref["clip_now"][sites] == 1).all())  # CPU precondition: the flag to be cleared is set
    for t in (got, ref):  # rule 3: site 1 never saw a tensor - whatever its scale and history hold is neither read nor written
        t["scale"][1] = NAN
        t["hist"][1] = NAN
    before = {key: got[key].cpu().clone() for key in keys}
    words = _poisoned_words(pre)
    assert int(words[1]) == 0
    got["amax"].copy_(words)
    ref["amax"].copy_(torch.where(torch.isfinite(words.view(F32)), words, torch.zeros_like(words)))
    _launch(k, got, N_SITES, hist_len, 1.25, account)
    _ref_update(ref, hist_len, 1.25, account)
    for key in keys:
        same_bits(got[key], ref[key], f"poisoned update: {key}")
    for key in ("scale", "hist", "count", "clip_steps", "worst"):
        same_bits(got[key].cpu()[sites], before[key][sites], f"poisoned update: {key} of the non-finite sites")
    assert int(got["clip_now"].cpu()[sites].abs().sum()) == 0 and int(got["amax"].cpu().abs().sum()) == 0
    for t in (got, twin):  # the twin skips the poisoned step altogether at those sites - and they are the ones compared
        t["amax"].copy_(_site_words(pre + 1))
    _launch(k, got, N_SITES, hist_len, 1.25, account)
    _ref_update(twin, hist_len, 1.25, account)
    for key in ("scale", "hist", "count"):
        same_bits(got[key].cpu()[sites], twin[key][sites], f"clean update after the poisoned one: {key} of the non-finite sites")


def test_plain_update_treats_a_nonfinite_site_as_unseen(dev):
    """comat_fp8_scales_update: the scale of a site whose word is +Inf or NaN is kept, its word cleared; every other site as ever"""
    k = ops.kernels()
    amax, scale = torch.zeros(N_SITES, dtype=torch.int32, device=dev), torch.zeros(N_SITES, device=dev)
    amax.copy_(_site_words(0))
    k.fp8_scales_update(amax, scale, N_SITES)
    before = scale.cpu().clone()
    words = _poisoned_words(1)
    amax.copy_(words)
    k.fp8_scales_update(amax, scale, N_SITES)
    a = words.view(F32)
    want = torch.where((words != 0) & torch.isfinite(a), torch.clamp(a, min=2.0 ** -100) / 448.0, before)
    same_bits(scale, want, "poisoned update: scale")
    assert int(amax.cpu().abs().sum()) == 0, "a running maximum was not cleared"
    sites = torch.tensor(sorted(POISONED))
    same_bits(scale.cpu()[sites], before[sites], "poisoned update: scale of the non-finite sites")
    assert bool(torch.isfinite(scale.cpu()).all())


# ================================================================================================================
# C. products
# ================================================================================================================
def _gemm_case(dev, dtype, M, N, K, where, plant, beta, family=None):
    """C = A B^T + bias + beta R on integer operands, one plant: A[M-1, K-1] poisons row M-1, B[N-1, K-1] column N-1, bias[N-1]
    column N-1, R[M-1, N-1] its own element when beta == 1 and nothing when beta == 0 (rule 3)"""
    k = ops.kernels()
    A, B, bias, R = ints(M, K, seed=1, hi=4), ints(N, K, seed=2, hi=4), ints(N, seed=3), ints(M, N, seed=4)
    clean = dict(A=A, B=B, bias=bias, R=R)
    v = PLANTS[plant]
    poisoned = dict(clean)
    poisoned[where] = put(clean[where], v, *{"A": (M - 1, K - 1), "B": (N - 1, K - 1), "bias": (N - 1,), "R": (M - 1, N - 1)}[where])
    dep = torch.zeros(M, N, dtype=torch.bool)
    if where == "A":
        dep[M - 1] = True
    elif where in ("B", "bias"):
        dep[:, N - 1] = True
    elif beta:
        dep[M - 1, N - 1] = True

    def ref(x):
        r = x["A"].double() @ x["B"].double().t() + x["bias"].double()
        return dict(C=r + x["R"].double() if beta else r)  # beta == 0: R is not read (not 0 * R)

    def call(x):
        Ad, Bd, Rd = dv(x["A"], dev, dtype), dv(x["B"], dev, dtype), dv(x["R"], dev, dtype)
        C = torch.empty((M, N), dtype=dtype, device=dev)
        k.gemm(Ad, Bd, C, M, N, K, K, K, N, bias=dv(x["bias"], dev), R=Rd, ldr=N, beta=float(beta))
        if family is not None and dev.type == "cuda":
            from comat_amd import _hip
            assert _hip.last_gemm_kernel() == family, f"served by kernel {_hip.last_gemm_kernel()}, the case is about {family}"
        return dict(C=C.cpu())
    what = f"gemm {M}x{N}x{K} {plant} in {where} beta={beta}"
    if where == "R" and not beta:  # rule 3: the bits of the clean call
        o0, o1 = call(clean), call(poisoned)
        assert_exact(o0["C"], ref(clean)["C"], dtype, what + ": clean")
        same_bits(o1["C"], o0["C"], what + ": rule 3 - R is read although beta == 0")
        return
    drive(call, ref, clean, poisoned, dict(C=dep), dtype, what, exact=dict(C=dtype))


@plants
@dtypes
@pytest.mark.parametrize("where,beta", [("A", 1), ("B", 1), ("bias", 1), ("R", 1), ("R", 0)])
def test_general_gemm(dev, dtype, where, beta, plant, default_opts):
    """comat_gemm on the general 64x64 kernel (family 0): a ragged last tile in M and N, a k-tail"""
    if dev.type == "cuda":
        _set_opts(gemm2=0, gemm3=0)
    _gemm_case(dev, dtype, 70, 40, 93, where, plant, beta, family=0)


@plants
@pytest.mark.parametrize("where,beta", [("A", 1), ("B", 1), ("bias", 1), ("R", 1), ("R", 0)])
def test_pipelined_gemm(dev, where, beta, plant, default_opts):
    """comat_gemm on the pipelined kernel (family 1), bf16, K a multiple of 64, a ragged last row tile"""
    if dev.type == "cuda":
        _set_opts(gemm2=1, gemm3=0, g2_cfg=0, g2_splits=0)
    _gemm_case(dev, BF16, 130, 72, 64, where, plant, beta, family=1)


@pytest.mark.gpu
@plants
def test_split_k_leaves_no_residue(hip, plant, default_opts):
    """split-K forced on the pipelined kernel: the slabs and tickets a poisoned call used serve the next clean call (rule 4)"""
    _set_opts(gemm2=1, gemm3=0, g2_cfg=0, g2_splits=4)
    _gemm_case(hip, BF16, 130, 72, 256, "A", plant, 1, family=1)


@pytest.mark.gpu
@plants
def test_forced_splits_leave_no_residue(hip, plant, default_opts):
    """option force_splits on the general kernel: the in-launch combine's slabs and tickets after a poisoned call (rule 4)"""
    _set_opts(gemm2=0, gemm3=0, force_splits=2)
    _gemm_case(hip, BF16, 70, 40, 93, "A", plant, 1, family=0)


@plants
@pytest.mark.parametrize("where,beta", [("A", 1), ("B", 1), ("bias", 1), ("R", 1), ("R", 0)])
def test_lean_gemm(dev, where, beta, plant, default_opts):
    """comat_gemm on the lean kernel (family 5): a ragged M = 33, N = 72, five chunks of 64 along k"""
    if dev.type == "cuda":
        _set_opts(gemm3=2, g3_cfg=0)
    _gemm_case(dev, BF16, 33, 72, 320, where, plant, beta, family=5)


def served(dev, family):
    if dev.type == "cuda":
        from comat_amd import _hip
        assert _hip.last_gemm_kernel() == family, f"served by kernel {_hip.last_gemm_kernel()}, the case is about {family}"


@pytest.mark.parametrize("where,beta", [("A", 1), ("B", 1), ("bias", 1), ("R", 1), ("R", 0)])
def test_fp8_gemm(dev, where, beta, default_opts):
    """comat_gemm with e4m3 operands (family 3): e4m3fn has no Inf, the plant in A / B is the NaN byte 0x7F; bias and R take a
    NaN value"""
    k = ops.kernels()
    if dev.type == "cuda":
        _set_opts(gemm2=1, gemm3=0, g2_cfg=0, g2_splits=0)
    M, N, K = 130, 72, 192
    A, B, bias, R = ints(M, K, seed=1), ints(N, K, seed=2), ints(N, seed=3), ints(M, N, seed=4)
    e4 = lambda t: t.to(torch.float8_e4m3fn).view(torch.uint8)
    clean = dict(A=e4(A), B=e4(B), bias=bias, R=R)
    poisoned = dict(clean)
    at = {"A": (M - 1, K - 1), "B": (N - 1, K - 1), "bias": (N - 1,), "R": (M - 1, N - 1)}[where]
    poisoned[where] = put(clean[where], 0x7F if where in "AB" else NAN, *at)
    dep = torch.zeros(M, N, dtype=torch.bool)
    if where == "A":
        dep[M - 1] = True
    elif where in ("B", "bias"):
        dep[:, N - 1] = True
    elif beta:
        dep[M - 1, N - 1] = True
    f8 = lambda q: q.view(torch.float8_e4m3fn).double()

    def ref(x):
        r = 0.5 * (f8(x["A"]) @ f8(x["B"]).t()) + x["bias"].double()
        return dict(C=r + x["R"].double() if beta else r)

    def call(x):
        C = torch.empty((M, N), dtype=BF16, device=dev)
        k.gemm(dv(x["A"], dev), dv(x["B"], dev), C, M, N, K, K, K, N, bias=dv(x["bias"], dev), R=dv(x["R"], dev, BF16), ldr=N,
               beta=float(beta), scales=(torch.tensor([0.5], device=dev), torch.tensor([1.0], device=dev)))
        served(dev, 3)
        return dict(C=C.cpu())
    what = f"fp8 gemm NaN in {where} beta={beta}"
    if where == "R" and not beta:
        o0, o1 = call(clean), call(poisoned)
        assert_exact(o0["C"], ref(clean)["C"], BF16, what + ": clean")
        same_bits(o1["C"], o0["C"], what + ": rule 3 - R is read although beta == 0")
        return
    drive(call, ref, clean, poisoned, dict(C=dep), BF16, what, exact=dict(C=BF16))


@plants
@pytest.mark.parametrize("where", ["A", "B", "C"])
def test_k_major_gemm(dev, where, plant, default_opts):
    """the k-major pipelined kernel (family 2; transA and transB, fp32 C accumulated in place, R = C, beta = 1): a plant in the
    last k-row of A poisons row M - 1, in B column N - 1, in C its own element"""
    k = ops.kernels()
    if dev.type == "cuda":
        _set_opts(gemm2=1, gemm2_tt=1, gemm3=0, g2_splits=0)
    M, N, K = 136, 72, 416
    clean = dict(A=ints(K, M, seed=21), B=ints(K, N, seed=22), C=ints(M, N, seed=23, hi=64))
    poisoned = dict(clean)
    poisoned[where] = put(clean[where], PLANTS[plant], *{"A": (K - 1, M - 1), "B": (K - 1, N - 1), "C": (M - 1, N - 1)}[where])
    dep = torch.zeros(M, N, dtype=torch.bool)
    if where == "A":
        dep[M - 1] = True
    elif where == "B":
        dep[:, N - 1] = True
    else:
        dep[M - 1, N - 1] = True
    ref = lambda x: dict(C=x["C"].double() + x["A"].double().t() @ x["B"].double())

    def call(x):
        C = dv(x["C"], dev)
        k.gemm(dv(x["A"], dev, BF16), dv(x["B"], dev, BF16), C, M, N, K, M, N, N, transA=True, transB=True, R=C, ldr=N, beta=1.0)
        served(dev, 2)
        return dict(C=C.cpu())
    drive(call, ref, clean, poisoned, dict(C=dep), F32, f"k-major gemm {plant} in {where}", exact=dict(C=F32))


@plants
@pytest.mark.parametrize("where", ["A", "B"])
def test_gemm_tt_grouped(dev, where, plant):
    """comat_gemm_tt_grouped (family 4), two problems in one launch, the plant in the second one's A (its last row is poisoned)
    or B (its last column); the first problem is exact"""
    k = ops.kernels()
    shapes = ((72, 40, 100), (136, 264, 1100))
    clean = {}
    for i, (M, N, K) in enumerate(shapes):
        clean.update({f"A{i}": ints(K, M, seed=101 + i), f"B{i}": ints(K, N, seed=111 + i), f"C{i}": ints(M, N, seed=121 + i, hi=64)})
    M1, N1, K1 = shapes[1]
    poisoned = dict(clean)
    poisoned[where + "1"] = put(clean[where + "1"], PLANTS[plant], K1 - 1, (M1 if where == "A" else N1) - 1)
    ref = lambda x: {f"C{i}": x[f"C{i}"].double() + x[f"A{i}"].double().t() @ x[f"B{i}"].double() for i in range(2)}

    def call(x):
        outs = [dv(x[f"C{i}"], dev) for i in range(2)]
        k.gemm_tt_grouped([(dv(x[f"A{i}"], dev, BF16), dv(x[f"B{i}"], dev, BF16), outs[i], M, N, K, M, N, N)
                           for i, (M, N, K) in enumerate(shapes)])
        served(dev, 4)
        return {f"C{i}": outs[i].cpu() for i in range(2)}
    hit = row_mask((M1, N1), M1 - 1) if where == "A" else row_mask((M1, N1), slice(None), N1 - 1)
    dep = dict(C0=torch.zeros(shapes[0][:2], dtype=torch.bool), C1=hit)
    drive(call, ref, clean, poisoned, dep, F32, f"gemm_tt_grouped {plant} in {where}", exact=dict(C0=F32, C1=F32))


SEG = {"general": (dict(gemm2=0, gemm3=0), 0, (93, 40)), "pipelined": (dict(gemm2=1, gemm3=0, g2_cfg=0, g2_splits=0), 1, (160, 96))}


@plants
@pytest.mark.parametrize("where,beta", [("h", 1), ("R", 0)])
@pytest.mark.parametrize("family", list(SEG))
def test_gemm_segments(dev, family, where, beta, plant, default_opts):
    """comat_gemm_segments, two problems that share x and read their h out of one [M, 2 K2] matrix: a plant in the last element
    of the LAST segment's operand poisons row M - 1 of the second problem only; R with beta == 0 is not read"""
    k = ops.kernels()
    opts, kernel, (K1, K2) = SEG[family]
    if dev.type == "cuda":
        _set_opts(**opts)
    G, M, N = 2, 130, 72
    clean = dict(x=ints(M, K1, seed=91), W=ints(G, N, K1, seed=92), h=ints(M, G * K2, seed=93), U=ints(G, N, K2, seed=94),
                 bias=ints(G, N, seed=95), R=ints(G, M, N, seed=96))
    poisoned = dict(clean)
    poisoned[where] = put(clean[where], PLANTS[plant], *((M - 1, G * K2 - 1) if where == "h" else (G - 1, M - 1, N - 1)))
    dep = torch.zeros(G, M, N, dtype=torch.bool)
    if where == "h":
        dep[G - 1, M - 1] = True

    def ref(x):
        r = (torch.einsum("mk,gnk->gmn", x["x"].double(), x["W"].double())
             + torch.einsum("mgr,gnr->gmn", x["h"].double().reshape(M, G, K2), x["U"].double()) + x["bias"].double()[:, None, :])
        return dict(C=r + x["R"].double() if beta else r)

    def call(x):
        d = {n_: dv(t, dev, BF16) for n_, t in x.items() if n_ != "bias"}
        segs = [(d["x"], d["W"], K1, K1, K1, 0, N * K1), (d["h"], d["U"], K2, G * K2, K2, K2, N * K2)]
        C = torch.empty((G, M, N), dtype=BF16, device=dev)
        k.gemm_segments(segs, C, M, N, N, bias=dv(x["bias"], dev), R=d["R"], ldr=N, beta=float(beta), batch=G, sC=M * N, sR=M * N)
        served(dev, kernel)
        return dict(C=C.cpu())
    what = f"gemm_segments {family} {plant} in {where} beta={beta}"
    if where == "R":
        o0, o1 = call(clean), call(poisoned)
        assert_exact(o0["C"], ref(clean)["C"], BF16, what + ": clean")
        same_bits(o1["C"], o0["C"], what + ": rule 3 - R is read although beta == 0")
        return
    drive(call, ref, clean, poisoned, dict(C=dep), BF16, what, exact=dict(C=BF16))


@pytest.mark.gpu
@plants
def test_lora_merge(hip, plant):
    """comat_lora_merge, two projections in one launch, the plant in the second one's U: row N - 1 of its Wm (column N - 1 of
    its WmT) is poisoned, the first projection is exact"""
    k = ops.kernels()
    G, N, K, r = 2, 72, 136, 16
    clean = dict(W=ints(G, N, K, seed=151, hi=4), U=ints(G, N, r, seed=152, hi=4), Dt=ints(G, K, r, seed=153, hi=4))
    poisoned = dict(clean, U=put(clean["U"], PLANTS[plant], G - 1, N - 1, r - 1))

    def ref(x):
        wm = x["W"].double() + 0.5 * torch.einsum("gnr,gkr->gnk", x["U"].double(), x["Dt"].double())
        return dict(Wm=wm, WmT=wm.transpose(1, 2).contiguous())

    def call(x):
        Wd, Ud, Dtd = (dv(x[n_], hip, BF16) for n_ in ("W", "U", "Dt"))
        Wm, WmT = torch.empty((G, N, K), dtype=BF16, device=hip), torch.empty((G, K, N), dtype=BF16, device=hip)
        problems = torch.tensor([[Wd[i].data_ptr(), Ud[i].data_ptr(), Dtd[i].data_ptr(), Wm[i].data_ptr(), WmT[i].data_ptr(), N, K, r, r, r]
                                 for i in range(G)], dtype=torch.int64, device=hip)
        tiles = torch.tensor([[i, n0, k0] for i in range(G) for n0 in range(0, N, 64) for k0 in range(0, K, 64)],
                             dtype=torch.int32, device=hip)
        assert k.lora_merge_ok(Wd[0], Ud[0], Dtd[0], r, r, r)
        k.lora_merge(problems, tiles, 0.5)
        return dict(Wm=Wm.cpu(), WmT=WmT.cpu())
    dep = dict(Wm=row_mask((G, N, K), G - 1, N - 1), WmT=row_mask((G, K, N), G - 1, slice(None), N - 1))
    r0 = ref(clean)["Wm"]
    fits = r0.float().to(BF16).double() == r0  # (W + s U D has more than 8 significant bits in a few elements: those are held to
    assert float(fits.double().mean()) > 0.99  # their one rounding by assert_exact, which rounds the reference itself)
    drive(call, ref, clean, poisoned, dep, BF16, f"lora_merge {plant}", exact=dict(Wm=BF16, WmT=BF16))


CONV = {"pipelined": (dict(gemm2=1, g2_cfg=0, g2_splits=0), BF16, 1), "general-fp32": (dict(gemm2=0), F32, 0)}


@plants
@pytest.mark.parametrize("where,beta", [("x", 1), ("R", 1), ("R", 0)])
@pytest.mark.parametrize("family", list(CONV))
def test_conv2d_forward(dev, family, where, beta, plant, default_opts):
    """comat_conv2d, 3 x 3, pad 1: a plant in one channel of the image CORNER (0, 0) of the second sample reaches the output
    through four taps only - the 2 x 2 output pixels at that corner, every output channel; nothing of the first sample"""
    k = ops.kernels()
    opts, dtype, kernel = CONV[family]
    if dev.type == "cuda":
        _set_opts(**opts)
    Bn, H, W, Cin, Cout = 2, 13, 9, 64, 72
    Mrows = Bn * H * W
    clean = dict(x=ints(Bn, H, W, Cin, seed=131), w=ints(Cout, 3, 3, Cin, seed=132, hi=4), bias=ints(Cout, seed=133),
                 R=ints(Mrows, Cout, seed=135))
    poisoned = dict(clean)
    poisoned[where] = put(clean[where], PLANTS[plant], *((Bn - 1, 0, 0, Cin - 1) if where == "x" else (Mrows - 1, Cout - 1)))
    dep = torch.zeros(Bn, H, W, Cout, dtype=torch.bool)
    if where == "x":
        dep[Bn - 1, :2, :2] = True
    elif beta:
        dep[Bn - 1, H - 1, W - 1, Cout - 1] = True
    dep = dep.reshape(Mrows, Cout)

    def ref(x):
        y = F.conv2d(x["x"].double().permute(0, 3, 1, 2), x["w"].double().permute(0, 3, 1, 2), padding=1)
        r = y.permute(0, 2, 3, 1).reshape(Mrows, Cout) + x["bias"].double()
        return dict(Y=r + x["R"].double() if beta else r)

    def call(x):
        Y = torch.empty((Mrows, Cout), dtype=dtype, device=dev)
        # the image lies between two NaN halos of two image rows each: a tap outside the image is not read (rule 3) - one that
        # were would find a NaN in the neighbouring memory
        halo = 2 * W * Cin
        buf = torch.full((Mrows * Cin + 2 * halo,), NAN, dtype=dtype, device=dev)
        xin = buf[halo:halo + Mrows * Cin].view(Mrows, Cin)
        xin.copy_(x["x"].reshape(Mrows, Cin))
        k.conv2d(xin, dv(x["w"], dev, dtype), Y, Bn, H, W, Cin, H, W, Cout, 3, 3, 1, 1, mode=0,
                 ups=1, bias=dv(x["bias"], dev), R=dv(x["R"], dev, dtype), beta=float(beta))
        served(dev, kernel)
        return dict(Y=Y.cpu())
    what = f"conv2d {family} {plant} in {where} beta={beta}"
    if where == "R" and not beta:
        o0, o1 = call(clean), call(poisoned)
        assert_exact(o0["Y"], ref(clean)["Y"], dtype, what + ": clean")
        same_bits(o1["Y"], o0["Y"], what + ": rule 3 - R is read although beta == 0")
        return
    drive(call, ref, clean, poisoned, dict(Y=dep), dtype, what, exact=dict(Y=dtype))


@plants
@pytest.mark.parametrize("family", list(CONV))
def test_conv2d_data_gradient(dev, family, plant, default_opts):
    """the data-gradient of the same convolution through ops.conv2d: a plant in one channel of the upstream gradient at the
    corner pixel reaches dx at the 2 x 2 corner pixels, every input channel"""
    opts, dtype, _ = CONV[family]
    if dev.type == "cuda":
        _set_opts(**opts)
    Bn, H, W, Cin, Cout = 2, 13, 9, 64, 96
    w, b = ints(Cout, Cin, 3, 3, seed=132, hi=4), ints(Cout, seed=133)
    x, g0 = ints(Bn * H * W, Cin, seed=131), ints(Bn, H, W, Cout, seed=136, hi=4)
    g1 = put(g0, PLANTS[plant], Bn - 1, 0, 0, Cout - 1)
    conv = ops.FrozenConv(w, b, dtype, dev, stride=1, pad=1)

    def ref(g):
        dx = F.conv_transpose2d(g.double().permute(0, 3, 1, 2), w.double(), padding=1)
        return dict(dx=dx.permute(0, 2, 3, 1).reshape(Bn * H * W, Cin))

    def call(g):
        xd = dv(x, dev, dtype).requires_grad_(True)
        y = ops.conv2d(xd, conv, Bn, H, W)
        y.backward(dv(g.reshape(Bn * H * W, Cout), dev, dtype))
        return dict(dx=xd.grad.cpu())
    dep = torch.zeros(Bn, H, W, Cin, dtype=torch.bool)
    dep[Bn - 1, :2, :2] = True
    drive(call, ref, g0, g1, dict(dx=dep.reshape(Bn * H * W, Cin)), dtype, f"conv2d data-gradient {family} {plant}", exact=dict(dx=dtype))


@plants
@pytest.mark.parametrize("where", ["x", "dy"])
@pytest.mark.parametrize("path", ["pipelined", "general"])
def test_conv2d_wgrad(dev, path, where, plant):
    """comat_conv2d_wgrad on both paths (families 6 and 7), dW accumulated into a non-zero start.  A plant in channel Cin - 1 of
    the corner pixel of X reaches dW[:, kh, kw, Cin - 1] for the four taps kh, kw in {0, 1} that read the corner; a plant in
    channel Cout - 1 of the corner pixel of dY reaches dW[Cout - 1, kh, kw, :] for the four taps kh, kw in {1, 2} whose input
    pixel lies inside the image, and nothing of any other output channel.  The five PADDING taps of dW[Cout - 1] are left
    open: whether the product of the plant with a padding zero is a term of the sum (0 * NaN) or no term is not settled by the
    definition - torch's own conv2d_weight answers NaN at all nine taps in fp64 at this geometry and at the four in-image taps
    in fp32 at a smaller one; the general path forms no such term, the pipelined one (a zero page under the gathered operand)
    does.  The header says so; those elements are masked out of the comparison."""
    from test_conv_wgrad import GEOMS, expected_path, out_hw
    k = ops.kernels()
    geom, dtype = GEOMS[1] if path == "pipelined" else GEOMS[9]
    Bn, Hin, Win, Cin, Cout, ks, stride, ups = geom
    Ho, Wo, pad = out_hw(geom)
    assert (ks, stride, ups, pad) == (3, 1, 1, 1)
    x0, dy0, dw0 = ints(Bn, Hin, Win, Cin, seed=141), ints(Bn, Ho, Wo, Cout, seed=142), ints(Cout, ks, ks, Cin, seed=143, hi=64)
    clean = dict(x=x0, dy=dy0)
    poisoned = dict(clean)
    poisoned[where] = put(clean[where], PLANTS[plant], Bn - 1, 0, 0, (Cin if where == "x" else Cout) - 1)

    def ref(t):
        x, dy = t["x"].double(), t["dy"].double()
        bad = ~torch.isfinite(dy)  # a non-finite dY element: its in-image taps one by one, the padding taps not at all
        gw = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), (Cout, Cin, ks, ks), dy.masked_fill(bad, 0.0).permute(0, 3, 1, 2),
                                         stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()
        for b, ho, wo, co in torch.nonzero(bad).tolist():
            for kh in range(ks):
                for kw in range(ks):
                    hi, wi = ho - pad + kh, wo - pad + kw
                    if 0 <= hi < Hin and 0 <= wi < Win:
                        gw[co, kh, kw] += dy[b, ho, wo, co] * x[b, hi, wi]
        return dict(dW=(dw0.double() + gw).masked_fill(open_, 0.0))

    def call(t):
        dw = dv(dw0, dev)
        k.conv2d_wgrad(dv(t["x"], dev, dtype), dv(t["dy"], dev, dtype), dw, Bn, Hin, Win, Cin, Ho, Wo, Cout, ks, ks, stride, pad, ups)
        served(dev, expected_path(geom, dtype))
        return dict(dW=dw.cpu().masked_fill(open_, 0.0))
    open_ = torch.zeros(Cout, ks, ks, Cin, dtype=torch.bool)  # the padding taps of the poisoned output channel (dY plant only)
    if where == "dy":
        open_[Cout - 1] = True
        open_[Cout - 1, 1:, 1:] = False
    dep = torch.zeros(Cout, ks, ks, Cin, dtype=torch.bool)
    if where == "x":
        dep[:, :2, :2, Cin - 1] = True  # x[0, 0] meets dy[ho, wo] at the tap (kh, kw) = (pad - ho, pad - wo), ho and wo in {0, 1}
    else:
        dep[Cout - 1, 1:, 1:, :] = True  # dy[0, 0] meets x[kh - pad, kw - pad]: inside the image for kh, kw in {1, 2}
    drive(call, ref, clean, poisoned, dict(dW=dep), F32, f"conv2d_wgrad {path} {plant} in {where}", exact=dict(dW=F32))


# ================================================================================================================
# D. softmax, fused attention, cross entropy
# ================================================================================================================
@plants
@dtypes
@pytest.mark.parametrize("cols", [65, 77])
@pytest.mark.parametrize("mode", ["plain", "causal", "masked"])
def test_softmax(dev, dtype, cols, mode, plant):
    """comat_softmax_fwd / _bwd: a plant in a visible score poisons its row (a -Inf score only itself: weight 0, the row keeps
    finite scores), every other row is within the sibling bound; a plant under the causal or the key mask changes no bit"""
    k = ops.kernels()
    B_, H, Nq = 2, 2, 7
    rows = B_ * H * Nq
    S0, dP = rnd(rows, cols, seed=1) * 2, rnd(rows, cols, seed=2)
    km = None
    visible = torch.ones(rows, cols, dtype=torch.bool)
    if mode == "causal":
        visible = torch.ones(Nq, cols, dtype=torch.bool).tril(diagonal=cols - Nq).repeat(B_ * H, 1)
    if mode == "masked":
        km = torch.ones(B_, cols, dtype=torch.int8)
        km[0, cols - cols // 3:] = 0
        km[1, :cols // 2] = 0
        visible = km.bool().repeat_interleave(H * Nq, 0)
    r = rows - 1 - (Nq - 1 if mode == "causal" else 0)  # (causal: the first query of the last head, which has masked keys)
    c_vis = int(torch.nonzero(visible[r])[-1])
    v = PLANTS[plant]

    def fwd_ref(S):
        p = torch.softmax(S.double().masked_fill(~visible, -INF), -1)
        return dict(P=torch.where(visible, p, torch.zeros_like(p)))  # a masked key has probability 0 whatever the row holds

    def fwd(S):
        P = torch.full((rows, cols), NAN, dtype=dtype, device=dev)
        k.softmax_fwd(dv(S, dev), P, rows, cols, q_len=Nq, causal=mode == "causal", causal_offset=cols - Nq,
                      key_mask=dv(km, dev) if km is not None else None, rows_per_mask=H * Nq)
        return dict(P=P.cpu())
    S1 = put(S0, v, r, c_vis)
    dep = torch.zeros(rows, cols, dtype=torch.bool) if plant == "-inf" else row_mask((rows, cols), r) & visible
    what = f"softmax {mode} cols={cols} {plant}"
    if plant == "-inf":  # the row keeps finite scores: the key has weight 0, nothing is non-finite
        r0, r1 = fwd_ref(S0)["P"], fwd_ref(S1)["P"]
        depends(r1, None, what)
        o1 = fwd(S1)
        carried_contained(o1["P"], r1, dtype, what)
        assert float(o1["P"][r, c_vis]) == 0.0
    else:
        o1 = drive(fwd, fwd_ref, S0, S1, dict(P=dep), dtype, what)
    if not bool(visible.all()):  # rule 3
        c_hid = int(torch.nonzero(~visible[r])[0])
        same_bits(fwd(put(S0, v, r, c_hid))["P"], fwd(S0)["P"], what + ": rule 3 - a masked score is read")

    # backward from a P with one poisoned element: its row is poisoned, the others are not
    P0 = fwd(S0)["P"]
    bwd_ref = lambda P: dict(dS=0.3 * P.double() * (dP.double() - (dP.double() * P.double()).sum(-1, keepdim=True)))

    def bwd(P):
        dS = torch.full((rows, cols), NAN, dtype=dtype, device=dev)
        k.softmax_bwd(dv(P, dev, dtype), dv(dP, dev), dS, rows, cols, 0.3)
        return dict(dS=dS.cpu())
    drive(bwd, bwd_ref, P0.float(), put(P0.float(), v, r, c_vis), dict(dS=row_mask((rows, cols), r)), dtype, what + " bwd")


def _flash_case(dev, where, plant, geo=(2, 3, 70, 45, 40), dtype=BF16):
    """comat_flash_attn_fwd / _bwd: a plant in Q poisons one query row of one head (O, lse, dQ of that row; dK and dV of the
    whole head, which sum over the queries), a plant in K or V the (batch, head); every other (batch, head) is within the
    sibling bounds (O tol, gradients tol * 3, as test_windows.py)"""
    k = ops.kernels()
    B_, H, Nq, Nk, d = geo
    HD, scale = H * d, d ** -0.5
    q0, k0, v0, g0 = (rnd(B_ * n_, HD, dtype=dtype, seed=s_) for n_, s_ in ((Nq, 1), (Nk, 2), (Nk, 3), (Nq, 4)))
    b, h = B_ - 1, H - 1
    val = PLANTS[plant]
    clean = dict(q=q0, k=k0, v=v0)
    poisoned = dict(clean)
    if where == "q":
        poisoned["q"] = put(q0, val, b * Nq + Nq - 1, h * d + d - 1)
    else:
        poisoned[where] = put(clean[where], val, b * Nk + Nk - 1, h * d)
    heads = lambda t, n: t.double().reshape(B_, n, H, d).permute(0, 2, 1, 3)
    unheads = lambda t, n: t.permute(0, 2, 1, 3).reshape(B_ * n, HD)

    def ref(x):
        qh, kh, vh = (heads(x["q"], Nq).requires_grad_(True), heads(x["k"], Nk).requires_grad_(True),
                      heads(x["v"], Nk).requires_grad_(True))
        s = qh @ kh.transpose(-1, -2) * scale
        o = torch.softmax(s, -1) @ vh
        o.backward(heads(g0, Nq))
        return dict(o=unheads(o.detach(), Nq), lse=torch.logsumexp(s.detach(), -1), dq=unheads(qh.grad, Nq),
                    dk=unheads(kh.grad, Nk), dv=unheads(vh.grad, Nk))

    dbuf = torch.empty(B_, H, Nq, device=dev)  # ONE D buffer for the clean, the poisoned and the second clean call (rule 4)

    def call(x):
        qd, kd, vd, gd = dv(x["q"], dev, dtype), dv(x["k"], dev, dtype), dv(x["v"], dev, dtype), dv(g0, dev, dtype)
        o, lse = torch.empty_like(qd), torch.empty(B_, H, Nq, device=dev)
        k.flash_attn_fwd(qd, kd, vd, o, lse, B_, H, Nq, Nk, d, HD, HD, HD, HD, scale)
        dq, dk, dv_ = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
        k.flash_attn_bwd(qd, kd, vd, o, gd, lse, dbuf, dq, dk, dv_, B_, H, Nq, Nk, d, HD, HD, HD, HD, scale)
        return dict(o=o.cpu(), lse=lse.cpu(), dq=dq.cpu(), dk=dk.cpu(), dv=dv_.cpu())
    # The dependent sets, stated from the definition (drive() asserts them on the fp64 reference before any kernel runs).
    head_q, head_k = _head_rows(B_, H, Nq, d, b, h), _head_rows(B_, H, Nk, d, b, h)
    none_k, lse_of = torch.zeros(B_ * Nk, HD, dtype=torch.bool), lambda rows_: rows_.reshape(B_, Nq, H, d)[..., 0].permute(0, 2, 1)
    if where == "q":
        # the query's scores are all NaN (or +-Inf of both signs): its row of O, lse and dQ; P of that row enters dK and dV of every
        # key of the head
        row = _head_rows(B_, H, Nq, d, b, h, Nq - 1)
        dep = dict(o=row, lse=lse_of(row), dq=row, dk=head_k, dv=head_k)
    elif where == "k":
        # the key's score is q_i[c] * plant, c the planted head dim: NaN for every query; +-Inf poisons the queries whose product is
        # +Inf (0 * Inf: NaN) - for the others the key has weight 0, O and lse stay finite, but dQ[i, c] = dS_ij * k_j[c] = 0 * Inf
        qc = q0.reshape(B_, Nq, HD)[b, :, h * d]
        hit = torch.ones(Nq, dtype=torch.bool) if plant == "nan" else ~(qc * val == -INF)
        assert 0 < int(hit.sum()) and (plant == "nan" or int(hit.sum()) < Nq)
        hit_rows = torch.zeros(B_, Nq, dtype=torch.bool)
        hit_rows[b] = hit
        rows_ = head_q & hit_rows.reshape(B_ * Nq, 1)
        col = torch.zeros(B_ * Nq, HD, dtype=torch.bool)
        col[b * Nq:(b + 1) * Nq, h * d] = True
        dep = dict(o=rows_, lse=lse_of(rows_), dq=rows_ | col, dk=head_k, dv=head_k)
    else:
        # V[j, c] enters column c of every O row of the head, and through dP_ij = dO_i . v_j the D and dS of every row: dQ and dK of
        # the head; dV does not depend on V, lse neither
        col = torch.zeros(B_ * Nq, HD, dtype=torch.bool)
        col[b * Nq:(b + 1) * Nq, h * d] = True
        dep = dict(o=col, lse=torch.zeros(B_, H, Nq, dtype=torch.bool), dq=head_q, dk=head_k, dv=none_k)
    drive(call, ref, clean, poisoned, dep, dtype, f"flash attention {geo} {plant} in {where}",
          factors=dict(dq=3, dk=3, dv=3, lse=5))


@plants
@pytest.mark.parametrize("where", ["q", "k", "v"])
def test_flash_attention(dev, where, plant):
    _flash_case(dev, where, plant)


def _option_sets():
    from test_exact_attention import OPTION_SETS  # the kernel variants that module enumerates
    return [o for o in OPTION_SETS if o]


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["q", "k"])
@pytest.mark.parametrize("geo", [(1, 4, 70, 130, 40), (1, 2, 256, 77, 40)], ids=["two-tile", "query-split"])
@pytest.mark.parametrize("opts", _option_sets(), ids=lambda o: "-".join(f"{k_}{v_}" for k_, v_ in o.items()))
def test_flash_attention_variants(hip, where, geo, opts, default_opts):
    """every option set of test_exact_attention.py (each selects another forward, dQ or dK/dV kernel, the trim, the merge of a
    split key range) on the shapes that reach the two-tile kernels and the query-split dK/dV pass; a NaN plant"""
    _set_opts(**opts)
    _flash_case(hip, where, "nan", geo=geo)


@plants
@dtypes
@pytest.mark.parametrize("V", [70, 257])
def test_cross_entropy(dev, dtype, V, plant):
    """comat_cross_entropy_fwd / _bwd: a plant in a VALID row makes the loss non-finite, that row's log-probability and gradient
    too, the other rows' stay within the sibling bounds; a plant in an IGNORED row changes no bit of loss, count, log-probs and
    gradient, and that row's gradient is 0"""
    k = ops.kernels()
    T, ls = 9, 0.1
    z0 = rnd(T, V, dtype=dtype, seed=1, scale=3.0)
    labels = torch.randint(0, V, (T,), generator=torch.Generator().manual_seed(2))
    labels[3] = -100
    v = PLANTS[plant]

    def call(z):
        zd, ld = dv(z, dev, dtype), dv(labels, dev)
        logp, rlse, lsc = (torch.full((n_,), NAN, device=dev) for n_ in (T, T, 2))
        k.cross_entropy_fwd(zd, ld, logp, rlse, lsc, T, V, V, -100, ls)
        dz = torch.full((T, V), NAN, dtype=dtype, device=dev)
        k.cross_entropy_bwd(zd, ld, rlse, dz, T, V, V, -100, ls, torch.tensor([2.5], device=dev), lsc)
        lsc = lsc.cpu()
        return dict(loss=(lsc[0] / lsc[1]).reshape(1), count=lsc[1:], logp=logp.cpu(), dz=dz.cpu())

    valid = labels >= 0
    onehot = F.one_hot(labels.clamp(min=0), V).double()

    def ref(z):
        """the header's definition: loss = mean over the valid rows of (1 - ls) (-logp[label]) + ls mean_v(-logp[v]),
        dz = g_up / count * (softmax(z) - ls / V - (1 - ls) onehot) on the valid rows, 0 on the others"""
        lsm = torch.log_softmax(z.double(), -1)
        lp = lsm.gather(1, labels.clamp(min=0)[:, None])[:, 0]
        row = (1 - ls) * (-lp) + ls * (-lsm).mean(-1)
        dz = 2.5 / float(valid.sum()) * (torch.softmax(z.double(), -1) - ls / V - (1 - ls) * onehot)
        return dict(loss=(row[valid].sum() / valid.sum()).reshape(1), count=valid.sum().double().reshape(1),
                    logp=torch.where(valid, lp, torch.zeros_like(lp)), dz=torch.where(valid[:, None], dz, torch.zeros_like(dz)))
    what = f"cross entropy V={V} {plant}"
    r = T - 1
    z1 = put(z0, v, r, V - 1 if labels[r] != V - 1 else V - 2)  # (not the label's own logit: -Inf there is a -Inf log-probability)
    # NaN, +Inf: the row's log-sum-exp is non-finite - its log-probability and gradient too.  -Inf: exp(-inf) = 0, one class
    # less - log-probability and gradient finite; the smoothing term averages -logp over ALL classes, so the loss is +inf
    hit = plant != "-inf"
    dep = dict(loss=torch.ones(1, dtype=torch.bool), count=torch.zeros(1, dtype=torch.bool),
               logp=row_mask((T,), r) if hit else torch.zeros(T, dtype=torch.bool),
               dz=row_mask((T, V), r) if hit else torch.zeros(T, V, dtype=torch.bool))
    drive(call, ref, z0, z1, dep, dtype, what, factors=dict(loss=5, logp=5))
    # rule 3: the ignored row
    o0, o3 = call(z0), call(put(z0, v, 3, 0))
    for name in o0:
        same_bits(o3[name], o0[name], f"{what}: rule 3 - {name} with the plant in an ignored row")
    assert float(o3["dz"][3].abs().max()) == 0.0


# ================================================================================================================
# E. norms and column reductions
# ================================================================================================================
@plants
@dtypes
@pytest.mark.parametrize("shape", [(5, 70), (37, 96)], ids=["scalar", "vector"])
def test_layernorm(dev, dtype, shape, plant):
    """comat_layernorm_fwd / _bwd / _bwd_affine (with and without scratch): the poisoned row's y, statistics and dx are
    non-finite, every other row within the sibling bounds (y tol, dx tol * 2); the affine gradients sum over the rows, so every
    column of dgamma is poisoned (x-hat of the row is), dbeta - a sum of dy alone - is not"""
    k = ops.kernels()
    M, C = shape
    x0 = rnd(M, C, dtype=dtype, seed=1) * 1.5 - 0.4
    gamma, beta = rnd(C, seed=2) * 0.5 + 1, rnd(C, seed=3) * 0.3
    gy, add = rnd(M, C, dtype=dtype, seed=4), rnd(M, C, dtype=dtype, seed=5)
    r = M - 1
    x1 = put(x0, PLANTS[plant], r, C - 1)

    def ref(x):
        xr = x.double().requires_grad_(True)
        g_, b_ = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        y = F.layer_norm(xr, (C,), g_, b_, eps=1e-5)
        y.backward(gy.double())
        return dict(y=y.detach(), dx=xr.grad + add.double(), dgamma=g_.grad, dbeta=b_.grad, dgamma1=g_.grad, dbeta1=b_.grad)

    def call(x):
        xd, gd = dv(x, dev, dtype), dv(gy, dev, dtype)
        y, dx, st = torch.empty_like(xd), torch.empty_like(xd), torch.full((M, 2), NAN, device=dev)
        k.layernorm_fwd(xd, dv(gamma, dev), dv(beta, dev), y, st, M, C, 1e-5)
        k.layernorm_bwd(gd, xd, dv(gamma, dev), st, dx, M, C, add=dv(add, dev, dtype))
        out = dict(y=y.cpu(), dx=dx.cpu(), stats=st.cpu())
        for tag, scratch in (("", True), ("1", False)):
            dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
            k.layernorm_bwd_affine(gd, xd, st, dg, db, M, C, scratch=scratch)
            out["dgamma" + tag], out["dbeta" + tag] = dg.cpu(), db.cpu()
        return out
    row, allc, none = row_mask((M, C), r), torch.ones(C, dtype=torch.bool), torch.zeros(C, dtype=torch.bool)
    dep = dict(y=row, dx=row, dgamma=allc, dbeta=none, dgamma1=allc, dbeta1=none)
    o1 = drive(call, ref, x0, x1, dep, dtype, f"layernorm {shape} {plant}",
               factors=dict(dx=2, dgamma=20, dbeta=20, dgamma1=20, dbeta1=20))
    assert bool(nonfinite(o1["stats"])[r].any()) and not bool(nonfinite(o1["stats"])[:r].any()), "statistics: rules 1 / 2"


def _groupnorm_case(dev, dtype, shape, silu, plant):
    k = ops.kernels()
    B_, HW, C, G = shape
    cpg = C // G
    x0 = rnd(B_, HW, C, dtype=dtype, seed=1) * 2 + 0.7
    gamma, beta = rnd(C, seed=2) * 0.5 + 1, rnd(C, seed=3) * 0.3
    gy, add = rnd(B_ * HW, C, dtype=dtype, seed=4), rnd(B_ * HW, C, dtype=dtype, seed=5)
    b, c = B_ - 1, C - 1
    x1 = put(x0, PLANTS[plant], b, HW - 1, c)

    def ref(x):
        xr = x.double().requires_grad_(True)
        g_, b_ = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        y = F.group_norm(xr.permute(0, 2, 1), G, g_, b_, eps=1e-5).permute(0, 2, 1)
        y = (F.silu(y) if silu else y).reshape(B_ * HW, C)
        y.backward(gy.double())
        return dict(y=y.detach(), dx=xr.grad.reshape(B_ * HW, C) + add.double(), dgamma=g_.grad, dbeta=b_.grad)

    def call(x):
        xd, gd = dv(x.reshape(B_ * HW, C), dev, dtype), dv(gy, dev, dtype)
        y, dx, st = torch.empty_like(xd), torch.empty_like(xd), torch.full((B_, G, 2), NAN, device=dev)
        gm, bt = dv(gamma, dev), dv(beta, dev)
        k.groupnorm_fwd(xd, gm, bt, y, st, B_, HW, C, G, 1e-5, silu)
        k.groupnorm_bwd(gd, xd, gm, bt, st, dx, B_, HW, C, G, silu, add=dv(add, dev, dtype))
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        k.groupnorm_bwd_affine(gd, xd, gm, bt, st, dg, db, B_, HW, C, G, silu)
        return dict(y=y.cpu(), dx=dx.cpu(), stats=st.cpu(), dgamma=dg.cpu(), dbeta=db.cpu())
    unit = torch.zeros(B_, HW, G, cpg, dtype=torch.bool)
    unit[b, :, c // cpg] = True
    unit = unit.reshape(B_ * HW, C)
    chans = torch.zeros(C, dtype=torch.bool)
    chans[c // cpg * cpg:(c // cpg + 1) * cpg] = True
    # dbeta sums dy (times silu'(y-hat) with SiLU, which the poisoned group's y-hat poisons) over samples and positions
    dep = dict(y=unit, dx=unit, dgamma=chans, dbeta=chans if silu else torch.zeros(C, dtype=torch.bool))
    o1 = drive(call, ref, x0, x1, dep, dtype, f"groupnorm {shape} silu={silu} {plant}", factors=dict(dx=2, dgamma=20, dbeta=20))
    g = row_mask((B_, G), b, c // cpg)
    assert bool(nonfinite(o1["stats"])[g].any()) and not bool(nonfinite(o1["stats"])[~g].any()), "statistics: rules 1 / 2"


GN_SHAPES = [(3, 77, 24, 8), (2, 64, 80, 8), (1, 300, 72, 8)]  # C = 80, 72: two column blocks of 64


@plants
@dtypes
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("shape", GN_SHAPES)
def test_groupnorm(dev, dtype, shape, silu, plant):
    """comat_groupnorm_fwd / _bwd / _bwd_affine: one (sample, group) is poisoned - y, dx, its statistics, its channels of
    dgamma (and of dbeta with SiLU); every other group and channel within the sibling bounds"""
    _groupnorm_case(dev, dtype, shape, silu, plant)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("shape", GN_SHAPES[:2])
def test_groupnorm_variants(hip, mode, shape, default_opts):
    """every norm_fused mode, a NaN plant, bf16 and fp32"""
    _set_opts(norm_fused=mode)
    for dtype in DTYPES:
        _groupnorm_case(hip, dtype, shape, True, "nan")


@plants
@dtypes
def test_colsum(dev, dtype, plant):
    """comat_colsum / comat_colsum_batched at a padded leading dimension: the plant's column (of its sample) is poisoned, every
    other column is finite and within the bias gradient's bound"""
    k = ops.kernels()
    B_, M, C, ld = 2, 37, 72, 80
    x0 = rnd(B_ * M, ld, dtype=dtype, seed=1)
    r, c = B_ * M - 1, C - 1
    x1 = put(x0, PLANTS[plant], r, c)

    def ref(x):
        v = x[:, :C].double()
        return dict(one=v.sum(0), per=v.reshape(B_, M, C).sum(1))

    def call(x):
        xd = dv(x, dev, dtype)
        one, per = torch.zeros(C, device=dev), torch.full((B_, C), NAN, device=dev)
        k.colsum(xd, one, B_ * M, C, ld)
        k.colsum_batched(xd, per, B_, M, C, ld)
        return dict(one=one.cpu(), per=per.cpu())
    dep = dict(one=row_mask((C,), c), per=row_mask((B_, C), B_ - 1, c))
    drive(call, ref, x0, x1, dep, dtype, f"colsum {plant}", factors=dict(one=5, per=5))
    pad = put(x0, PLANTS[plant], 0, C)  # rule 3: a pad column beyond C is not part of the operand
    o0, o3 = call(x0), call(pad)
    for name in o0:
        same_bits(o3[name], o0[name], f"colsum: rule 3 - {name} with the plant in a pad column")


# ================================================================================================================
# F. the tail
# ================================================================================================================
TAIL = [(n, p) for n in (5, 1027) for p in sorted({0, n - 1})]
tail = pytest.mark.parametrize("n,pos", TAIL, ids=[f"n{n}-at{p}" for n, p in TAIL])


@plants
@tail
def test_sumsq_and_grad_norm(dev, n, pos, plant):
    """comat_sumsq is non-finite for each plant (it is what the optimizer's skip reads), and so is the norm of
    comat_grad_norm_scale; the rescaled gradient follows the definition g * target / |g|: NaN everywhere under a NaN norm,
    0 (and the planted element NaN) under an infinite one"""
    k = ops.kernels()
    g0 = rnd(n, seed=n)
    g1 = put(g0, PLANTS[plant], pos)

    def call(g):
        gd = dv(g, dev)
        ssq, norm, out = torch.zeros(1, device=dev), torch.zeros(1, device=dev), torch.full((n,), 7.0, device=dev)
        k.sumsq(gd, n, ssq)
        k.grad_norm_scale(gd, out, n, norm, 2.0)
        return dict(sumsq=ssq.cpu(), norm=norm.cpu(), scaled=out.cpu())

    def ref(g):
        nrm = g.double().pow(2).sum().sqrt()
        return dict(sumsq=g.double().pow(2).sum().reshape(1), norm=nrm.reshape(1), scaled=g.double() * (2.0 / nrm))
    one = torch.ones(1, dtype=torch.bool)
    dep = dict(sumsq=one, norm=one, scaled=torch.ones(n, dtype=torch.bool) if plant == "nan" else row_mask((n,), pos))
    drive(call, ref, g0, g1, dep, F32, f"sumsq / grad_norm_scale n={n} {plant} at {pos}", factors=dict(sumsq=5, norm=5))


@plants
@tail
@dtypes
def test_elementwise(dev, dtype, n, pos, plant):
    """comat_axpby, comat_unary (SiLU, GELU, affine) and their backward, comat_geglu_fwd / _bwd: elementwise - the planted
    element (for GEGLU its pair) is what the fp64 definition makes of it, every other one is within the sibling bound"""
    from sim_backend import UN_AFFINE, UN_GELU, UN_SILU
    k = ops.kernels()
    x0, y0, g0 = rnd(n, dtype=dtype, seed=1), rnd(n, dtype=dtype, seed=2), rnd(n, dtype=dtype, seed=3)
    x1 = put(x0, PLANTS[plant], pos)
    acts = {UN_SILU: F.silu, UN_GELU: F.gelu}

    def ref(x):
        x = x.double()
        out = dict(axpby=0.5 * x - 1.5 * y0.double(), affine=2.0 * x + 0.25)
        for op, f in acts.items():
            xr = x.clone().requires_grad_(True)
            y = f(xr)
            y.backward(g0.double())
            out[f"act{op}"], out[f"dact{op}"] = y.detach(), xr.grad
        return out

    def call(x):
        xd, yd, gd = dv(x, dev, dtype), dv(y0, dev, dtype), dv(g0, dev, dtype)
        out = {}
        new = lambda: torch.full((n,), NAN, dtype=dtype, device=dev)
        out["axpby"] = new()
        k.axpby(0.5, xd, -1.5, yd, out["axpby"], n)
        out["affine"] = new()
        k.unary(UN_AFFINE, xd, out["affine"], n, 2.0, 0.25)
        for op in acts:
            out[f"act{op}"], out[f"dact{op}"] = new(), new()
            k.unary(op, xd, out[f"act{op}"], n)
            k.unary_bwd(op, gd, xd, out[f"dact{op}"], n)
        return {name: t.cpu() for name, t in out.items()}
    r1 = ref(x1)
    for name, t in r1.items():  # CPU precondition: nothing but the planted element may depend on it
        assert not bool((~torch.isfinite(t))[torch.arange(n) != pos].any()), name
    # the dependent set: the planted element of every output under a NaN, of the two linear ones under +-Inf; an activation or
    # its derivative may have a finite limit at +-Inf (gelu'(+inf) = 1): there the fp64 reference says which, confined to `pos`
    at = row_mask((n,), pos)
    dep = {name: at if plant == "nan" or name in ("axpby", "affine") else ~torch.isfinite(t) for name, t in r1.items()}
    for name in dep:
        depends(r1[name], dep[name], name)
    r0, o0, o1, o2 = ref(x0), call(x0), call(x1), None
    for name in r0:
        depends(r0[name], None, name)
        carried_contained(o0[name], r0[name], dtype, f"clean {name}")
        carried_contained(o1[name], r1[name], dtype, f"{name} n={n} {plant} at {pos}")
    o2 = call(x0)
    for name in o0:
        same_bits(o2[name], o0[name], f"rule 4 - {name}")


@plants
@dtypes
@pytest.mark.parametrize("layout", ["plain", "interleaved"])
def test_geglu(dev, dtype, layout, plant):
    """comat_geglu_fwd / _bwd, x [M, 2 D] = (value | gate), and comat_geglu_il_fwd / _bwd, value and gate columns interleaved in
    sixteens: a plant in the last gate of the last row poisons its pair's output and both gradients of the pair"""
    k = ops.kernels()
    il = layout == "interleaved"
    M, D = (5, 48) if il else (5, 13)
    x0, g0 = rnd(M, 2 * D, dtype=dtype, seed=1), rnd(M, D, dtype=dtype, seed=2)
    cv, cg = (2 * D - 17, 2 * D - 1) if il else (D - 1, 2 * D - 1)  # the columns of the last pair's value and gate
    x1 = put(x0, PLANTS[plant], M - 1, cg)

    def ref(x):
        xr = x.double().requires_grad_(True)
        if il:
            t = xr.reshape(M, D // 16, 2, 16)
            y = (t[:, :, 0] * F.gelu(t[:, :, 1])).reshape(M, D)
        else:
            y = xr[:, :D] * F.gelu(xr[:, D:])
        y.backward(g0.double())
        return dict(y=y.detach(), dx=xr.grad)

    def call(x):
        xd = dv(x, dev, dtype)
        y, dx = torch.full((M, D), NAN, dtype=dtype, device=dev), torch.full((M, 2 * D), NAN, dtype=dtype, device=dev)
        (k.geglu_il_fwd if il else k.geglu_fwd)(xd, y, M, D)
        (k.geglu_il_bwd if il else k.geglu_bwd)(dv(g0, dev, dtype), xd, dx, M, D)
        return dict(y=y.cpu(), dx=dx.cpu())
    r1 = ref(x1)
    # y of the pair; d value = dy gelu(gate) and d gate = dy value gelu'(gate) - both under a NaN; under +-Inf gelu' has a finite
    # limit, so d gate is taken from the reference
    pair = row_mask((M, 2 * D), M - 1, cv) | row_mask((M, 2 * D), M - 1, cg)
    dep = dict(y=row_mask((M, D), M - 1, D - 1), dx=pair if plant == "nan" else ~torch.isfinite(r1["dx"]))
    assert not bool((dep["dx"] & ~pair).any()) and bool(dep["dx"][M - 1, cv])
    drive(call, ref, x0, x1, dep, dtype, f"geglu {layout} {plant}")


# ---- F, continued: the sampler's kernels, the image path, the loss heads --------------------------------------------------------
SAMPLER = dict(s=7.5, cx=0.93, ce=-0.21, sg=0.05, px=1.1, pe=-0.4, phi=0.7)


@plants
@tail
@dtypes
def test_cfg_ddpm_and_add_noise(dev, dtype, n, pos, plant):
    """comat_cfg_ddpm_fwd / _bwd and comat_add_noise_fwd: elementwise - a plant in the conditional half of eps2 (in the upstream
    gradient; in the noise) reaches element `pos` of every output and nothing else"""
    k = ops.kernels()
    c = SAMPLER
    x, z, g0 = rnd(n, seed=1), rnd(n, seed=2), rnd(n, seed=4)
    e0 = rnd(2 * n, dtype=dtype, seed=3)
    v = PLANTS[plant]
    clean, poisoned = dict(e=e0, g=g0), dict(e=put(e0, v, n + pos), g=put(g0, v, pos))

    def ref(t):
        e, g = t["e"].double(), t["g"].double()
        return dict(x_prev=c["cx"] * x.double() + c["ce"] * (e[:n] + c["s"] * (e[n:] - e[:n])) + c["sg"] * z.double(),
                    dx=c["cx"] * g, deps=torch.cat([c["ce"] * (1 - c["s"]) * g, c["ce"] * c["s"] * g]),
                    noisy=0.8 * x.double() + 0.6 * e[n:], xin=(0.8 * x.double() + 0.6 * e[n:]).repeat(2))

    def call(t):
        ed, gd, xd = dv(t["e"], dev, dtype), dv(t["g"], dev), dv(x, dev)
        o, dx, de = torch.full((n,), NAN, device=dev), torch.full((n,), NAN, device=dev), torch.full((2 * n,), NAN, dtype=dtype, device=dev)
        k.cfg_ddpm_fwd(xd, ed, dv(z, dev), o, n, c["s"], c["cx"], c["ce"], c["sg"])
        k.cfg_ddpm_bwd(gd, dx, de, n, c["s"], c["cx"], c["ce"])
        noisy, xin = torch.full((n,), NAN, device=dev), torch.full((2 * n,), NAN, dtype=dtype, device=dev)
        k.add_noise_fwd(xd, ed[n:].float().contiguous(), noisy, xin, n, 0.8, 0.6, 2)
        return dict(x_prev=o.cpu(), dx=dx.cpu(), deps=de.cpu(), noisy=noisy.cpu(), xin=xin.cpu())
    at, at2 = row_mask((n,), pos), row_mask((n,), pos).repeat(2)
    drive(call, ref, clean, poisoned, dict(x_prev=at, dx=at, deps=at2, noisy=at, xin=at2), dtype, f"cfg_ddpm / add_noise n={n} {plant} at {pos}")


@plants
@dtypes
@pytest.mark.parametrize("kernel", ["cfg_rescale", "step2"])
def test_rescaled_guidance(dev, dtype, kernel, plant):
    """comat_cfg_rescale_ddpm_* and comat_ddpm_step2_* with phi > 0: the per-sample statistics (means and squared deviations of
    the conditional and the guided prediction) couple the elements of a SAMPLE.  A plant in the second sample's eps: its four
    statistics and its whole x_prev (x0) are non-finite, the first sample's are within tol; a plant in the upstream gradient
    of the second sample: its own dx element, and - through D = sum d e - the sample's whole deps"""
    k = ops.kernels()
    c = SAMPLER
    batch, P = 2, 516  # P % 4 == 0, more than one 256-wide pass per sample
    n = batch * P
    x, z, g0 = rnd(n, seed=1), rnd(n, seed=2), rnd(n, seed=4)
    e0 = rnd(2 * n, dtype=dtype, seed=3)
    v = PLANTS[plant]
    clean, poisoned = dict(e=e0, g=g0), dict(e=put(e0, v, 2 * n - 1), g=put(g0, v, n - 1))

    def ref(t):
        er = t["e"].double().requires_grad_(True)
        eu, ec = er[:n].reshape(batch, P), er[n:].reshape(batch, P)
        eg = eu + c["s"] * (ec - eu)
        mu_t, mu_c = ec.mean(1, keepdim=True), eg.mean(1, keepdim=True)
        V_t, V_c = ((ec - mu_t) ** 2).sum(1, keepdim=True), ((eg - mu_c) ** 2).sum(1, keepdim=True)
        kk = c["phi"] * torch.sqrt(V_t / V_c) + (1 - c["phi"])
        xp = c["cx"] * x.double() + c["ce"] * (kk * eg).reshape(-1) + c["sg"] * z.double()
        out = dict(x_prev=xp.detach(), stats=torch.cat([mu_t, V_t, mu_c, V_c], 1).detach())
        # the backward of the CLEAN forward's graph under the (possibly poisoned) upstream gradient - as the kernel, which reads eps
        er0 = e0.double().requires_grad_(True)
        eu0, ec0 = er0[:n].reshape(batch, P), er0[n:].reshape(batch, P)
        eg0 = eu0 + c["s"] * (ec0 - eu0)
        k0 = c["phi"] * (ec0.std(1, keepdim=True) / eg0.std(1, keepdim=True)) + (1 - c["phi"])
        (c["ce"] * (k0 * eg0).reshape(-1)).backward(t["g"].double())
        out.update(dx=c["cx"] * t["g"].double(), deps=er0.grad)
        return out

    def call(t):
        ed, gd, xd, zd = dv(t["e"], dev, dtype), dv(t["g"], dev), dv(x, dev), dv(z, dev)
        e0d = dv(e0, dev, dtype)
        new = lambda m, dt_=F32: torch.full((m,), NAN, dtype=dt_, device=dev)
        o, dx, de, st, st0 = new(n), new(n), new(2 * n, dtype), new(4 * batch), new(4 * batch)
        if kernel == "cfg_rescale":
            k.cfg_rescale_ddpm_fwd(xd, ed, zd, o, n, c["s"], c["cx"], c["ce"], c["sg"], c["phi"], batch, P, st)
            k.cfg_rescale_ddpm_fwd(xd, e0d, zd, new(n), n, c["s"], c["cx"], c["ce"], c["sg"], c["phi"], batch, P, st0)
            k.cfg_rescale_ddpm_bwd(gd, e0d, st0, dx, de, n, c["s"], c["cx"], c["ce"], c["phi"], batch, P)
        else:
            k.ddpm_step2_fwd(xd, ed, zd, o, None, n, 2, c["s"], c["cx"], c["ce"], c["sg"], c["px"], c["pe"], c["phi"], batch, P, st)
            k.ddpm_step2_fwd(xd, e0d, zd, new(n), None, n, 2, c["s"], c["cx"], c["ce"], c["sg"], c["px"], c["pe"], c["phi"], batch, P, st0)
            k.ddpm_step2_bwd(gd, None, e0d, st0, dx, de, n, 2, c["s"], c["cx"], c["ce"], c["px"], c["pe"], c["phi"], batch, P)
        return dict(x_prev=o.cpu(), stats=st.cpu().reshape(batch, 4), dx=dx.cpu(), deps=de.cpu())
    second = torch.zeros(batch, P, dtype=torch.bool)
    second[1] = True
    dep = dict(x_prev=second.reshape(-1), stats=row_mask((batch, 4), 1), dx=row_mask((n,), n - 1), deps=second.reshape(-1).repeat(2))
    drive(call, ref, clean, poisoned, dep, dtype, f"{kernel} {plant}", factors=dict(stats=5, deps=3))
    if kernel == "step2":  # rule 3 - "without deps (an untrained step) eps and stats are not read": a plant in either changes no bit of dx
        st0 = torch.full((4 * batch,), NAN, device=dev)
        k.ddpm_step2_fwd(dv(x, dev), dv(e0, dev, dtype), dv(z, dev), torch.empty(n, device=dev), None, n, 2, c["s"], c["cx"], c["ce"], c["sg"],
                         c["px"], c["pe"], c["phi"], batch, P, st0)

        def only_dx(e, st):
            dx = torch.full((n,), NAN, device=dev)
            k.ddpm_step2_bwd(dv(g0, dev), None, dv(e, dev, dtype), st, dx, None, n, 2, c["s"], c["cx"], c["ce"], c["px"], c["pe"], c["phi"],
                             batch, P, eps_dtype=dtype)
            return dx.cpu()
        want = only_dx(e0, st0)
        carried_contained(want, c["cx"] * g0.double(), F32, "step2 dx alone")
        same_bits(only_dx(put(e0, v, 2 * n - 1), st0), want, "step2: rule 3 - eps is read although deps is NULL")
        same_bits(only_dx(e0, put(st0.cpu(), v, 4 * batch - 1).to(dev)), want, "step2: rule 3 - stats are read although deps is NULL")


@plants
@dtypes
def test_patchify_and_embedding(dev, dtype, plant):
    """comat_patchify (both directions) and comat_embedding move values: the plant arrives where the permutation (the ids) put
    it, every other element keeps its bits; a table row that no id names is not read"""
    k = ops.kernels()
    B_, H, W, C, P = 2, 8, 12, 3, 4
    img0 = rnd(B_ * H * W, C, dtype=dtype, seed=3)
    vocab, dim, n = 9, 7, 13
    ids = torch.randint(0, vocab - 1, (n,), generator=torch.Generator().manual_seed(n))  # (row vocab - 1 is never named)
    ids[0], ids[-1] = 3, 3
    tab0 = rnd(vocab, dim, dtype=dtype, seed=5)
    v = PLANTS[plant]
    clean = dict(img=img0, tab=tab0)
    poisoned = dict(img=put(img0, v, B_ * H * W - 1, C - 1), tab=put(tab0, v, 3, dim - 1))
    perm = lambda t: t.reshape(B_, H // P, P, W // P, P, C).permute(0, 1, 3, 2, 4, 5).reshape(B_ * (H // P) * (W // P), P * P * C)

    def ref(t):
        return dict(patches=perm(t["img"].double()), back=t["img"].double(), emb=t["tab"].double()[ids])

    def call(t):
        imgd = dv(t["img"], dev, dtype)
        patches = torch.full((B_ * (H // P) * (W // P), P * P * C), NAN, dtype=dtype, device=dev)
        back = torch.full((B_ * H * W, C), NAN, dtype=dtype, device=dev)
        k.patchify(imgd, patches, B_, H, W, C, P, False)
        k.patchify(back, patches, B_, H, W, C, P, True)
        emb = torch.full((n, dim), NAN, dtype=dtype, device=dev)
        k.embedding(dv(ids, dev), dv(t["tab"], dev, dtype), emb, n, dim, vocab)
        return dict(patches=patches.cpu(), back=back.cpu(), emb=emb.cpu())
    dep_img = row_mask((B_ * H * W, C), B_ * H * W - 1, C - 1)
    dep = dict(patches=perm(dep_img), back=dep_img, emb=(ids == 3)[:, None] & row_mask((1, dim), 0, dim - 1))
    assert int(dep["emb"].sum()) >= 2
    o1 = drive(call, ref, clean, poisoned, dep, dtype, f"patchify / embedding {plant}")
    o0 = call(clean)
    for name in o0:  # moves: bit-equal outside the plant
        same_bits(o1[name][~dep[name]], o0[name][~dep[name]], f"{name}: rule 2 - bits outside the plant")
    o3 = call(dict(clean, tab=put(tab0, v, vocab - 1, 0)))
    same_bits(o3["emb"], o0["emb"], "embedding: rule 3 - a table row that no id names is read")


@plants
@dtypes
def test_resample2d(dev, dtype, plant):
    """comat_resample2d (bicubic, antialias, crop) with scale and shift: a plant in one source pixel and channel reaches the output
    pixels whose row AND column windows hold it with a non-zero weight, in that channel of that sample - the set is read off the
    tables on the CPU; a plant outside the crop is not read"""
    from comat_amd.resize import resize_tables
    k = ops.kernels()
    B_, C, Hf, size, crop = 2, 3, 20, (8, 8), (2, 3, 15, 14)
    img0 = rnd(B_ * Hf * Hf, C, dtype=dtype, seed=1)
    fwd, bwd = resize_tables(Hf, Hf, crop, size, "bicubic")
    tab = ops.ResampleTables(fwd, bwd, Hf, Hf, size[0], size[1], dev)
    t = tab.fwd
    KT = int(t["KT"])
    scale, shift = torch.tensor([2.0, 0.5, 1.5]), torch.tensor([0.1, -0.2, 0.3])

    def dense(start, wt, n_out, n_in):
        Mx = torch.zeros(n_out, n_in, dtype=F64)
        for o in range(n_out):
            for j in range(KT):
                i = int(start[o]) + j
                if 0 <= i < n_in:
                    Mx[o, i] += float(wt[o, j])
        return Mx
    Wy = dense(t["ystart"].cpu(), t["ywt"].cpu().reshape(size[0], KT), size[0], Hf)
    Wx = dense(t["xstart"].cpu(), t["xwt"].cpu().reshape(size[1], KT), size[1], Hf)
    py, px = crop[0] + crop[2] // 2, crop[1] + crop[3] // 2  # a pixel in the middle of the crop
    assert bool((Wy[:, py] != 0).any()) and bool((Wx[:, px] != 0).any())
    unread = [(yy, xx) for yy in range(Hf) for xx in range(Hf) if not bool((Wy[:, yy] != 0).any()) or not bool((Wx[:, xx] != 0).any())]
    assert unread, "the crop leaves no pixel unread - a broken case"

    def ref(img):
        x = img.double().reshape(B_, Hf, Hf, C)
        dead_y, dead_x = ~(Wy != 0).any(0), ~(Wx != 0).any(0)  # rows / columns no window reads: not part of the operand
        x = x.clone()
        x[:, dead_y] = 0
        x[:, :, dead_x] = 0
        # a window position of weight 0 is no tap (the tables pad every window to KT entries): a non-finite pixel contributes
        # weight * value where the weight is not 0 and nothing where it is - not 0 * NaN
        bad = ~torch.isfinite(x)
        y = torch.einsum("pw,bowc->bopc", Wx, torch.einsum("oh,bhwc->bowc", Wy, x.masked_fill(bad, 0.0)))
        for bb, yy, xx, cc in torch.nonzero(bad).tolist():
            w2 = Wy[:, yy, None] * Wx[None, :, xx]
            y[bb, :, :, cc] += torch.where(w2 != 0, w2 * x[bb, yy, xx, cc], torch.zeros_like(w2))
        return dict(out=(y * scale.double() + shift.double()).reshape(-1, C))

    def call(img):
        out_ = torch.full((B_ * size[0] * size[1], C), NAN, dtype=dtype, device=dev)
        k.resample2d(dv(img, dev, dtype), out_, B_, Hf, Hf, size[0], size[1], C, t["ystart"], t["ywt"], t["xstart"], t["xwt"], t["KT"],
                     dv(scale, dev), dv(shift, dev))
        return dict(out=out_.cpu())
    dep = torch.zeros(B_, size[0], size[1], C, dtype=torch.bool)
    dep[1, :, :, C - 1] = (Wy[:, py] != 0)[:, None] & (Wx[:, px] != 0)[None, :]
    img1 = put(img0, PLANTS[plant], (1 * Hf + py) * Hf + px, C - 1)
    drive(call, ref, img0, img1, dict(out=dep.reshape(-1, C)), dtype, f"resample2d {plant}")
    yy, xx = unread[0]
    same_bits(call(put(img0, PLANTS[plant], yy * Hf + xx, 0))["out"], call(img0)["out"], "resample2d: rule 3 - a pixel outside every window is read")


@plants
@dtypes
def test_attnmap_gather(dev, dtype, plant):
    """comat_attnmap_gather_fwd / _bwd: a plant in the attention map at (head, pixel, a gathered token column) reaches num and
    den of that (head, token) and avg of that (token, pixel); a column no token names is not read.  Backward: a plant in
    g_num[head, token] reaches dA[head, :, that token's column]"""
    k = ops.kernels()
    h, npix, L = 3, 70, 77
    a0 = rnd(h, npix, L, dtype=dtype, seed=1).abs()
    mask = (rnd(2, npix, seed=2) > 0).float()
    tok_idx = torch.tensor([2, 0, 6, 76, 3], dtype=torch.int32)
    tok_obj = torch.tensor([0, 0, 1, 1, 1], dtype=torch.int32)
    nt = 5
    gn0, gd, ga = rnd(h, nt, seed=3), rnd(h, nt, seed=4), rnd(nt, npix, seed=5)
    v = PLANTS[plant]
    hh, pp, tt = h - 1, npix - 1, 3  # token 3 reads column 76
    clean = dict(a=a0, gn=gn0)
    poisoned = dict(a=put(a0, v, hh, pp, 76), gn=put(gn0, v, hh, tt))
    m = mask.double()[tok_obj.long()]

    def ref(t):
        sel = t["a"].double()[:, :, tok_idx.long()]
        g = t["gn"].double()[:, None, :] * m.t()[None] + gd.double()[:, None, :] + ga.double().t()[None] / h
        d = torch.zeros(h, npix, L, dtype=F64)
        d[:, :, tok_idx.long()] = g
        return dict(num=torch.einsum("hpt,tp->ht", sel, m), den=sel.sum(1), avg=sel.mean(0).t(), dA=d)

    def call(t):
        ad, md, ti, to = dv(t["a"], dev, dtype), dv(mask, dev), dv(tok_idx, dev), dv(tok_obj, dev)
        num, den, avg = torch.zeros(h, nt, device=dev), torch.zeros(h, nt, device=dev), torch.zeros(nt, npix, device=dev)
        k.attnmap_gather_fwd(ad, md, ti, to, num, den, avg, h, npix, L, nt)
        dA = torch.full((h, npix, L), NAN, dtype=dtype, device=dev)
        k.attnmap_gather_bwd(dv(t["gn"], dev), dv(gd, dev), dv(ga, dev), md, ti, to, dA, h, npix, L, nt)
        return dict(num=num.cpu(), den=den.cpu(), avg=avg.cpu(), dA=dA.cpu())
    dA_dep = torch.zeros(h, npix, L, dtype=torch.bool)
    dA_dep[hh, :, 76] = True
    dep = dict(num=row_mask((h, nt), hh, tt), den=row_mask((h, nt), hh, tt), avg=row_mask((nt, npix), tt, pp), dA=dA_dep)
    drive(call, ref, clean, poisoned, dep, dtype, f"attnmap_gather {plant}", factors=dict(num=5, den=5, avg=5))
    o0, o3 = call(clean), call(dict(clean, a=put(a0, v, 0, 0, 50)))  # column 50: no token
    for name in o0:
        same_bits(o3[name], o0[name], f"attnmap_gather: rule 3 - {name} with the plant in a column no token names")


@plants
@dtypes
def test_disc_heads(dev, dtype, plant):
    """comat_disc_head_* (Linear(4, 1) + BCE) and comat_disc_convhead_* (3 x 3 conv to one channel + BCE): the loss is a mean
    over all pixels - non-finite; dx of the planted pixel (conv head: of the 3 x 3 pixels around it) and every weight gradient
    are non-finite, dx of every other pixel is within the sibling bound"""
    k = ops.kernels()
    v = PLANTS[plant]
    # ---- the linear head
    P, pps = 1027, 514
    x0, w, b = rnd(P, 4, dtype=dtype, seed=1), rnd(4, seed=2), rnd(1, seed=3)
    target = torch.tensor([0.0, 1.0])
    tfull = target.double().repeat_interleave(pps)[:P]

    def ref(x):
        xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
        loss = F.binary_cross_entropy_with_logits(xr @ wr + br, tfull)
        zz = (xr @ wr + br).detach()
        dz = 1.7 * (torch.sigmoid(zz) - tfull) / P  # (the definition; autograd's BCE backward clamps differently at +-Inf)
        return dict(loss=loss.detach().reshape(1), dx=dz[:, None] * w.double()[None], dwb=torch.cat([dz @ x.double(), dz.sum().reshape(1)]))

    def call(x):
        xd, wd, bd, td = dv(x, dev, dtype), dv(w, dev), dv(b, dev), dv(target, dev)
        loss, dx, dwb = torch.full((1,), NAN, device=dev), torch.full((P, 4), NAN, dtype=dtype, device=dev), torch.zeros(5, device=dev)
        k.disc_head_fwd(xd, wd, bd, td, loss, P, pps)
        k.disc_head_bwd(xd, wd, bd, td, torch.tensor([1.7], device=dev), dx, dwb, P, pps)
        return dict(loss=loss.cpu(), dx=dx.cpu(), dwb=dwb.cpu())
    p = P - 1
    one = torch.ones(1, dtype=torch.bool)
    assert float(tfull[p]) == 1.0 and float(w[3]) != 0.0
    # z[p] = NaN: the loss, dz[p] and with it dx[p] and every weight gradient.  z[p] = +-Inf: the loss of a pixel with target 1 is
    # max(z, 0) - z + log1p(exp(-|z|)) = inf - inf or +inf, sigmoid saturates and dz[p] is finite - dx is finite everywhere, and of
    # the weight gradients only dw[3] = sum dz x[:, 3] meets the Inf
    if plant == "nan":
        dep = dict(loss=one, dx=row_mask((P, 4), p), dwb=torch.ones(5, dtype=torch.bool))
    else:
        dep = dict(loss=one, dx=torch.zeros(P, 4, dtype=torch.bool), dwb=row_mask((5,), 3))
    drive(call, ref, x0, put(x0, v, p, 3), dep, dtype, f"disc_head {plant}", factors=dict(loss=5, dwb=20))
    # ---- the conv head: forward, then the backward from the forward's z (or from a z with a plant of its own)
    B_, H, W, C = 2, 5, 7, 8
    Pc = B_ * H * W
    xc0, wc, bc = rnd(Pc, C, dtype=dtype, seed=4), rnd(9, C, seed=5) * 0.3, rnd(1, seed=6)
    tc = torch.tensor([0.0, 1.0])
    wconv = wc.double().reshape(3, 3, C).permute(2, 0, 1).unsqueeze(0)
    pz = (1 * H + 2) * W + 3  # an interior pixel of sample 1 for the plant in z

    def cref(t):
        x = t["x"].double()
        xi = x.reshape(B_, H, W, C).permute(0, 3, 1, 2)
        zz = F.conv2d(xi, wconv, bc.double(), padding=1).reshape(B_, H * W)
        loss = F.binary_cross_entropy_with_logits(zz, tc.double()[:, None].expand(B_, H * W)).reshape(1)
        zb = zz.reshape(-1).clone()
        if t["z"] is not None:
            zb[pz] = t["z"]
        dz = (1.7 / Pc * (torch.sigmoid(zb.reshape(B_, H * W)) - tc.double()[:, None])).reshape(B_, 1, H, W)
        dx = F.conv_transpose2d(dz, wconv, padding=1).permute(0, 2, 3, 1).reshape(Pc, C)
        # dw[tap, c] = sum over pixels of dz[p] x[p + tap, c], a tap outside the image is no term; non-finite x elements one by one
        bad = ~torch.isfinite(xi)
        dw = torch.nn.grad.conv2d_weight(xi.masked_fill(bad, 0.0), wconv.shape, dz, padding=1)[0].permute(1, 2, 0).contiguous()  # [3, 3, C]
        for b, c, hi, wi in torch.nonzero(bad).tolist():
            for ky in range(3):
                for kx in range(3):
                    ho, wo = hi + 1 - ky, wi + 1 - kx
                    if 0 <= ho < H and 0 <= wo < W:
                        dw[ky, kx, c] += dz[b, 0, ho, wo] * xi[b, c, hi, wi]
        return dict(z=zz.reshape(-1), loss=loss, dx=dx, dwb=torch.cat([dw.reshape(-1), dz.sum().reshape(1)]).masked_fill(open_w[0], 0.0))

    def ccall(t):
        xd, wd, td = dv(t["x"], dev, dtype), dv(wc, dev), dv(tc, dev)
        z, loss = torch.full((Pc,), NAN, device=dev), torch.full((1,), NAN, device=dev)
        k.disc_convhead_fwd(xd, wd, dv(bc, dev), td, z, loss, B_, H, W, C)
        zb = z.clone()
        if t["z"] is not None:
            zb[pz] = t["z"]
        dx, dwb = torch.full((Pc, C), NAN, dtype=dtype, device=dev), torch.zeros(9 * C + 1, device=dev)
        k.disc_convhead_bwd(xd, wd, zb, td, torch.tensor([1.7], device=dev), dx, dwb, B_, H, W, C)
        return dict(z=z.cpu(), loss=loss.cpu(), dx=dx.cpu(), dwb=dwb.cpu().masked_fill(open_w[0], 0.0))
    open_w = [torch.zeros(9 * C + 1, dtype=torch.bool)]  # elements of dwb left out of the comparison (below)
    img = lambda: torch.zeros(B_, H, W, dtype=torch.bool)
    near, block, around = img(), img(), img()
    near[1, H - 2:, W - 2:] = True    # the 2 x 2 pixels whose 3 x 3 window holds the corner pixel (H - 1, W - 1) of sample 1
    block[1, H - 3:, W - 3:] = True   # the pixels within one step of those
    around[1, 1:4, 2:5] = True        # the 3 x 3 pixels round the plant in z
    none_x, all_w = torch.zeros(Pc, C, dtype=torch.bool), torch.ones(9 * C + 1, dtype=torch.bool)
    px = lambda m: m.reshape(Pc, 1).expand(Pc, C)
    clean = dict(x=xc0, z=None)
    # (a) the plant in x (the corner pixel, channel C - 1): z of the four near pixels, the loss (target 1: as the linear head).
    #     NaN: dz of those four - dx of the block round them and every weight gradient (pixel (H - 2, W - 2) has all nine
    #     neighbours inside the image).  +-Inf: dz is finite - dx finite, and only dw[ky, kx, C - 1] of the four taps ky, kx in
    #     {1, 2} under which a pixel of the image sees the corner.  Under the other five taps the corner would meet a pixel
    #     OUTSIDE the image: whether that product (0 * Inf) is formed is not settled by the definition (test_conv2d_wgrad has the
    #     same question and torch's two answers); the kernel forms it, the header says it may - those five elements are left open
    if plant == "nan":
        dep = dict(z=near.reshape(-1), loss=one, dx=px(block), dwb=all_w)
    else:
        taps = torch.zeros(3, 3, C, dtype=torch.bool)
        taps[1:, 1:, C - 1] = True
        dep = dict(z=near.reshape(-1), loss=one, dx=none_x, dwb=torch.cat([taps.reshape(-1), torch.zeros(1, dtype=torch.bool)]))
        other = torch.zeros(3, 3, C, dtype=torch.bool)
        other[:, :, C - 1] = True
        open_w[0] = torch.cat([(other & ~taps).reshape(-1), torch.zeros(1, dtype=torch.bool)])
    drive(ccall, cref, clean, dict(x=put(xc0, v, Pc - 1, C - 1), z=None), dep, dtype, f"disc_convhead {plant} in x",
          factors=dict(z=5, loss=5, dwb=20))
    # (b) the plant in the z the backward reads: NaN poisons dx of the 3 x 3 pixels round it and every weight gradient; +-Inf
    #     saturates the sigmoid - nothing is non-finite
    open_w[0] = torch.zeros(9 * C + 1, dtype=torch.bool)
    no_z, no_l = torch.zeros(Pc, dtype=torch.bool), torch.zeros(1, dtype=torch.bool)
    if plant == "nan":
        dep = dict(z=no_z, loss=no_l, dx=px(around), dwb=all_w)
    else:
        dep = dict(z=no_z, loss=no_l, dx=none_x, dwb=torch.zeros(9 * C + 1, dtype=torch.bool))
    drive(ccall, cref, clean, dict(x=xc0, z=v), dep, dtype, f"disc_convhead {plant} in z", factors=dict(z=5, loss=5, dwb=20))


# ================================================================================================================
# G. the step
# ================================================================================================================
@pytest.fixture
def fp8_dev(dev):
    from helpers import fp8_state
    with fp8_state():
        yield dev


STEP_KW = dict(training_steps=[1, 2], crop=(1, 0, 63, 63), attrcon_steps=[2])
SCALINGS = {"jit": ("jit", None), "delayed": ("delayed", None), "delayed-history": ("delayed", dict(history=4, margin=1.25))}


def _logs(logs):
    return {key: v.detach().cpu().clone() for key, v in logs.items() if torch.is_tensor(v)}


def _step_world(dev, scaling, recipe):
    from test_fp8 import _fp8_step_world
    ops.set_fp8_scaling(scaling)
    if recipe is not None:
        ops.set_fp8_recipe(**recipe)
    trainer, bank, batch, _, _ = _fp8_step_world(dev, F32)
    if scaling == "delayed":
        assert trainer.fp8_calibrate(batch)
    return trainer, bank, batch


def _trainer_state(trainer, bank):
    """what a skipped update must leave as it was: LoRA factors, moments, the applied counter"""
    return dict(flat=bank.flat.detach().cpu().clone(), m=[t.cpu().clone() for t in trainer.opt.m], v=[t.cpu().clone() for t in trainer.opt.v],
                applied=int(trainer.opt.counters[0]), skipped=int(trainer.opt.counters[1]))


def _site_state(dev):
    from comat_amd import fp8
    st = fp8.fp8_state(dev)
    return {key: getattr(st, key)[:st.n].cpu().clone() for key in ("scale", "hist", "count", "amax")}, st.n


@pytest.mark.parametrize("how", ["batch", "mid-network"])
@pytest.mark.parametrize("scaling", list(SCALINGS))
def test_poisoned_step_is_skipped_and_leaves_no_trace(fp8_dev, scaling, how):
    """C5 in miniature (test_fp8._fp8_step_world): a clean step, a step with ONE NaN - planted in the batch's latents, or born
    mid-network: the output of the third convolution of the step gets it, by a wrapped kernel method - and a clean step again.
    The poisoned step is counted as skipped; LoRA factors, moments and the applied counter keep their bits; under delayed
    scaling every site's scale, history and count keep theirs and every running maximum is cleared.  The third step has the
    logs and the gradient, bit for bit, of the second step of a twin that ran two clean steps."""
    dev = fp8_dev
    mode, recipe = SCALINGS[scaling]
    twin, tbank, tbatch = _step_world(dev, mode, recipe)
    twin.train_step(tbatch, **STEP_KW)
    want_logs = _logs(twin.train_step(tbatch, **STEP_KW))
    want_grad = tbank.flat_grad.detach().cpu().clone()
    n_twin = _site_state(dev)[1] if mode == "delayed" else 0

    trainer, bank, batch = _step_world(dev, mode, recipe)
    trainer.train_step(batch, **STEP_KW)
    before = _trainer_state(trainer, bank)
    sites = _site_state(dev)[0] if mode == "delayed" else None
    k = ops.kernels()
    if how == "batch":
        bad = dict(batch, latents=put(batch["latents"], NAN, 0, 0, 0, 0))
        logs = trainer.train_step(bad, **STEP_KW)
    else:
        calls, conv = [0], k.conv2d

        def poisoned_conv(X, W, Y, *a, **kw):
            conv(X, W, Y, *a, **kw)
            calls[0] += 1
            if calls[0] == 3:
                Y.view(-1)[:1].fill_(NAN)
        k.conv2d = poisoned_conv
        try:
            logs = trainer.train_step(batch, **STEP_KW)
        finally:
            del k.conv2d
        assert calls[0] >= 3
    assert not bool(torch.isfinite(logs["grad_norm_sq"].cpu()).all()), "the NaN did not reach comat_sumsq: the gradient norm is finite"
    after = _trainer_state(trainer, bank)
    assert after["skipped"] == before["skipped"] + 1 and after["applied"] == before["applied"], "the poisoned step is not counted as skipped"
    same_bits(after["flat"], before["flat"], "LoRA factors after the skipped update")
    for a, b in zip(after["m"] + after["v"], before["m"] + before["v"]):
        same_bits(a, b, "a moment after the skipped update")
    if mode == "delayed":
        now = _site_state(dev)[0]
        assert now["scale"].numel() > n_twin > 0
        for key in ("scale", "hist", "count"):
            same_bits(now[key], sites[key], f"fp8 sites after the skipped step: {key}")
        assert int(now["amax"].abs().sum()) == 0, "a running maximum survived the skipped step"
    got_logs = _logs(trainer.train_step(batch, **STEP_KW))
    same_bits(bank.flat_grad, want_grad, "rule 4 - the gradient of the clean step after the poisoned one against the twin's second step")
    for key, want in want_logs.items():
        same_bits(got_logs[key], want, f"rule 4 - logs[{key!r}] of the clean step after the poisoned one")


def test_full_finetuning_skip_keeps_the_quantised_weights(fp8_dev):
    """--full_finetuning with the fp8 forward: a NaN in the flat gradient skips the update; the refresh behind it re-quantises an
    unchanged master - q8 and scales keep their bits"""
    from test_full_finetuning_fp8 import CROP, TS, fp8_step_world
    ops.set_fp8_scaling("delayed")
    cfg, batch, _, tr = fp8_step_world(F32, fp8_dev, gan=False)
    assert tr.fp8_calibrate(batch)
    tr.train_step(batch, training_steps=TS, crop=CROP)
    bank = tr.bank
    q8, scales = bank.flat_q8, bank.w_scale
    q0, s0, p0 = q8.cpu().clone(), scales.cpu().clone(), bank.flat.cpu().clone()
    counters = tr.opt.counters.cpu().clone()
    tr._forward_backward(batch, dict(training_steps=TS, crop=CROP))
    bank.flat_grad[3] = NAN
    tr._apply_updates()
    assert int(tr.opt.counters[1]) == int(counters[1]) + 1 and int(tr.opt.counters[0]) == int(counters[0])
    same_bits(bank.flat, p0, "the master after the skipped update")
    same_bits(q8, q0, "the quantised weights after the skipped update")
    same_bits(scales, s0, "the weight scales after the skipped update")


def test_a_non_finite_scale_recovers_in_a_skipped_step(fp8_dev):
    """A site without a scale that meets a NaN in its first, just-in-time step keeps NaN in its scale word and is marked ready
    (an uncalibrated first step that was poisoned).  Every later step of it quantises to NaN bytes and is skipped; the skip
    clears the running maxima - but not that of a site whose scale is not finite: its first finite abs-max replaces the scale.
    Sites with a finite scale keep scale and maximum handling of a skipped step."""
    from comat_amd import fp8
    dev = fp8_dev
    ops.set_fp8_scaling("delayed")
    st = fp8.fp8_state(dev)

    class Holder:
        pass
    holders = [Holder() for _ in range(3)]
    for h in holders:
        fp8.fp8_site(h, dev)
        fp8._use(h)
    st.scale[:3] = torch.tensor([0.5, NAN, 0.25], device=dev)
    st.amax[:3] = torch.tensor([3.0, 7.0, NAN]).view(torch.int32).to(dev)
    ops.fp8_end_of_step(torch.tensor([NAN], device=dev))  # a skipped step
    same_bits(st.scale[:3], torch.tensor([0.5, 7.0 / 448.0, 0.25]), "scales after the skipped step")
    assert int(st.amax[:3].cpu().abs().sum()) == 0
    st.amax[:3] = torch.tensor([3.0, 14.0, 2.0]).view(torch.int32).to(dev)
    ops.fp8_end_of_step(torch.tensor([1.0], device=dev))  # an applied step: every site follows its maximum
    same_bits(st.scale[:3], torch.tensor([3.0, 14.0, 2.0]) / 448.0, "scales after the applied step")
