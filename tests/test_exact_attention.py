"""Fused and unfused attention on operands for which the answer is known in closed form: the attention counterpart of
test_exact_products.py.

The method.  Every query attends a SET of keys whose raw scores are all equal (c^2, with c^2 * scale = 128 and scale a power of
two); every other key scores 0, at least 104 / scale lower, and exp(-104) is below the smallest fp32 denormal.  The un-normalised
probabilities are then exactly 1 or 0 and the online-softmax rescale factor exactly 1 or 0; with set sizes that are powers of two
the recomputed probabilities of the backward snap to exactly 1 / |S| in the bf16 pack; with integer V and dO every partial sum
of every kernel - forward, dQ, dK/dV, the one-launch backward, the fp32 partials of the query-split pass and their reduction - is
an fp32 number in any order.  The output is then independent of tile shape, one or two tiles per iteration, trim, transpose
staging, block renumbering and query split, and must be the ONE round-to-nearest-even of a value known in closed form
(helpers.exact_attention_forward / _backward: P = indicator / |S|, not a softmax).  helpers.check, which bounds max |err| / max |ref|
by 2e-2, is blind to a key dropped from or counted twice in one row of a 577-key softmax (1 / 577 of |v|), to a dropped last ragged
key, to a wrong row in one lane's transpose read; each is a wrong number here, and the failure names the key
(test_comparators_reject_single_key_mutants proves that on the CPU: no hidden mutant).

What the kernels leave of exactness, read in attention.hip: fma(s, c2, -m * c2) keeps the rounding residual of m * c2, so an
attended P~ is 1 + eps (eps <= ~5e-6) before the bf16 pack removes it; l = |S| (1 + eps) moves O by that much and the store snaps it
back, because the exact O is a bf16 number (a precondition); p * scale * (dp - D) is exact scaling.  Preconditions, asserted by
every case on its own inputs (the helpers): the score gap, |raw scores| < 2^24, exact O and scale * dS of power-of-two rows are
bf16 numbers, every partial sum is a multiple of a unit below 2^24 units.

Assertions.  hip, bf16, rows / keys of power-of-two sets: O, dQ, dK, dV bit for bit (the dense dO: dV; its dS is not a bf16
number, dQ and dK go through helpers.check).  lse, every leg: 16 fp32 ulps of the closed form (2.4e-4 at 130; a miscounted key
moves it by ln(33 / 32) = 0.031 at least).  The one remainder set (not a power of two: P = 1/3 is rounded in the pack, and the
backward's D comes from an O that was rounded to bf16): helpers.check per head with the sibling test's factors, on every bf16
leg.  fp32 storage, both backends: per element tol(float32) * A, A the same formula on absolute values.  sim, bf16 (fp32
arithmetic on un-snapped probabilities, ONE rounding at the store): helpers.attn_rounded_error - the stored number lies between
the bf16 roundings of exact -+ tol(float32) * A, which is the exact value itself where that is a bf16 number and one of its two
neighbours elsewhere, EXCEPT where the terms cancel (a sum of +-v / 3 that is exactly zero, dQ in a code column): there fp32
leaves a residual of 1e-8 that an equality with zero cannot admit.  The unfused path stores P and dS in bf16 on both backends,
so its bf16 legs are held bit for bit on both.

Which template a case reaches (launch_fwd / launch_bwd / dispatch of attention.hip; bf16; TR = hardware transpose reads, on for
every bf16 head dim unless flash_tr = 0; defaults flash_kt = 4, flash_merge = 1, flash_tr = 1, flash_trim = 1, flash_xcd = 1):

    tile width:  d <= 32: 32 | 33..48: 64, trimmed to 48 | 49..64: 64 | 65..80: 96, trimmed to 80 | 81..96: 96 | else 160
    TWO (the two-tile kernels exist): bf16 and TR and tile width <= 96
    forward:   flash_fwd2_kernel   iff TWO and flash_kt >= 2 and Nk > 64, else flash_fwd_kernel
    dQ:        the two-tile body   iff TWO and flash_kt >= 3 and Nk > 64
    merged:    flash_delta_kernel + flash_bwd_kernel<DQ2 = the dQ rule> iff flash_merge = 2, or = 1 and the two grids hold <= 768
               blocks (every case here: the defaults run the merged kernel, flash_merge = 0 the separate ones)
    dK/dV:     flash_dkdv2_kernel  iff TWO and not merged and Nq > 64 and (flash_kt >= 5, or flash_kt = 4 and tile width <= 64)
    query split of dK/dV into fp32 partials + flash_kv_reduce_kernel: qsplit_of below (merged or not)

    option set                    what it moves
    defaults                      fwd2 / merged with DQ2 where Nk > 64
    flash_kt = 1                  the one-tile kernels everywhere
    flash_kt = 5                  as the defaults (merged): the option alone
    flash_kt = 5, flash_merge = 0 flash_dq2 + flash_dkdv2 at tile widths up to 96 (Nq > 64: 72 x 200 x 80)
    flash_merge = 0               flash_dq2 + flash_dkdv2 (tile width <= 64, Nq > 64: 130 x 65 x 64, 70 x 130 x 40, 96 x 577 x 64) or flash_dkdv
    flash_merge = 2               merged whatever the block count
    flash_tr = 0                  plain LDS reads, one tile per iteration (TWO is false); fp32: no transposed image
    flash_tr = 2                  fp32: the software-transposed image for every head dim
    flash_trim = 0                the untrimmed 64- and 96-wide tiles for d = 40 and 80
    flash_xcd = 0                 blocks not renumbered

Found by these tests: nothing so far - every case passes on the library as it stands.
"""
import functools

import pytest
import torch

from comat_amd import ops
from helpers import (ATTN_ORDERS, _set_opts, attn_bits_error, attn_close_error, attn_group_sizes, attn_lse_error, attn_rounded_error,
                     bf16_number, check, exact_attention_backward, exact_attention_forward, exact_attention_operands, explain_O_row,
                     restore_default_opts, single_term_explanation)

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [BF16, F32]
SCALE = 0.125  # c = 32

# (B, H, Nq, Nk, d): the smallest shapes that reach each template and edge
SHAPES = [
    (1, 4, 70, 130, 40),   # trim 64 -> 48; two-tile forward and dQ; ragged last key tile of 2; ragged query tile
    (2, 2, 130, 65, 64),   # one key alone in the third tile; flash_dkdv2 at flash_kt = 4 (flash_merge = 0)
    (1, 2, 96, 577, 64),   # the ViT's odd key count
    (1, 2, 64, 64, 16),    # the 32-wide family; Nk = 64 stays on the one-tile kernels
    (1, 2, 64, 64, 32),
    (1, 2, 72, 200, 80),   # trim 96 -> 80; two-tile dK/dV only at flash_kt = 5
    (1, 2, 40, 96, 96),    # head dim 96
    (1, 1, 33, 72, 160),   # the 160-wide family
    (1, 1, 33, 72, 128),
    (1, 2, 256, 77, 40),   # the query-split dK/dV pass
    (1, 2, 5, 577, 96),    # few queries, many keys
]
OPTION_SETS = [dict(), dict(flash_kt=1), dict(flash_kt=5), dict(flash_kt=5, flash_merge=0), dict(flash_merge=0), dict(flash_merge=2),
               dict(flash_tr=0), dict(flash_tr=2), dict(flash_trim=0), dict(flash_xcd=0)]
UNIFORM = [(d, Nk) for d in (32, 40, 96, 160) for Nk in (64, 128, 77)]  # one per tile-width family


def sid(s):
    return "x".join(str(v) for v in s)


def cdiv(a, b):
    return -(-a // b)


def qsplit_of(B, H, Nq, Nk, d, ws_bytes=(256 << 20) - 256 * 1024, flash_qs=0):
    """the query-split rule of comat_flash_attn_bwd (attention.hip)"""
    base, ntq = cdiv(Nk, 128) * B * H, cdiv(Nq, 32)
    if not (d % 4 == 0 and base < 256 and ntq >= 8):
        return 1
    qs = min(cdiv(flash_qs if flash_qs > 0 else 512, base), ntq // 4, ws_bytes // (2 * B * H * Nk * d * 4), 64)
    return qs if qs >= 2 else 1


@pytest.fixture
def options(dev):
    """options(**kernel_selection): set on the hip leg from the library's defaults (the simulator has one kernel per entry
    point), the defaults restored afterwards"""
    used = []

    def f(**kw):
        if dev.type == "cuda":
            restore_default_opts()
            _set_opts(**kw)
            used.append(True)
    yield f
    if used:
        restore_default_opts()


def flat(x, dev, dtype):
    """[B, H, N, d] -> the [B * N, H * d] matrix the kernels address heads in"""
    B, H, N, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * N, H * d).to(device=dev, dtype=dtype).contiguous()


def heads(t, B, H, N, d):
    return t.detach().cpu().reshape(B, N, H, d).permute(0, 2, 1, 3).contiguous()


@functools.lru_cache(maxsize=None)
def build(shape, order, layout, uniform=False, mode="plain", with_gP=False):
    """operands, closed-form results for both dO and the preconditions (asserted inside the helpers), computed once per case"""
    B, H, Nq, Nk, d = shape
    c = exact_attention_operands(B, H, Nq, Nk, d, order=order, layout=layout, scale=SCALE, seed=sum(shape) + 17 * layout, uniform=uniform)
    allowed = None
    if mode == "causal":
        allowed = (torch.arange(Nk)[None, :] <= torch.arange(Nq)[:, None] + (Nk - Nq)).expand(B, H, Nq, Nk)
    elif mode == "masked":
        c["key_mask"] = key_mask_of(c["kg"], c["sizes"], B, Nk)
        allowed = c["key_mask"].bool()[:, None, None, :].expand(B, H, Nq, Nk)
    c["allowed"] = allowed
    c["fwd"] = fwd = exact_attention_forward(c["Q"], c["K"], c["V"], SCALE, allowed)
    rp2 = fwd["row_pow2"]
    assert bool(bf16_number(fwd["O"][rp2]).all()), "O of a power-of-two row is not a bf16 number: the store would not snap l = |S| (1 + eps) back"
    c["gP"] = None
    if with_gP:  # small integers on attended entries
        g = torch.Generator().manual_seed(5)
        c["gP"] = (torch.randint(1, 3, fwd["M"].shape, generator=g) * (torch.randint(0, 2, fwd["M"].shape, generator=g) * 2 - 1)).double() * fwd["M"]
    exact_dS = not uniform  # (uniform sets of 64 / 128 keys: dS has more levels than a bf16 number - dV and dK = 0 are still exact)
    c["sparse"] = exact_attention_backward(c["Q"], c["K"], c["V"], SCALE, fwd, c["dO_sparse"], gP=c["gP"], exact_dS=exact_dS)
    c["dense"] = exact_attention_backward(c["Q"], c["K"], c["V"], SCALE, fwd, c["dO_dense"], gP=c["gP"], exact_dS=False)
    return c


def key_mask_of(kg, sizes, B, Nk):
    """[B, Nk] int8, shared by the heads of a batch entry (the key order must be too): sets of 32 / 8 / 2 lose half their members,
    a set of 4 three, a set of 16 five (11 left: not a power of two); the last batch entry instead loses its first set
    altogether - the rows that target it then attend every remaining key alike"""
    assert bool((kg == kg[:, :1]).all()), "a key mask is per batch entry: the heads must share the key order"
    km = torch.ones(B, Nk, dtype=torch.int8)
    lose = {32: 16, 8: 4, 2: 1, 4: 3, 16: 5}
    for b in range(B):
        for g, s in enumerate(sizes):
            members = torch.nonzero(kg[b, 0] == g).flatten()
            if b == B - 1 and B > 1:
                if g == 0:
                    km[b, members] = 0
            else:
                km[b, members[:lose.get(s, 0)]] = 0
    return km


# ---- explanations: which single key (query) reproduces a wrong row -------------------------------------------------------------
def explain_O(c):
    return lambda b, h, r, row: single_term_explanation(row, explain_O_row(c["V"][b, h], c["fwd"]["M"][b, h, r]), "key")


def explain_terms(terms_of, noun):
    def f(b, h, r, row):
        t = terms_of(b, h, r)
        tot = t.sum(0)
        return single_term_explanation(row, {"dropped": tot - t, "counted twice": tot + t}, noun)
    return f


def explainers(c, bw, dO):
    P, dS = c["fwd"]["P"], bw["dS"]
    return dict(
        dV=explain_terms(lambda b, h, j: P[b, h, :, j, None] * dO[b, h], "query"),
        dQ=explain_terms(lambda b, h, i: SCALE * dS[b, h, i, :, None] * c["K"][b, h], "key"),
        dK=explain_terms(lambda b, h, j: SCALE * dS[b, h, :, j, None] * c["Q"][b, h], "query"))


# ---- the comparators of each leg ------------------------------------------------------------------------------------------------
def fail_if(*errors):
    errors = [e for e in errors if e]
    assert not errors, "\n".join(errors)


def remainder_error(got, exact64, sel, what, factor):
    """helpers.check per head on the rows `sel` leaves out (the one set that is not a power of two)"""
    B, H = sel.shape[:2]
    for b in range(B):
        for h in range(H):
            rows = ~sel[b, h]
            if bool(rows.any()):
                try:
                    check(got[b, h][rows], exact64[b, h][rows], BF16, f"{what}, remainder set of (batch, head) = ({b}, {h})", factor=factor)
                except AssertionError as e:
                    return str(e)
    return None


def forward_errors(hip, dtype, c, o, lse, what, snapped=None):
    """snapped: the probabilities were stored in bf16 before P V (the kernels' pack; the unfused path on either backend)"""
    fwd = c["fwd"]
    snapped = hip if snapped is None else snapped
    errs = [attn_lse_error(lse, fwd["lse"], f"{what} lse")] if lse is not None else []
    if dtype == F32:
        errs.append(attn_close_error(o, fwd["O"], fwd["A_O"], f"{what} O", explain=explain_O(c)))
    elif snapped:
        errs.append(attn_bits_error(o, fwd["O"], fwd["row_pow2"], f"{what} O", explain_O(c)))
        errs.append(remainder_error(o, fwd["O"], fwd["row_pow2"], f"{what} O", 1))
    else:
        errs.append(attn_rounded_error(o, fwd["O"], fwd["A_O"], f"{what} O", explain=explain_O(c)))
    return errs


def backward_errors(hip, dtype, c, which, dq, dk, dv, what, snapped=None):
    """bf16: rows / keys of power-of-two sets are held bit for bit where probabilities and dS were snapped, to the rounding of
    the fp32 bound where they were not (the simulator's fused backward); the remainder set goes through helpers.check on every
    bf16 leg - its D = rowsum(dO . O) is computed from an O that was ROUNDED to bf16, which no fp32 bound covers"""
    bw, dO = c[which], c["dO_" + which]
    rows, keys = c["fwd"]["row_pow2"], bw["key_pow2"]
    snapped = hip if snapped is None else snapped
    ex = explainers(c, bw, dO)
    if dtype == F32:
        return [attn_close_error(dq, bw["dQ"], bw["A_dQ"], f"{what} dQ", explain=ex["dQ"]), attn_close_error(dk, bw["dK"], bw["A_dK"], f"{what} dK", explain=ex["dK"]),
                attn_close_error(dv, bw["dV"], bw["A_dV"], f"{what} dV", explain=ex["dV"])]
    errs = [remainder_error(dv, bw["dV"], keys, f"{what} dV", 3), remainder_error(dq, bw["dQ"], rows, f"{what} dQ", 3),
            remainder_error(dk, bw["dK"], keys, f"{what} dK", 3)]
    if not snapped:
        return errs + [attn_rounded_error(dq, bw["dQ"], bw["A_dQ"], f"{what} dQ", rows, ex["dQ"]), attn_rounded_error(dk, bw["dK"], bw["A_dK"], f"{what} dK", keys, ex["dK"]),
                       attn_rounded_error(dv, bw["dV"], bw["A_dV"], f"{what} dV", keys, ex["dV"])]
    errs.append(attn_bits_error(dv, bw["dV"], keys, f"{what} dV", ex["dV"]))
    if which == "sparse":  # scale * dS is a bf16 number: dQ and dK are exact too
        errs += [attn_bits_error(dq, bw["dQ"], rows, f"{what} dQ", ex["dQ"]), attn_bits_error(dk, bw["dK"], keys, f"{what} dK", ex["dK"])]
    else:  # dense dO: dS is rounded in the pack
        errs += [remainder_error(dq, bw["dQ"], torch.zeros_like(rows), f"{what} dQ", 3), remainder_error(dk, bw["dK"], torch.zeros_like(keys), f"{what} dK", 3)]
    return errs


# ---- the fused kernels -----------------------------------------------------------------------------------------------------------
def run_flash(dev, dtype, c, shape, dOs):
    """forward, then one backward per dO, at the kernel level: (O, lse, {name: (dQ, dK, dV)}) as [B, H, N, d] on the CPU"""
    B, H, Nq, Nk, d = shape
    HD = H * d
    K = ops.kernels()
    q, k, v = (flat(c[n], dev, dtype) for n in "QKV")
    o = torch.full_like(q, float("nan"))
    lse = torch.full((B, H, Nq), float("nan"), device=dev)
    K.flash_attn_fwd(q, k, v, o, lse, B, H, Nq, Nk, d, HD, HD, HD, HD, SCALE)
    grads = {}
    for name in dOs:
        g = flat(c["dO_" + name], dev, dtype)
        dq, dk, dv = torch.full_like(q, float("nan")), torch.full_like(k, float("nan")), torch.full_like(v, float("nan"))
        dbuf = torch.empty((B, H, Nq), device=dev)
        K.flash_attn_bwd(q, k, v, o, g, lse, dbuf, dq, dk, dv, B, H, Nq, Nk, d, HD, HD, HD, HD, SCALE)
        grads[name] = (heads(dq, B, H, Nq, d), heads(dk, B, H, Nk, d), heads(dv, B, H, Nk, d))
    return heads(o, B, H, Nq, d), lse.cpu(), grads


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("order", ATTN_ORDERS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_flash_exact(dev, options, shape, order, dtype):
    """every fused kernel variant on every case: all option sets share ONE expected tensor - the exact answer does not depend
    on the option"""
    hip = dev.type == "cuda"
    c = build(shape, order, (SHAPES.index(shape) + ATTN_ORDERS.index(order)) % 2)
    if shape == (1, 2, 256, 77, 40):
        assert qsplit_of(*shape) >= 2, "the case is about the query-split dK/dV pass"
    sizes = attn_group_sizes(shape[3])
    assert (1 in sizes and 32 in sizes) or shape[3] < 63
    for opts in (OPTION_SETS if hip else [dict()]):
        options(**opts)
        what = f"{sid(shape)} {order} {opts or 'defaults'}:"
        o, lse, grads = run_flash(dev, dtype, c, shape, ("sparse", "dense"))
        fail_if(*forward_errors(hip, dtype, c, o, lse, what))
        for which, (dq, dk, dv) in grads.items():
            fail_if(*backward_errors(hip, dtype, c, which, dq, dk, dv, f"{what} {which} dO:"))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[1], SHAPES[9]], ids=sid)
def test_flash_exact_through_ops(dev, shape, dtype):
    """the same operands through ops.attention(need_probs=False, scale=...) and autograd: the layout of the heads, the saved
    O / lse and the one gradient allocation of _FlashAttention"""
    B, H, Nq, Nk, d = shape
    hip = dev.type == "cuda"
    c = build(shape, "tail", 1)
    q, k, v = (flat(c[n], dev, dtype).requires_grad_(True) for n in "QKV")
    o, p = ops.attention(q, k, v, B, Nq, Nk, H, d, scale=SCALE, need_probs=False)
    assert p is None
    (o.float() * flat(c["dO_sparse"], dev, F32)).sum().backward()
    what = f"ops.attention {sid(shape)}:"
    fail_if(*forward_errors(hip, dtype, c, heads(o, B, H, Nq, d), None, what),
            *backward_errors(hip, dtype, c, "sparse", heads(q.grad, B, H, Nq, d), heads(k.grad, B, H, Nk, d), heads(v.grad, B, H, Nk, d), what))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("d,Nk", UNIFORM)
def test_flash_uniform(dev, options, d, Nk, dtype):
    """Q = 0: every key counts once, O = mean of V (one fp32 division of an exact sum, whatever Nk), lse = ln Nk, dK = 0;
    bit-exact O and dV for the power-of-two Nk"""
    hip = dev.type == "cuda"
    shape = (1, 2, 70, Nk, d)
    c = build(shape, "ascending", 0, uniform=True)
    fwd = c["fwd"]
    assert bool((fwd["n"] == Nk).all())
    pow2 = Nk & (Nk - 1) == 0
    every = torch.ones_like(fwd["row_pow2"])
    for opts in (OPTION_SETS if hip else [dict()]):
        options(**opts)
        what = f"uniform {sid(shape)} {opts or 'defaults'}:"
        o, lse, grads = run_flash(dev, dtype, c, shape, ("dense",))
        dq, dk, dv = grads["dense"]
        bw = c["dense"]
        errs = [attn_lse_error(lse, fwd["lse"], f"{what} lse")]
        if dtype == F32:
            errs += [attn_close_error(o, fwd["O"], fwd["A_O"], f"{what} O"), attn_close_error(dv, bw["dV"], bw["A_dV"], f"{what} dV"),
                     attn_close_error(dq, bw["dQ"], bw["A_dQ"], f"{what} dQ")]
        elif hip and pow2:
            allk = torch.ones_like(bw["key_pow2"])
            errs += [attn_bits_error(o, fwd["O"], every, f"{what} O", explain_O(c)),
                     attn_bits_error(dv, bw["dV"], allk, f"{what} dV", explainers(c, bw, c["dO_dense"])["dV"]),
                     remainder_error(dq, bw["dQ"], ~every, f"{what} dQ", 3)]
        elif hip:
            errs += [remainder_error(o, fwd["O"], ~every, f"{what} O", 1), remainder_error(dv, bw["dV"], torch.zeros_like(bw["key_pow2"]), f"{what} dV", 3),
                     remainder_error(dq, bw["dQ"], ~every, f"{what} dQ", 3)]
        else:
            errs += [attn_rounded_error(o, fwd["O"], fwd["A_O"], f"{what} O"), attn_rounded_error(dv, bw["dV"], bw["A_dV"], f"{what} dV")]
        fail_if(*errs)
        assert bool((dk == 0).all()), f"{what} dK: Q = 0, every product is zero"


# ---- the unfused path: the captured probability map feeds the grounding losses ---------------------------------------------------
UNFUSED = [  # (shape, key order, mode, gradient on P)
    ((2, 2, 40, 72, 16), "tail", "plain", False), ((2, 2, 40, 72, 64), "tail", "plain", False),
    ((2, 2, 40, 72, 16), "strided", "causal", False), ((2, 2, 40, 72, 64), "strided", "causal", False),
    ((2, 2, 40, 72, 16), "ascending", "masked", False), ((2, 2, 40, 72, 64), "strided", "masked", False),
    ((1, 2, 40, 40, 16), "strided", "plain", True),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", UNFUSED, ids=lambda c: f"{sid(c[0])}-{c[1]}-{c[2]}{'-gP' if c[3] else ''}")
def test_unfused_exact(dev, case, dtype):
    """ops.attention(need_probs=True, scale=2^-3): the captured map equals indicator / |S| bit for bit in bf16, O and the
    gradients are held as those of the fused kernels; causal and key-masked sets shrink (the closed form takes the row maximum
    over the allowed keys), and the rows whose shrunk set is still a power of two stay bit-exact"""
    shape, order, mode, with_gP = case
    B, H, Nq, Nk, d = shape
    hip = dev.type == "cuda"
    c = build(shape, order, UNFUSED.index(case) % 2, mode=mode, with_gP=with_gP)
    fwd, bw = c["fwd"], c["sparse"]
    rows = fwd["row_pow2"]
    assert int(rows.sum()) * 4 >= rows.numel(), "too few rows keep a power-of-two set"
    if mode != "plain":
        assert bool((fwd["n"] != build(shape, order, UNFUSED.index(case) % 2)["fwd"]["n"]).any()), "the mask shrinks no set"
    q, k, v = (flat(c[n], dev, dtype).requires_grad_(True) for n in "QKV")
    km = c["key_mask"].to(dev) if mode == "masked" else None
    o, p = ops.attention(q, k, v, B, Nq, Nk, H, d, scale=SCALE, causal=mode == "causal", key_mask=km, need_probs=True)
    loss = (o.float() * flat(c["dO_sparse"], dev, F32)).sum()
    if with_gP:
        loss = loss + (p.float() * c["gP"].to(device=dev, dtype=F32)).sum()
    loss.backward()
    what = f"unfused {sid(shape)} {order} {mode}:"
    pm = p.detach().cpu()
    assert pm.dtype == dtype
    if dtype == BF16:  # the map itself: exact on both backends (a softmax of scores that are exactly 128 or 0)
        # (the other rows: the ONE rounding of an fp32 quotient within 2e-4 of 1 / |S|)
        errs = [attn_bits_error(pm, fwd["P"], rows, f"{what} P"), attn_rounded_error(pm, fwd["P"], fwd["P"], f"{what} P", ~rows)]
    else:
        errs = [attn_close_error(pm, fwd["P"], fwd["P"], f"{what} P")]
    errs += forward_errors(hip, dtype, c, heads(o, B, H, Nq, d), None, what, snapped=True)
    errs += backward_errors(hip, dtype, c, "sparse", heads(q.grad, B, H, Nq, d), heads(k.grad, B, H, Nk, d), heads(v.grad, B, H, Nk, d), what, snapped=True)
    fail_if(*errs)


# ---- the comparators are live: single-key mutants of the reference, on the CPU, no backend ---------------------------------------
def mutant_positions(c, Nq, Nk):
    """(b, h, row, key) with key in the row's set: both sides of every 32-key tile boundary, the first and the last key, each
    with the first and the last row that attends it (the last one sits in the last query tile wherever a set has such a row),
    and every key of the sets of the last query tile's first and last row"""
    M = c["fwd"]["M"]
    B, H = M.shape[:2]
    keys = sorted({0, Nk - 1} | {j for t in range(32, Nk, 32) for j in (t - 1, t)})
    out = []
    for b in range(B):
        for h in range(H):
            for j in keys:
                rows = torch.nonzero(M[b, h, :, j]).flatten().tolist()
                out += [(b, h, r, j) for r in sorted({rows[0], rows[-1]})] if rows else []
            for r in sorted({(Nq - 1) // 32 * 32, Nq - 1}):
                out += [(b, h, r, j) for j in torch.nonzero(M[b, h, r]).flatten().tolist()]
    return sorted(set(out))


def hip_rejects_forward(c, O, lse):
    return any(forward_errors(True, BF16, c, O.float().to(BF16), lse.float(), "mutant"))


def hip_rejects_dV(c, dV):
    bw = c["dense"]
    return bool(attn_bits_error(dV.float().to(BF16), bw["dV"], bw["key_pow2"], "mutant dV") or
                remainder_error(dV.float().to(BF16), bw["dV"], bw["key_pow2"], "mutant dV", 3))


@pytest.mark.parametrize("order", ATTN_ORDERS)
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_comparators_reject_single_key_mutants(shape, order):
    """a subtly wrong kernel, played on the reference: one key dropped from one row (renormalised), one key counted twice, the
    last key dropped for all rows, the first key of every 32-key tile dropped for one row, one row's set taken from the next
    head.  The hip-leg comparator must reject every one on O or lse, and the matching dV mutant on dV: the cap is ZERO hidden."""
    B, H, Nq, Nk, d = shape
    c = build(shape, order, (SHAPES.index(shape) + ATTN_ORDERS.index(order)) % 2)
    fwd, V, dO = c["fwd"], c["V"], c["dO_dense"]
    assert not hip_rejects_forward(c, fwd["O"], fwd["lse"]) and not hip_rejects_dV(c, c["dense"]["dV"]), "the comparator refuses the reference itself"
    top = 128.0

    def mutate(Mm, own_lse):
        """O, lse, dV of a mutated multiplicity map Mm [B, H, Nq, Nk] (a key counted twice has multiplicity 2): the forward
        normalises by what it counted; the backward recomputes its probabilities from the log-sum-exp it is given - the true
        one (own_lse: the mutated one), so that a key it counts twice or drops changes that key's dV alone"""
        n = Mm.sum(-1, keepdim=True)
        Pb = Mm / (n if own_lse else fwd["n"][..., None])
        return (Mm / n) @ V, top + torch.log(n[..., 0]), Pb.transpose(-1, -2) @ dO

    hidden, total = [], 0
    M0 = fwd["M"].double()

    def judge(Mm, name, dv_rows_pow2, own_lse=False):
        nonlocal total
        total += 1
        O, lse, dV = mutate(Mm, own_lse)
        if not hip_rejects_forward(c, O, lse):
            hidden.append(name + " (forward)")
        if dv_rows_pow2 and not hip_rejects_dV(c, dV):
            hidden.append(name + " (dV)")

    rp2 = fwd["row_pow2"]
    for b, h, r, j in mutant_positions(c, Nq, Nk):
        n = int(fwd["n"][b, h, r])
        if n > 1:
            Mm = M0.clone()
            Mm[b, h, r, j] = 0
            judge(Mm, f"key {j} dropped from row {(b, h, r)}", bool(rp2[b, h, r]))
        Mm = M0.clone()
        Mm[b, h, r, j] = 2
        judge(Mm, f"key {j} counted twice in row {(b, h, r)}", bool(rp2[b, h, r]))
    Mm = M0.clone()
    Mm[..., Nk - 1] = 0
    if bool((Mm.sum(-1) > 0).all()) and bool(fwd["M"][..., Nk - 1].any()):  # (5 queries attend 5 of 23 sets: the last key's only in the 'tail' order)
        judge(Mm, "the last key dropped for all rows", bool(rp2[fwd["M"][..., Nk - 1]].any()))
    for b in range(B):
        for h in range(H):
            for r in sorted({0, (Nq - 1) // 32 * 32, Nq - 1}):
                Mm = M0.clone()
                Mm[b, h, r, 0::32] = 0
                if float(Mm[b, h, r].sum()) not in (0.0, float(fwd["n"][b, h, r])):
                    judge(Mm, f"the first key of every tile dropped from row {(b, h, r)}", bool(rp2[b, h, r]))
                b2, h2 = divmod((b * H + h + 1) % (B * H), H)
                if (b2, h2) != (b, h) and not torch.equal(M0[b2, h2, r], M0[b, h, r]) and bool(rp2[b, h, r]):
                    Mm = M0.clone()
                    Mm[b, h, r] = M0[b2, h2, r]
                    judge(Mm, f"row {(b, h, r)} attends the set of head {(b2, h2)}", True, own_lse=True)
    assert total >= 20
    assert not hidden, f"{len(hidden)} of {total} mutants pass the comparators: {hidden[:5]}"
