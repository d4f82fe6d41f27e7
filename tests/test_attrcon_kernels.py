"""The attribute-concentration kernels entry point by entry point (comat_mask_resize_any, comat_attrcon_workspace_floats,
comat_attrcon_gather_fwd, comat_attrcon_loss, comat_attrcon_gather_bwd; include/comat_hip.h, "Attribute concentration on the
device"), called directly through ops.attrcon_kernels() on both legs of `attrcon_dev`: the CPU mirror of tests/attrcon_sim.py
and, marked gpu, the library.  ops._AttrconLayerLoss zero-fills everything it hands to the kernels, which turns a skipped store
and a store that should not have happened into a plausible 0; here

* every output lies in a flat NaN-filled buffer with guard elements on both sides (`Guarded`), `avg` starts from a dyadic
  non-zero value (the header says +=), the workspace is refilled with NaN before every call, and after the calls every element
  the header does not list as written must carry the bits it had;
* every input the header says is not read is poisoned: the map slices, mask rows and table rows of skipped samples, the map
  columns no token names, the mask rows of objects >= n_obj, the table entries at t >= n_tok (their column is a NaN column);
* the reference is `reference` below: the header's formulas restated in plain fp64 on the dtype-rounded inputs, independent of
  oracle/losses.py and of the mirror.

Bounds: the fp32 outputs (num, den, avg, g_num, g_den, g_avg, out) are held to helpers.check at tol(float32) for both map
dtypes - per sample, and g_num / g_den per (sample, map), so that a sample with small values cannot hide behind a large one;
damap per (sample, head) at tol(float32) * 2 for an fp32 map and per element at 2^-8 |ref| + tol(float32) * 2 max|ref| for a
bf16 map (one round-to-nearest-even of an fp32 value, with a factor two).  Precondition, asserted by `headroom`: the same
formulas in torch fp32 on the CPU stay within a tenth of each bound; the mask coverage of the toleranced cases is drawn until
1 - act >= 0.05 for every token (the cancellation in 1 - act is otherwise outside that precondition; act = 1 and act = 0 are
the exact cases).

Which kernel form a case reaches is derived from chunks_vectorise (attrcon.hip) - the library has no query for it:
(npix, L) = (16, 11) and (300, 12) staged everywhere (300 rows: 3 chunks of 128 in the fp32 gather and the gradient writer, 2 of
256 in the bf16 gather, a ragged last one); (9, 11) and (257, 11) plain everywhere; (16, 127) staged everywhere, 65 040 B of LDS
in both gathers; (16, 128) plain in both gathers (65 552 B), staged in the gradient writer with exactly 65 536 B; (16, 130) plain
everywhere; any shape from a base one element off 16 bytes: plain by the pointer.

The precondition's worst figures over all cases (fp32 vs fp64, as helpers.check measures): num 1.6e-7, den 1.9e-7, avg 9.8e-8,
out 2.1e-7, g_num 7.1e-7, g_den 1.2e-6, g_avg 1.8e-7 (bound 2e-4), damap 8.3e-7 (bound 4e-4).

That the module tells a right kernel from a wrong one was tried on the mirror, one change at a time: `=` for `+=` on a repeated
column (the three repeated-column cases fail), num written at t >= n_tok (every case with a padded table row), the zero rows
of a skipped sample not written (every case with a skipped sample), the derivative of a clamped logarithm taken as 1 / p
(test_clamps_of_the_pixel_loss).

Found: the library passes every case as it stands.  The mirror did not: it indexed with raw table values (a negative column
wrapped around to the last one) where the kernels give an out-of-range column the value 0 and clamp tok_obj, and it summed num
in another order than den, so that a full mask did not give num the bits of den.  The mirror now does what the kernels do and
the header says what that is."""
import math
import types

import numpy as np
import pytest
import torch

from attrcon_sim import attrcon_dev  # noqa: F401 - a fixture
from comat_amd import losses, ops
from helpers import tol

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
DTYPES = [F32, BF16]
NAN = float("nan")
GUARD = 64        # guard elements on both sides of every buffer (a multiple of 16 bytes in every element size)
AVG0 = 2.0 ** -7  # what avg holds before the first gather: the header says +=
GO = (0.75, 1.5)  # upstream gradients of out[0], out[1]
WORST = {}        # quantity -> the worst fp32-vs-fp64 figure the precondition saw, as a fraction of the bound


def _bits(t):
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


class Guarded:
    """`shape` elements in one flat poisoned buffer (NaN; bytes 0xA5) with GUARD elements before and after; `off` more elements
    in front move the base off its 16-byte boundary.  arm() before the calls, assert_kept() after: the guards, and the elements
    of `keep`, must carry the bits they had."""

    def __init__(self, shape, dtype, dev, fill=None, off=0):
        n = math.prod(shape)
        self.buf = torch.full((2 * GUARD + off + n,), NAN if dtype.is_floating_point else 0xA5, dtype=dtype, device=dev)
        self.span = slice(GUARD + off, GUARD + off + n)
        self.view = self.buf[self.span].view(shape)
        if fill is not None:
            self.view.fill_(fill)
        if dev.type == "cuda":
            assert self.view.data_ptr() % 16 == off * self.buf.element_size() % 16
        self.snap = None

    def put(self, x):
        self.view.copy_(x.to(self.buf.dtype).reshape(self.view.shape))
        return self

    def arm(self):
        self.snap = _bits(self.buf).clone()
        return self

    def get(self):
        return self.view.detach().cpu().clone()

    def assert_kept(self, what, keep=None):
        same = (_bits(self.buf) == self.snap).cpu()
        inside = same[self.span].clone().view(self.view.shape)
        same[self.span] = True
        assert bool(same.all()), f"{what}: {int((~same).sum())} guard element(s) overwritten, first at {int(torch.nonzero(~same)[0]) - self.span.start}"
        if keep is not None:
            bad = ~inside & keep
            assert not bool(bad.any()), f"{what}: {int(bad.sum())} element(s) the header leaves alone were written, first at {tuple(torch.nonzero(bad)[0].tolist())}"


# ---- the case builder -------------------------------------------------------------------------------------------------------
def make_case(npix, L, dtype, toks, heads=2, M=2, seed=0, n_obj=None, n_tok=None, TOK=None, OBJ=None, mask_value=None,
              poison_unnamed=True):
    """toks: per sample None (skipped: n_obj = 0) or its tokens [(column, object), ...] in table order.  Maps [bs, heads, npix, L]
    per m: rows of a softmax times 0.3 (a column named three times by one object still sums below 1) times a per-pixel magnitude
    spread over 1e-6 .. 1, rounded to dtype, kept as fp64.  Everything the header says is not read is poisoned."""
    bs = len(toks)
    rows = [list(t or []) for t in toks]
    TOK = TOK or max(1, max(len(r) for r in rows))
    nobj = list(n_obj) if n_obj is not None else [max((o for _, o in r), default=-1) + 1 for r in rows]
    OBJ = OBJ or max(1, max(nobj))
    raw = list(n_tok) if n_tok is not None else [len(r) if t is not None else 7 for r, t in zip(rows, toks)]
    nt = [min(max(raw[b], 0), TOK) if nobj[b] > 0 else 0 for b in range(bs)]
    assert all(len(rows[b]) >= nt[b] for b in range(bs))
    named = [sorted({c for c, _ in rows[b][:nt[b]] if 0 <= c < L}) for b in range(bs)]
    free = [c for c in range(L) if all(c not in s for s in named)]
    tok_idx = torch.full((bs, TOK), free[0] if free else -5, dtype=torch.int32)  # beyond n_tok: a column of NaNs
    tok_obj = torch.full((bs, TOK), OBJ - 1, dtype=torch.int32)
    inv_len = torch.full((bs, TOK), NAN, dtype=F32)
    for b in range(bs):
        for t in range(nt[b]):
            c, o = rows[b][t]
            tok_idx[b, t], tok_obj[b, t] = c, o
            inv_len[b, t] = 1.0 / sum(1 for _, o2 in rows[b][:nt[b]] if o2 == o)
    g = torch.Generator().manual_seed(1000 + seed)
    maps = []
    for _ in range(M):
        p = torch.softmax(torch.randn(bs, heads, npix, L, generator=g) * 2, -1) * 0.3
        p = (p * 10.0 ** (-6.0 * torch.rand(bs, heads, npix, 1, generator=g))).to(dtype).double()
        for b in range(bs):
            if nt[b] == 0:
                p[b] = NAN
            elif poison_unnamed:
                p[b][:, :, [c for c in range(L) if c not in named[b]]] = NAN
        maps.append(p)
    c = types.SimpleNamespace(bs=bs, heads=heads, npix=npix, L=L, OBJ=OBJ, TOK=TOK, M=M, dtype=dtype, nobj=nobj, nt=nt, maps=maps,
                              n_obj=torch.tensor(nobj, dtype=torch.int32), n_tok=torch.tensor(raw, dtype=torch.int32),
                              tok_idx=tok_idx, tok_obj=tok_obj, inv_len=inv_len)
    for attempt in range(64):  # the mask coverage: drawn until 1 - act >= 0.05 everywhere (module docstring)
        gm = torch.Generator().manual_seed(5000 + 64 * seed + attempt)
        masks = (torch.rand(bs, OBJ, npix, generator=gm) < 0.5).float() if mask_value is None else torch.full((bs, OBJ, npix), float(mask_value))
        for b in range(bs):
            masks[b, nobj[b] if nt[b] else 0:] = NAN
        c.masks = masks
        c.ref = reference(c, F64)
        act = c.ref.act[~torch.isnan(c.ref.act)]
        if mask_value is not None or act.numel() == 0 or float((1.0 - act).min()) >= 0.05:
            return c
    raise AssertionError("no mask coverage with 1 - act >= 0.05 in 64 draws")


def reference(c, dt):
    """The header's formulas, plainly, in precision dt: gather_fwd, loss with its derivatives, gather_bwd of every map under the
    upstream gradients GO.  A column outside [0, L) has the value 0 and no gradient; tok_obj is clamped where a mask row is
    picked; n_tok is clamped into [0, TOK] (c.nt)."""
    bs, heads, npix, L, OBJ, TOK, M = c.bs, c.heads, c.npix, c.L, c.OBJ, c.TOK, c.M
    maps, masks, inv_len = [m.to(dt) for m in c.maps], c.masks.to(dt), c.inv_len.to(dt)
    z = lambda *s: torch.zeros(s, dtype=dt)
    num, den, g_num, g_den = z(M, bs, heads, TOK), z(M, bs, heads, TOK), z(M, bs, heads, TOK), z(M, bs, heads, TOK)
    avg, g_avg, damap = torch.full((bs, TOK, npix), AVG0, dtype=dt), z(bs, TOK, npix), z(M, bs, heads, npix, L)
    act_all = torch.full((M, bs, TOK), NAN, dtype=dt)
    col_of = lambda b, t: int(c.tok_idx[b, t])
    row_of = lambda b, t: min(max(int(c.tok_obj[b, t]), 0), OBJ - 1)
    for b in range(bs):
        for t in range(c.nt[b]):
            for m in range(M):
                v = maps[m][b, :, :, col_of(b, t)] if 0 <= col_of(b, t) < L else z(heads, npix)
                num[m, b, :, t] = (v * masks[b, row_of(b, t)]).sum(-1)
                den[m, b, :, t] = v.sum(-1)
                avg[b, t] += v.sum(0) / heads
    tl, pl = z(), z()
    for b in range(bs):
        nt, no = c.nt[b], min(c.nobj[b], OBJ)
        if nt == 0:
            continue
        n, d = num[:, b, :, :nt], den[:, b, :, :nt]
        act = (n / d).sum(1) / heads  # [M, nt]
        act_all[:, b, :nt] = act
        w = inv_len[b, :nt] / (c.nobj[b] * bs)
        tl = tl + (w * (1.0 - act) ** 2).sum()
        ga = (-2.0 * w * (1.0 - act) / heads)[:, None, :]
        g_num[:, b, :, :nt] = ga / d
        g_den[:, b, :, :nt] = -ga * n / (d * d)
        for i in range(no):
            ts = [t for t in range(nt) if int(c.tok_obj[b, t]) == i]
            p = avg[b, ts].sum(0) / M if ts else z(npix)
            y = masks[b, i]
            lp, lq = torch.log(p), torch.log(1.0 - p)
            cp, cq = torch.where(lp < -100.0, torch.full_like(lp, -100.0), lp), torch.where(lq < -100.0, torch.full_like(lq, -100.0), lq)
            carried = torch.where(torch.isnan(p), p, torch.zeros_like(p))
            dcp, dcq = torch.where(lp >= -100.0, 1.0 / p, carried), torch.where(lq >= -100.0, -1.0 / (1.0 - p), carried)
            pl = pl + ((y - 1.0) * cq - y * cp).sum() / npix / no / bs
            if ts:
                g_avg[b, ts] = (((y - 1.0) * dcq - y * dcp) / (no * npix * bs * M))[None].expand(len(ts), npix)
    for m in range(M):
        for b in range(bs):
            for t in range(c.nt[b]):
                if 0 <= col_of(b, t) < L:
                    damap[m, b, :, :, col_of(b, t)] += (GO[0] * (g_num[m, b, :, t, None] * masks[b, row_of(b, t)][None] + g_den[m, b, :, t, None])
                                                        + GO[1] * g_avg[b, t][None] / heads)
    return types.SimpleNamespace(num=num, den=den, avg=avg, out=torch.stack([tl, pl]), g_num=g_num, g_den=g_den, g_avg=g_avg,
                                 damap=damap, act=act_all)


_CASES = {}


def case_of(key, make):
    """a case and its fp64 reference, computed once per module and left unchanged"""
    if key not in _CASES:
        _CASES[key] = make()
    return _CASES[key]


# ---- calling the entry points -----------------------------------------------------------------------------------------------
def run(k, dev, c, off=0, reuse=None):
    """M gather_fwd calls, one loss call, M gather_bwd calls on guarded buffers; map and damap bases `off` elements off their
    16-byte boundary.  reuse: an earlier run whose forward and loss outputs feed the gather_bwd calls alone."""
    M, bs, heads, npix, L, OBJ, TOK = c.M, c.bs, c.heads, c.npix, c.L, c.OBJ, c.TOK
    G = lambda shape, dtype=F32, fill=None, o=0: Guarded(shape, dtype, dev, fill, o)
    r = types.SimpleNamespace(c=c)
    tab = reuse.tab if reuse else {n: getattr(c, n).to(dev) for n in ("masks", "n_obj", "n_tok", "tok_idx", "tok_obj", "inv_len")}
    r.tab = tab
    dims = dict(bs=bs, heads=heads, npix=npix, OBJ=OBJ, TOK=TOK)
    gather = dict(masks=tab["masks"], n_obj=tab["n_obj"], n_tok=tab["n_tok"], tok_idx=tab["tok_idx"], tok_obj=tab["tok_obj"], L=L, **dims)
    if reuse is None:
        nws = k.attrcon_workspace_floats(M, bs, heads, npix, TOK)
        assert nws >= max(bs * heads * TOK * (-(-npix // 128) * 2 + npix), bs * -(-npix // 256))
        r.amap = [G((bs * heads, npix, L), c.dtype, o=off).put(m) for m in c.maps]
        r.num, r.den, r.g_num, r.g_den = (G((M, bs, heads, TOK)) for _ in range(4))
        r.avg, r.g_avg, r.out, r.ws = G((bs, TOK, npix), fill=AVG0), G((bs, TOK, npix)), G((2,)), G((nws,))
        for x in (r.num, r.den, r.g_num, r.g_den, r.avg, r.g_avg, r.out, r.ws):
            x.arm()
        r.fwd_args = [dict(amap=r.amap[m].view, num=r.num.view[m], den=r.den.view[m], avg=r.avg.view, ws=r.ws.view, **gather) for m in range(M)]
        r.loss_args = dict(num=r.num.view, den=r.den.view, avg=r.avg.view, masks=tab["masks"], n_obj=tab["n_obj"], n_tok=tab["n_tok"],
                           tok_obj=tab["tok_obj"], inv_len=tab["inv_len"], g_num=r.g_num.view, g_den=r.g_den.view, g_avg=r.g_avg.view,
                           out=r.out.view, ws=r.ws.view, M=M, **dims)
        for a in r.fwd_args:
            r.ws.view.fill_(NAN)  # the workspace carries no state between calls
            k.attrcon_gather_fwd(**a)
        r.ws.view.fill_(NAN)
        k.attrcon_loss(**r.loss_args)
    else:
        for n in ("num", "den", "g_num", "g_den", "avg", "g_avg", "out", "ws"):
            setattr(r, n, getattr(reuse, n))
    r.go = torch.tensor(GO, dtype=F32, device=dev)
    r.damap = [G((bs * heads, npix, L), c.dtype, o=off).arm() for _ in range(M)]
    r.bwd_args = [dict(g_num=r.g_num.view[m], g_den=r.g_den.view[m], g_avg=r.g_avg.view, go=r.go, damap=r.damap[m].view, **gather) for m in range(M)]
    for a in r.bwd_args:
        k.attrcon_gather_bwd(**a)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    r.cpu = types.SimpleNamespace(damap=torch.stack([d.get() for d in r.damap]).view(M, bs, heads, npix, L),
                                  **{n: getattr(r, n).get() for n in ("num", "den", "avg", "out", "g_num", "g_den", "g_avg")})
    return r


OUTPUTS = ("num", "den", "avg", "out", "g_num", "g_den", "g_avg", "damap")


def units(c, res):
    """(quantity, label, values) of everything the header lists as written: num, den, avg, g_avg per sample, g_num, g_den per
    (sample, map), the two scalars each on its own, damap per (map, sample, head)"""
    for b in range(c.bs):
        nt = c.nt[b]
        if nt:
            for q in ("num", "den"):
                yield q, f"{q} [sample {b}]", getattr(res, q)[:, b, :, :nt]
            for q in ("avg", "g_avg"):
                yield q, f"{q} [sample {b}]", getattr(res, q)[b, :nt]
            for m in range(c.M):
                for q in ("g_num", "g_den"):
                    yield q, f"{q} [sample {b}, map {m}]", getattr(res, q)[m, b, :, :nt]
        for m in range(c.M):
            for h in range(c.heads):
                yield "damap", f"damap [map {m}, sample {b}, head {h}]", res.damap[m, b, h]
    yield "out", "out[0], the token loss", res.out[0:1]
    yield "out", "out[1], the pixel loss", res.out[1:2]


def unit_err(got, ref, what):
    """helpers.check's quantity, max |got - ref| / (max |ref| + 1e-6), with a NaN of the reference a NaN that must be carried"""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaNs at {torch.nonzero(torch.isnan(got) != nan)[:4].tolist()} (a NaN is carried, and only where the reference has one)"
    got, ref = got.masked_fill(nan, 0.0), ref.masked_fill(nan, 0.0)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    return float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-6)


def bound_of(q):
    return tol(F32) * (2 if q == "damap" else 1)


def headroom(c):
    """the precondition: the reference's formulas in torch fp32 within a tenth of every bound (test_value_ranges.headroom)"""
    r32 = reference(c, F32)
    for (q, what, a), (_, _, b) in zip(units(c, r32), units(c, c.ref)):
        e = unit_err(a, b, what + " in fp32")
        WORST[q] = max(WORST.get(q, 0.0), e / bound_of(q))
        assert e < bound_of(q) / 10, f"{what}: plain fp32 is {e:.2e} from fp64 - the inputs ask more than the bound / 10"


def written(c):
    tokw = torch.tensor([[t < c.nt[b] for t in range(c.TOK)] for b in range(c.bs)])
    return tokw[None, :, None, :].expand(c.M, c.bs, c.heads, c.TOK), tokw[:, :, None].expand(c.bs, c.TOK, c.npix)


def assert_untouched(c, r, what):
    """guards, and every element the header does not list as written"""
    nd, av = written(c)
    for n in ("num", "den", "g_num", "g_den"):
        getattr(r, n).assert_kept(f"{what}: {n}", ~nd)
    for n in ("avg", "g_avg"):
        getattr(r, n).assert_kept(f"{what}: {n}", ~av)
    for n, x in [("out", r.out), ("ws", r.ws)] + [(f"damap {m}", d) for m, d in enumerate(r.damap)]:
        x.assert_kept(f"{what}: {n}")


def verify(c, r, what, skip=()):
    assert_untouched(c, r, what)
    for (q, label, got), (_, _, ref) in zip(units(c, r.cpu), units(c, c.ref)):
        if q in skip:
            continue
        if q == "damap" and c.dtype == BF16:
            assert got.dtype == BF16
            lim = 2.0 ** -8 * ref.abs() + bound_of(q) * float(ref.abs().max())
            bad = ~((got.double() - ref).abs() <= lim)  # (a NaN is bad)
            assert not bool(bad.any()), (f"{what}: {label}: {int(bad.sum())} of {bad.numel()} elements beyond 2^-8 |ref| + {bound_of(q)} max|ref|, first at "
                                         f"{tuple(torch.nonzero(bad)[0].tolist())}")
        else:
            e = unit_err(got, ref, f"{what}: {label}")
            assert e < bound_of(q), f"{what}: {label}: max err / scale {e:.3e} (bound {bound_of(q)})"
    for b in range(c.bs):
        if c.nt[b] == 0:
            assert bool((r.cpu.damap[:, b] == 0).all()), f"{what}: damap of skipped sample {b} is not all zeros"


def assert_same_outputs(a, b, what, names=OUTPUTS):
    for n in names:
        assert same_bits(getattr(a.cpu, n), getattr(b.cpu, n)), f"{what}: {n} differs in bits"


# ---- 1. the variants of the gather and of the gradient writer ---------------------------------------------------------------
VARIANTS = [(16, 11), (9, 11), (300, 12), (257, 11), (16, 127), (16, 128), (16, 130)]


def tokens3(L):
    """sample 1 skipped; column 0 and the last column named"""
    return [[(2, 0), (L - 1, 0), (0, 1)], None, [(5, 0), (3, 0)]]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("npix, L", VARIANTS)
def test_gather_variants_aligned_and_one_element_off(attrcon_dev, npix, L, dtype):
    """every shape from an aligned base (the form chunks_vectorise picks for it: module docstring) and from a base one element off
    16 bytes (plain by the pointer).  The two gradient writers give the same bits from the same g_*; a bf16 map's num / den / avg
    agree bit for bit (256-row chunks in both forms), an fp32 map's only within the bound (128 vs 256 rows)."""
    c = case_of(("variant", npix, L, dtype), lambda: make_case(npix, L, dtype, tokens3(L), seed=npix + L))
    headroom(c)
    k = ops.attrcon_kernels()
    r0 = run(k, attrcon_dev, c)
    verify(c, r0, "aligned")
    r1 = run(k, attrcon_dev, c, off=1)
    verify(c, r1, "one element off")
    r2 = run(k, attrcon_dev, c, off=1, reuse=r0)  # the same g_*, the other writer
    assert_same_outputs(r0, r2, "gradient writer, aligned vs one element off", ("damap",))
    if dtype == BF16:
        assert_same_outputs(r0, r1, "bf16 map, aligned vs one element off")


# ---- 2. table edges, 3. repeated columns, 4. an object without tokens -----------------------------------------------------
A, B = [(2, 0), (4, 0), (7, 1)], [(5, 0), (3, 0)]
FORTY = [(i, i // 8) for i in range(40)]
EDGES = {
    "heads_1": dict(toks=[A, None, B], heads=1),
    "bs_1": dict(toks=[A]),
    "TOK_1": dict(toks=[[(3, 0)], None, [(5, 0)]]),
    "TOK_40_next_to_2": dict(toks=[FORTY, [(3, 0), (9, 1)]], L=41),
    "skipped_first": dict(toks=[None, A, B]),
    "skipped_last": dict(toks=[A, B, None]),
    "all_skipped": dict(toks=[None, None, None], TOK=2, OBJ=1),
    "n_tok_above_TOK_and_negative": dict(toks=[A, None, B], n_obj=[2, 0, 1], n_tok=[8, 1, -3]),
    "first_and_last_column": dict(toks=[[(0, 0), (10, 1)], None, [(10, 0), (0, 0)]]),
    "column_named_by_two_objects": dict(toks=[[(2, 0), (4, 0), (4, 1), (6, 1)], None, B]),
    "column_named_twice_by_one_object": dict(toks=[[(4, 0), (4, 0), (6, 1)], None, B]),
    "column_named_three_times": dict(toks=[[(4, 0), (2, 0), (4, 1), (4, 0)], None, [(3, 0), (3, 0), (3, 0)]]),
    "object_without_tokens": dict(toks=[[(2, 0), (4, 0)], None, B], n_obj=[2, 0, 1]),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("npix", [16, 9], ids=["staged", "plain"])
@pytest.mark.parametrize("name", list(EDGES))
def test_table_edges(attrcon_dev, name, npix, dtype):
    """the forward treats every mention of a column on its own, damap is their sum in ascending t; n_tok is clamped into [0, TOK]
    as sample_tokens does (a negative count skips the sample); all samples skipped: no output touched but out = (0, 0) and damap,
    all zeros"""
    kw = dict(EDGES[name])
    c = case_of(("edge", name, npix, dtype), lambda: make_case(npix, kw.pop("L", 11), dtype, kw.pop("toks"), seed=len(name), **kw))
    headroom(c)
    r = run(ops.attrcon_kernels(), attrcon_dev, c)
    verify(c, r, name)
    if name == "all_skipped":
        assert same_bits(r.cpu.out, torch.zeros(2)) and bool((r.cpu.damap == 0).all())
    if name == "n_tok_above_TOK_and_negative":
        assert c.nt == [3, 0, 0]
    if name == "object_without_tokens":  # its word is 0: the pixel loss gains 100 * mean(mask) for it, weighted 1 / (n_obj bs)
        one, none = types.SimpleNamespace(**vars(c)), types.SimpleNamespace(**vars(c))
        one.nobj, none.nt = [1, 0, 1], [0, 0, c.nt[2]]  # sample 0 with object 0 alone; sample 0 skipped
        pl_one, rest = float(reference(one, F64).out[1]), float(reference(none, F64).out[1])
        gain = 100.0 * float(c.masks[0, 1].double().mean()) / (2 * c.bs)
        assert gain > 0 and abs(float(c.ref.out[1]) - ((pl_one - rest) / 2 + gain + rest)) < 1e-12


@pytest.mark.parametrize("npix", [16, 9], ids=["staged", "plain"])
def test_column_outside_the_map_has_the_value_0_and_no_gradient(attrcon_dev, npix):
    """tok_idx = L and tok_idx = -1: num = den = 0, nothing added to avg, so the token loss is the carried 0 / 0 - exactly that;
    the other tokens, the pixel loss and every gradient are what they are without the two"""
    c = case_of(("outside", npix), lambda: make_case(npix, 11, F32, [[(2, 0), (11, 0), (-1, 1), (4, 1)], None, B]))
    headroom(c)
    r = run(ops.attrcon_kernels(), attrcon_dev, c)
    verify(c, r, "column outside the map")
    for t in (1, 2):
        assert bool((r.cpu.num[:, 0, :, t] == 0).all()) and bool((r.cpu.den[:, 0, :, t] == 0).all())
        assert same_bits(r.cpu.avg[0, t], torch.full((npix,), AVG0))
        assert bool(torch.isnan(r.cpu.g_num[:, 0, :, t]).all()) and bool(torch.isnan(r.cpu.g_den[:, 0, :, t]).all())
    assert math.isnan(float(r.cpu.out[0])) and math.isfinite(float(r.cpu.out[1]))
    assert bool(torch.isfinite(r.cpu.damap).all()) and bool(torch.isfinite(r.cpu.g_num[:, 0, :, [0, 3]]).all())


@pytest.mark.parametrize("npix", [16, 9], ids=["staged", "plain"])
def test_object_index_outside_the_table_picks_a_clamped_mask_row(attrcon_dev, npix):
    """tok_obj = 5 and -3 with OBJ = 2: the gather takes mask rows 1 and 0; the loss call counts the two tokens towards no object,
    so the pixel loss is that of the others and their g_avg rows are left alone (which leaves gather_bwd nothing defined to read
    there: g_avg and damap are not compared)"""
    c = case_of(("tok_obj", npix), lambda: make_case(npix, 11, F32, [[(2, 0), (4, 1), (6, 5), (7, -3)], None, B], n_obj=[2, 0, 1], OBJ=2))
    headroom(c)
    r = run(ops.attrcon_kernels(), attrcon_dev, c)
    verify(c, r, "tok_obj outside [0, OBJ)", skip=("g_avg", "damap"))
    keep = torch.zeros(c.bs, c.TOK, npix, dtype=torch.bool)
    keep[0, 2:] = True
    r.g_avg.assert_kept("g_avg of the tokens without an object", keep)
    assert bool(torch.isfinite(r.cpu.g_avg[0, :2]).all())


# ---- 5. exact cases -----------------------------------------------------------------------------------------------------------
EXACT_TOKS = [[(1, 0), (3, 1), (5, 1)], [(0, 0), (2, 0), (4, 0), (10, 0)]]  # objects of 1, 2 and 4 tokens: inv_len dyadic


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("npix", [16, 9], ids=["staged", "plain"])
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("mask_value", [1, 0], ids=["full_masks", "empty_masks"])
def test_full_and_empty_masks_exactly(attrcon_dev, mask_value, M, npix, dtype):
    c = case_of(("exact", mask_value, M, npix, dtype), lambda: make_case(npix, 11, dtype, EXACT_TOKS, M=M, mask_value=mask_value, seed=M))
    r = run(ops.attrcon_kernels(), attrcon_dev, c)
    assert_untouched(c, r, "exact")
    o, nd = r.cpu, written(c)[0]
    if mask_value:  # v * 1 = v and the same order of sums: num is den, act = 1, the token loss and its derivatives are 0
        assert same_bits(o.num, o.den) and float(o.out[0]) == 0.0
        assert bool((o.g_num[nd] == 0).all()) and bool((o.g_den[nd] == 0).all())
        # damap = go[0] (g_num mask + g_den) + go[1] g_avg / heads: the token part is what is left at go[1] = 0
        r.go.copy_(torch.tensor([GO[0], 0.0]))
        for a in r.bwd_args:
            ops.attrcon_kernels().attrcon_gather_bwd(**a)
        assert bool(torch.isfinite(o.g_avg[written(c)[1]]).all()) and all(bool((d.get() == 0).all()) for d in r.damap)
    else:  # v * 0 = 0: act = 0, every token adds inv_len / (n_obj bs) - dyadic, so no order of sums rounds - and the tokens of
        # a sample add up to 1 / bs per map: out[0] = M * (active samples) / bs = M * 2 / 2
        assert bool((o.num[nd] == 0).all()) and float(o.out[0]) == float(M)
    assert unit_err(o.out[1:2], c.ref.out[1:2], "pixel loss") < tol(F32)


# ---- 6. the clamps of the pixel loss -----------------------------------------------------------------------------------------
def loss_of_one_pixel(k, dev, word, mask):
    """comat_attrcon_loss on hand-made num / den / avg: one sample, head, object, token, pixel and map, so that out[1] is the
    loss of that pixel and g_avg its derivative; num / den = 1 / 2"""
    G = lambda shape, fill=None: Guarded(shape, F32, dev, fill).arm()
    one = lambda v, dt: torch.tensor([v], dtype=dt, device=dev)
    b = types.SimpleNamespace(num=Guarded((1,), F32, dev, 0.5), den=Guarded((1,), F32, dev, 1.0), avg=Guarded((1,), F32, dev).put(one(word, F32)),
                              g_num=G((1,)), g_den=G((1,)), g_avg=G((1,)), out=G((2,)), ws=G((k.attrcon_workspace_floats(1, 1, 1, 1, 1),)))
    k.attrcon_loss(num=b.num.view, den=b.den.view, avg=b.avg.view, masks=one(mask, F32), n_obj=one(1, torch.int32), n_tok=one(1, torch.int32),
                   tok_obj=one(0, torch.int32), inv_len=one(1.0, F32), g_num=b.g_num.view, g_den=b.g_den.view, g_avg=b.g_avg.view,
                   out=b.out.view, ws=b.ws.view, M=1, bs=1, heads=1, npix=1, OBJ=1, TOK=1)
    for n in ("g_num", "g_den", "g_avg", "out", "ws"):
        getattr(b, n).assert_kept(n)
    return b.out.get(), float(b.g_avg.get())


def test_clamps_of_the_pixel_loss(attrcon_dev):
    k = ops.attrcon_kernels()
    clean, d_mid = loss_of_one_pixel(k, attrcon_dev, 0.5, 1.0)
    assert float(clean[0]) == 0.25 and abs(float(clean[1]) - math.log(2.0)) < tol(F32) and abs(d_mid + 2.0) < 2.0 * tol(F32)
    # (word, mask) -> (loss, derivative): a clamped logarithm has the derivative 0, the other one its own
    for (word, mask), (loss, deriv) in {(0.0, 0.0): (0.0, 1.0), (0.0, 1.0): (100.0, 0.0), (1.0, 0.0): (100.0, 0.0), (1.0, 1.0): (0.0, -1.0)}.items():
        out, d = loss_of_one_pixel(k, attrcon_dev, word, mask)
        assert float(out[1]) == loss and d == deriv and same_bits(out[0:1], clean[0:1]), (word, mask, out, d)
    for word in (1.0 + 2.0 ** -20, NAN):  # log of a negative number, a NaN: carried into out[1], not trapped; out[0] as it was
        for mask in (0.0, 1.0):
            out, d = loss_of_one_pixel(k, attrcon_dev, word, mask)
            assert math.isnan(float(out[1])) and same_bits(out[0:1], clean[0:1]), (word, mask, out)


# ---- 7. non-finite inputs, 8. two calls ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("npix", [16, 9], ids=["staged", "plain"])
def test_non_finite_values_stay_in_their_sample(attrcon_dev, npix, dtype):
    toks = [A, None, B, A]
    c = case_of(("nonfinite", npix, dtype), lambda: make_case(npix, 11, dtype, toks, seed=3))
    k = ops.attrcon_kernels()
    clean = run(k, attrcon_dev, c)
    verify(c, clean, "clean")
    # the columns no token names hold NaN in `c`: with finite values there instead, no bit anywhere changes
    filled = make_case(npix, 11, dtype, toks, seed=3, poison_unnamed=False)
    assert all(bool(torch.isfinite(m[[0, 2, 3]]).all()) for m in filled.maps)
    assert_same_outputs(clean, run(k, attrcon_dev, filled), "unnamed columns finite instead of NaN")
    for poison in (NAN, float("inf")):
        bad = types.SimpleNamespace(**vars(c))
        bad.maps = [m.clone() for m in c.maps]
        bad.maps[1][0, 0, 3, 4] = poison  # sample 0, head 0, pixel 3, the column of token 1
        r = run(k, attrcon_dev, bad)
        assert_untouched(bad, r, f"{poison}")
        assert not math.isfinite(float(r.cpu.out[0])) and not math.isfinite(float(r.cpu.out[1]))
        assert not bool(torch.isfinite(r.cpu.damap[:, 0].float()).all()), "the poison did not reach sample 0's gradient"
        for n in ("damap", "num", "den"):
            for b in (1, 2, 3):
                assert same_bits(getattr(r.cpu, n)[:, b], getattr(clean.cpu, n)[:, b]), f"{poison} in sample 0 changed {n} of sample {b}"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_two_calls_give_the_same_bits(attrcon_dev, dtype):
    c = case_of(("variant", 300, 12, dtype), lambda: make_case(300, 12, dtype, tokens3(12), seed=312))
    k = ops.attrcon_kernels()
    assert_same_outputs(run(k, attrcon_dev, c), run(k, attrcon_dev, c), "two calls")


# ---- 9. comat_mask_resize_any -------------------------------------------------------------------------------------------------
def resize_call(k, dev, src, win, n, H, W, res, off=0):
    s = Guarded(tuple(src.shape), torch.uint8, dev, off=off).put(src)
    out = Guarded((max(n, 1), res * res), F32, dev).arm()
    w = [torch.as_tensor(np.ascontiguousarray(x), dtype=torch.int32).to(dev) for x in win]
    k.mask_resize_any(s.view, w[0], w[1], w[2], w[3], out.view, n, H, W, res)
    out.assert_kept(f"resize {H} x {W} -> {res}, {off} bytes off")
    return out.get()


def mask_bytes(n, H, W, seed):
    """[n, H, W] uint8: sparse random, empty, one pixel in the last corner (beyond 3: sparse random); set bytes are 1, 2 or 255"""
    rng = np.random.default_rng(seed)
    m = rng.random((n, H, W)) < 0.03
    m[1] = False
    m[2] = False
    m[2, H - 1, W - 1] = True
    return m, torch.from_numpy(np.where(m, rng.choice(np.array([1, 2, 255], dtype=np.uint8), size=m.shape), 0).astype(np.uint8))


# res > one block's threads; the LDS clear loop strides (W > 4096); one column; one row; every row at another alignment
@pytest.mark.parametrize("H, W, res, offs", [(8, 8, 300, (0,)), (2, 5000, 4, (0,)), (5, 1, 3, (0,)), (1, 17, 2, (0,)), (33, 47, 7, (1, 5, 15))])
def test_resize_beyond_the_shapes_of_the_loss(attrcon_dev, H, W, res, offs):
    m, src = mask_bytes(3, H, W, H + W)
    ref = losses.resize_masks(m, res)
    win = np.concatenate([losses.any_windows(H, res), losses.any_windows(W, res)])
    for off in offs:
        got = resize_call(ops.attrcon_kernels(), attrcon_dev, src, win, 3, H, W, res, off)
        assert np.array_equal(got.numpy(), ref), f"{off} bytes off"


def test_resize_clamps_its_windows_and_n_0_writes_nothing(attrcon_dev):
    """windows that start below 0, end beyond H / W, and an empty one (lo == hi: 0)"""
    H, W, res, k = 6, 7, 3, ops.attrcon_kernels()
    m, src = mask_bytes(4, H, W, 9)
    m[3] = True
    src[3] = 255
    win = np.array([[-2, 4, 3], [2, 9, 3], [0, -1, 6], [7, 3, 12]], dtype=np.int32)
    ref = np.zeros((4, res, res), dtype=np.float32)
    for oy in range(res):
        for ox in range(res):
            ref[:, oy, ox] = m[:, max(win[0, oy], 0):min(win[1, oy], H), max(win[2, ox], 0):min(win[3, ox], W)].any((1, 2))
    assert ref[3].tolist() == [[1, 1, 1], [1, 1, 1], [0, 0, 0]]
    assert np.array_equal(resize_call(k, attrcon_dev, src, win, 4, H, W, res).numpy().reshape(4, res, res), ref)
    assert bool(torch.isnan(resize_call(k, attrcon_dev, src, win, 0, H, W, res)).all())  # n = 0: out untouched (and its guards)


# ---- 10. refusals by name -----------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_name(attrcon_dev):
    dev, k = attrcon_dev, ops.attrcon_kernels()
    c = case_of(("variant", 16, 11, F32), lambda: make_case(16, 11, F32, tokens3(11), seed=27))
    r = run(k, dev, c)
    after = {n: getattr(r, n).get() for n in ("num", "den", "avg", "g_num", "g_den", "g_avg", "out")}
    u8 = torch.zeros(c.bs * c.heads * c.npix * c.L, dtype=torch.uint8, device=dev)
    refused = [("attrcon_gather_fwd", r.fwd_args[0], ch) for ch in (dict(masks=None), dict(ws=None), dict(bs=0), dict(heads=65536), dict(amap=u8))]
    refused += [("attrcon_loss", r.loss_args, ch) for ch in (dict(inv_len=None), dict(out=None), dict(bs=0), dict(heads=65536), dict(M=0), dict(M=1025))]
    refused += [("attrcon_gather_bwd", r.bwd_args[0], ch) for ch in (dict(go=None), dict(g_avg=None), dict(bs=0), dict(heads=65536), dict(damap=u8))]
    for fn, good, change in refused:
        with pytest.raises(RuntimeError, match=rf"comat_{fn} failed \(rc=-1\): comat_{fn}"):
            getattr(k, fn)(**{**good, **change})
    z = torch.zeros(4, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match=r"comat_mask_resize_any failed \(rc=-1\): comat_mask_resize_any"):
        k.mask_resize_any(torch.zeros(32769, dtype=torch.uint8, device=dev), z, z, z, z, torch.zeros(16, device=dev), 1, 1, 32769, 4)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    for n, x in after.items():
        assert same_bits(getattr(r, n).get(), x), f"a refused call wrote {n}"
    assert k.attrcon_workspace_floats(0, 1, 1, 1, 1) == 0 and k.attrcon_workspace_floats(1, 1, 1, 1, 1) == 3
