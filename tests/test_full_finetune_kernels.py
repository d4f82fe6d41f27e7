"""comat_weights_refresh, comat_layernorm_bwd_affine, comat_colsum_batched (include/comat_hip.h): the entry points of a fully
trained UNet (`--full_finetuning`, training_utils/pipeline.py:60-61).

Every case runs on the ABI simulator (tests/sim_backend.py) and, marked gpu, on the library.  The two reductions are held to
fp64 sums of the same (bf16-rounded) operands under helpers.check(..., dtype), the bound tests/test_conv_wgrad.py uses.  The refresh
is a copy with one rounding: it is compared bit for bit with torch (`master.to(bf16)`, `.t()`, `.flip(1, 2).permute(3, 1, 2, 0)`), every
destination inside a NaN halo that must survive.  The tile table is enumerated on the CPU first: every destination element of every
problem is written exactly once.
"""
import functools

import numpy as np
import pytest
import torch

from comat_amd import refresh
from helpers import check

F32, BF16 = torch.float32, torch.bfloat16


def kernels():
    from comat_amd import ops
    return ops.kernels()


# ---- comat_layernorm_bwd_affine --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ln_data(M, C, dtype):
    """dy, x rounded to dtype, the statistics the forward saves, initial dgamma / dbeta and the fp64 result; shared, never written"""
    g = torch.Generator().manual_seed(1000 * M + C)
    x = (torch.randn(M, C, generator=g) * 1.5 + 0.3).to(dtype)
    dy = torch.randn(M, C, generator=g).to(dtype)
    d0, b0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    xd = x.double()
    mean, rstd = xd.mean(-1, keepdim=True), (xd.var(-1, unbiased=False, keepdim=True) + 1e-5).rsqrt()
    stats = torch.cat([mean, rstd], -1).float()
    xh = (xd - stats[:, :1].double()) * stats[:, 1:].double()  # xhat as the contract defines it: from the SAVED fp32 statistics
    return dy, x, stats, d0, b0, d0.double() + (dy.double() * xh).sum(0), b0.double() + dy.double().sum(0)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", [8, 24, 320, 1280])
@pytest.mark.parametrize("M", [1, 7, 64, 4099])
def test_layernorm_bwd_affine(dev, M, C, dtype):
    dy, x, stats, d0, b0, rg, rb = ln_data(M, C, dtype)
    args = (dy.to(dev), x.to(dev), stats.to(dev))
    dgamma, dbeta = d0.clone().to(dev), b0.clone().to(dev)  # non-zero: the result is accumulated
    kernels().layernorm_bwd_affine(*args, dgamma, dbeta, M, C)
    for name, got, ref in (("dgamma", dgamma, rg), ("dbeta", dbeta, rb)):
        err = (got.cpu().double() - ref).abs().max().item() / (ref.abs().max().item() + 1e-6)
        print(f"layernorm_bwd_affine {M}x{C} {dtype} {name}: max err / max |ref| = {err:.3e}")
        check(got, ref, dtype, f"layernorm_bwd_affine {M}x{C} {name}")
    dg2, db2 = d0.clone().to(dev), b0.clone().to(dev)  # the same inputs give the same bits
    kernels().layernorm_bwd_affine(*args, dg2, db2, M, C)
    assert torch.equal(dg2, dgamma) and torch.equal(db2, dbeta), "two runs differ"
    dg3, db3 = d0.clone().to(dev), b0.clone().to(dev)  # no scratch: one long chunk, the same values within the bound
    kernels().layernorm_bwd_affine(*args, dg3, db3, M, C, scratch=False)
    check(dg3, rg, dtype, f"layernorm_bwd_affine {M}x{C} dgamma, no scratch")
    check(db3, rb, dtype, f"layernorm_bwd_affine {M}x{C} dbeta, no scratch")


def test_layernorm_bwd_affine_refusals(dev):
    k = kernels()
    M, C = 4, 8
    t = lambda *s: torch.zeros(*s, dtype=F32, device=dev)
    ok = [t(M, C), t(M, C), t(M, 2), t(C), t(C)]
    for nul in range(5):
        a = list(ok)
        a[nul] = None
        with pytest.raises(RuntimeError, match="comat_layernorm_bwd_affine"):
            k.layernorm_bwd_affine(*a, M, C)
    with pytest.raises(RuntimeError, match="comat_layernorm_bwd_affine"):
        k.layernorm_bwd_affine(*ok, M, 0)
    assert float(ok[3].abs().max()) == 0.0 and float(ok[4].abs().max()) == 0.0  # nothing was launched


# ---- comat_colsum_batched --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", [(1, 1, 3, 3), (2, 4, 4, 4), (3, 64, 24, 24), (2, 4099, 320, 320), (3, 4099, 24, 40), (1, 64, 320, 320),
                                   (3, 1, 4, 4), (2, 4, 3, 3)], ids=lambda s: "x".join(map(str, s)))
def test_colsum_batched(dev, shape, dtype):
    B, M, C, ld = shape
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B * M, ld, generator=g).to(dtype)
    ref = x[:, :C].double().reshape(B, M, C).sum(1)
    xd = x.to(dev)
    out = torch.full((B, C), float("nan"), dtype=F32, device=dev)  # the output is written, not accumulated
    kernels().colsum_batched(xd, out, B, M, C, ld)
    err = (out.cpu().double() - ref).abs().max().item() / (ref.abs().max().item() + 1e-6)
    print(f"colsum_batched {shape} {dtype}: max err / max |ref| = {err:.3e}")
    check(out, ref, F32, f"colsum_batched {shape}")
    again = torch.full((B, C), float("nan"), dtype=F32, device=dev)
    kernels().colsum_batched(xd, again, B, M, C, ld)
    assert torch.equal(again, out), "two runs differ"


def test_colsum_batched_refusals(dev):
    k = kernels()
    x, out = torch.zeros(8, 4, dtype=F32, device=dev), torch.zeros(2, 4, dtype=F32, device=dev)
    for a in ((None, out, 2, 4, 4, 4), (x, None, 2, 4, 4, 4), (x, out, 0, 4, 4, 4), (x, out, 2, 0, 4, 4), (x, out, 2, 4, 0, 4),
              (x, out, 2, 4, 4, 3)):
        with pytest.raises(RuntimeError, match="comat_colsum_batched"):
            k.colsum_batched(*a)


# ---- comat_weights_refresh -------------------------------------------------------------------------------------------------
# one table over all of these: ("lin", N, K) / ("conv", Cout, k, Cin); odd sizes and sizes over one tile each way
# order: the sizes that are multiples of 8 first (each starts on a 16-element boundary: the 16-byte paths, (128, 64) with two row
# tiles, (32, 3, 96) with two column tiles), then the odd ones ((65, 63): two row tiles, element by element, unaligned start)
LAYERS = [("lin", 24, 32), ("lin", 128, 64), ("conv", 32, 3, 4), ("conv", 4, 3, 32), ("conv", 32, 3, 96), ("conv", 24, 1, 40),
          ("lin", 5, 7), ("lin", 65, 63)]
HALO = 11  # elements between two destinations: odd, so that a destination behind an odd-sized one is NOT 16-byte aligned


def refresh_layout(layers=LAYERS, halo=HALO):
    """[(layer, master offset, destination offset)], buffer length, problem rows.  A layer whose element count is a multiple of 8
    is followed by a 16-element boundary, any other by the bare halo: (24, 32), (128, 64) and the convs start aligned (16-byte rows
    wherever their pitch allows), (65, 63) does not (element by element)."""
    place, problems, off = [], [], 16
    for L in layers:
        n = L[1] * L[2] if L[0] == "lin" else L[1] * L[2] * L[2] * L[3]
        place.append((L, off, off))
        if L[0] == "lin":
            problems += refresh.linear_problem(off, off, off, L[1], L[2])
        else:
            problems += refresh.conv_problems(off, off, off, L[1], L[2], L[2], L[3])
        off += n + halo
        if n % 8 == 0:
            off = -(-off // 16) * 16
    return place, off + 16, problems


def test_refresh_tile_table_covers_once():
    """CPU only: over the table of the cases below, every element of every w and of every wt / wd is written exactly once and
    nothing else is"""
    place, n, problems = refresh_layout()
    by_layer = {L: off for L, off, _ in place}
    assert by_layer[("lin", 128, 64)] % 16 == 0 and by_layer[("conv", 32, 3, 96)] % 16 == 0 and by_layer[("lin", 65, 63)] % 8 != 0
    tiles = refresh.tile_table(problems)
    assert tiles.dtype == np.int32 and tiles.shape[1] == 3
    assert (tiles[:, 1] % refresh.TILE == 0).all() and (tiles[:, 2] % refresh.TILE == 0).all()
    cw, ct = refresh.covered(problems, tiles, n, n)
    inside = np.zeros(n, bool)
    for L, off, _ in place:
        cnt = L[1] * L[2] if L[0] == "lin" else L[1] * L[2] * L[2] * L[3]
        inside[off:off + cnt] = True
    assert (cw[inside] == 1).all() and (ct[inside] == 1).all(), "a destination element is missed or written twice"
    assert (cw[~inside] == 0).all() and (ct[~inside] == 0).all(), "the table reaches outside the destinations"
    # and the transposed index really is the flipped-tap data-gradient layout: checked on values below


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_weights_refresh(dev, dtype):
    place, n, problems = refresh_layout()
    g = torch.Generator().manual_seed(23)
    master = torch.randn(n, generator=g)
    nan = float("nan")
    w = None if dtype == F32 else torch.full((n,), nan, dtype=dtype, device=dev)
    wt = torch.full((n,), nan, dtype=dtype, device=dev)
    plan = refresh.RefreshPlan(problems, dev)
    md = master.to(dev)
    plan.run(md, w, wt)
    assert torch.equal(md.cpu(), master), "the master was written"
    wc, wtc = (master if w is None else w.cpu()), wt.cpu()
    untouched_w, untouched_t = torch.ones(n, dtype=torch.bool), torch.ones(n, dtype=torch.bool)
    for L, off, doff in place:
        if L[0] == "lin":
            N, K = L[1:]
            m = master[off:off + N * K].view(N, K)
            got_w, got_t = wc[doff:doff + N * K].view(N, K), wtc[doff:doff + N * K].view(K, N)
            want_t = m.to(dtype).t()
        else:
            Co, k, Ci = L[1:]
            m = master[off:off + Co * k * k * Ci].view(Co, k, k, Ci)
            got_w, got_t = wc[doff:doff + m.numel()].view(Co, k, k, Ci), wtc[doff:doff + m.numel()].view(Ci, k, k, Co)
            want_t = m.to(dtype).flip(1, 2).permute(3, 1, 2, 0)
        assert torch.equal(got_w, m.to(dtype)), f"{L}: w != master.to(dtype)"
        assert torch.equal(got_t, want_t), f"{L}: the second orientation differs"
        untouched_w[doff:doff + m.numel()] = False
        untouched_t[doff:doff + m.numel()] = False
    if w is not None:
        assert torch.isnan(wc[untouched_w].float()).all(), "w: the halo was written"
    assert torch.isnan(wtc[untouched_t].float()).all(), "wt: the halo was written"


def test_weights_refresh_refusals(dev):
    _, n, problems = refresh_layout(LAYERS[:1])
    plan = refresh.RefreshPlan(problems, dev)
    k = kernels()
    m, w, wt = torch.zeros(n, device=dev), torch.zeros(n, dtype=BF16, device=dev), torch.zeros(n, dtype=BF16, device=dev)
    for a in ((None, w, wt, plan.d_problems, plan.d_tiles), (m, w, None, plan.d_problems, plan.d_tiles),
              (m, None, wt, plan.d_problems, plan.d_tiles), (m, w, wt, None, plan.d_tiles), (m, w, wt, plan.d_problems, None),
              (m, w, wt, plan.d_problems, plan.d_tiles[:0])):
        with pytest.raises(RuntimeError, match="comat_weights_refresh"):
            k.weights_refresh(*a)
    assert float(w.float().abs().max()) == 0.0 and float(wt.float().abs().max()) == 0.0  # nothing was launched
