"""Exact integer-operand parity of the block shape of gemm2.hip above tile code 13 - 14: 128 x 128 with 8 waves and 128-byte k-tiles
(bf16 only; falls back to its twin, code 7, where a segment is an odd number of 64-byte k-tiles, a conv has Cin % 64 != 0 or the
operands are fp8) - and of the table that selects it (gemm2_plans_wide.inc).

The method is that of test_exact_products.py: operands are small non-zero integers, every partial sum in any order is an fp32
number (assert_sums_exact), so the stored result is known bit for bit whatever the tile, the k-tile size, the slice count or the
combine order.  The code and the slice count are forced through the options g2_cfg / g2_splits; on the library the cases also
assert which kernel served them.  Shapes are the smallest that reach every path of a shape: one block tile and a ragged remainder
each way (130 rows; BN + 8 columns), contractions of a few k-tiles cut into 1 and into 3 slices."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from helpers import assert_act_exact_pre, assert_exact, assert_sums_exact, ints
from test_exact_products import (CONV_PIXELS, PLAN_ROW, ROOT, WS_BYTES, cdiv, clamp_splits, empty, force, geglu_il_fp64, kern,  # noqa: F401 - force is a fixture
                                 put, served_by, to8)

F32, BF16 = torch.float32, torch.bfloat16
WIDE_TILES = {14: (128, 128)}  # tile code -> (rows, columns) of the block tile (g2_cfgs of gemm2.hip)
K4_TWIN = {14: 7}              # 128-byte k-tile codes and the 64-byte code they fall back to
WIDE_FILE = os.path.join(ROOT, "comat_amd", "csrc", "gemm2_plans_wide.inc")


def slices_run(code, slices, nkt64, ntiles, k4):
    """the slice count plan2 + finish_launch make of a forced code / count: nkt64 = 64-byte k-tiles of the problem, k4 = the
    128-byte k-tile form runs, which counts its slices in those tiles"""
    bm, bn = WIDE_TILES[code]
    s = clamp_splits(slices, ntiles, bm * bn, nkt64, WS_BYTES)
    if k4:
        n2 = nkt64 // 2
        s = min(s, max(n2, 1))
        s = cdiv(n2, cdiv(n2, s))
    return s


def run_gemm(dev, force, code, slices, nkt64, fp8=False, want_slices=None):
    """alpha A B^T + bias + beta R on M = 130, N = BN + 8 under a forced code and count; nkt64 = 64-byte k-tiles of the contraction"""
    bm, bn = WIDE_TILES[code]
    M, N = bm + 2, bn + 8
    K = nkt64 * (64 if fp8 else 32)
    k4 = code in K4_TWIN and not fp8 and nkt64 % 2 == 0
    eff = slices_run(code, slices, nkt64, cdiv(M, bm) * cdiv(N, bn), k4)
    if want_slices is not None:
        assert eff == want_slices, f"code {code}: {nkt64} k-tiles give {eff} slices, the case is about {want_slices}"
    force(gemm2=1, gemm3=0, g2_cfg=code, g2_splits=slices)
    A, B = ints(M, K, seed=500 + code), ints(N, K, seed=600 + slices)
    bias, R = ints(N, seed=3, hi=64), ints(M, N, seed=4, hi=64)
    assert_sums_exact(K, A, B)
    if fp8:
        Ad, Bd = to8(A, dev), to8(B, dev)
        scales = (torch.tensor([2.0], device=dev), torch.tensor([0.25], device=dev))
        alpha, f = 0.5, 0.25
    else:
        Ad, Bd, scales, alpha, f = put(A, dev, BF16), put(B, dev, BF16), None, 0.25, 0.25
    ref = f * (A.double() @ B.double().t()) + bias.double() + 0.5 * R.double()
    for out_dt in (F32, BF16):
        C = empty((M, N), out_dt, dev)
        kern().gemm(Ad, Bd, C, M, N, K, K, K, N, bias=put(bias, dev, F32), R=put(R, dev, BF16), ldr=N, alpha=alpha, beta=0.5,
                    scales=scales)
        served_by(dev, 3 if fp8 else 1)
        assert_exact(C, ref, out_dt, f"gemm code {code} fp8={fp8} slices {slices} ({eff} run) {M}x{N}x{K} out {out_dt}", alpha=f)


def run_conv(dev, force, code, slices, Cin, fp8=False, want_slices=None):
    """conv 3 x 3 pad 1 on 2 x 13 x 5 pixels (130 rows), Cout = BN + 8, with bias, per-sample bias2 and residual"""
    bm, bn = WIDE_TILES[code]
    Bn, H, W = CONV_PIXELS[bm]
    M, Cout = Bn * H * W, bn + 8
    K = 9 * Cin
    nkt64 = K // (64 if fp8 else 32)
    k4 = code in K4_TWIN and not fp8 and Cin % 64 == 0
    eff = slices_run(code, slices, nkt64, cdiv(M, bm) * cdiv(Cout, bn), k4)
    if want_slices is not None:
        assert eff == want_slices, f"code {code}: Cin {Cin} gives {eff} slices, the case is about {want_slices}"
    force(gemm2=1, gemm3=0, g2_cfg=code, g2_splits=slices)
    x, w = ints(Bn, H, W, Cin, seed=700 + code), ints(Cout, 3, 3, Cin, seed=800 + slices)
    bias, bias2, R = ints(Cout, seed=5, hi=64), ints(Bn, Cout, seed=6, hi=64), ints(M, Cout, seed=7, hi=64)
    assert_sums_exact(K, x, w)
    if fp8:
        xd, wd = to8(x, dev), to8(w, dev)
        scales = (torch.tensor([0.5], device=dev), torch.tensor([1.0], device=dev))
        alpha, f = 0.5, 0.25
    else:
        xd, wd, scales, alpha, f = put(x, dev, BF16), put(w, dev, BF16), None, 0.25, 0.25
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1).reshape(M, Cout)
    ref = f * y + bias.double() + bias2.double().repeat_interleave(H * W, 0) + 0.5 * R.double()
    for out_dt in (F32, BF16):
        Y = empty((M, Cout), out_dt, dev)
        kern().conv2d(xd.reshape(M, Cin), wd, Y, Bn, H, W, Cin, H, W, Cout, 3, 3, 1, 1, mode=0, ups=1, bias=put(bias, dev, F32),
                      bias2=put(bias2, dev, F32), R=put(R, dev, BF16), alpha=alpha, beta=0.5, scales=scales)
        served_by(dev, 3 if fp8 else 1)
        assert_exact(Y, ref, out_dt, f"conv code {code} fp8={fp8} slices {slices} ({eff} run) {Bn}x{H}x{W} {Cin}->{Cout} out {out_dt}",
                     alpha=f)


@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("nkt128", [3, 7])
def test_gemm_128x128_w8_k4(dev, force, nkt128, slices):
    """130 x 136, 3 and 7 k-tiles of 128 bytes, whole and in 3 slices (1 + 1 + 1, 3 + 3 + 1: uneven, none empty)"""
    run_gemm(dev, force, 14, slices, 2 * nkt128, want_slices=slices)


@pytest.mark.parametrize("slices", [1, 3])
def test_gemm_128x128_w8_k4_falls_back(dev, force, slices):
    """7 k-tiles of 64 bytes - no whole number of 128-byte tiles: code 7 runs, its slices counted in 64-byte tiles"""
    run_gemm(dev, force, 14, slices, 7, want_slices=slices)


@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("Cin", [64, 32])
def test_conv(dev, force, Cin, slices):
    """conv 3 x 3 pad 1: Cin = 64 (nine 128-byte k-tiles, one per tap) and Cin = 32 (taps would straddle a 128-byte tile: code 7 runs)"""
    run_conv(dev, force, 14, slices, Cin, want_slices=slices)


def test_fp8_falls_back(dev, force):
    """e4m3 operands have no 128-byte k-tile form: code 7 runs (5 k-tiles of 64 elements in 3 slices)"""
    run_gemm(dev, force, 14, 3, 5, fp8=True, want_slices=3)


@pytest.mark.parametrize("keep", [True, False], ids=["epi2=1", "epi2=2"])
def test_geglu_forward(dev, force, keep):
    """the GEGLU forward epilogue behind the 128-byte k-tile loop (the table gives such problems to this code): 130 x 160, two
    column blocks, the second ragged; two k-tiles of 128 bytes"""
    force(gemm2=1, gemm3=0, g2_cfg=14, g2_splits=0)
    M, N, K = 130, 160, 128
    A, B, bias = ints(M, K, seed=71, hi=2), ints(N, K, seed=72, hi=2), ints(N, seed=73, hi=4)
    assert_sums_exact(K, A, B)
    pre = 2.0 ** -4 * (A.double() @ B.double().t()) + bias.double()
    assert float(pre.abs().max()) < 24
    C = empty((M, N), BF16, dev) if keep else None
    y = empty((M, N // 2), BF16, dev)
    kern().gemm(put(A, dev, BF16), put(B, dev, BF16), C, M, N, K, K, K, N, bias=put(bias, dev, F32), alpha=2.0 ** -4, geglu=(y, keep))
    served_by(dev, 1)
    assert_act_exact_pre(y, pre, geglu_il_fp64, BF16, f"GEGLU forward code 14 keep={keep}")
    if keep:
        assert_exact(C, pre, BF16, "GEGLU forward code 14: stored pre-activations", alpha=2.0 ** -4)


def test_tail_columns(dev, force):
    """epi2 = 4: 136 main columns and 16 tail columns from B2 - the seam lies inside the second column block; two k-tiles of 128 bytes"""
    force(gemm2=1, gemm3=0, g2_cfg=14, g2_splits=0)
    M, N1, K, n2 = 130, 136, 128, 16
    A, B, B2 = ints(M, K, seed=61), ints(1, N1, K, seed=62), ints(n2, K, seed=63)
    bias, R = ints(N1, seed=64, hi=64), ints(1, M, N1, seed=65, hi=64)
    assert_sums_exact(K, A, B)
    assert_sums_exact(K, A, B2, factor=3)
    main = 0.25 * torch.einsum("mk,gnk->gmn", A.double(), B.double()) + bias.double() + 0.5 * R.double()
    tail = 0.75 * (A.double() @ B2.double().t())
    for out_dt in (F32, BF16):
        C, h = empty((1, M, N1), out_dt, dev), empty((M, n2), out_dt, dev)
        kern().gemm(put(A, dev, BF16), put(B, dev, BF16), C, M, N1 + n2, K, K, K, N1, batch=(1, 1), sA=(0, 0), sB=(N1 * K, 0),
                    sC=(M * N1, 0), sR=(M * N1, 0), bias=put(bias, dev, F32), R=put(R, dev, BF16), ldr=N1, alpha=0.25, beta=0.5,
                    tail=(put(B2, dev, BF16), h, n2, n2, n2 * K, n2, 0.75))
        served_by(dev, 1)
        assert_exact(C, main, out_dt, f"tail columns code 14 out {out_dt}: main part", alpha=0.25)
        assert_exact(h, tail, out_dt, f"tail columns code 14 out {out_dt}: tail", alpha=0.75)


# ---------------------------------------------------------------------------------------------------------------------------
# the second plan table
# ---------------------------------------------------------------------------------------------------------------------------
def wide_rows():
    with open(WIDE_FILE) as f:
        text = f.read()
    rows = [tuple(int(v) for v in r) for r in PLAN_ROW.findall(text)]
    braced = [ln for ln in text.splitlines() if ln.lstrip().startswith("{")]
    return rows, braced


WIDE_TRIPLES = sorted({(r[0], r[5], r[6]) for r in wide_rows()[0]})


def test_wide_table_parser():
    """the table holds rows, every one of them parsed; only the codes above 13 stand here (gemm2_plans.inc holds the others), the
    128-byte k-tile code only for bf16 kinds"""
    rows, braced = wide_rows()
    assert len(rows) >= 1 and len(rows) == len(braced), (len(rows), len(braced))
    assert len({r[:5] for r in rows}) == len(rows), "one row per problem"
    with open(os.path.join(ROOT, "comat_amd", "csrc", "gemm2_plans.inc")) as f:
        assert all(int(r[5]) <= 13 for r in PLAN_ROW.findall(f.read())), "codes above 13 belong to gemm2_plans_wide.inc"
    assert re.search(r"static const Plan2Entry g2_plans_wide\[\]", open(WIDE_FILE).read())
    for kind, M, N, nkt, batch, code, slices in rows:
        assert kind in (0, 1, 2, 3) and code in WIDE_TILES and 1 <= slices <= 32, (kind, code, slices)
        assert kind < 2 or code not in K4_TWIN, "fp8 problems have no 128-byte k-tile form"
        assert M >= 1 and N >= 1 and nkt >= 1 and batch >= 1
        if code in K4_TWIN:
            assert nkt % 2 == 0 and slices <= nkt // 2, "a row of the 128-byte k-tile code whose problem could not run it"


def k_cuts(code, slices, nkt64):
    """the k positions (64-byte k-tiles) at which a plan row cuts a contraction: plan2's no-empty-slices rule, finish_launch's
    count in 128-byte tiles for the K4 codes, the kernel's per = ceil(tiles / slices)"""
    unit = 2 if code in (8, 9, 10, 11, 14) else 1
    n = nkt64 // unit
    s = 1 if code in (12, 13) else max(1, min(slices, n, 32))
    per = cdiv(n, cdiv(n, cdiv(n, s)))
    return [min(i * per, n) * unit for i in range(cdiv(n, per) + 1)]


def test_wide_rows_keep_the_sums():
    """every row cuts k exactly where the problem's row of gemm2_plans.inc cuts it.  All block shapes run the same 32 x 32 x 16 MFMA
    steps in k order and add the slices' slabs in slice order, so equal cuts mean equal partial sums in equal order: the table moves
    the time of a launch and not one bit of what the step computes"""
    with open(os.path.join(ROOT, "comat_amd", "csrc", "gemm2_plans.inc")) as f:
        base = {tuple(int(v) for v in r[:5]): (int(r[5]), int(r[6])) for r in PLAN_ROW.findall(f.read())}
    for row in wide_rows()[0]:
        key, code, slices = row[:5], row[5], row[6]
        assert key in base, f"{key}: no row in gemm2_plans.inc to keep the sums of"
        assert key[3] % 2 == 0
        assert k_cuts(code, slices, key[3]) == k_cuts(*base[key], key[3]), (key, (code, slices), base[key])


def wide_counts(kind, code, slices, ntiles):
    """64-byte k-tile counts for one triple: the shortest contraction with uneven, non-empty slices (2 per slice and one more, in the
    code's own k-tiles) and, where clamp_splits' no-empty-slices rule cuts the forced count at that length, also the shortest
    that keeps it.  A conv 3 x 3 has 9 Cin / 32 k-tiles: its counts are multiples of 9 (of 18 for a 128-byte code: Cin % 64 == 0)."""
    per64 = 2 if code in K4_TWIN else 1
    unit = (9 if kind in (1, 3) else 1) * per64
    first = cdiv((2 * slices + 1) * per64, unit) * unit
    if slices_run(code, slices, first, ntiles, per64 == 2) == slices:
        return [first]
    for n in range(first, first + 64 * unit, unit):
        if slices_run(code, slices, n, ntiles, per64 == 2) == slices:
            return [first, n]
    raise AssertionError(f"no contraction keeps {slices} slices of tile code {code}")


@pytest.mark.parametrize("kind,code,slices", WIDE_TRIPLES, ids=[f"kind{k_}-code{c}-slices{s}" for k_, c, s in WIDE_TRIPLES])
def test_wide_table_triples(dev, force, kind, code, slices):
    """every distinct (kind, tile code, slices) of gemm2_plans_wide.inc on a small problem of that kind, code and count forced; the
    last contraction of wide_counts is asserted to run exactly `slices`"""
    bm, bn = WIDE_TILES[code]
    conv, fp8 = kind in (1, 3), kind >= 2
    ntiles = cdiv(bm + 2, bm) * cdiv(bn + 8, bn)
    counts = wide_counts(kind, code, slices, ntiles)
    for i, n in enumerate(counts):
        want = slices if i == len(counts) - 1 else None
        if conv:
            run_conv(dev, force, code, slices, n // 9 * (64 if fp8 else 32), fp8=fp8, want_slices=want)
        else:
            run_gemm(dev, force, code, slices, n, fp8=fp8, want_slices=want)
