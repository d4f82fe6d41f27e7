"""Exact integer-operand parity of every matrix-product path: comat_gemm in its general, pipelined, k-major, lean and fp8 forms,
comat_gemm_segments, comat_gemm_tt_grouped, comat_conv2d forward and data-gradient, comat_conv2d_wgrad and comat_lora_merge.

The method.  Operands are non-zero integers from +-{1 .. 8} (exact in bf16 and in e4m3), scale factors powers of two (apart from
the one alpha2 = 0.75), biases and residuals integers.  Every product and - by the bound each case asserts on its own inputs,
K max|a| max|b| < 2^24 - every partial sum in ANY order is then an fp32 number: the accumulator holds the exact result whatever
the tile shape, the k-tail, the split count or the combine order, and the stored value is its one round-to-nearest-even to the
output type (f32_to_bf16, common.h).  The expected output is therefore known bit for bit (helpers.assert_exact), where
helpers.check bounds max |err| / max |ref| by 3e-2 for bf16: one a*b product dropped from one element of a 70 x 40 x 96 problem
moves that figure by ~2e-2, of a 257 x 136 x 4096 one by 1e-3 (test_the_net_is_tight).  A k-tail that is off by one, a split-K
boundary element counted twice or not at all, a slice left out of the combine: each is a wrong integer here.

Epilogues with an activation have an exact pre-activation and an inexact activation: helpers.assert_act_exact_pre holds them
per element to 2e-4 max(1, |ref|) (a bf16 output: to the one rounding of such a value), with alpha = 2^-4 and short contractions so that one missing product
(>= 2^-4) exceeds the bound wherever the activation's slope is near 1.

The plan table (comat_amd/csrc/gemm2_plans.inc) is keyed by production shapes no small test reaches: test_plan_table_triples
reads it as text and runs every distinct (kind, tile code, slices) triple on a small problem with the code and the slice count
forced.  The cases run on the ABI simulator (the references, the preconditions and the table parser are proven without a GPU)
and, marked gpu, on the library, where they also assert which kernel served them (comat_last_gemm_kernel); the forced slice
counts of the general kernel and comat_lora_merge (which the simulator does not have) run on the library only.
"""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from comat_amd import ops
from helpers import (ACT_FP64, _set_opts, assert_act_exact_pre, assert_exact, assert_sums_exact, check, default_opts,  # noqa: F401 - default_opts is a fixture
                     ints, restore_default_opts)
from test_conv_wgrad import GEOMS as WGRAD_GEOMS
from test_conv_wgrad import IDS as WGRAD_IDS
from test_conv_wgrad import expected_path as wgrad_path
from test_conv_wgrad import out_hw as wgrad_out_hw

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def kern():
    return ops.kernels()


@pytest.fixture
def force(dev):
    """force(**options): kernel-selection options on the hip leg (the simulator has one kernel per entry point), restored afterwards"""
    used = []

    def f(**kw):
        if dev.type == "cuda":
            _set_opts(**kw)
            used.append(True)
    yield f
    if used:
        restore_default_opts()


def served_by(dev, want):
    if dev.type == "cuda":
        from comat_amd import _hip
        got = _hip.last_gemm_kernel()
        assert got == want, f"served by kernel {got} ({_hip.GEMM_KERNEL_NAMES.get(got)}), the case is about kernel {want}"


def put(x, dev, dtype):
    return x.to(device=dev, dtype=dtype, copy=True).contiguous()  # (a copy on the CPU too: accumulated outputs must not alias their start values)


def to8(x, dev):
    """integers in [-8, 8] are e4m3 values: the bytes hold them exactly"""
    q = x.to(torch.float8_e4m3fn)
    assert torch.equal(q.float(), x)
    return q.view(torch.uint8).to(dev).contiguous()


def empty(shape, dtype, dev):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the plan table's own (kind, tile code, slices) triples
# ---------------------------------------------------------------------------------------------------------------------------
PLAN_FILE = os.path.join(ROOT, "comat_amd", "csrc", "gemm2_plans.inc")
PLAN_ROW = re.compile(r"^\s*\{\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\}", re.M)
# tile code -> (rows, columns) of the block tile (g2_cfgs of gemm2.hip); 8 .. 11 have 128-byte k-tiles, 12 and 13 are never split
G2_TILES = {1: (128, 128), 2: (128, 64), 3: (256, 128), 4: (64, 128), 5: (128, 128), 6: (64, 64), 7: (128, 128), 8: (64, 64),
            9: (128, 64), 10: (64, 128), 11: (128, 128), 12: (256, 256), 13: (256, 128)}
G2_K4 = (8, 9, 10, 11)
G2_UNSPLIT = (12, 13)
WS_COUNTER_BYTES = 256 * 1024  # COMAT_WS_COUNTER_BYTES
WS_COUNTERS = WS_COUNTER_BYTES // 4
WS_BYTES = 256 << 20  # HipKernels.WS_BYTES: the workspace every call of the binding hands over
CONV_PIXELS = {64: (1, 11, 6), 128: (2, 13, 5), 256: (2, 13, 10)}  # (B, H, W): one tile of rows and a ragged remainder


def plan_rows():
    with open(PLAN_FILE) as f:
        text = f.read()
    rows = [tuple(int(v) for v in r) for r in PLAN_ROW.findall(text)]
    braced = [ln for ln in text.splitlines() if ln.lstrip().startswith("{")]
    return rows, braced


def plan_triples():
    return sorted({(r[0], r[5], r[6]) for r in plan_rows()[0]})


TRIPLES = plan_triples()


def test_plan_table_parser():
    """a change of the table's format must not empty the table-driven test silently"""
    rows, braced = plan_rows()
    assert len(rows) >= 400 and len(rows) == len(braced), (len(rows), len(braced))
    assert len(TRIPLES) >= 40
    for kind, code, slices in TRIPLES:
        assert kind in (0, 1, 2, 3) and 1 <= code <= 13 and code in G2_TILES and 1 <= slices <= 32, (kind, code, slices)
    for kind, M, N, nkt, batch, code, slices in rows:
        assert M >= 1 and N >= 1 and nkt >= 1 and batch >= 1
        assert slices == 1 or code not in G2_UNSPLIT, "the 256-row tiles are never split"


def clamp_splits(s, ntiles, tile_elems, nkt, ws_bytes):
    """clamp_splits of gemm2.hip"""
    slab = ws_bytes - WS_COUNTER_BYTES
    if slab <= 0 or ntiles > WS_COUNTERS:
        return 1
    s = max(1, min(s, slab // (ntiles * tile_elems * 4), nkt, 32))
    return cdiv(nkt, cdiv(nkt, s))


def effective_slices(code, slices, nkt64, ntiles, k4):
    """the slice count plan2 + finish_launch of gemm2.hip make of a forced g2_cfg / g2_splits: nkt64 = 64-byte k-tiles; k4 = the
    128-byte k-tile form runs (bf16, whole 128-byte tiles), which counts its slices in those"""
    if code in G2_UNSPLIT:
        return 1
    bm, bn = G2_TILES[code]
    s = clamp_splits(slices, ntiles, bm * bn, nkt64, WS_BYTES)
    if k4:
        n2 = nkt64 // 2
        s = min(s, max(n2, 1))
        s = cdiv(n2, cdiv(n2, s))
    return s


def own_ktiles(kind, code):
    """(elements per k-tile of this code as the case counts them, 64-byte k-tiles per such tile)"""
    if kind >= 2:
        return 64, 1  # fp8: 64-byte tiles of 64 elements whatever the code (a 128-byte code runs as its 64-byte twin)
    return (64, 2) if code in G2_K4 else (32, 1)


def ktile_counts(kind, code, slices, ntiles):
    """k-tile counts (in the code's own k-tiles) of one triple: 2 slices + 1 - uneven slices, every one non-empty - and, where the
    no-empty-slices rule of clamp_splits cuts the forced count at that length (from 4 slices on: ceil((2 s + 1) / 3) < s), also the
    shortest contraction that KEEPS the forced count with an uneven last slice of at least two tiles (3 s - 1 for a GEMM).  A conv
    3 x 3 has 9 Cin / 32 k-tiles: its counts are rounded up to multiples of 9."""
    unit = 9 if kind in (1, 3) else 1
    per64 = own_ktiles(kind, code)[1]
    k4 = per64 == 2
    first = cdiv(2 * slices + 1, unit) * unit
    counts = [first]
    if code in G2_UNSPLIT or effective_slices(code, slices, first * per64, ntiles, k4) == slices:
        return counts
    for ragged in (True, False):
        for n in range(first, first + 64 * unit, unit):
            per = cdiv(n, slices)
            last = n - (slices - 1) * per
            if effective_slices(code, slices, n * per64, ntiles, k4) == slices and (not ragged or (2 <= last < per)):
                return counts + [n]
    raise AssertionError(f"no contraction keeps {slices} slices of tile code {code}")


def gemm_problem(code):
    bm, bn = G2_TILES[code]
    return bm + 2, bn + 8  # one tile and a ragged remainder each way; N % 8 == 0: the 16-byte epilogue


def run_plan_gemm(dev, force, kind, code, slices, n, want_slices=None):
    fp8 = kind >= 2
    M, N = gemm_problem(code)
    bm, bn = G2_TILES[code]
    ke, per64 = own_ktiles(kind, code)
    K = n * ke
    eff = effective_slices(code, slices, n * per64, cdiv(M, bm) * cdiv(N, bn), per64 == 2)
    if want_slices is not None:
        assert eff == want_slices, f"code {code}: {n} k-tiles give {eff} slices, the case is about {want_slices}"
    force(gemm2=1, gemm3=0, g2_cfg=code, g2_splits=slices)
    A, B = ints(M, K, seed=100 + code), ints(N, K, seed=200 + slices)
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
        assert_exact(C, ref, out_dt, f"plan gemm kind {kind} code {code} slices {slices} ({eff} run) {M}x{N}x{K} out {out_dt}", alpha=f)


def run_plan_conv(dev, force, kind, code, slices, n, want_slices=None):
    fp8 = kind >= 2
    bm, bn = G2_TILES[code]
    Bn, H, W = CONV_PIXELS[bm]
    M, Cout = Bn * H * W, bn + 8
    ke, per64 = own_ktiles(kind, code)
    assert n % 9 == 0
    Cin = n // 9 * ke
    K = 9 * Cin
    eff = effective_slices(code, slices, n * per64, cdiv(M, bm) * cdiv(Cout, bn), per64 == 2)
    if want_slices is not None:
        assert eff == want_slices, f"code {code}: {n} k-tiles give {eff} slices, the case is about {want_slices}"
    force(gemm2=1, gemm3=0, g2_cfg=code, g2_splits=slices)
    x, w = ints(Bn, H, W, Cin, seed=300 + code), ints(Cout, 3, 3, Cin, seed=400 + slices)
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
        assert_exact(Y, ref, out_dt, f"plan conv kind {kind} code {code} slices {slices} ({eff} run) {Bn}x{H}x{W} {Cin}->{Cout} "
                                     f"out {out_dt}", alpha=f)


@pytest.mark.parametrize("kind,code,slices", TRIPLES, ids=[f"kind{k_}-code{c}-slices{s}" for k_, c, s in TRIPLES])
def test_plan_table_triples(dev, force, kind, code, slices):
    """every distinct (kind, tile code, slices) of gemm2_plans.inc on a small problem of that kind (0 / 2: GEMM, bf16 / fp8; 1 / 3:
    conv 3 x 3 pad 1, bf16 / fp8) with the code and the count forced, fp32 and bf16 output; the workspace of the binding keeps
    the forced count by clamp_splits' own formula, and the last contraction of ktile_counts is asserted to run exactly `slices`"""
    bm, bn = G2_TILES[code]
    run = run_plan_conv if kind in (1, 3) else run_plan_gemm
    M, N = (math.prod(CONV_PIXELS[bm]), bn + 8) if kind in (1, 3) else gemm_problem(code)
    counts = ktile_counts(kind, code, slices, cdiv(M, bm) * cdiv(N, bn))
    for i, n in enumerate(counts):
        run(dev, force, kind, code, slices, n, want_slices=slices if i == len(counts) - 1 else None)


def test_plan_slices_at_the_clamps(dev, force):
    """32 slices, the most clamp_splits allows (tile code 8, 128-byte k-tiles); and fewer k-tiles than forced slices, where the
    count must come down (6 forced on 4 k-tiles: 4 run) and the result stays exact"""
    ntiles = cdiv(66, 64) * cdiv(72, 64)
    n32 = ktile_counts(0, 8, 32, ntiles)[-1]
    run_plan_gemm(dev, force, 0, 8, 32, n32, want_slices=32)
    run_plan_gemm(dev, force, 0, 1, 6, 4, want_slices=4)
    run_plan_gemm(dev, force, 0, 8, 6, 4, want_slices=4)


@pytest.mark.parametrize("K2", [16, 48])
@pytest.mark.parametrize("splits", [0, 2])
def test_fp8_batched_with_bf16_k_tail(dev, force, splits, K2):
    """the other forms of the fp8 launch (comat_gemm_params::A2k, s_scale_b): three problems that share their e4m3 input and carry
    a power-of-two scale per weight, each with a bf16 k-tail read out of one [M, 3 K2] matrix - alpha (scale_a scale_b A B^T + A2
    B2^T) + bias + beta R; with the e4m3 contraction cut in two the tail must still be added exactly once"""
    G, M, N, K = 3, 130, 72, 192
    force(gemm2=1, gemm3=0, g2_cfg=0, g2_splits=splits)
    A, B = ints(M, K, seed=161), ints(G, N, K, seed=162)
    h, U = ints(M, G * K2, seed=163), ints(G, N, K2, seed=164)
    bias, R = ints(N, seed=165, hi=64), ints(G, M, N, seed=166, hi=64)
    sb = torch.tensor([0.25, 0.5, 1.0])
    assert_sums_exact(K + 4 * K2, torch.cat([A.reshape(-1), h.reshape(-1)]), torch.cat([B.reshape(-1), U.reshape(-1)]))  # (the tail against 1/4 of the product)
    ref = (0.5 * (0.5 * sb.double()[:, None, None] * torch.einsum("mk,gnk->gmn", A.double(), B.double())
                  + torch.einsum("mgr,gnr->gmn", h.double().reshape(M, G, K2), U.double()))
           + bias.double() + 0.5 * R.double())
    for out_dt in (F32, BF16):
        C = empty((G, M, N), out_dt, dev)
        kern().gemm(to8(A, dev), to8(B, dev), C, M, N, K, K, K, N, batch=(G, 1), sB=(N * K, 0), sC=(M * N, 0), sR=(M * N, 0),
                    bias=put(bias, dev, F32), R=put(R, dev, BF16), ldr=N, alpha=0.5, beta=0.5,
                    scales=(torch.tensor([0.5], device=dev), sb.to(dev), 1), ktail=(put(h, dev, BF16), put(U, dev, BF16), K2, G * K2, K2, K2, N * K2))
        served_by(dev, 3)
        assert_exact(C, ref, out_dt, f"fp8 batched + bf16 k-tail K2={K2} splits={splits} out {out_dt}", alpha=0.125)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. every routing family of comat_gemm
# ---------------------------------------------------------------------------------------------------------------------------
def window(x, dev, dtype, pad, left):
    """x [rows, cols] at leading dimension cols + pad, `left` elements into its buffer (left = 8: 16-byte aligned; left = 1 with
    an odd ld: the scalar paths) -> (view whose data_ptr() the kernel gets, ld)"""
    rows, cols = x.shape
    ld = cols + pad
    buf = torch.zeros(left + rows * ld + 8, dtype=dtype, device=dev)
    v = torch.as_strided(buf, (rows, cols), (ld, 1), left)
    v.copy_(x.to(device=dev, dtype=dtype))
    return v, ld


def general_case(dev, dtype, M, N, K, tA, tB, epi, what):
    """one problem of the general 64 x 64 kernel with the whole first epilogue: alpha = 0.25, bias, per-row-group bias2, residual
    at its own leading dimension, beta = 0.5; fp32 and bf16 output"""
    pad, left = (8, 8) if epi == "vec" else (3, 1)
    A, B = ints(M, K, seed=11), ints(N, K, seed=12)
    bias, bias2 = ints(N, seed=13, hi=64), ints(3, N, seed=14, hi=64)
    rpb = (M + 2) // 3
    assert_sums_exact(K, A, B)
    Av, lda = window(A.t() if tA else A, dev, dtype, pad, left)
    Bv, ldb = window(B.t() if tB else B, dev, dtype, pad, left)
    prod = 0.25 * (A.double() @ B.double().t()) + bias.double() + bias2.double().repeat_interleave(rpb, 0)[:M]
    for out_dt in (F32, BF16):
        R = ints(M, N, seed=15, hi=64)
        Rv, ldr = window(R, dev, out_dt, pad + (8 if epi == "vec" else 2), left)
        Cv, ldc = window(torch.full((M, N), NAN), dev, out_dt, pad, left)
        kern().gemm(Av, Bv, Cv, M, N, K, lda, ldb, ldc, transA=tA, transB=tB, bias=put(bias, dev, F32), bias2=put(bias2, dev, F32),
                    rows_per_bias2=rpb, R=Rv, ldr=ldr, alpha=0.25, beta=0.5)
        served_by(dev, 0)
        assert_exact(Cv.clone(), prod + 0.5 * R.double(), out_dt, f"{what} out {out_dt}", alpha=0.25)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("transA", [False, True])
@pytest.mark.parametrize("transB", [False, True])
@pytest.mark.parametrize("K", [40, 93, 4100])
@pytest.mark.parametrize("epi", ["vec", "scalar"])
def test_general_kernel(dev, force, dtype, transA, transB, K, epi):
    """gemm.hip: every operand layout, a contraction under one k-tile, a ragged one and one the planner splits on its own;
    16-byte and per-element epilogues; bf16 and the fp32 parity mode (fp32 integer operands are exact too)"""
    force(gemm2=0, gemm3=0)
    general_case(dev, dtype, 70, 40, K, transA, transB, epi, f"general kernel 70x40x{K} tA={transA} tB={transB} {epi} {dtype}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("splits", [2, 5, 16])
def test_general_kernel_forced_splits(hip, dtype, splits, default_opts):
    """the in-launch split-K combine of the general kernel at forced slice counts: uneven slices (K = 4100, 93), every layout"""
    _set_opts(gemm2=0, gemm3=0, force_splits=splits)
    for K in (4100, 93):
        for tA, tB, epi in ((False, False, "vec"), (True, False, "scalar"), (False, True, "scalar"), (True, True, "vec")):
            general_case(hip, dtype, 70, 40, K, tA, tB, epi, f"general kernel, {splits} slices forced, 70x40x{K} tA={tA} tB={tB} {dtype}")


@pytest.mark.parametrize("splits", [0, 3])
def test_k_major_pipelined_kernel(dev, force, splits):
    """gemm2_tt (transA && transB, the LoRA weight-gradient pattern): fp32 accumulation in place into a non-zero integer C, a
    second call adds the product again; ragged 128-tiles; the planner's own split and 3 forced slices of 5 + 5 + 3 k-tiles"""
    M, N, K = 136, 72, 416
    force(gemm2=1, gemm2_tt=1, gemm3=0, g2_splits=splits)
    A, B, C0 = ints(K, M, seed=21), ints(K, N, seed=22), ints(M, N, seed=23, hi=64)
    assert_sums_exact(K, A, B, factor=2, extra=64)
    ref = A.double().t() @ B.double()
    C = put(C0, dev, F32)
    for rep in (1, 2):
        kern().gemm(put(A, dev, BF16), put(B, dev, BF16), C, M, N, K, M, N, N, transA=True, transB=True, R=C, ldr=N, beta=1.0)
        served_by(dev, 2)
        assert_exact(C, C0.double() + rep * ref, F32, f"k-major pipelined kernel splits={splits}, call {rep}")


@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_lean_kernel(dev, force, cfg):
    """gemm3.hip, every tile shape (option gemm3 = 2: every eligible problem): M = 16 and a ragged 33, N = 72 (ragged for the 32- and
    the 64-column tiles), fewer (5) and more (19) than 16 chunks of 64 along k - the two wave counts of its rule"""
    force(gemm3=2, g3_cfg=cfg)
    for M in (16, 33):
        for K in (320, 1216):
            N = 72
            A, B, bias, R = ints(M, K, seed=31), ints(N, K, seed=32), ints(N, seed=33, hi=64), ints(M, N, seed=34, hi=64)
            assert_sums_exact(K, A, B)
            ref = 0.25 * (A.double() @ B.double().t()) + bias.double() + 0.5 * R.double()
            for out_dt in (F32, BF16):
                C = empty((M, N), out_dt, dev)
                kern().gemm(put(A, dev, BF16), put(B, dev, BF16), C, M, N, K, K, K, N, bias=put(bias, dev, F32), R=put(R, dev, BF16),
                            ldr=N, alpha=0.25, beta=0.5)
                served_by(dev, 5)
                assert_exact(C, ref, out_dt, f"lean kernel cfg {cfg} {M}x{N}x{K} out {out_dt}", alpha=0.25)


# name -> (options, operand dtype, comat_last_gemm_kernel)
FAMILIES = {"general": (dict(gemm2=0, gemm3=0), BF16, 0), "general-fp32": (dict(gemm2=0, gemm3=0), F32, 0),
            "pipelined": (dict(gemm2=1, gemm3=0, g2_cfg=0, g2_splits=0), BF16, 1),
            "pipelined-3-slices": (dict(gemm2=1, gemm3=0, g2_cfg=0, g2_splits=3), BF16, 1),
            "lean": (dict(gemm3=2, g3_cfg=0), BF16, 5)}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_batched_in_place_and_row_group_bias(dev, force, family):
    """per kernel family: a batched launch with batch strides that are not the matrix sizes, per-row-group bias2, and in-place
    accumulation (R == C, beta = 1) called twice, which must give exactly twice the product"""
    opts, dtype, kernel = FAMILIES[family]
    force(**opts)
    nb, M, N, K = 3, 130, 72, 320
    A, B = ints(nb, M + 1, K, seed=41), ints(nb, N + 2, K, seed=42)  # a row / two rows of slack between the batch entries
    bias = ints(N, seed=43, hi=64)
    assert_sums_exact(K, A, B, factor=2)
    prod = torch.einsum("bmk,bnk->bmn", A[:, :M].double(), B[:, :N].double())
    Ad, Bd = put(A, dev, dtype), put(B, dev, dtype)
    for out_dt in (F32, BF16):
        R = ints(nb, M, N, seed=44, hi=64)
        C = empty((nb, M + 3, N), out_dt, dev)
        kern().gemm(Ad, Bd, C, M, N, K, K, K, N, batch=(nb, 1), sA=((M + 1) * K, 0), sB=((N + 2) * K, 0), sC=((M + 3) * N, 0),
                    sR=(M * N, 0), bias=put(bias, dev, F32), R=put(R, dev, out_dt), ldr=N, alpha=0.25, beta=0.5)
        served_by(dev, kernel)
        assert_exact(C[:, :M], 0.25 * prod + bias.double() + 0.5 * R.double(), out_dt, f"{family}: batched launch out {out_dt}", alpha=0.25)
        assert bool(torch.isnan(C[:, M:].float()).all()), f"{family}: rows between the batch entries were written"
    # per-row-group bias2 (one row of it per 44 rows of C), one problem
    bias2 = ints(3, N, seed=45, hi=64)
    C = empty((M, N), F32, dev)
    kern().gemm(Ad[0], Bd[0], C, M, N, K, K, K, N, bias2=put(bias2, dev, F32), rows_per_bias2=44, alpha=0.5)
    served_by(dev, kernel)
    assert_exact(C, 0.5 * prod[0] + bias2.double().repeat_interleave(44, 0)[:M], F32, f"{family}: bias2", alpha=0.5)
    # in-place accumulation into a non-zero integer fp32 buffer
    C0 = ints(M, N, seed=46, hi=64)
    C = put(C0, dev, F32)
    for rep in (1, 2):
        kern().gemm(Ad[1], Bd[1], C, M, N, K, K, K, N, R=C, ldr=N, beta=1.0)
        served_by(dev, kernel)
        assert_exact(C, C0.double() + rep * prod[1], F32, f"{family}: in-place accumulation, call {rep}")


@pytest.mark.parametrize("act", ["silu", "gelu"])
@pytest.mark.parametrize("family", ["general", "general-fp32", "pipelined", "lean"])
def test_activation_epilogues(dev, force, family, act):
    """act(alpha A B^T + bias) + beta R: |pre| stays near 16 (operands from +-{1, 2}, alpha = 2^-4, three k-tiles), so that a
    missing product of 2^-4 or more is beyond the bound wherever the activation's slope is near 1"""
    opts, dtype, kernel = FAMILIES[family]
    force(**opts)
    M, N, K = 70, 72, 192
    A, B, bias, R = ints(M, K, seed=51, hi=2), ints(N, K, seed=52, hi=2), ints(N, seed=53, hi=4), ints(M, N, seed=54, hi=4)
    assert_sums_exact(K, A, B)
    pre = 2.0 ** -4 * (A.double() @ B.double().t()) + bias.double()
    assert float(pre.abs().max()) < 24
    code = {"silu": ops.ACT_SILU, "gelu": ops.ACT_GELU}[act]
    for out_dt in (F32, BF16):
        C = empty((M, N), out_dt, dev)
        kern().gemm(put(A, dev, dtype), put(B, dev, dtype), C, M, N, K, K, K, N, bias=put(bias, dev, F32), R=put(R, dev, BF16), ldr=N,
                    alpha=2.0 ** -4, beta=0.5, act=code)
        served_by(dev, kernel)
        assert_act_exact_pre(C, pre, lambda t: ACT_FP64[act](t) + 0.5 * R.double(), out_dt, f"{family}: {act} epilogue out {out_dt}")


# ---------------------------------------------------------------------------------------------------------------------------
# 3. second epilogues
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("form", ["one-launch", "two-launch"])
def test_tail_columns(dev, force, form, G):
    """epi2 = 4: the last n2 columns come from B2 and go to C2 as alpha2 = 0.75 times the product (3 x sum < 2^24: exact), the
    first N1 get the whole first epilogue; the pipelined kernel's one launch and the two-launch form outside it"""
    force(gemm2=1 if form == "one-launch" else 0, gemm3=0, g2_cfg=0, g2_splits=0)
    M, N1, K, n2 = 130, 72, 96, 16
    A, B, B2 = ints(M, K, seed=61), ints(G, N1, K, seed=62), ints(G * n2, K, seed=63)
    bias, R = ints(N1, seed=64, hi=64), ints(G, M, N1, seed=65, hi=64)
    assert_sums_exact(K, A, B)
    assert_sums_exact(K, A, B2, factor=3)
    main = 0.25 * torch.einsum("mk,gnk->gmn", A.double(), B.double()) + bias.double() + 0.5 * R.double()
    tail = 0.75 * (A.double() @ B2.double().t())
    for out_dt in (F32, BF16):
        C, h = empty((G, M, N1), out_dt, dev), empty((M, G * n2), out_dt, dev)
        kern().gemm(put(A, dev, BF16), put(B, dev, BF16), C, M, N1 + n2, K, K, K, N1, batch=(G, 1), sA=(0, 0), sB=(N1 * K, 0),
                    sC=(M * N1, 0), sR=(M * N1, 0), bias=put(bias, dev, F32), R=put(R, dev, BF16), ldr=N1, alpha=0.25, beta=0.5,
                    tail=(put(B2, dev, BF16), h, n2, G * n2, n2 * K, n2, 0.75))
        served_by(dev, 1 if form == "one-launch" else 0)
        assert_exact(C, main, out_dt, f"tail columns {form} G={G} out {out_dt}: main part", alpha=0.25)
        assert_exact(h, tail, out_dt, f"tail columns {form} G={G} out {out_dt}: tail", alpha=0.75)


def geglu_il_fp64(pre64):
    """value * gelu(gate) over columns interleaved in sixteens, both rounded to bf16 first (comat_gemm_params::epi2)"""
    M, N = pre64.shape
    t = pre64.float().to(BF16).double().reshape(M, N // 32, 2, 16)
    return (t[:, :, 0] * F.gelu(t[:, :, 1])).reshape(M, N // 2)


@pytest.mark.parametrize("keep", [True, False], ids=["epi2=1", "epi2=2"])
@pytest.mark.parametrize("form", ["fused", "two-launch"])
def test_geglu_forward(dev, force, form, keep):
    """epi2 = 1 / 2: C2 = value * gelu(gate) of the exact pre-activations; with epi2 = 1 the stored pre-activations are bit-exact"""
    force(gemm2=1 if form == "fused" else 0, gemm3=0, g2_cfg=0, g2_splits=0)
    M, N, K = 70, 96, 96
    A, B, bias = ints(M, K, seed=71, hi=2), ints(N, K, seed=72, hi=2), ints(N, seed=73, hi=4)
    assert_sums_exact(K, A, B)
    pre = 2.0 ** -4 * (A.double() @ B.double().t()) + bias.double()
    assert float(pre.abs().max()) < 24
    C = empty((M, N), BF16, dev) if keep else None
    y = empty((M, N // 2), BF16, dev)
    kern().gemm(put(A, dev, BF16), put(B, dev, BF16), C, M, N, K, K, K, N, bias=put(bias, dev, F32), alpha=2.0 ** -4, geglu=(y, keep))
    served_by(dev, 1 if form == "fused" else 0)
    assert_act_exact_pre(y, pre, geglu_il_fp64, BF16, f"GEGLU forward {form} keep={keep}")
    if keep:
        assert_exact(C, pre, BF16, f"GEGLU forward {form}: stored pre-activations", alpha=2.0 ** -4)


@pytest.mark.parametrize("form", ["fused", "two-launch"])
def test_geglu_backward(dev, force, form):
    """epi2 = 3: the product is dF (rounded to bf16 first), the output the gradient of the saved interleaved pre-activations:
    d value = dF gelu(gate), d gate = dF value gelu'(gate)"""
    force(gemm2=1 if form == "fused" else 0, gemm3=0, g2_cfg=0, g2_splits=0)
    M, D, K = 70, 48, 96
    g, W = ints(M, K, seed=81, hi=2), ints(D, K, seed=82, hi=2)
    pre = (ints(M, 2 * D, seed=83, hi=16) * 0.25).to(BF16)  # multiples of 1/4 up to 4: bf16 values
    assert_sums_exact(K, g, W)
    dF = 2.0 ** -4 * (g.double() @ W.double().t())

    def backward(dF64):
        d = dF64.float().to(BF16).double().reshape(M, D // 16, 16)
        t = pre.double().reshape(M, D // 16, 2, 16)
        v, gt = t[:, :, 0], t[:, :, 1]
        cdf = 0.5 * (1.0 + torch.erf(gt / math.sqrt(2.0)))
        pdf = torch.exp(-0.5 * gt * gt) / math.sqrt(2.0 * math.pi)
        return torch.stack([d * gt * cdf, d * v * (cdf + gt * pdf)], dim=2).reshape(M, 2 * D)
    out = empty((M, 2 * D), BF16, dev)
    kern().gemm(put(g, dev, BF16), put(W, dev, BF16), out, M, D, K, K, K, 2 * D, alpha=2.0 ** -4, geglu=(put(pre, dev, BF16), "bwd"))
    served_by(dev, 1 if form == "fused" else 0)
    assert_act_exact_pre(out, dF, backward, BF16, f"GEGLU backward {form}")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. K-segmented and grouped k-major products
# ---------------------------------------------------------------------------------------------------------------------------
# name -> (options, operand dtype, kernel, (K1, K2)): K2 is ragged where the family takes a ragged contraction (the general kernel
# any, the pipelined kernel whole 32-element k-tiles, the lean kernel whole 64-element chunks)
SEG_FAMILIES = {"general": (dict(gemm2=0, gemm3=0), BF16, 0, (93, 40)), "general-fp32": (dict(gemm2=0, gemm3=0), F32, 0, (93, 40)),
                "pipelined": (dict(gemm2=1, gemm3=0, g2_cfg=0, g2_splits=0), BF16, 1, (160, 96)),
                "pipelined-2-slices": (dict(gemm2=1, gemm3=0, g2_cfg=0, g2_splits=2), BF16, 1, (160, 96)),
                "lean": (dict(gemm3=2, g3_cfg=0), BF16, 5, (320, 64))}


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("family", list(SEG_FAMILIES))
def test_gemm_segments(dev, force, family, G):
    """comat_gemm_segments: frozen + low-rank (y = x W^T + h U^T), G problems in one launch that share x and read their h out of
    one [M, G K2] matrix; bias [G, N], residual, alpha, beta"""
    opts, dtype, kernel, (K1, K2) = SEG_FAMILIES[family]
    force(**opts)
    M, N = 130, 72
    x, W = ints(M, K1, seed=91), ints(G, N, K1, seed=92)
    h, U = ints(M, G * K2, seed=93), ints(G, N, K2, seed=94)
    bias, R = ints(G, N, seed=95, hi=64), ints(G, M, N, seed=96, hi=64)
    assert_sums_exact(K1 + K2, torch.cat([x.reshape(-1), h.reshape(-1)]), torch.cat([W.reshape(-1), U.reshape(-1)]))
    ref = (0.25 * (torch.einsum("mk,gnk->gmn", x.double(), W.double())
                   + torch.einsum("mgr,gnr->gmn", h.double().reshape(M, G, K2), U.double()))
           + bias.double()[:, None, :] + 0.5 * R.double())
    segs = [(put(x, dev, dtype), put(W, dev, dtype), K1, K1, K1, 0, N * K1), (put(h, dev, dtype), put(U, dev, dtype), K2, G * K2, K2, K2, N * K2)]
    for out_dt in (F32, BF16):
        C = empty((G, M, N), out_dt, dev)
        kern().gemm_segments(segs, C, M, N, N, bias=put(bias, dev, F32), R=put(R, dev, out_dt), ldr=N, alpha=0.25, beta=0.5, batch=G,
                             sC=M * N, sR=M * N)
        served_by(dev, kernel)
        assert_exact(C, ref, out_dt, f"gemm_segments {family} G={G} out {out_dt}", alpha=0.25)


def test_gemm_tt_grouped(dev):
    """comat_gemm_tt_grouped: three problems of different M / N / K in one launch (a contraction under one k-tile, a ragged one,
    one that is cut into two slices: 35 k-tiles), accumulated into non-zero integer dW, twice"""
    probs, refs, starts, outs = [], [], [], []
    for i, (M, N, K) in enumerate(((8, 8, 33), (72, 40, 100), (136, 264, 1100))):
        A, B, C0 = ints(K, M, seed=101 + i), ints(K, N, seed=111 + i), ints(M, N, seed=121 + i, hi=64)
        assert_sums_exact(K, A, B, factor=2, extra=64)
        C = put(C0, dev, F32)
        probs.append((put(A, dev, BF16), put(B, dev, BF16), C, M, N, K, M, N, N))
        refs.append(A.double().t() @ B.double())
        starts.append(C0.double())
        outs.append(C)
    for rep in (1, 2):
        kern().gemm_tt_grouped(probs)
        served_by(dev, 4)
        for i, C in enumerate(outs):
            assert_exact(C, starts[i] + rep * refs[i], F32, f"gemm_tt_grouped problem {i}, call {rep}")


# ---------------------------------------------------------------------------------------------------------------------------
# 5. convolutions through ops.conv2d, forward and data-gradient
# ---------------------------------------------------------------------------------------------------------------------------
# (B, H, W, Cin, Cout, k, stride, ups): ragged pixel counts (2 x 13 x 9 = 234), Cout ragged for the 64-column tiles; Cout = 96 where
# the data-gradient (whose contraction runs over Cout) should reach the pipelined kernel too (whole 32-element k-tiles)
CONV_GEOMS = [(2, 13, 9, 64, 72, 3, 1, 1), (2, 13, 9, 64, 96, 3, 1, 1), (2, 13, 9, 64, 96, 3, 2, 1), (1, 7, 9, 64, 96, 3, 1, 2),
              (2, 13, 9, 64, 72, 1, 1, 1)]
# name -> (options, dtype, kernel)
CONV_FAMILIES = {"pipelined": (dict(gemm2=1, g2_cfg=0, g2_splits=0), BF16, 1), "pipelined-2-slices": (dict(gemm2=1, g2_cfg=0, g2_splits=2), BF16, 1),
                 "general": (dict(gemm2=0), BF16, 0), "general-fp32": (dict(gemm2=0), F32, 0)}


@pytest.mark.parametrize("geom", CONV_GEOMS, ids=["x".join(map(str, g)) for g in CONV_GEOMS])
@pytest.mark.parametrize("family", list(CONV_FAMILIES))
def test_conv2d_forward_and_data_gradient(dev, force, family, geom):
    """padding taps contribute exactly 0: a wrong border is a wrong integer.  Integer bias, per-sample time-embedding bias2 and
    residual.  ops.conv2d stores in the compute dtype: the expected output is the one rounding of the exact integer; the
    data-gradient of the fused 2x upsample is the 2 x 2 sum of the ROUNDED gradient of the upsampled input (ops._Conv.backward:
    a conv, then comat_sumpool2x2 - sums of four integers, exact in fp32), rounded once more"""
    opts, dtype, kernel = CONV_FAMILIES[family]
    force(**opts)
    Bn, H, W, Cin, Cout, ks, stride, ups = geom
    pad = ks // 2
    x, w = ints(Bn, Cin, H, W, seed=131), ints(Cout, Cin, ks, ks, seed=132, hi=4)
    b, b2 = ints(Cout, seed=133, hi=64), ints(Bn, Cout, seed=134, hi=64)
    assert_sums_exact(ks * ks * Cin, x, w)
    tokf = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    xu = (F.interpolate(x.double(), scale_factor=2, mode="nearest") if ups == 2 else x.double()).requires_grad_(True)
    yr = F.conv2d(xu, w.double(), b.double(), stride=stride, padding=pad) + b2.double()[:, :, None, None]
    res = ints(*yr.shape, seed=135, hi=64)
    g = ints(*yr.shape, seed=136, hi=4)
    assert_sums_exact(ks * ks * Cout, g, w)
    (du,) = torch.autograd.grad(yr, xu, g.double())
    conv = ops.FrozenConv(w, b, dtype, dev, stride=stride, pad=pad)
    xd = put(tokf(x), dev, dtype).requires_grad_(True)
    y = ops.conv2d(xd, conv, Bn, H, W, ups=ups, bias2=put(b2, dev, F32), residual=put(tokf(res), dev, dtype))
    served_by(dev, kernel)
    what = f"conv {family} {geom}"
    assert_exact(y.detach(), tokf(yr.detach() + res.double()), dtype, what)
    y.backward(put(tokf(g), dev, dtype))
    # (the data-gradient runs on autograd's thread and comat_last_gemm_kernel is per thread: this thread cannot tell which kernel
    # served it.  A contraction over Cout = 72 is no whole number of k-tiles and goes to the general kernel under every family;
    # Cout = 96 and the zero-stuffed stride-2 gather are eligible for the pipelined one: test_ops.py asserts that routing from the
    # calling thread, test_strided_conv_dgrad_runs_on_the_pipelined_kernel.)
    if ups == 2:
        du = du.float().to(dtype).double()
        du = du.reshape(Bn, Cin, H, 2, W, 2).sum(dim=(3, 5))
    assert_exact(xd.grad, tokf(du), dtype, what + " data-gradient")


# ---------------------------------------------------------------------------------------------------------------------------
# 6. comat_conv2d_wgrad
# ---------------------------------------------------------------------------------------------------------------------------
def run_wgrad(dev, geom, dtype):
    Bn, Hin, Win, Cin, Cout, ks, stride, ups = geom
    Ho, Wo, pad = wgrad_out_hw(geom)
    x, dy = ints(Bn, Hin, Win, Cin, seed=141), ints(Bn, Ho, Wo, Cout, seed=142)
    dw0 = ints(Cout, ks, ks, Cin, seed=143, hi=64)
    assert_sums_exact(Bn * Ho * Wo, x, dy, factor=2, extra=64)
    xn = x.double().permute(0, 3, 1, 2)
    if ups == 2:
        xn = F.interpolate(xn, scale_factor=2, mode="nearest")
    ref = torch.nn.grad.conv2d_weight(xn, (Cout, Cin, ks, ks), dy.double().permute(0, 3, 1, 2), stride=stride, padding=pad)
    ref = ref.permute(0, 2, 3, 1).contiguous()
    dw = put(dw0, dev, F32)
    xd, dyd = put(x, dev, dtype), put(dy, dev, dtype)
    for rep in (1, 2):
        kern().conv2d_wgrad(xd, dyd, dw, Bn, Hin, Win, Cin, Ho, Wo, Cout, ks, ks, stride, pad, ups)
        served_by(dev, wgrad_path(geom, dtype))
        assert_exact(dw, dw0.double() + rep * ref, F32, f"conv2d_wgrad {geom} {dtype}, call {rep}")


@pytest.mark.parametrize("geom,dtype", WGRAD_GEOMS, ids=WGRAD_IDS)
def test_conv_wgrad(dev, geom, dtype):
    """the ten geometries of test_conv_wgrad.GEOMS: dW is fp32 and accumulated - from a non-zero integer dW0 the result is dW0 + ref
    exactly, after a second call dW0 + 2 ref"""
    run_wgrad(dev, geom, dtype)


def test_conv_wgrad_forced_splits(dev):
    """two slices of one k-tile each on the smallest problem (option force_splits)"""
    if dev.type == "cuda":
        _set_opts(force_splits=2)
    try:
        run_wgrad(dev, *WGRAD_GEOMS[0])
    finally:
        if dev.type == "cuda":
            restore_default_opts()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. comat_lora_merge
# ---------------------------------------------------------------------------------------------------------------------------
def lora_merge_data():
    """W, U, D^T integers up to 4, r = 16, scale 1/2: W + s U D is a multiple of 1/2 of magnitude <= 4 + 128.  Where that has more
    than 8 significant bits (|.| >= 128 with a half: rare) the expected value is its round-to-nearest-even, as for every bf16
    output of this module"""
    G, N, K, r = 2, 72, 136, 16
    W, U, Dt = ints(G, N, K, seed=151, hi=4), ints(G, N, r, seed=152, hi=4), ints(G, K, r, seed=153, hi=4)
    assert_sums_exact(r, U, Dt)
    ref = W.double() + 0.5 * torch.einsum("gnr,gkr->gnk", U.double(), Dt.double())
    return (G, N, K, r), W, U, Dt, ref


def test_lora_merge_reference():
    (G, N, K, r), W, U, Dt, ref = lora_merge_data()
    assert torch.equal(ref.float().double(), ref) and float(ref.abs().max()) <= 132
    assert float((ref.float().to(BF16).double() == ref).double().mean()) > 0.99  # nearly every element has at most 8 significant bits


@pytest.mark.gpu
def test_lora_merge(hip):
    """Wm = bf16(W + s U D) and WmT = Wm^T of two projections in one launch, ragged 64 x 64 tiles"""
    (G, N, K, r), W, U, Dt, ref = lora_merge_data()
    Wd, Ud, Dtd = put(W, hip, BF16), put(U, hip, BF16), put(Dt, hip, BF16)
    Wm, WmT = empty((G, N, K), BF16, hip), empty((G, K, N), BF16, hip)
    problems = torch.tensor([[Wd[i].data_ptr(), Ud[i].data_ptr(), Dtd[i].data_ptr(), Wm[i].data_ptr(), WmT[i].data_ptr(), N, K, r, r, r]
                             for i in range(G)], dtype=torch.int64, device=hip)
    tiles = torch.tensor([[i, n0, k0] for i in range(G) for n0 in range(0, N, 64) for k0 in range(0, K, 64)], dtype=torch.int32, device=hip)
    assert kern().lora_merge_ok(Wd[0], Ud[0], Dtd[0], r, r, r) and all(int(a) % 16 == 0 for a in problems[:, :5].reshape(-1).tolist())
    kern().lora_merge(problems, tiles, 0.5)
    assert_exact(Wm, ref, BF16, "lora_merge: Wm", alpha=0.5)
    assert_exact(WmT, ref.transpose(1, 2).contiguous(), BF16, "lora_merge: WmT", alpha=0.5)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the net is tight (CPU only, no kernel)
# ---------------------------------------------------------------------------------------------------------------------------
def drop_one_product(A, B, alpha, at):
    """the exact alpha A B^T and the same with ONE a * b product (k = 0) missing from the one element `at`"""
    ref = alpha * (A.double() @ B.double().t())
    wrong = ref.clone()
    m, n = at
    wrong[m, n] -= alpha * float(A[m, 0]) * float(B[n, 0])
    return ref, wrong


@pytest.mark.parametrize("shape", [(70, 40, 96), (257, 136, 4096)], ids=lambda s: "x".join(map(str, s)))
def test_the_net_is_tight(shape):
    """what this module sees that helpers.check does not: one product missing from one element of the result passes the bf16 bound
    of the sibling tests (3e-2 of the maximum, and with room: the figure moves by ~2e-2 at 70 x 40 x 96, 1e-3 at 257 x 136 x
    4096) and their fp32 bound at the larger shape, and is rejected by assert_exact.  A bf16 OUTPUT shows a dropped product only
    where it exceeds half an ulp of the result - the element of least magnitude here - which is why every split case has an fp32
    output as well.  Whoever loosens assert_exact into an allclose breaks this test."""
    M, N, K = shape
    A, B = ints(M, K, seed=1), ints(N, K, seed=2)
    assert_sums_exact(K, A, B)
    ref, wrong = drop_one_product(A, B, 0.25, (M // 2, N // 2))
    moved = float((wrong - ref).abs().max() / ref.abs().max())
    print(f"one product out of {M}x{N}x{K}: err / max |ref| moves by {moved:.2e}")
    assert moved < 3e-2
    check(wrong.float(), ref, BF16, "helpers.check accepts a dropped product (bf16 bound)")
    assert_exact(ref.float(), ref, F32, "the exact result")
    with pytest.raises(AssertionError, match="1 of .* elements differ.*difference / alpha"):
        assert_exact(wrong.float(), ref, F32, "fp32 output", alpha=0.25)
    # bf16 output: the element whose exact value is smallest
    at = divmod(int(ref.abs().argmin()), N)
    ref, wrong = drop_one_product(A, B, 0.25, at)
    if abs(float(ref[at])) < 32:  # half an ulp of a value below 32 is at most 1/16 < the smallest product, 1/4
        with pytest.raises(AssertionError, match="1 of .* elements differ"):
            assert_exact(wrong.float().to(BF16), ref, BF16, "bf16 output", alpha=0.25)
    else:
        pytest.fail(f"no element below 32 in {shape}: choose other seeds")


def test_the_net_is_tight_behind_an_activation():
    """assert_act_exact_pre at the shapes of test_activation_epilogues: one product of 2^-4 (the smallest) missing from the
    pre-activation of one element is rejected where the activation's slope is near 1; helpers.check at the siblings' bf16
    tolerance accepts it"""
    M, N, K = 70, 72, 192
    A, B = ints(M, K, seed=51, hi=2), ints(N, K, seed=52, hi=2)
    pre = 2.0 ** -4 * (A.double() @ B.double().t())
    at = divmod(int(torch.where(pre > 1.0, pre, torch.full_like(pre, 1e9)).argmin()), N)  # the smallest pre-activation above 1
    wrong = pre.clone()
    wrong[at] -= 2.0 ** -4 * abs(float(A[at[0], 0]) * float(B[at[1], 0]))
    for act in ("silu", "gelu"):
        ref = ACT_FP64[act](pre)
        check(ACT_FP64[act](wrong).float(), ref, BF16, "helpers.check accepts a dropped product behind an activation")
        for out_dt in (F32, BF16):
            assert_act_exact_pre(ref.float().to(out_dt), pre, act, out_dt, "the exact result")
            with pytest.raises(AssertionError, match="1 of .* elements beyond the bound"):
                assert_act_exact_pre(ACT_FP64[act](wrong).float().to(out_dt), pre, act, out_dt, f"{act} out {out_dt}")
    # the precondition itself: a reference that is no fp32 number proves nothing and is refused
    with pytest.raises(AssertionError, match="not exact in fp32"):
        assert_exact(torch.zeros(1), torch.tensor([1.0 + 2.0 ** -40], dtype=F64), F32, "inexact reference")
