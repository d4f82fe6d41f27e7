"""Window semantics of the kernel entry points (include/comat_hip.h): a kernel reads [rows, cols] at a leading dimension,
writes [rows, cols] at a leading dimension, and touches nothing else.

Every operand of every case sits in a helpers.Window: inputs in a NaN halo (a row past M, a column past d, a key past Nk or a
tap outside the image that reaches a result poisons it), outputs in a guard band that is compared bit for bit with its
snapshot.  The shapes are the smallest at which each kernel has a ragged edge; the reference is fp64 on the dtype-rounded
window contents, the tolerance test_ops.py's `check` with the factor its sibling test uses for the same quantity.  Guard and
finiteness checks are exact.

Combinations the header documents as illegal are not generated (they are the caller's error, not a window):
  * fused attention operands that are not 16-byte aligned, leading dimensions that are no 16-byte multiple, head dims that are
    no multiple of 8 (bf16) / 4 (fp32): "Head dim d <= 160, multiple of 8 (bf16) / 4 (fp32); leading dims and base pointers
    16-byte aligned" (comat_flash_attn_fwd);
  * comat_copy2d_pair with partial vectors or unaligned pointers: "cols_i and every leading dimension in whole 16-byte vectors,
    16-byte aligned pointers (else COMAT_EINVAL: use comat_copy2d twice)";
  * comat_gemm_tt_grouped with M, N no multiple of 8, lda / ldb no multiple of 8, ldc no multiple of 4 or unaligned operands:
    "M_p, N_p multiples of 8 (>= 8); ...; lda, ldb multiples of 8, ldc of 4; operands 16-byte aligned";
  * GEGLU epilogues (epi2 = 1 .. 3) on rows that are not 16-byte aligned, with a residual, bias2, activation or batch: "bf16
    output, N % 32 == 0, 16-byte aligned rows; no residual, bias2, activation or batch"; their C2 / pre / q8 operands are
    contiguous in the binding, so those windows have guard ROWS only;
  * comat_geglu_il_fwd / _bwd with D no multiple of 16 or unaligned operands: "D % 16 == 0, 16-byte aligned operands";
  * the e4m3 outputs on rows that are not 8-byte (GEGLU epilogue: "8-byte aligned rows and ldq8 >= N / 2") / 4-byte (fused
    attention: "ldq8 % 4 == 0, d % 4 == 0") aligned;
  * comat_fp8_quantize* on an unaligned x: "x: n elements of `dtype` (fp32 or bf16), 16-byte aligned";
  * comat_cfg_rescale_ddpm_* with per_sample no multiple of 4 or unaligned operands: "per_sample % 4 == 0, 16-byte aligned fp32
    operands, 8-byte aligned bf16 ones";
  * comat_lora_merge with N, K no multiple of 8 or r no multiple of 16: "N % 8 == K % 8 == 0, r % 16 == 0, ldu % 8 == lddt % 8
    == 0, every address 16-byte aligned";
  * comat_layernorm_fwd_q / comat_groupnorm_fwd_q on shapes their _ok predicates decline ("other shapes return
    COMAT_EUNSUPPORTED and the caller runs the two calls").
The norm, softmax and flat elementwise kernels have no leading dimension: their windows have guard rows (elements) only."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from comat_amd import ops
from comat_amd.resize import resize_tables
from helpers import Window, _set_opts, default_opts, restore_default_opts  # noqa: F401 - default_opts is a fixture
from oracle import fp8 as OF
from test_ops import check, rnd  # the suite's existing tolerance: tol(dtype) * factor of the reference's scale

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
ACTS = {ops.ACT_NONE: lambda t: t, ops.ACT_SILU: F.silu, ops.ACT_GELU: F.gelu}


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
    """the kernel family that served the last gemm / gemm_segments / conv2d call (comat_last_gemm_kernel)"""
    if dev.type == "cuda":
        from comat_amd import _hip
        got = _hip.last_gemm_kernel()
        assert got == want, f"served by kernel {got} ({_hip.GEMM_KERNEL_NAMES.get(got)}), the case is about kernel {want}"


def coarser(*dtypes):
    """the dtype whose rounding bounds a result that passed through all of `dtypes`"""
    return BF16 if BF16 in dtypes else F32


def win(x, dtype, dev, pad=8, left=8, lead=2, trail=2):
    """input window: the 2-D (flattened) `x` at leading dimension cols + pad inside a NaN halo"""
    x = x.reshape(-1, x.shape[-1])
    return Window(x.shape[0], x.shape[1], x.shape[1] + pad, dtype, dev, lead, trail, left).put(x)


def vecw(x, dtype, dev, left=8):
    """a vector (bias, statistics, a device scalar) between guard elements"""
    x = x.reshape(1, -1)
    return Window(1, x.shape[1], x.shape[1], dtype, dev, lead=8, trail=8, left=left).put(x)


def out(rows, cols, dtype, dev, pad=8, left=8, lead=2, trail=2, batch=1, gap=0):
    return Window(rows, cols, cols + pad, dtype, dev, lead, trail, left, batch, gap).arm()


def settle(w, ref, dtype, what, factor=1.0):
    """the three conditions of an output window: guard intact (exact), every element written and finite (exact), values"""
    w.assert_guard_intact(what)
    w.assert_written(what)
    check(w.get(), ref.reshape(w.view.shape), dtype, what, factor)


# ----------------------------------------------------------------------------------------------------------------
# general 64x64 kernel
# ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gemm_data(M, N, K, dtype, nb=1):
    A, B = rnd(nb, M, K, dtype=dtype, seed=1, scale=0.5), rnd(nb, N, K, dtype=dtype, seed=2, scale=0.5)
    bias, bias2 = rnd(N, seed=3), rnd(3, N, seed=4)
    prod = torch.einsum("bmk,bnk->bmn", A.double(), B.double())
    return A, B, bias, bias2, prod


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("transA", [False, True])
@pytest.mark.parametrize("transB", [False, True])
@pytest.mark.parametrize("shape", [(70, 40, 93), (33, 5, 40), (130, 72, 64)])
@pytest.mark.parametrize("epi", ["vec", "scalar"])
def test_general_gemm_windows(dev, force, dtype, transA, transB, shape, epi):
    """comat_gemm on the general kernel, every operand layout: vec = 16-byte aligned windows at ld + 8 (the 8-column epilogue
    stores where N % 8 == 0), scalar = windows one element off alignment at an odd ld (per-element loads and stores); bias,
    per-row-group bias, activation, a residual at its own padded ldr, output in the operand dtype and in the other one"""
    M, N, K = shape
    force(gemm2=0, gemm3=0)
    pad, left = (8, 8) if epi == "vec" else (3, 1)
    A, B, bias, bias2, prod = _gemm_data(M, N, K, dtype)
    rpb = (M + 2) // 3
    k = ops.kernels()
    Aw = win(A[0].t() if transA else A[0], dtype, dev, pad, left)
    Bw = win(B[0].t() if transB else B[0], dtype, dev, pad, left)
    bw, b2w = vecw(bias, F32, dev, left), win(bias2, F32, dev, 0, left)
    for out_dt in DTYPES:
        R = rnd(M, N, dtype=out_dt, seed=5)
        Rw = win(R, out_dt, dev, pad + (8 if epi == "vec" else 2), left)
        ref = F.silu(0.5 * prod[0] + bias.double() + bias2.double().repeat_interleave(rpb, 0)[:M]) + 2.0 * R.double()
        Cw = out(M, N, out_dt, dev, pad, left)
        k.gemm(Aw.view, Bw.view, Cw.view, M, N, K, Aw.ld, Bw.ld, Cw.ld, transA=transA, transB=transB, bias=bw.view,
               bias2=b2w.view, rows_per_bias2=rpb, R=Rw.view, ldr=Rw.ld, alpha=0.5, beta=2.0, act=ops.ACT_SILU)
        served_by(dev, 0)
        settle(Cw, ref, coarser(dtype, out_dt), f"general gemm {shape} tA={transA} tB={transB} {epi} out={out_dt}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_general_gemm_heads_in_place(dev, force, dtype):
    """the two-level batch of ops._Attention: heads addressed in place inside [tokens, heads * dim] matrices.  Each head's
    [Nq, d] block lies in a [B * Nq, 3 * 40 + 8] window - heads are neighbours, the last 8 columns guard: the QK^T read (q, k
    strided by head) and the P V write (O strided by head)"""
    B_, H, Nq, Nk, d = 2, 3, 70, 45, 40
    HD = H * d
    force(gemm2=0, gemm3=0)
    k = ops.kernels()
    q, kk, v = (rnd(B_ * n, HD, dtype=dtype, seed=s) for n, s in ((Nq, 1), (Nk, 2), (Nk, 3)))
    qw, kw, vw = (win(t, dtype, dev) for t in (q, kk, v))
    Sw = out(B_ * H * Nq, Nk, F32, dev)
    k.gemm(qw.view, kw.view, Sw.view, Nq, Nk, d, qw.ld, kw.ld, Sw.ld, batch=(B_, H), sA=(Nq * qw.ld, d), sB=(Nk * kw.ld, d),
           sC=(H * Nq * Sw.ld, Nq * Sw.ld), alpha=0.3)
    served_by(dev, 0)
    qh, kh, vh = (t.double().reshape(B_, -1, H, d).permute(0, 2, 1, 3) for t in (q, kk, v))
    settle(Sw, 0.3 * qh @ kh.transpose(-1, -2), dtype, "QK^T, heads read in place")
    P = torch.softmax(rnd(B_, H, Nq, Nk, seed=4), -1).to(dtype).float()
    Pw = win(P, dtype, dev)
    Ow = out(B_ * Nq, HD, dtype, dev)
    k.gemm(Pw.view, vw.view, Ow.view, Nq, d, Nk, Pw.ld, vw.ld, Ow.ld, transB=True, batch=(B_, H),
           sA=(H * Nq * Pw.ld, Nq * Pw.ld), sB=(Nk * vw.ld, d), sC=(Nq * Ow.ld, d))
    served_by(dev, 0)
    settle(Ow, (P.double() @ vh).permute(0, 2, 1, 3).reshape(B_ * Nq, HD), dtype, "P V, heads written in place")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("splits", [2, 5])
def test_general_gemm_split_k_windows(hip, dtype, splits, default_opts):
    """the in-launch split-K combine of the general kernel (the last-arriving block runs the epilogue) into a padded ldc"""
    M, N, K = 64, 64, 1000
    _set_opts(gemm2=0, gemm3=0, force_splits=splits)
    A, B, bias, _, prod = _gemm_data(M, N, K, dtype)
    R = rnd(M, N, dtype=dtype, seed=5)
    Aw, Bw, Rw, bw = win(A[0], dtype, hip), win(B[0], dtype, hip), win(R, dtype, hip, 16), vecw(bias, F32, hip)
    for pad, left in ((8, 8), (3, 1)):
        Cw = out(M, N, F32, hip, pad, left)
        ops.kernels().gemm(Aw.view, Bw.view, Cw.view, M, N, K, Aw.ld, Bw.ld, Cw.ld, bias=bw.view, R=Rw.view, ldr=Rw.ld,
                           alpha=0.25, beta=1.0)
        served_by(hip, 0)
        settle(Cw, 0.25 * prod[0] + bias.double() + R.double(), dtype, f"split-K {splits} ldc=N+{pad}")


# ----------------------------------------------------------------------------------------------------------------
# gemm2: the LDS-DMA pipelined kernel, every block shape
# ----------------------------------------------------------------------------------------------------------------
G2_CFGS = list(range(14))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", G2_CFGS)
@pytest.mark.parametrize("splits", [0, 3])
def test_gemm2_windows(hip, cfg, splits, default_opts):
    """every block tile x split count of the pipelined kernel into ldc = N + 8 (the 8-column epilogue) and ldc = N + 4
    (epi_vec_ok refuses: the per-column path of the same epilogue): ragged M / N, bf16 and fp32 outputs, bias, bias2, residual
    at its own ldr; a batched launch whose entries lie 16 elements apart"""
    dtype = BF16
    k = ops.kernels()
    _set_opts(gemm2=1, g2_cfg=cfg, g2_splits=splits)
    for (M, N, K) in ((257, 136, 64), (300, 200, 320), (64, 64, 32), (130, 4, 96)):
        A, B, bias, bias2, prod = _gemm_data(M, N, K, dtype)
        rpb = (M + 2) // 3
        Aw, Bw, bw, b2w = win(A[0], dtype, hip), win(B[0], dtype, hip), vecw(bias, F32, hip), win(bias2, F32, hip, 0)
        pre = 0.25 * prod[0] + bias.double() + bias2.double().repeat_interleave(rpb, 0)[:M]
        for pad in (8, 4):
            for out_dt, act in ((BF16, ops.ACT_NONE), (F32, ops.ACT_SILU)):
                R = rnd(M, N, dtype=out_dt, seed=5)
                Rw = win(R, out_dt, hip, pad + 8)
                Cw = out(M, N, out_dt, hip, pad)
                k.gemm(Aw.view, Bw.view, Cw.view, M, N, K, Aw.ld, Bw.ld, Cw.ld, bias=bw.view, bias2=b2w.view, rows_per_bias2=rpb,
                       R=Rw.view, ldr=Rw.ld, alpha=0.25, beta=0.5, act=act)
                served_by(hip, 1)
                settle(Cw, ACTS[act](pre) + 0.5 * R.double(), dtype, f"gemm2 cfg={cfg} splits={splits} {(M, N, K)} ldc=N+{pad} out={out_dt}")
    M, N, K, nb = 257, 136, 64, 3
    A, B, bias, _, prod = _gemm_data(M, N, K, dtype, nb)
    R = rnd(nb, M, N, dtype=dtype, seed=5)
    Aw = Window(M, K, K + 8, dtype, hip, batch=nb, gap=16).put(A)
    Bw = Window(N, K, K + 8, dtype, hip, batch=nb, gap=16).put(B)
    Rw = Window(M, N, N + 16, dtype, hip, batch=nb, gap=16).put(R)
    bw = vecw(bias, F32, hip)
    for pad in (8, 4):
        Cw = out(M, N, dtype, hip, pad, batch=nb, gap=16)
        k.gemm(Aw.view, Bw.view, Cw.view, M, N, K, Aw.ld, Bw.ld, Cw.ld, bias=bw.view, R=Rw.view, ldr=Rw.ld, alpha=0.25, beta=0.5,
               batch=(nb, 1), sA=(Aw.stride, 0), sB=(Bw.stride, 0), sC=(Cw.stride, 0), sR=(Rw.stride, 0))
        served_by(hip, 1)
        settle(Cw, 0.25 * prod + bias.double() + 0.5 * R.double(), dtype, f"gemm2 cfg={cfg} splits={splits} batched ldc=N+{pad}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g2", [1, 0])
@pytest.mark.parametrize("case", [(130, 96, 64, 8, 2), (154, 64, 96, 16, 2)])
def test_gemm_tail_columns_windows(dev, force, dtype, g2, case):
    """comat_gemm_params::epi2 = 4: C windows at ldc = N1 + 8 (batch entries 16 elements apart), the tail columns as column
    slices of ONE [M, G * n2 + 8] window - the slices are neighbours, the last 8 columns guard - in one launch (pipelined
    kernel, bf16) and as the library's two launches"""
    M, N1, K, n2, G = case
    force(gemm2=g2, gemm3=0, g2_cfg=0, g2_splits=0)
    A = rnd(M, K, dtype=dtype, seed=1, scale=0.5)
    B, B2 = rnd(G, N1, K, dtype=dtype, seed=2, scale=0.5), rnd(G * n2, K, dtype=dtype, seed=3, scale=0.5)
    Aw, B2w = win(A, dtype, dev), win(B2, dtype, dev)
    Bw = Window(N1, K, K + 8, dtype, dev, batch=G, gap=16).put(B)
    Cw = out(M, N1, dtype, dev, batch=G, gap=16)
    Hw = out(M, G * n2, dtype, dev)
    ops.kernels().gemm(Aw.view, Bw.view, Cw.view, M, N1 + n2, K, Aw.ld, Bw.ld, Cw.ld, batch=(G, 1), sA=(0, 0), sB=(Bw.stride, 0),
                       sC=(Cw.stride, 0), tail=(B2w.view, Hw.view, n2, Hw.ld, n2 * B2w.ld, n2, 0.75))
    served_by(dev, 1 if g2 and dtype == BF16 else 0)
    what = f"tail columns gemm2={g2} {dtype} {case}"
    settle(Cw, torch.einsum("mk,gnk->gmn", A.double(), B.double()), dtype, what)
    settle(Hw, 0.75 * A.double() @ B2.double().t(), dtype, what + " (tail)")


@pytest.mark.gpu
@pytest.mark.parametrize("M", [77, 130])
@pytest.mark.parametrize("N", [64, 96])
def test_geglu_epilogue_windows(hip, M, N, default_opts):
    """the GEGLU epilogues of the pipelined kernel (epi2 = 1, 2, their e4m3 form, and the backward epi2 = 3).  The binding takes
    C2, the saved pre-activations and q8 contiguous: guard rows; C (pre-activations out / their gradient) at a padded ldc.  The
    bf16 results and the bytes are those of the two-launch form (plain product on the same kernel, then the interleaved-layout
    kernel / comat_fp8_quantize_scaled), bit for bit; the values against fp64."""
    dtype, K = BF16, 64
    k = ops.kernels()
    _set_opts(gemm2=1, gemm3=0, g2_cfg=0, g2_splits=0)
    D = N // 2
    x, w, b = rnd(M, K, dtype=dtype, seed=1), rnd(N, K, dtype=dtype, seed=2, scale=K ** -0.5), rnd(N, seed=3)
    xw, ww, bw = win(x, dtype, hip), win(w, dtype, hip), vecw(b, F32, hip)
    pre0, y0 = out(M, N, dtype, hip, 0), out(M, D, dtype, hip, 0)  # two launches
    k.gemm(xw.view, ww.view, pre0.view, M, N, K, xw.ld, ww.ld, N, bias=bw.view)
    served_by(hip, 1)
    k.geglu_il_fwd(pre0.view, y0.view, M, D)
    ref_pre = x.double() @ w.double().t() + b.double()
    settle(pre0, ref_pre, dtype, "pre-activations (plain product)")
    t = pre0.get().cpu().double().reshape(M, N // 32, 2, 16)
    ref_y = (t[:, :, 0] * F.gelu(t[:, :, 1])).reshape(M, D)
    settle(y0, ref_y, dtype, "geglu_il_fwd")
    scale = vecw((OF.scale_of(y0.get().cpu()) * 0.8).reshape(1), F32, hip)
    bytes0 = OF.quantize_with_scale(y0.get().cpu(), scale.get().cpu()[0, 0])
    for keep, with_y, with_q in ((True, True, False), (False, True, False), (True, True, True), (False, False, True)):
        what = f"geglu epilogue M={M} N={N} keep_pre={keep} y={with_y} q8={with_q}"
        prew = out(M, N, dtype, hip) if keep else None
        yw = out(M, D, dtype, hip, 0) if with_y else None
        qw = Window(M, D, D, torch.uint8, hip).arm() if with_q else None
        amax = Window(1, 1, 1, torch.int32, hip, lead=8, trail=8)
        amax.view.zero_()
        amax.arm()
        scale.arm()
        k.gemm(xw.view, ww.view, prew.view if keep else None, M, N, K, xw.ld, ww.ld, prew.ld if keep else N, bias=bw.view,
               geglu=(yw.view if with_y else None, keep), q8=(qw.view, scale.view, amax.view) if with_q else None)
        served_by(hip, 1)
        if keep:
            prew.assert_guard_intact(what)
            assert torch.equal(prew.get(), pre0.get()), what + ": pre-activations differ from the plain product"
        if with_y:
            yw.assert_guard_intact(what)
            assert torch.equal(yw.get(), y0.get()), what + ": product differs from the two-launch form"
        if with_q:
            qw.assert_guard_intact(what)
            amax.assert_guard_intact(what)
            scale.assert_guard_intact(what)
            assert torch.equal(qw.get().cpu(), bytes0), what + ": bytes differ from comat_fp8_quantize_scaled of the product"
            assert float(amax.get().cpu().view(F32)) == float(y0.get().float().abs().max()), what + ": abs-max"
    # backward epilogue (epi2 = 3): product dF [M, Nb], saved pre-activations [M, 2 Nb] in, their gradient [M, 2 Nb] out
    Nb = N
    g, w2 = rnd(M, K, dtype=dtype, seed=5), rnd(Nb, K, dtype=dtype, seed=6, scale=K ** -0.5)
    pre = rnd(M, 2 * Nb, dtype=dtype, seed=7)
    gw, w2w, pw = win(g, dtype, hip), win(w2, dtype, hip), win(pre, dtype, hip, 0)
    dF0, dx0 = out(M, Nb, dtype, hip, 0), out(M, 2 * Nb, dtype, hip, 0)
    k.gemm(gw.view, w2w.view, dF0.view, M, Nb, K, gw.ld, w2w.ld, Nb)
    k.geglu_il_bwd(dF0.view, pw.view, dx0.view, M, Nb)
    settle(dF0, g.double() @ w2.double().t(), dtype, "dF (plain product)")
    pr = pre.double().reshape(M, Nb // 16, 2, 16).requires_grad_(True)
    (pr[:, :, 0] * F.gelu(pr[:, :, 1])).reshape(M, Nb).backward(dF0.get().cpu().double())
    settle(dx0, pr.grad.reshape(M, 2 * Nb), dtype, "geglu_il_bwd")
    dxw = out(M, 2 * Nb, dtype, hip)
    k.gemm(gw.view, w2w.view, dxw.view, M, Nb, K, gw.ld, w2w.ld, dxw.ld, geglu=(pw.view, "bwd"))
    served_by(hip, 1)
    dxw.assert_guard_intact("geglu backward epilogue")
    assert torch.equal(dxw.get(), dx0.get()), "geglu backward epilogue differs from the two-launch form"


# ----------------------------------------------------------------------------------------------------------------
# gemm3: the lean kernel, every tile shape
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_gemm3_windows(hip, cfg, default_opts):
    """gemm3.hip under every tile shape into ldc = N + 8 and N + 4: a batched launch with gaps, bias + residual, and the
    K-segmented form whose second A operand is a column slice of a [M, G * r + 8] window (lda = G * r + 8)"""
    dtype = BF16
    k = ops.kernels()
    _set_opts(gemm3=2, g3_cfg=cfg)
    for (M, N, K, nb, extra) in ((130, 96, 64, 2, False), (300, 200, 320, 1, True)):
        A, B, bias, _, prod = _gemm_data(M, N, K, dtype, nb)
        R = rnd(nb, M, N, dtype=dtype, seed=5)
        Aw = Window(M, K, K + 8, dtype, hip, batch=nb, gap=16).put(A)
        Bw = Window(N, K, K + 8, dtype, hip, batch=nb, gap=16).put(B)
        Rw = Window(M, N, N + 16, dtype, hip, batch=nb, gap=16).put(R)
        bw = vecw(bias, F32, hip)
        for pad in (8, 4):
            for out_dt in (BF16, F32):
                Cw = out(M, N, out_dt, hip, pad, batch=nb, gap=16)
                k.gemm(Aw.view, Bw.view, Cw.view, M, N, K, Aw.ld, Bw.ld, Cw.ld, bias=bw.view if extra else None,
                       R=Rw.view if extra else None, ldr=Rw.ld, beta=1.0 if extra else 0.0, batch=(nb, 1), sA=(Aw.stride, 0),
                       sB=(Bw.stride, 0), sC=(Cw.stride, 0), sR=(Rw.stride, 0))
                served_by(hip, 5)
                ref = prod + (bias.double() + R.double() if extra else 0.0)
                settle(Cw, ref, dtype, f"gemm3 cfg={cfg} {(M, N, K, nb)} ldc=N+{pad} out={out_dt}")
    M, N, K1, r, G = 130, 96, 64, 64, 2
    x, W = rnd(M, K1, dtype=dtype, seed=31, scale=0.3), rnd(G, N, K1, dtype=dtype, seed=32, scale=0.3)
    H_, U = rnd(M, G * r, dtype=dtype, seed=33, scale=0.3), rnd(G, N, r, dtype=dtype, seed=34, scale=0.3)
    xw, Hw = win(x, dtype, hip), win(H_, dtype, hip)
    Ww = Window(N, K1, K1 + 8, dtype, hip, batch=G, gap=16).put(W)
    Uw = Window(N, r, r + 8, dtype, hip, batch=G, gap=16).put(U)
    ref = torch.stack([x.double() @ W[i].double().t() + H_[:, i * r:(i + 1) * r].double() @ U[i].double().t() for i in range(G)])
    for pad in (8, 4):
        Cw = out(M, N, dtype, hip, pad, batch=G, gap=16)
        k.gemm_segments([(xw.view, Ww.view, K1, xw.ld, Ww.ld, 0, Ww.stride), (Hw.view, Uw.view, r, Hw.ld, Uw.ld, r, Uw.stride)],
                        Cw.view, M, N, Cw.ld, batch=G, sC=Cw.stride)
        served_by(hip, 5)
        settle(Cw, ref, dtype, f"gemm3 cfg={cfg} K-segmented, batched, ldc=N+{pad}")


# ----------------------------------------------------------------------------------------------------------------
# K-segmented and grouped k-major products
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g2", [1, 0])
@pytest.mark.parametrize("shape", [(130, 64, 8), (70, 40, 4), (257, 96, 16)])
def test_gemm_segments_windows(dev, force, dtype, g2, shape):
    """test_gemm_segments' shapes with NaN in the lda / ldb padding, a residual at ldr and the output's ldc padding compared
    bit for bit; segment widths that keep the pipelined kernel eligible (bf16, K_s % 32 == 0) and ones that do not"""
    M, N, r = shape
    force(gemm2=g2, gemm3=0)
    k = ops.kernels()
    for Ks, fam in (([72, 3 * r, 33 if dtype == F32 else 40, r], 0), ([64, 32, 96], 1 if g2 and dtype == BF16 else 0)):
        segs, acc = [], torch.zeros(M, N, dtype=torch.float64)
        for i, K in enumerate(Ks):
            A, B = rnd(M, K, dtype=dtype, seed=10 + i), rnd(N, K, dtype=dtype, seed=20 + i, scale=K ** -0.5)
            Aw, Bw = win(A, dtype, dev, 8 if i % 2 else 16), win(B, dtype, dev, 16 if i == 2 else 8)
            acc = acc + A.double() @ B.double().t()
            segs.append((Aw.view, Bw.view, K, Aw.ld, Bw.ld))
        bias, R = rnd(N, seed=3), rnd(M, N, dtype=dtype, seed=4)
        bw, Rw = vecw(bias, F32, dev), win(R, dtype, dev, 16)
        for pad, left in ((8, 8), (3, 1)):
            Cw = out(M, N, dtype, dev, pad, left)
            k.gemm_segments(segs, Cw.view, M, N, Cw.ld, bias=bw.view, R=Rw.view, ldr=Rw.ld, alpha=0.5, beta=2.0)
            served_by(dev, fam)
            settle(Cw, 0.5 * acc + bias.double() + 2.0 * R.double(), dtype, f"gemm_segments {shape} Ks={Ks} ldc=N+{pad}")


def test_gemm_tt_grouped_windows(dev):
    """comat_gemm_tt_grouped on test_gemm_tt_grouped's small shapes: NaN in the lda / ldb padding, the accumulated-into C at a
    padded ldc whose pad columns (and guard rows) are compared bit for bit"""
    dtype = BF16
    k = ops.kernels()
    shapes = [(8, 8, 1), (136, 264, 77), (16, 24, 31), (128, 136, 300)]
    probs, wins, refs = [], [], []
    for i, (M, N, K) in enumerate(shapes):
        A, B = rnd(K, M, dtype=dtype, seed=100 + i, scale=0.5), rnd(K, N, dtype=dtype, seed=300 + i, scale=0.5)
        C0 = rnd(M, N, seed=500 + i)
        Aw, Bw = win(A, dtype, dev, 8 * (i % 2 + 1)), win(B, dtype, dev, 16 if i % 2 else 8)
        Cw = Window(M, N, N + 4 * (i % 3 + 1), F32, dev).put(C0).arm()
        probs.append((Aw.view, Bw.view, Cw.view, M, N, K, Aw.ld, Bw.ld, Cw.ld))
        assert k.tt_group_ok(*probs[-1])
        wins.append(Cw)
        refs.append(C0.double() + A.double().t() @ B.double())
    k.gemm_tt_grouped(probs)
    served_by(dev, 4)
    for Cw, ref, shp in zip(wins, refs, shapes):
        settle(Cw, ref, F32, f"tt_grouped {shp}")


# ----------------------------------------------------------------------------------------------------------------
# conv2d as implicit GEMM
# ----------------------------------------------------------------------------------------------------------------
CONV_CASES = [  # B, H, W, Cin, Cout, stride, ups, factor of the data-gradient's tolerance in the sibling test of test_ops.py
    (2, 13, 9, 32, 72, 1, 1, 2),   # test_gemm2_segments_and_conv
    (1, 15, 17, 32, 32, 2, 1, 1),  # test_conv2d_fwd_bwd
    (1, 8, 8, 96, 64, 1, 2, 2),    # test_gemm2_segments_and_conv
    (1, 9, 7, 4, 40, 1, 1, 1),     # test_conv2d_fwd_bwd
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g2", [1, 0])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv2d_windows(dev, force, dtype, g2, case):
    """comat_conv2d, the launches of ops.conv2d's forward and data-gradient (mode 0 with the flipped weight; mode 1 for the
    strided conv; the 2x upsample's sum pooling): the image sits between NaN guard rows, so a tap that leaves it by the top of
    sample 0 or the bottom of the last sample reads poison; Y, dX (and the residual) between guard rows.  Cout = 72 / 40: a
    ragged last column tile."""
    B_, H, W, Cin, Cout, stride, ups, dgrad_factor = case
    force(gemm2=g2, gemm3=0)
    k = ops.kernels()
    x = rnd(B_, Cin, H, W, dtype=dtype, seed=1)
    w = rnd(Cout, Cin, 3, 3, dtype=dtype, seed=2, scale=1.0 / math.sqrt(Cin * 9))
    b, temb = rnd(Cout, seed=3), rnd(B_, Cout, seed=4)
    conv = ops.FrozenConv(w, b, dtype, dev, stride=stride, pad=1)
    Ho, Wo = ops.conv_out_hw(conv, H, W, ups)
    res, gy = rnd(B_, Cout, Ho, Wo, dtype=dtype, seed=5), rnd(B_, Cout, Ho, Wo, dtype=dtype, seed=6)
    xr = x.double().requires_grad_(True)
    xin = F.interpolate(xr, scale_factor=2, mode="nearest") if ups == 2 else xr
    yref = F.conv2d(xin, w.double(), b.double(), stride=stride, padding=1) + temb.double()[:, :, None, None] + res.double()
    yref.backward(gy.double())
    tok = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    xw, rw, gw = win(tok(x), dtype, dev, 0), win(tok(res), dtype, dev, 0), win(tok(gy), dtype, dev, 0)
    ww, wdw = win(conv.w.reshape(Cout, -1), dtype, dev, 0), win(conv.wd.reshape(Cin, -1), dtype, dev, 0)
    bw, tw = vecw(b, F32, dev), win(temb, F32, dev, 0)
    bf = dtype == BF16
    Yw = out(B_ * Ho * Wo, Cout, dtype, dev, 0)
    k.conv2d(xw.view, ww.view, Yw.view, B_, H, W, Cin, Ho, Wo, Cout, 3, 3, stride, 1, mode=0, ups=ups, bias=bw.view, bias2=tw.view,
             R=rw.view, beta=1.0)
    served_by(dev, 1 if g2 and bf and Cin % 32 == 0 and B_ * Ho * Wo >= 48 else 0)
    what = f"conv {case} {dtype} gemm2={g2}"
    settle(Yw, tok(yref), dtype, what)
    Hs, Ws = H * ups, W * ups
    if stride == 1:
        duw = out(B_ * Hs * Ws, Cin, dtype, dev, 0)
        k.conv2d(gw.view, wdw.view, duw.view, B_, Ho, Wo, Cout, Hs, Ws, Cin, 3, 3, 1, 1, mode=0)
        served_by(dev, 1 if g2 and bf and Cout % 32 == 0 and B_ * Hs * Ws >= 48 else 0)
        if ups == 2:
            duw.assert_guard_intact(what + " dgrad (upsampled)")
            duw.assert_written(what + " dgrad (upsampled)")
            dxw = out(B_ * H * W, Cin, dtype, dev, 0)
            duw.arm()
            k.sumpool2x2(duw.view, dxw.view, B_, H, W, Cin)
            duw.assert_guard_intact(what + " sumpool input")
        else:
            dxw = duw
    else:
        dxw = out(B_ * H * W, Cin, dtype, dev, 0)
        k.conv2d(gw.view, wdw.view, dxw.view, B_, Ho, Wo, Cout, H, W, Cin, 3, 3, stride, 1, mode=1)
        served_by(dev, 1 if g2 and bf and Cout % 32 == 0 and B_ * H * W >= 48 else 0)
    settle(dxw, tok(xr.grad), dtype, what + " dgrad", factor=dgrad_factor)


# ----------------------------------------------------------------------------------------------------------------
# fused attention, forward and backward, at the level of the C ABI
# ----------------------------------------------------------------------------------------------------------------
FLASH_SELF = [(2, 130, 130, 2, 40),   # trimmed 64-wide tile, two query blocks, the second tile of the last 64-key pair wholly beyond Nk
              (1, 197, 197, 3, 64), (2, 70, 70, 2, 80),  # 80: trimmed 96-wide tile
              (1, 33, 33, 1, 160), (2, 16, 16, 2, 16)]
FLASH_CROSS = [(1, 257, 77, 2, 40),   # 9 query tiles, < 256 base blocks: qsplit = 2, flash_kv_reduce_kernel into strided dK / dV
               (2, 64, 77, 2, 160)]
FLASH_GEOS = [g + (True,) for g in FLASH_SELF] + [g + (False,) for g in FLASH_CROSS]


@functools.lru_cache(maxsize=None)
def _flash_data(geo, dtype):
    B_, Nq, Nk, H, d, _ = geo
    D = H * d
    q, kk, v = (rnd(B_ * n, D, dtype=dtype, seed=s) for n, s in ((Nq, 1), (Nk, 2), (Nk, 3)))
    go = rnd(B_ * Nq, D, dtype=dtype, seed=4)
    qr, kr, vr = (t.double().reshape(B_, -1, H, d).permute(0, 2, 1, 3).clone().requires_grad_(True) for t in (q, kk, v))
    o = (torch.softmax(qr @ kr.transpose(-1, -2) * d ** -0.5, -1) @ vr).permute(0, 2, 1, 3).reshape(B_ * Nq, D)
    o.backward(go.double())
    back = lambda t: t.grad.permute(0, 2, 1, 3).reshape(-1, D)
    return q, kk, v, go, o.detach(), back(qr), back(kr), back(vr)


def _flash_windows(dev, dtype, geo):
    """forward + backward of one geometry with every operand in a window.  Self-attention: q, k, v are column slices of a
    [B N, 3 D + 8] window (the layout of _FusedQKVAttention), dQ, dK, dV column slices of a guarded one; cross-attention: k, v
    (dK, dV) slices of a [B Nk, 2 D + 8] window.  O / dO at ld D + 8; lse, Dbuf between guard elements."""
    B_, Nq, Nk, H, d, self_attn = geo
    D = H * d
    q, kk, v, go, o_ref, dq_ref, dk_ref, dv_ref = _flash_data(geo, dtype)
    k = ops.kernels()
    if self_attn:
        inw = win(torch.cat([q, kk, v], 1), dtype, dev)
        gw = out(B_ * Nq, 3 * D, dtype, dev)
        qv, kv, vv = (inw.view[:, i * D:(i + 1) * D] for i in range(3))
        dqv, dkv, dvv = (gw.view[:, i * D:(i + 1) * D] for i in range(3))
        ldq = ldk = inw.ld
        gws = [gw]
        grefs = [torch.cat([dq_ref, dk_ref, dv_ref], 1)]
    else:
        qw, kvw = win(q, dtype, dev), win(torch.cat([kk, v], 1), dtype, dev)
        gqw, gkvw = out(B_ * Nq, D, dtype, dev), out(B_ * Nk, 2 * D, dtype, dev)
        qv, kv, vv = qw.view, kvw.view[:, :D], kvw.view[:, D:]
        dqv, dkv, dvv = gqw.view, gkvw.view[:, :D], gkvw.view[:, D:]
        ldq, ldk = qw.ld, kvw.ld
        gws = [gqw, gkvw]
        grefs = [dq_ref, torch.cat([dk_ref, dv_ref], 1)]
    Ow, gow = out(B_ * Nq, D, dtype, dev), win(go, dtype, dev)
    lse = Window(1, B_ * H * Nq, None, F32, dev, lead=8, trail=8).arm()
    what = f"flash {geo} {dtype}"
    k.flash_attn_fwd(qv, kv, vv, Ow.view, lse.flat.view(B_, H, Nq), B_, H, Nq, Nk, d, ldq, ldk, ldk, Ow.ld, d ** -0.5)
    settle(Ow, o_ref, dtype, what + " O")
    lse.assert_guard_intact(what + " lse")
    lse.assert_written(what + " lse")
    dbuf = Window(1, B_ * H * Nq, None, F32, dev, lead=8, trail=8).arm()
    Ow.arm()
    lse.arm()
    k.flash_attn_bwd(qv, kv, vv, Ow.view, gow.view, lse.flat.view(B_, H, Nq), dbuf.flat.view(B_, H, Nq), dqv, dkv, dvv, B_, H, Nq, Nk, d, ldq, ldk, ldk, Ow.ld, d ** -0.5)
    for w, name in ((dbuf, "D"), (Ow, "saved O"), (lse, "saved lse")):
        w.assert_guard_intact(what + " " + name)
        w.assert_written(what + " " + name)
    for w, ref in zip(gws, grefs):
        settle(w, ref, dtype, what + " dQ / dK / dV", factor=3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geo", FLASH_GEOS)
def test_flash_windows(dev, dtype, geo):
    _flash_windows(dev, dtype, geo)


FLASH_VARIANTS = [(BF16, kt, mg, 1) for kt in (1, 4) for mg in (0, 1)] + [(F32, 4, mg, tr) for mg in (0, 1) for tr in (0, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", FLASH_VARIANTS)
@pytest.mark.parametrize("geo", FLASH_GEOS)
def test_flash_variant_windows(hip, variant, geo, default_opts):
    """the one-tile and two-tile bodies (flash_kt), the merged and the separate backward launches (flash_merge) and - fp32 - the
    plain and the transposed-image staging (flash_tr) all meet the windows"""
    dtype, kt, mg, tr = variant
    _set_opts(flash_kt=kt, flash_merge=mg, flash_tr=tr)
    _flash_windows(hip, dtype, geo)


def test_flash_q8_windows(dev):
    """comat_flash_attn_fwd_q: the e4m3 bytes at ldq8 = D + 8 in a guarded byte window, bit for bit comat_fp8_quantize_scaled of O"""
    geo = (2, 70, 70, 2, 40, True)
    B_, Nq, Nk, H, d, _ = geo
    D, dtype = H * d, BF16
    q, kk, v, _, o_ref = _flash_data(geo, dtype)[:5]
    k = ops.kernels()
    inw = win(torch.cat([q, kk, v], 1), dtype, dev)
    qv, kv, vv = (inw.view[:, i * D:(i + 1) * D] for i in range(3))
    Ow = out(B_ * Nq, D, dtype, dev)
    lse = Window(1, B_ * H * Nq, None, F32, dev, lead=8, trail=8).arm()
    q8 = Window(B_ * Nq, D, D + 8, torch.uint8, dev).arm()
    scale = vecw((OF.scale_of(o_ref) * 0.7).reshape(1), F32, dev).arm()
    amax = Window(1, 1, 1, torch.int32, dev, lead=8, trail=8)
    amax.view.zero_()
    amax.arm()
    k.flash_attn_fwd(qv, kv, vv, Ow.view, lse.flat.view(B_, H, Nq), B_, H, Nq, Nk, d, inw.ld, inw.ld, inw.ld, Ow.ld, d ** -0.5,
                     q8=(q8.padded, scale.flat, amax.flat))
    settle(Ow, o_ref, dtype, "flash q8: O")
    for w, name in ((lse, "lse"), (q8, "bytes"), (scale, "scale"), (amax, "abs-max")):
        w.assert_guard_intact("flash q8: " + name)
    o = Ow.get()
    am2 = torch.zeros(1, dtype=torch.int32, device=dev)
    assert torch.equal(q8.get(), k.fp8_quantize_scaled(o, scale.flat, am2)), "bytes differ from comat_fp8_quantize_scaled(O)"
    assert torch.equal(q8.get().cpu(), OF.quantize_with_scale(o.cpu(), scale.get().cpu()[0, 0]))
    assert float(amax.get().cpu().view(F32)) == float(o.float().abs().max())


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_qkv_attention_op(dev, dtype):
    """ops.fused_qkv_attention itself (the strided fused attention behind BLIP's ViT) against the split-projection reference:
    output and the input gradient, from an input between NaN guard rows"""
    B_, N, H, d, Kd = 2, 70, 2, 40, 48
    D = H * d
    x, w, b = rnd(B_ * N, Kd, dtype=dtype, seed=1), rnd(3 * D, Kd, dtype=dtype, seed=2, scale=Kd ** -0.5), rnd(3 * D, seed=3)
    go = rnd(B_ * N, D, dtype=dtype, seed=4)
    xr = x.double().requires_grad_(True)
    qh, kh, vh = ((xr @ w.double()[i * D:(i + 1) * D].t() + b.double()[i * D:(i + 1) * D]).reshape(B_, N, H, d).permute(0, 2, 1, 3)
                  for i in range(3))
    o_ref = (torch.softmax(qh @ kh.transpose(-1, -2) * d ** -0.5, -1) @ vh).permute(0, 2, 1, 3).reshape(B_ * N, D)
    o_ref.backward(go.double())
    xw, gw = win(x, dtype, dev, 0), win(go, dtype, dev, 0)
    xd = xw.view.requires_grad_(True)
    o = ops.fused_qkv_attention(xd, ops.FrozenLinear(w, b, dtype, dev), B_, N, H)
    o.backward(gw.view)
    check(o, o_ref, dtype, "fused qkv attention")
    assert torch.isfinite(o.float()).all() and torch.isfinite(xd.grad.float()).all()
    check(xd.grad, xr.grad, dtype, "fused qkv attention dx", factor=3)


# ----------------------------------------------------------------------------------------------------------------
# normalisation: no leading dimension - guard rows on x, dy, add, y, dx, the statistics and the bytes
# ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ln_data(M, C, dtype):
    x = rnd(M, C, dtype=dtype, seed=1) * 1.5 - 0.4
    gamma, beta = rnd(C, seed=2) * 0.5 + 1, rnd(C, seed=3) * 0.3
    gy, add = rnd(M, C, dtype=dtype, seed=4), rnd(M, C, dtype=dtype, seed=5)
    xr = x.double().requires_grad_(True)
    yr = F.layer_norm(xr, (C,), gamma.double(), beta.double(), eps=1e-5)
    yr.backward(gy.double())
    return x, gamma, beta, gy, add, yr.detach(), xr.grad + add.double()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(5, 70),      # scalar kernel
                                   (37, 96),
                                   (3, 520),     # bf16: 65 16-byte vectors - the second per-lane slot holds one lane
                                   (2, 2056)])   # more than 4 vectors per lane: scalar kernel
def test_layernorm_windows(dev, dtype, shape):
    M, C = shape
    x, gamma, beta, gy, add, y_ref, dx_ref = _ln_data(M, C, dtype)
    k = ops.kernels()
    xw, gyw, aw = (win(t, dtype, dev, 0) for t in (x, gy, add))
    gw, bw = vecw(gamma, F32, dev), vecw(beta, F32, dev)
    yw, sw = out(M, C, dtype, dev, 0), out(M, 2, F32, dev, 0)
    k.layernorm_fwd(xw.view, gw.flat, bw.flat, yw.view, sw.view, M, C, 1e-5)
    settle(yw, y_ref, dtype, f"ln fwd {shape}")
    sw.assert_guard_intact("ln stats")
    sw.assert_written("ln stats")
    dxw = out(M, C, dtype, dev, 0)
    sw.arm()
    k.layernorm_bwd(gyw.view, xw.view, gw.flat, sw.view, dxw.view, M, C, add=aw.view)
    settle(dxw, dx_ref, dtype, f"ln bwd {shape}", factor=2)
    sw.assert_guard_intact("ln stats (read by bwd)")
    if k.layernorm_fwd_q_ok(xw.view):
        y2, s2 = out(M, C, dtype, dev, 0), out(M, 2, F32, dev, 0)
        q8 = Window(M, C, C, torch.uint8, dev).arm()
        scale = vecw((OF.scale_of(y_ref) * 0.8).reshape(1), F32, dev).arm()
        amax = Window(1, 1, 1, torch.int32, dev, lead=8, trail=8)
        amax.view.zero_()
        amax.arm()
        k.layernorm_fwd_q(xw.view, gw.flat, bw.flat, y2.view, s2.view, M, C, 1e-5, q8.view, scale.flat, amax.flat)
        for w, name in ((y2, "y"), (s2, "stats"), (q8, "bytes"), (scale, "scale"), (amax, "abs-max")):
            w.assert_guard_intact(f"ln fwd_q {shape}: {name}")
        assert torch.equal(y2.get(), yw.get()) and torch.equal(s2.get(), sw.get()), "ln fwd_q: y / stats differ from layernorm_fwd"
        assert torch.equal(q8.get().cpu(), OF.quantize_with_scale(yw.get().cpu(), scale.get().cpu()[0, 0]))
        assert float(amax.get().cpu().view(F32)) == float(yw.get().float().abs().max())


@functools.lru_cache(maxsize=None)
def _gn_data(B_, HW, C, G, dtype):
    x = rnd(B_, HW, C, dtype=dtype, seed=1) * 2 + 0.7
    gamma, beta = rnd(C, seed=2) * 0.5 + 1, rnd(C, seed=3) * 0.3
    gy, add = rnd(B_ * HW, C, dtype=dtype, seed=4), rnd(B_ * HW, C, dtype=dtype, seed=5)
    res = {}
    for silu in (False, True):
        xr = x.double().requires_grad_(True)
        yr = F.group_norm(xr.permute(0, 2, 1), G, gamma.double(), beta.double(), eps=1e-5).permute(0, 2, 1)
        yr = (F.silu(yr) if silu else yr).reshape(B_ * HW, C)
        yr.backward(gy.double())
        res[silu] = (yr.detach(), xr.grad.reshape(B_ * HW, C) + add.double())
    return x, gamma, beta, gy, add, res


GN_SHAPES = [(3, 77, 24, 8), (2, 50, 32, 8), (2, 64, 80, 8)]


def _groupnorm_windows(dev, dtype, shape, silu):
    B_, HW, C, G = shape
    x, gamma, beta, gy, add, res = _gn_data(B_, HW, C, G, dtype)
    y_ref, dx_ref = res[silu]
    k = ops.kernels()
    xw, gyw, aw = (win(t, dtype, dev, 0) for t in (x, gy, add))
    gw, bw = vecw(gamma, F32, dev), vecw(beta, F32, dev)
    yw, sw = out(B_ * HW, C, dtype, dev, 0), out(B_ * G, 2, F32, dev, 0)
    stats = sw.view.view(B_, G, 2)
    what = f"gn {shape} silu={silu} {dtype}"
    k.groupnorm_fwd(xw.view, gw.flat, bw.flat, yw.view, stats, B_, HW, C, G, 1e-5, silu)
    settle(yw, y_ref, dtype, what + " fwd")
    sw.assert_guard_intact(what + " stats")
    sw.assert_written(what + " stats")
    dxw = out(B_ * HW, C, dtype, dev, 0)
    sw.arm()
    k.groupnorm_bwd(gyw.view, xw.view, gw.flat, bw.flat, stats, dxw.view, B_, HW, C, G, silu, add=aw.view)
    settle(dxw, dx_ref, dtype, what + " bwd", factor=2)
    sw.assert_guard_intact(what + " stats (read by bwd)")
    if k.groupnorm_fwd_q_ok(xw.view, B_, HW, C, G):
        y2, s2 = out(B_ * HW, C, dtype, dev, 0), out(B_ * G, 2, F32, dev, 0)
        q8 = Window(B_ * HW, C, C, torch.uint8, dev).arm()
        scale = vecw((OF.scale_of(y_ref) * 0.8).reshape(1), F32, dev).arm()
        amax = Window(1, 1, 1, torch.int32, dev, lead=8, trail=8)
        amax.view.zero_()
        amax.arm()
        k.groupnorm_fwd_q(xw.view, gw.flat, bw.flat, y2.view, s2.view.view(B_, G, 2), B_, HW, C, G, 1e-5, silu, q8.view, scale.flat,
                          amax.flat)
        for w, name in ((y2, "y"), (s2, "stats"), (q8, "bytes"), (scale, "scale"), (amax, "abs-max")):
            w.assert_guard_intact(what + " fwd_q: " + name)
        assert torch.equal(y2.get(), yw.get()) and torch.equal(s2.get(), sw.get()), what + " fwd_q: y / stats differ from groupnorm_fwd"
        assert torch.equal(q8.get().cpu(), OF.quantize_with_scale(yw.get().cpu(), scale.get().cpu()[0, 0]))
        assert float(amax.get().cpu().view(F32)) == float(yw.get().float().abs().max())
        return True
    return False


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("shape", GN_SHAPES + [(1, 300, 32, 8)])  # the last one: a shape comat_groupnorm_fwd_q takes
def test_groupnorm_windows(dev, dtype, silu, shape):
    took_q = _groupnorm_windows(dev, dtype, shape, silu)
    assert took_q or shape[1] <= 256, "comat_groupnorm_fwd_q declined the shape that is here for it"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [0, 3, 5])
@pytest.mark.parametrize("shape", GN_SHAPES)
def test_groupnorm_variant_windows(hip, dtype, mode, shape, default_opts):
    """option norm_fused: the three-launch form (0), one launch always (3) and where it pays (5)"""
    _set_opts(norm_fused=mode)
    for silu in (False, True):
        _groupnorm_windows(hip, dtype, shape, silu)


# ----------------------------------------------------------------------------------------------------------------
# softmax and cross-entropy
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", [1, 65, 77])
@pytest.mark.parametrize("mode", ["plain", "causal", "masked"])
def test_softmax_windows(dev, dtype, cols, mode):
    """comat_softmax_fwd / _bwd as ops._Attention calls them: fp32 scores in, probabilities in the storage dtype out; causal with
    causal_offset = Nk - Nq; a key mask per sample.  The probabilities hold to the tolerance of test_attention's "attn probs";
    dS = scale P (dP - sum dP P) is the same kind of quantity - one row reduction, one rounding to the storage dtype - and holds
    to the same one."""
    B_, H = 2, 2
    Nq = min(7, cols)
    rows = B_ * H * Nq
    S = rnd(rows, cols, seed=1) * 2
    dP = rnd(rows, cols, seed=2)
    s = S.double().reshape(B_, H, Nq, cols)
    km = None
    if mode == "causal":
        s = s.masked_fill(~torch.ones(Nq, cols, dtype=torch.bool).tril(diagonal=cols - Nq), float("-inf"))
    if mode == "masked":
        km = torch.ones(B_, cols, dtype=torch.int8)
        km[0, cols - cols // 3:] = 0
        km[1, :cols // 2] = 0
        s = s.masked_fill(~km.bool()[:, None, None, :], float("-inf"))
    p_ref = torch.softmax(s, -1).reshape(rows, cols)
    k = ops.kernels()
    Sw = win(S, F32, dev, 0)
    kmw = Window(B_, cols, cols, torch.int8, dev).put(km) if km is not None else None
    Pw = out(rows, cols, dtype, dev, 0)
    k.softmax_fwd(Sw.view, Pw.view, rows, cols, q_len=Nq, causal=mode == "causal", causal_offset=cols - Nq,
                  key_mask=kmw.view if kmw is not None else None, rows_per_mask=H * Nq)
    settle(Pw, p_ref, dtype, f"softmax fwd cols={cols} {mode}")
    p = Pw.get().cpu().double()
    dPw = win(dP, F32, dev, 0)
    dSw = out(rows, cols, dtype, dev, 0)
    Pw.arm()
    k.softmax_bwd(Pw.view, dPw.view, dSw.view, rows, cols, 0.3)
    Pw.assert_guard_intact("softmax bwd: P")
    settle(dSw, 0.3 * p * (dP.double() - (dP.double() * p).sum(-1, keepdim=True)), dtype, f"softmax bwd cols={cols} {mode}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [70, 257])
@pytest.mark.parametrize("ls", [0.0, 0.1])
def test_cross_entropy_windows(dev, dtype, V, ls):
    """comat_cross_entropy_fwd / _bwd on logits [T, V] at ld = V + 8 with NaN pad columns; dlogits guarded at the same ld; an
    ignored row; every small operand (labels, log-probs, row statistics, the loss pair, the upstream gradient) between guards"""
    T = 9
    z = rnd(T, V, dtype=dtype, seed=1, scale=3.0)
    labels = torch.randint(0, V, (T,), generator=torch.Generator().manual_seed(2))
    labels[3] = -100
    labels[0], labels[T - 1] = 0, V - 1
    zr = z.double().requires_grad_(True)
    ref = F.cross_entropy(zr, labels, ignore_index=-100, label_smoothing=ls)
    (2.5 * ref).backward()
    lp_ref = torch.log_softmax(z.double(), -1).gather(1, labels.clamp(min=0)[:, None])[:, 0] * (labels >= 0)
    k = ops.kernels()
    zw = win(z, dtype, dev)
    lw = Window(1, T, None, torch.int64, dev, lead=8, trail=8).put(labels.reshape(1, T))
    logp, rlse, lsc = (Window(1, n, None, F32, dev, lead=8, trail=8).arm() for n in (T, T, 2))
    k.cross_entropy_fwd(zw.view, lw.flat, logp.flat, rlse.flat, lsc.flat, T, V, zw.ld, -100, ls)
    for w, name in ((logp, "log-probs"), (rlse, "row lse"), (lsc, "loss sum / count")):
        w.assert_guard_intact("ce fwd: " + name)
        w.assert_written("ce fwd: " + name)
    loss = lsc.get().cpu()[0, 0] / lsc.get().cpu()[0, 1]
    assert float(lsc.get().cpu()[0, 1]) == T - 1
    check(loss.reshape(1), ref.detach().reshape(1), F32, "ce loss", factor=5)
    check(logp.get().reshape(T), lp_ref, F32, "token log-probs", factor=5)
    gup = vecw(torch.tensor([2.5]), F32, dev).arm()
    dzw = out(T, V, dtype, dev)
    rlse.arm()
    lsc.arm()
    k.cross_entropy_bwd(zw.view, lw.flat, rlse.flat, dzw.view, T, V, zw.ld, -100, ls, gup.flat, lsc.flat)
    for w, name in ((rlse, "row lse"), (lsc, "loss sum / count"), (gup, "upstream gradient")):
        w.assert_guard_intact("ce bwd: " + name)
    settle(dzw, zr.grad, dtype, f"ce bwd V={V} ls={ls}")


# ----------------------------------------------------------------------------------------------------------------
# Tier 2: the flat kernels at ragged element counts - one table of (name, call + reference, dtypes, sizes)
# ----------------------------------------------------------------------------------------------------------------
RAGGED = [1, 7, 8 * 33 + 3, 256 * 5 + 1]
OPTIM_N = [1, 257, 4099]
OTHER = {F32: BF16, BF16: F32}


def flat(x, dtype, dev):
    """a vector between 64 guard elements on either side (16-byte aligned for every dtype)"""
    x = x.reshape(1, -1)
    return Window(1, x.shape[1], x.shape[1] + 64, dtype, dev, lead=0, trail=0, left=64).put(x)


def flat_out(n, dtype, dev):
    return Window(1, n, n + 64, dtype, dev, lead=0, trail=0, left=64).arm()


def exact(w, ref, what):
    w.assert_guard_intact(what)
    assert torch.equal(w.get().cpu().reshape(ref.shape), ref), what + ": not the exact copy"


def _t_unary(k, dev, dtype, n):
    x = rnd(n, dtype=dtype, seed=1) * 2
    xw = flat(x, dtype, dev)
    for op, f in ((ops.UN_COPY, lambda t: t), (ops.UN_SILU, F.silu), (ops.UN_GELU, F.gelu), (ops.UN_AFFINE, lambda t: 0.5 * t + 0.25)):
        for ydt in ((dtype, OTHER[dtype]) if op == ops.UN_COPY else (dtype,)):
            yw = flat_out(n, ydt, dev)
            k.unary(op, xw.flat, yw.flat, n, 0.5, 0.25)
            settle(yw, f(x.double()), coarser(dtype, ydt), f"unary op={op} n={n} {dtype}->{ydt}")


def _t_unary_bwd(k, dev, dtype, n):
    x, g = rnd(n, dtype=dtype, seed=1) * 2, rnd(n, dtype=dtype, seed=2)
    xw, gw = flat(x, dtype, dev), flat(g, dtype, dev)
    for op, f in ((ops.UN_SILU, F.silu), (ops.UN_GELU, F.gelu)):
        xr = x.double().requires_grad_(True)
        f(xr).backward(g.double())
        dxw = flat_out(n, dtype, dev)
        k.unary_bwd(op, gw.flat, xw.flat, dxw.flat, n)
        settle(dxw, xr.grad, dtype, f"unary_bwd op={op} n={n}")


def _t_axpby(k, dev, dtype, n):
    x, y = rnd(n, dtype=dtype, seed=1), rnd(n, dtype=OTHER[dtype], seed=2)
    xw, yw = flat(x, dtype, dev), flat(y, OTHER[dtype], dev)
    for odt in DTYPES:
        ow = flat_out(n, odt, dev)
        k.axpby(0.5, xw.flat, -2.0, yw.flat, ow.flat, n)
        settle(ow, 0.5 * x.double() - 2.0 * y.double(), BF16, f"axpby n={n} out={odt}")
    ow = flat_out(n, dtype, dev)
    k.axpby(0.5, xw.flat, 0.0, None, ow.flat, n)
    settle(ow, 0.5 * x.double(), dtype, f"axpby (y = NULL) n={n}")


def _t_geglu(k, dev, dtype, n):
    for M, D in ((n, 3), (max(1, n // 16), 16)):  # odd D: per-element; D = 16: whole 16-byte vectors
        x, g = rnd(M, 2 * D, dtype=dtype, seed=1) * 2, rnd(M, D, dtype=dtype, seed=2)
        xr = x.double().requires_grad_(True)
        ref = xr[:, :D] * F.gelu(xr[:, D:])
        ref.backward(g.double())
        xw, gw = win(x, dtype, dev, 0), win(g, dtype, dev, 0)
        yw, dxw = out(M, D, dtype, dev, 0), out(M, 2 * D, dtype, dev, 0)
        k.geglu_fwd(xw.view, yw.view, M, D)
        k.geglu_bwd(gw.view, xw.view, dxw.view, M, D)
        settle(yw, ref.detach(), dtype, f"geglu M={M} D={D}")
        settle(dxw, xr.grad, dtype, f"geglu bwd M={M} D={D}")


def _t_geglu_il(k, dev, dtype, n):
    M, D = min(n, 300), 16 if n % 2 else 48
    x, g = rnd(M, 2 * D, dtype=dtype, seed=1) * 2, rnd(M, D, dtype=dtype, seed=2)
    xr = x.double().reshape(M, D // 16, 2, 16).requires_grad_(True)
    ref = (xr[:, :, 0] * F.gelu(xr[:, :, 1])).reshape(M, D)
    ref.backward(g.double())
    xw, gw = win(x, dtype, dev, 0), win(g, dtype, dev, 0)
    yw, dxw = out(M, D, dtype, dev, 0), out(M, 2 * D, dtype, dev, 0)
    k.geglu_il_fwd(xw.view, yw.view, M, D)
    k.geglu_il_bwd(gw.view, xw.view, dxw.view, M, D)
    settle(yw, ref.detach(), dtype, f"geglu_il M={M} D={D}")
    settle(dxw, xr.grad.reshape(M, 2 * D), dtype, f"geglu_il bwd M={M} D={D}")


def _t_add_rowvec(k, dev, dtype, n):
    for cols in (7, 8):
        rows = max(1, n // cols)
        x, v = rnd(rows, cols, dtype=dtype, seed=1), rnd(cols, dtype=dtype, seed=2)
        xw, vw, ow = win(x, dtype, dev, 0), flat(v, dtype, dev), out(rows, cols, dtype, dev, 0)
        k.add_rowvec(xw.view, vw.flat, ow.view, rows, cols)
        settle(ow, x.double() + v.double(), dtype, f"add_rowvec {rows}x{cols}")


def _t_copy2d(k, dev, dtype, n):
    rows, cols = 5, n
    x = rnd(rows, cols, dtype=dtype, seed=1)
    for (ps, ls), (pd, ld_) in (((8, 8), (16, 8)), ((3, 1), (5, 1))):  # 16-byte aligned rows / odd strides one element off alignment
        sw = win(x, dtype, dev, ps, ls)
        for odt in DTYPES:
            dw = out(rows, cols, odt, dev, pd, ld_)
            k.copy2d(sw.view, sw.ld, dw.view, dw.ld, rows, cols)
            dw.assert_written(f"copy2d {rows}x{cols}")
            exact(dw, x.to(odt), f"copy2d {rows}x{cols} {dtype}->{odt} ld {sw.ld}->{dw.ld}")


def _t_copy2d_pair(k, dev, dtype, n):
    rows, c0, c1 = 3, (n + 7) // 8 * 8, 8  # whole 16-byte vectors (include/comat_hip.h)
    a, b = rnd(rows, c0, dtype=dtype, seed=1), rnd(rows, c1, dtype=dtype, seed=2)
    aw, bw = win(a, dtype, dev, 8), win(b, dtype, dev, 16)
    # concat: both land in column slices of one [rows, c0 + c1 + 8] window
    cw = out(rows, c0 + c1, dtype, dev, 8)
    items = [(aw.view, aw.ld, cw.view[:, :c0], cw.ld, c0), (bw.view, bw.ld, cw.view[:, c0:], cw.ld, c1)]
    assert k.copy2d_pair_ok(items)
    k.copy2d_pair(items, rows)
    cw.assert_written("copy2d_pair")
    exact(cw, torch.cat([a, b], 1).to(dtype), f"copy2d_pair (concat) {rows}x({c0}+{c1})")
    # split: the backward direction
    a2, b2 = out(rows, c0, dtype, dev, 16), out(rows, c1, dtype, dev, 8)
    cw.arm()
    k.copy2d_pair([(cw.view[:, :c0], cw.ld, a2.view, a2.ld, c0), (cw.view[:, c0:], cw.ld, b2.view, b2.ld, c1)], rows)
    cw.assert_guard_intact("copy2d_pair source")
    exact(a2, a.to(dtype), "copy2d_pair (split) first half")
    exact(b2, b.to(dtype), "copy2d_pair (split) second half")


def _t_sumpool(k, dev, dtype, n):
    B_, H, C = 2, 1, 3  # odd channel count
    W = max(1, n // (B_ * C))
    u = rnd(B_, 2 * H, 2 * W, C, dtype=dtype, seed=1)
    uw, yw = win(u.reshape(-1, C), dtype, dev, 0), out(B_ * H * W, C, dtype, dev, 0)
    k.sumpool2x2(uw.view, yw.view, B_, H, W, C)
    settle(yw, u.double().reshape(B_, H, 2, W, 2, C).sum(dim=(2, 4)), dtype, f"sumpool W={W}")


def _t_permute(k, dev, dtype, n):
    B_, C, H = 2, 3, 1
    W = max(1, n // (B_ * C))
    img = rnd(B_, C, H, W, dtype=dtype, seed=1)
    iw = flat(img, dtype, dev)
    for odt in DTYPES:
        tw = flat_out(img.numel(), odt, dev)
        k.permute_nchw_nhwc(iw.flat, tw.flat, B_, C, H, W, True)
        tw.assert_written("to nhwc")
        exact(tw, img.permute(0, 2, 3, 1).reshape(1, -1).to(odt), f"nchw -> nhwc W={W} {dtype}->{odt}")
    bw = flat_out(img.numel(), dtype, dev)
    tw.arm()
    k.permute_nchw_nhwc(tw.flat, bw.flat, B_, C, H, W, False)
    bw.assert_written("to nchw")
    exact(bw, img.reshape(1, -1).to(odt).to(dtype), f"nhwc -> nchw W={W}")


def _t_cfg_ddpm(k, dev, dtype, n):
    x, z, g = rnd(n, seed=1), rnd(n, seed=2), rnd(n, seed=4)
    e = rnd(2 * n, dtype=dtype, seed=3)
    s, cx, ce, sg = 7.5, 0.93, -0.21, 0.05
    xr, er = x.double().requires_grad_(True), e.double().requires_grad_(True)
    ref = cx * xr + ce * (er[:n] + s * (er[n:] - er[:n])) + sg * z.double()
    ref.backward(g.double())
    xw, zw, gw, ew = flat(x, F32, dev), flat(z, F32, dev), flat(g, F32, dev), flat(e, dtype, dev)
    ow, dxw, dew = flat_out(n, F32, dev), flat_out(n, F32, dev), flat_out(2 * n, dtype, dev)
    k.cfg_ddpm_fwd(xw.flat, ew.flat, zw.flat, ow.flat, n, s, cx, ce, sg)
    k.cfg_ddpm_bwd(gw.flat, dxw.flat, dew.flat, n, s, cx, ce)
    settle(ow, ref.detach(), F32, f"ddpm fwd n={n}")
    settle(dxw, xr.grad, F32, f"ddpm dx n={n}")
    settle(dew, er.grad, dtype, f"ddpm deps n={n}")


def _t_cfg_rescale(k, dev, dtype, n):
    batch, P = 2, max(4, n // 8 * 4)  # per_sample % 4 == 0 (include/comat_hip.h)
    n = batch * P
    x, z, g = rnd(n, seed=1), rnd(n, seed=2), rnd(n, seed=4)
    e = rnd(2 * n, dtype=dtype, seed=3)
    s, cx, ce, sg, phi = 7.5, 0.93, -0.21, 0.05, 0.7
    xr, er = x.double().requires_grad_(True), e.double().requires_grad_(True)
    eu, ec = er[:n].reshape(batch, P), er[n:].reshape(batch, P)
    eg = eu + s * (ec - eu)
    kk = phi * (ec.std(1, keepdim=True) / eg.std(1, keepdim=True)) + (1 - phi)
    ref = cx * xr + ce * (kk * eg).reshape(-1) + sg * z.double()
    ref.backward(g.double())
    xw, zw, gw, ew = flat(x, F32, dev), flat(z, F32, dev), flat(g, F32, dev), flat(e, dtype, dev)
    ow, dxw, dew, stw = flat_out(n, F32, dev), flat_out(n, F32, dev), flat_out(2 * n, dtype, dev), flat_out(4 * batch, F32, dev)
    k.cfg_rescale_ddpm_fwd(xw.flat, ew.flat, zw.flat, ow.flat, n, s, cx, ce, sg, phi, batch, P, stw.flat)
    stw.assert_guard_intact("rescale stats")
    stw.assert_written("rescale stats")
    stw.arm()
    k.cfg_rescale_ddpm_bwd(gw.flat, ew.flat, stw.flat, dxw.flat, dew.flat, n, s, cx, ce, phi, batch, P)
    stw.assert_guard_intact("rescale stats (read by bwd)")
    settle(ow, ref.detach(), F32, f"rescale fwd P={P}")
    settle(dxw, xr.grad, F32, f"rescale dx P={P}")
    settle(dew, er.grad, dtype, f"rescale deps2 P={P}")


def _t_fp8_quantize(k, dev, dtype, n):
    x = (rnd(n, seed=n) * 3).to(dtype)
    xw = flat(x, dtype, dev)
    q_ref, s_ref = OF.quantize(x)
    yw, sw = flat_out(n, torch.uint8, dev), flat_out(1, F32, dev)
    k.fp8_quantize(xw.flat, out=yw.flat, scale=sw.flat)
    sw.assert_guard_intact("fp8_quantize scale")
    assert float(sw.get().cpu()) == float(s_ref)
    exact(yw, q_ref.reshape(1, -1), f"fp8_quantize n={n}")
    scale = flat((s_ref * 0.8).reshape(1), F32, dev).arm()
    amax = flat_out(1, torch.int32, dev)
    amax.view.zero_()
    amax.arm()
    y2 = flat_out(n, torch.uint8, dev)
    k.fp8_quantize_scaled(xw.flat, scale.flat, amax.flat, out=y2.flat)
    scale.assert_guard_intact("fp8_quantize_scaled scale")
    amax.assert_guard_intact("fp8_quantize_scaled abs-max")
    exact(y2, OF.quantize_with_scale(x, scale.get().cpu()[0, 0]).reshape(1, -1), f"fp8_quantize_scaled n={n}")
    assert float(amax.get().cpu().view(F32)) == float(x.float().abs().max())


def _t_transpose_cast_tiles(k, dev, dtype, n):
    rows, cols = max(1, n // 7), 7 if n > 1 else 1
    src = rnd(rows * cols + 5, seed=1)
    sw, dw = flat(src, F32, dev), flat_out(rows * cols, dtype, dev)
    tiles = [(3, 0, rows, cols, r0, c0) for r0 in range(0, rows, 32) for c0 in range(0, cols, 32)]
    k.transpose_cast_tiles(sw.flat, dw.flat, torch.tensor(tiles, dtype=torch.int64).to(dev))
    dw.assert_written("transpose_cast_tiles")
    exact(dw, src[3:3 + rows * cols].view(rows, cols).t().contiguous().to(dtype).reshape(1, -1), f"transpose_cast_tiles {rows}x{cols}")


@pytest.mark.gpu
def test_lora_merge_windows(hip):
    """comat_lora_merge on (1, 200, 136, 16): W, U (ldu = r + 8), D^T (lddt = r + 16) in NaN halos, Wm and WmT between guard rows;
    ragged 64 x 64 tiles on both axes (the simulator has no such entry point: the real kernel only)"""
    k, dev, dtype = ops.kernels(), hip, BF16
    N, K, r, sc = 200, 136, 16, 0.75
    W, U, D = rnd(N, K, dtype=dtype, seed=1, scale=K ** -0.5), rnd(N, r, dtype=dtype, seed=2, scale=0.05), rnd(r, K, dtype=dtype, seed=3, scale=K ** -0.5)
    Ww, Uw, Dtw = win(W, dtype, dev, 0), win(U, dtype, dev, 8), win(D.t(), dtype, dev, 16)
    Wm, WmT = out(N, K, dtype, dev, 0), out(K, N, dtype, dev, 0)
    assert k.lora_merge_ok(Ww.view, Uw.view, Dtw.view, r, Uw.ld, Dtw.ld)
    probs = torch.tensor([[Ww.view.data_ptr(), Uw.view.data_ptr(), Dtw.view.data_ptr(), Wm.view.data_ptr(), WmT.view.data_ptr(), N, K, r,
                           Uw.ld, Dtw.ld]], dtype=torch.int64).to(dev)
    tiles = torch.tensor([(0, n0, k0) for n0 in range(0, N, 64) for k0 in range(0, K, 64)], dtype=torch.int32).to(dev)
    k.lora_merge(probs, tiles, sc)
    for w, name in ((Wm, "Wm"), (WmT, "WmT")):
        w.assert_guard_intact("lora_merge " + name)
        w.assert_written("lora_merge " + name)
    ref = (W.double() + sc * (U.double() @ D.double())).float().to(dtype).float()
    diff = (Wm.get().cpu().float() - ref).abs()  # as test_lora_merge_grouped_kernel: the last bf16 bit on a few elements
    assert diff.max() <= 2.0 ** -7 * ref.abs().max() and (diff > 0).float().mean() < 2e-2
    assert torch.equal(WmT.get(), Wm.get().t()), "transposed merged weight is not the forward copy's transpose"


def _t_resample(k, dev, dtype, n):
    B_, C, Hf, crop, size = 2, 3, 20, (1, 2, 17, 17), (12, 12)
    img = rnd(B_, C, Hf, Hf, dtype=dtype, seed=1)
    mean, std = torch.tensor([0.48, 0.45, 0.40]), torch.tensor([0.27, 0.26, 0.28])
    ir = img.double().requires_grad_(True)
    y0, x0, ch, cw = crop
    ref = F.interpolate(ir[:, :, y0:y0 + ch, x0:x0 + cw], size=size, mode="bicubic", antialias=True, align_corners=False)
    ref = (ref - mean.double()[None, :, None, None]) / std.double()[None, :, None, None]
    g = rnd(B_, C, *size, dtype=dtype, seed=2)
    ref.backward(g.double())
    fwd, bwd = resize_tables(Hf, Hf, crop, size, "bicubic")
    tab = ops.ResampleTables(fwd, bwd, Hf, Hf, size[0], size[1], dev)
    tok = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    iw, gw = win(tok(img), dtype, dev, 0), win(tok(g), dtype, dev, 0)
    scw, shw = flat(1 / std, F32, dev), flat(-mean / std, F32, dev)
    ow, dw = out(B_ * size[0] * size[1], C, dtype, dev, 0), out(B_ * Hf * Hf, C, dtype, dev, 0)
    t = tab.fwd
    k.resample2d(iw.view, ow.view, B_, Hf, Hf, size[0], size[1], C, t["ystart"], t["ywt"], t["xstart"], t["xwt"], t["KT"], scw.flat, shw.flat)
    settle(ow, tok(ref.detach()), dtype, "resample fwd")
    t = tab.bwd
    k.resample2d(gw.view, dw.view, B_, size[0], size[1], Hf, Hf, C, t["ystart"], t["ywt"], t["xstart"], t["xwt"], t["KT"], scw.flat, None)
    settle(dw, tok(ir.grad), dtype, "resample bwd")


def _t_patchify(k, dev, dtype, n):
    B_, H, W, C, P = 2, 8, 12, 3, 4
    pr = rnd(B_, H, W, C, dtype=dtype, seed=3)
    refp = pr.reshape(B_, H // P, P, W // P, P, C).permute(0, 1, 3, 2, 4, 5).reshape(B_ * (H // P) * (W // P), P * P * C)
    iw, pw = win(pr.reshape(-1, C), dtype, dev, 0), out(refp.shape[0], refp.shape[1], dtype, dev, 0)
    k.patchify(iw.view, pw.view, B_, H, W, C, P, False)
    pw.assert_written("patchify")
    exact(pw, refp.to(dtype), "patchify")
    bw = out(B_ * H * W, C, dtype, dev, 0)
    pw.arm()
    k.patchify(bw.view, pw.view, B_, H, W, C, P, True)
    pw.assert_guard_intact("patchify (inverse) source")
    bw.assert_written("patchify inverse")
    exact(bw, pr.reshape(-1, C).to(dtype), "patchify inverse")


def _t_embedding(k, dev, dtype, n):
    vocab = 9
    for dim in (7, 16):
        ids = torch.randint(0, vocab, (n,), generator=torch.Generator().manual_seed(n))
        ids[0], ids[-1] = vocab - 1, 0
        if n > 1:
            ids[1] = 0
        table = rnd(vocab, dim, dtype=dtype, seed=5)
        tw, idw, ow = win(table, dtype, dev, 0), flat(ids, torch.int64, dev), out(n, dim, dtype, dev, 0)
        k.embedding(idw.flat, tw.view, ow.view, n, dim, vocab)
        ow.assert_written("embedding")
        exact(ow, table[ids].to(dtype), f"embedding n={n} dim={dim}")


def _t_disc_head(k, dev, dtype, n):
    P = n
    pps = (P + 1) // 2
    bs = (P + pps - 1) // pps
    x, w, b = rnd(P, 4, dtype=dtype, seed=1), rnd(4, seed=2), rnd(1, seed=3)
    target = torch.tensor([0.0, 1.0])[:bs]
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    ref = F.binary_cross_entropy_with_logits(xr @ wr + br, target.double().repeat_interleave(pps)[:P])
    (1.7 * ref).backward()
    xw, ww, bw, tw = win(x, dtype, dev, 0), flat(w, F32, dev), flat(b, F32, dev), flat(target, F32, dev)
    lw = flat_out(1, F32, dev)
    k.disc_head_fwd(xw.view, ww.flat, bw.flat, tw.flat, lw.flat, P, pps)
    settle(lw, ref.detach().reshape(1, 1), F32, f"bce P={P}", factor=5)
    gup = flat(torch.tensor([1.7]), F32, dev)
    dxw = out(P, 4, dtype, dev, 0)
    dwb = flat(torch.zeros(5), F32, dev).arm()
    k.disc_head_bwd(xw.view, ww.flat, bw.flat, tw.flat, gup.flat, dxw.view, dwb.flat, P, pps)
    settle(dxw, xr.grad, dtype, f"bce dx P={P}")
    dwb.assert_guard_intact("bce dw / db")
    check(dwb.get()[0, :4], wr.grad, F32, "bce dw", factor=20)
    check(dwb.get()[0, 4:], br.grad, F32, "bce db", factor=20)


def _t_attnmap(k, dev, dtype, n):
    h, npix, L = 2, 130, 77
    a = torch.softmax(rnd(h, npix, L, seed=1), -1).to(dtype).float()
    mask = (rnd(2, npix, seed=2) > 0).float()
    tok_idx = torch.tensor([2, 0, 6, 76, 3], dtype=torch.int32)
    tok_obj = torch.tensor([0, 0, 1, 1, 1], dtype=torch.int32)
    nt = 5
    gn, gd, ga = rnd(h, nt, seed=3), rnd(h, nt, seed=4), rnd(nt, npix, seed=5)
    ar = a.double().requires_grad_(True)
    sel = ar[:, :, tok_idx.long()]
    num_r, den_r, avg_r = torch.einsum("hpt,tp->ht", sel, mask.double()[tok_obj.long()]), sel.sum(1), sel.mean(0).t()
    ((num_r * gn.double()).sum() + (den_r * gd.double()).sum() + (avg_r * ga.double()).sum()).backward()
    aw, mw = flat(a, dtype, dev), win(mask, F32, dev, 0)
    iw, ow_ = flat(tok_idx, torch.int32, dev), flat(tok_obj, torch.int32, dev)
    numw, denw, avgw = (Window(r, c, c, F32, dev).put(torch.zeros(r, c)).arm() for r, c in ((h, nt), (h, nt), (nt, npix)))
    k.attnmap_gather_fwd(aw.flat.view(h, npix, L), mw.view, iw.flat, ow_.flat, numw.view, denw.view, avgw.view, h, npix, L, nt)
    settle(numw, num_r.detach(), F32, "num", factor=5)
    settle(denw, den_r.detach(), F32, "den", factor=5)
    settle(avgw, avg_r.detach(), F32, "avg", factor=5)
    gnw, gdw, gaw = win(gn, F32, dev, 0), win(gd, F32, dev, 0), win(ga, F32, dev, 0)
    dw = flat_out(h * npix * L, dtype, dev)
    k.attnmap_gather_bwd(gnw.view, gdw.view, gaw.view, mw.view, iw.flat, ow_.flat, dw.flat.view(h, npix, L), h, npix, L, nt)
    settle(dw, ar.grad.reshape(1, -1), dtype, "damap")


def _t_sumsq_adamw(k, dev, dtype, n):
    p0, g0 = rnd(n, seed=1), rnd(n, seed=2) * 3
    pr = p0.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pr], lr=5e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    pw, mw, vw = (flat(t, F32, dev).arm() for t in (p0, torch.zeros(n), torch.zeros(n)))
    for step in (1, 2):
        g = g0 * step
        pr.grad = g.clone()
        torch.nn.utils.clip_grad_norm_([pr], 0.1)
        opt.step()
        gw = flat(g, F32, dev).arm()
        nsq = flat(torch.zeros(1), F32, dev).arm()
        k.sumsq(gw.flat, n, nsq.flat)
        settle(nsq, (g.double() ** 2).sum().reshape(1, 1), F32, f"sumsq n={n}", factor=5)
        k.adamw(pw.flat, gw.flat, mw.flat, vw.flat, n, 5e-3, 0.9, 0.999, 1e-8, 1e-2, step, nsq.flat, 0.1)
        gw.assert_guard_intact("adamw gradient")
    for w, name in ((mw, "m"), (vw, "v")):
        w.assert_guard_intact("adamw " + name)
        w.assert_written("adamw " + name)
    settle(pw, pr.detach().reshape(1, -1), F32, f"adamw n={n}", factor=0.5)


def _t_grad_norm_scale(k, dev, dtype, n):
    g = (rnd(n, seed=n % 1000) * 3e-4).to(dtype)
    want = g.double().norm()
    gw = flat(g, dtype, dev).arm()
    norm, ow = flat_out(1, F32, dev), flat_out(n, dtype, dev)
    k.grad_norm_scale(gw.flat, ow.flat, n, norm.flat, 1e4)
    gw.assert_guard_intact("grad_norm_scale input")
    norm.assert_guard_intact("grad_norm_scale norm")
    assert abs(float(norm.get().cpu()) - float(want)) / float(want) < 1e-5  # the bound of test_grad_norm_scale_kernel
    settle(ow, (g.double() * (1e4 / want)).reshape(1, -1), dtype, f"normalised gradient n={n}")


TIER2 = [  # name, call + reference, dtypes, sizes
    ("unary", _t_unary, DTYPES, RAGGED), ("unary_bwd", _t_unary_bwd, DTYPES, RAGGED),
    ("axpby", _t_axpby, DTYPES, RAGGED), ("geglu", _t_geglu, DTYPES, RAGGED),
    ("geglu_il", _t_geglu_il, DTYPES, RAGGED), ("add_rowvec", _t_add_rowvec, DTYPES, RAGGED),
    ("copy2d", _t_copy2d, DTYPES, RAGGED), ("copy2d_pair", _t_copy2d_pair, DTYPES, RAGGED),
    ("sumpool2x2", _t_sumpool, DTYPES, RAGGED), ("permute_nchw_nhwc", _t_permute, DTYPES, RAGGED),
    ("cfg_ddpm", _t_cfg_ddpm, DTYPES, RAGGED), ("cfg_rescale_ddpm", _t_cfg_rescale, DTYPES, RAGGED),
    ("fp8_quantize", _t_fp8_quantize, DTYPES, RAGGED), ("transpose_cast_tiles", _t_transpose_cast_tiles, DTYPES, RAGGED),
    ("resample2d", _t_resample, DTYPES, [0]),
    ("patchify", _t_patchify, DTYPES, [0]), ("embedding", _t_embedding, DTYPES, RAGGED),
    ("disc_head", _t_disc_head, DTYPES, [1, 257]), ("attnmap_gather", _t_attnmap, DTYPES, [0]),
    ("sumsq_adamw", _t_sumsq_adamw, [F32], OPTIM_N), ("grad_norm_scale", _t_grad_norm_scale, DTYPES, OPTIM_N),
]
TIER2_CASES = [pytest.param(fn, dt, n, id=f"{name}-{str(dt).split('.')[-1]}-{n}") for name, fn, dts, ns in TIER2 for dt in dts for n in ns]


@pytest.mark.parametrize("fn,dtype,n", TIER2_CASES)
def test_flat_kernels_ragged(dev, fn, dtype, n):
    """every flat / elementwise / image / loss / optimizer entry point at a ragged element count (n = 0: the entry's own
    shape), inputs in NaN halos, outputs in guards"""
    fn(ops.kernels(), dev, dtype, n)
