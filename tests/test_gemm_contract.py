"""The contract and the routing of comat_gemm / comat_gemm_segments / comat_conv2d, through ctypes.

libcomat_hip.so loads without a GPU and validates before it launches anything, so both tables run anywhere:
  * INVALID: calls that violate include/comat_hip.h return their error code with a message, whatever kernel family the shape would
    have gone to;
  * ROUTING: valid calls reach the launch of the family the router chose (comat_last_gemm_kernel); without a device the launch
    itself fails cleanly (COMAT_ELAUNCH), with one it must succeed.
Every pointer handed to the library points to an allocation as large as the call describes (device memory when there is a device,
host memory otherwise): a call that unexpectedly passes validation launches something harmless.

The expected families of ROUTING and the values of tests/golden/gemm_workspace_bytes.json were recorded by running these tables
against the library built from the commit BEFORE the host-side refactor of the GEMM routing (same kernels, same plans): they pin
the routing and the workspace sizes to what that library did."""
import ctypes as C
import json
import os

import pytest
import torch

from comat_amd import _hip

F32, BF16, FP8 = _hip.F32, _hip.BF16, _hip.FP8
EINVAL, ELAUNCH, EUNSUPPORTED = -1, -2, -3
ESIZE = {F32: 4, BF16: 2, FP8: 1}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_workspace_bytes.json")


class Alloc:
    """`nbytes` of zeroed memory, resolved to a pointer when the call is built"""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)


class Call:
    """one library call: the struct(s), and the tensors that back its pointers (kept alive until the call has run)"""

    def __init__(self, device):
        self.device = device
        self.keep = []

    def ptr(self, v):
        if not isinstance(v, Alloc):
            return v
        t = torch.zeros(max(v.nbytes, 16), dtype=torch.uint8, device=self.device)
        assert t.data_ptr() % 16 == 0
        self.keep.append(t)
        return t.data_ptr()

    def fill(self, struct, fields):
        for k, v in fields.items():
            setattr(struct, k, self.ptr(v))
        return struct


def gemm_fields(lib, m, n, k, dt=BF16, out=BF16, transA=0, transB=0, ws=False, **over):
    """a valid plain product m x n x k with buffers of its own; `over` replaces / adds fields afterwards"""
    es, eo = ESIZE[dt], ESIZE[out]
    f = dict(A=Alloc(m * k * es), B=Alloc(n * k * es), C=Alloc(m * n * eo), M=m, N=n, K=k,
             lda=m if transA else k, ldb=n if transB else k, ldc=n, batch1=1, batch2=1, alpha=1.0,
             transA=transA, transB=transB, in_dtype=dt, out_dtype=out)
    if ws:
        nb = lib.comat_gemm_workspace_bytes(m, n, k, 1, dt) + m * n * 2  # + the scratch of the two-launch second epilogues
        f.update(ws=Alloc(nb), ws_bytes=nb)
    f.update(over)
    return f


def segments(call, M, N, ks, nseg=None):
    n = nseg or len(ks)
    arr = (_hip.GemmSegment * n)()
    for i in range(n):
        k = ks[i % len(ks)]
        call.fill(arr[i], dict(A=Alloc(M * k * 2), B=Alloc(N * k * 2), K=k, lda=k, ldb=k))
    return arr, n


def conv_fields(Cin, Cout=32, B=2, H=8, W=8, **over):
    f = dict(X=Alloc(B * H * W * Cin * 2), W=Alloc(Cout * 9 * Cin * 2), Y=Alloc(B * H * W * Cout * 2), B=B, Hin=H, Win=W, Cin=Cin,
             Hout=H, Wout=W, Cout=Cout, KH=3, KW=3, stride=1, pad=1, mode=0, ups=1, alpha=1.0, in_dtype=BF16, out_dtype=BF16)
    f.update(over)
    return f


def run(lib, device, kind, build, options=()):
    """-> (rc, message, family).  kind: 'gemm' | 'segments' | 'conv'; build(lib) -> fields (segments: (fields, M, N, ks, nseg))"""
    call = Call(device)
    for name, value in options:
        assert lib.comat_set_option(name.encode(), value) == 0
    try:
        if kind == "gemm":
            rc = lib.comat_gemm(C.byref(call.fill(_hip.GemmParams(), build(lib))), None)
        elif kind == "conv":
            rc = lib.comat_conv2d(C.byref(call.fill(_hip.ConvParams(), build(lib))), None)
        else:
            fields, M, N, ks, nseg = build(lib)
            arr, n = segments(call, M, N, ks, nseg)
            rc = lib.comat_gemm_segments(C.byref(call.fill(_hip.GemmParams(), fields)), arr, n, None)
        if device != "cpu":
            torch.cuda.synchronize()
    finally:
        for name, _ in options:
            lib.comat_set_option(name.encode(), 1)  # (the options used here default to 1)
    return rc, lib.comat_last_error().decode(), lib.comat_last_gemm_kernel()


def seg_fields(M, N, **over):
    f = dict(C=Alloc(M * N * 2), M=M, N=N, ldc=N, batch1=1, batch2=1, alpha=1.0, in_dtype=BF16, out_dtype=BF16)
    f.update(over)
    return f


def ktail(M, N):
    return dict(A2k=Alloc(M * 16 * 2), B2k=Alloc(N * 16 * 2), K2=16, lda2k=16, ldb2k=16)


def geglu(M, N, **over):
    f = dict(epi2=2, C2=Alloc(M * N), ldc2=N // 2)
    f.update(over)
    return f


# id -> (kind, build, options, expected rc, substring of comat_last_error())
INVALID = {
    "null_operand": ("gemm", lambda lib: gemm_fields(lib, 64, 64, 64, A=None), (), EINVAL, "null operand"),
    "non_positive_shape": ("gemm", lambda lib: gemm_fields(lib, 64, 64, 64, M=0), (), EINVAL, "bad shape"),
    "bad_dtype": ("gemm", lambda lib: gemm_fields(lib, 64, 64, 64, in_dtype=7), (), EINVAL, "bad dtype"),
    "too_many_batches": ("gemm", lambda lib: gemm_fields(lib, 64, 64, 64, batch1=256, batch2=257), (), EINVAL, "bad batch"),
    "bias2_without_rows": ("gemm", lambda lib: gemm_fields(lib, 64, 64, 64, bias2=Alloc(64 * 64 * 4), rows_per_bias2=0), (), EINVAL,
                           "bias2 needs rows_per_bias2"),
    "lda_below_k": ("gemm", lambda lib: gemm_fields(lib, 64, 64, 64, lda=63), (), EINVAL, "leading dimension too small"),
    "epi2_5": ("gemm", lambda lib: gemm_fields(lib, 64, 64, 64, epi2=5, C2=Alloc(64 * 64 * 2), ldc2=64), (), EINVAL,
               "bad second epilogue"),
    "tail_columns_n2_not_below_n": ("gemm", lambda lib: gemm_fields(lib, 64, 64, 64, epi2=4, n2=64, B2=Alloc(64 * 64 * 2),
                                                                    C2=Alloc(64 * 64 * 2), ldc2=64), (), EINVAL, "tail columns"),
    "fp8_k_not_multiple_of_64": ("gemm", lambda lib: gemm_fields(lib, 64, 64, 96, dt=FP8, scale_a=Alloc(4), scale_b=Alloc(4)), (), EINVAL,
                                 "fp8 operands need"),
    "q8_without_q_scale": ("gemm", lambda lib: gemm_fields(lib, 64, 64, 64, ws=True, q8=Alloc(64 * 32), q_amax=Alloc(4), ldq8=32,
                                                           **geglu(64, 64)), (), EINVAL, "q8 needs q_scale"),
    "nine_segments": ("segments", lambda lib: (seg_fields(64, 64), 64, 64, [64], 9), (), EINVAL, "segments supported"),
    "conv_mode_2": ("conv", lambda lib: conv_fields(32, mode=2), (), EINVAL, "mode must be 0 or 1"),
    "bf16_ktail_pipelined_shape": ("gemm", lambda lib: gemm_fields(lib, 2048, 768, 640, **ktail(2048, 768)), (), EINVAL, "bf16 k-tail"),
    # the two below were accepted before the validator ran ahead of the routing: the lean kernel took the first and dropped the k-tail;
    # the second launched the plain product before it found the unsupported leading dimension
    "bf16_ktail_lean_shape": ("gemm", lambda lib: gemm_fields(lib, 16, 768, 768, **ktail(16, 768)), (), EINVAL, "bf16 k-tail"),
    "geglu_pre_activations_strided_c": ("gemm", lambda lib: gemm_fields(lib, 64, 64, 64, ws=True, C=Alloc(64 * 72 * 2), ldc=72,
                                                                        **geglu(64, 64, epi2=1)),
                                        (("gemm2", 0),), EUNSUPPORTED, "epi2 == 1 needs ldc == N"),
}


def _tt(lib):
    return gemm_fields(lib, 64, 64, 256, transA=1, transB=1, ws=True)


# id -> (kind, build, options, family recorded from the library before the refactor)
ROUTING = {
    "bf16_2048x768x640": ("gemm", lambda lib: gemm_fields(lib, 2048, 768, 640, ws=True), (), 1),
    "bf16_512x1408x1280": ("gemm", lambda lib: gemm_fields(lib, 512, 1408, 1280, ws=True), (), 1),
    "bf16_16x768x768": ("gemm", lambda lib: gemm_fields(lib, 16, 768, 768, ws=True), (), 5),
    "bf16_8x320x1280": ("gemm", lambda lib: gemm_fields(lib, 8, 320, 1280, ws=True), (), 0),
    "bf16_100x70x33": ("gemm", lambda lib: gemm_fields(lib, 100, 70, 33, ws=True), (), 0),
    "f32_64x64x64": ("gemm", lambda lib: gemm_fields(lib, 64, 64, 64, dt=F32, out=F32, ws=True), (), 0),
    "fp8_64x64x64_scaled": ("gemm", lambda lib: gemm_fields(lib, 64, 64, 64, dt=FP8, ws=True, scale_a=Alloc(4), scale_b=Alloc(4)), (),
                            3),
    "k_major_64x64x256": ("gemm", _tt, (), 2),
    "two_segments_m64": ("segments", lambda lib: (seg_fields(64, 64), 64, 64, [64, 64], None), (), 1),
    "two_segments_m16": ("segments", lambda lib: (seg_fields(16, 64), 16, 64, [64, 64], None), (), 5),
    "conv3x3_cin32": ("conv", lambda lib: conv_fields(32), (), 1),
    "conv3x3_cin4": ("conv", lambda lib: conv_fields(4), (), 0),
    "bf16_2048x768x640_gemm2_off": ("gemm", lambda lib: gemm_fields(lib, 2048, 768, 640, ws=True), (("gemm2", 0),), 0),
}


def host_or_device():
    return "cuda:0" if torch.cuda.is_available() else "cpu"


@pytest.mark.parametrize("name", sorted(INVALID))
def test_contract_violation_is_an_error_before_any_launch(name):
    lib = _hip.load_library()
    kind, build, options, want_rc, want_msg = INVALID[name]
    rc, msg, _ = run(lib, host_or_device(), kind, build, options)
    assert rc == want_rc, (rc, msg)
    assert want_msg in msg, msg


def check_route(name, device):
    lib = _hip.load_library()
    kind, build, options, family = ROUTING[name]
    rc, msg, got = run(lib, device, kind, build, options)
    assert rc == (ELAUNCH if device == "cpu" else 0), (rc, msg)  # never a validation error: the launch was reached
    assert got == family, f"{name}: family {got}, recorded {family}"


@pytest.mark.parametrize("name", sorted(ROUTING))
def test_valid_problem_reaches_the_launch_of_its_family(name):
    check_route(name, host_or_device())


@pytest.mark.gpu
def test_routing_table_runs_on_the_gpu(hip):
    for name in sorted(ROUTING):
        check_route(name, str(hip))


def workspace_grid():
    """(M, N, K, batch, dtype): tiles on both sides of the 768-tile rule (47 x 16 = 752, 48 x 16 = 768), k-tiles on both sides of 16
    (bf16: 32 elements per k-tile, fp32: 16), ragged shapes, a batch, and the degenerate call"""
    pts = [(M, N, K, b, dt) for M in (1, 100, 3008, 3072) for N in (70, 1024) for K in (33, 240, 256, 480, 512, 16384)
           for b in (1, 3) for dt in (F32, BF16)]
    return pts + [(0, 64, 64, 1, BF16), (64, 64, 64, 0, F32)]


def test_workspace_bytes_are_what_they_were():
    lib = _hip.load_library()
    want = json.load(open(GOLDEN))
    grid = workspace_grid()
    assert len(want) == len(grid) >= 190
    got = [lib.comat_gemm_workspace_bytes(*pt) for pt in grid]
    assert got == want, [(pt, g, w) for pt, g, w in zip(grid, got, want) if g != w][:5]
    assert len(set(got)) > 20  # the grid does exercise the rule
