"""comat_eos_pool (include/comat_hip.h): the end token's position by transformers' two rules, and the final LayerNorm of that row
alone - on the simulator (tests/clip2_sim.py) and on the real kernel.

There is no tolerance in this file.  `pos` is torch's own expression on the same ids; `out[b]` is held bit for bit to row
b * L + pos[b] of ops.layer_norm over ALL rows of the same tensor on the same backend - the form the entry point replaces.  The
two take the same path where their pointers are aligned alike, so the reference of a misaligned `h` is computed on a misaligned
tensor too.  Paths by shape: 16-byte accesses where C is a multiple of 16 / sizeof T with at most 256 vectors a row - C = 64, 192
in both dtypes, 20 in fp32, 1280 in bf16 - and the scalar routine elsewhere: C = 20 in bf16, 1280 in fp32 (320 vectors), and any
misaligned `h`.

Every call runs on windowed operands (helpers.Window): `h` holds NaN in every row that is not selected and sits between NaN
guard rows, `out` and `pos` sit between armed guard bands."""
import pytest
import torch

from clip2_sim import Clip2SimKernels, clip2_dev, eos_positions, sim_matches_binding  # noqa: F401 - fixture
from comat_amd import ops
from helpers import Window

EOS, BIG = 7, 50  # the end token of the non-legacy rule is NOT the largest id present: the two rules disagree on the same ids
EPS = 1e-5
INT_OF = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


def bits(t):
    return t.contiguous().view(INT_OF[t.dtype]).cpu()


def make_ids(B, L, seed, shift=0):
    """ids in 8 .. 40 with the end token placed by (b + shift) % 4: at position 0, at L - 1, repeated from the middle on (the first
    occurrence wins), absent (position 0).  One BIG id elsewhere, repeated where there is room: the legacy rule's row."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(8, 41, (B, L), generator=g)
    for b in range(B):
        kind = (b + shift) % 4
        if kind == 0:
            ids[b, 0] = EOS
        elif kind == 1:
            ids[b, L - 1] = EOS
        elif kind == 2:
            ids[b, L // 2:] = EOS
        free = [p for p in range(1, L - 1) if int(ids[b, p]) != EOS]  # neither end, no end token
        if free:
            k = (b + seed) % len(free)
            ids[b, free[k]] = ids[b, free[(k + 2) % len(free)]] = BIG
    return ids


def operands(B, L, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    h = (torch.randn(B * L, C, generator=g) * 2 + 0.5).to(dtype)
    gamma = 1 + 0.2 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    return h, gamma, beta


def run_windowed(dev, ids, h, gamma, beta, rows, eos_id, left=8, want_pos=True):
    """the call on windowed operands: NaN in every row of h that is not in `rows`.  -> (out, pos)"""
    B, L = ids.shape
    C = h.shape[1]
    poisoned = torch.full_like(h, float("nan"))
    poisoned[rows] = h[rows]
    hw = Window(B * L, C, dtype=h.dtype, device=dev, left=left).put(poisoned)
    iw = Window(B, L, dtype=torch.int64, device=dev).put(ids)
    ow = Window(B, C, dtype=h.dtype, device=dev).arm()
    pw = Window(1, B, dtype=torch.int64, device=dev).arm()
    ops.pool_kernels().eos_pool(iw.view, hw.view, gamma.to(dev), beta.to(dev), ow.view, pw.flat if want_pos else None, B, L, C, eos_id,
                                EPS)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    ow.assert_guard_intact("out")
    pw.assert_guard_intact("pos")
    if not want_pos:
        assert torch.equal(pw.buf.view(torch.int64), pw._snap), "pos = NULL, yet the buffer was written"
    return ow.get().cpu(), pw.flat.clone().cpu()


def check_case(dev, B, L, C, dtype, seed, shift=0, left=8):
    ids = make_ids(B, L, seed, shift)
    h, gamma, beta = operands(B, L, C, dtype, seed + 1)
    if left == 8:
        x = h.to(dev)
    else:  # the reference on a tensor as misaligned as the window's: comat_layernorm_fwd then takes the scalar routine too
        x = torch.empty(B * L * C + left, dtype=dtype, device=dev)[left:].view(B * L, C)
        x.copy_(h)
        assert dev.type != "cuda" or x.data_ptr() % 16 != 0
    with torch.no_grad():
        ref = ops.layer_norm(x, gamma.to(dev), beta.to(dev), eps=EPS).cpu()
    assert torch.isfinite(ref.float()).all()
    seen = []
    for eos_id in (2, EOS):
        want = eos_positions(ids, eos_id)
        rows = torch.arange(B) * L + want
        out, pos = run_windowed(dev, ids, h, gamma, beta, rows, eos_id, left=left)
        assert torch.equal(pos, want), (eos_id, pos.tolist(), want.tolist())
        assert torch.equal(bits(out), bits(ref[rows])), f"eos_id {eos_id}: {int((bits(out) != bits(ref[rows])).sum())} elements differ"
        seen.append(want)
    return ids, seen


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [20, 64, 192, 1280])
@pytest.mark.parametrize("L", [1, 8, 77, 130])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_position_and_row_bits(clip2_dev, B, L, C, dtype):
    ids, (legacy, first) = check_case(clip2_dev, B, L, C, dtype, seed=B * 1000 + L, shift=L + C)
    if L >= 8 and B >= 3:
        assert not torch.equal(legacy, first), "the two rules agree on every sequence: the case shows one rule only"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [320, 768, 1024, 2048, 2056])
def test_every_count_of_vectors_per_lane(clip2_dev, C, dtype):
    """the vectorised routine is compiled once per count of 16-byte vectors a lane holds (1 .. 4): with the widths above, 1 .. 4 in
    fp32 (20, 320, 768, 1024) and in bf16 (64, 768, 1280, 2048); 2048 in fp32 and 2056 are beyond the registers: scalar"""
    check_case(clip2_dev, 5, 77, C, dtype, seed=C)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,L,C", [(5, 77, 192), (3, 130, 64), (5, 8, 1280)])
def test_misaligned_h_takes_the_scalar_path(clip2_dev, B, L, C, dtype):
    check_case(clip2_dev, B, L, C, dtype, seed=B + L + C, left=1)


@pytest.mark.parametrize("L", [8, 77, 130])
def test_end_token_placements(clip2_dev, L):
    """position 0, L - 1, repeated (the first occurrence), absent (0): one sequence each, and a fifth that crosses the block"""
    ids = make_ids(5, L, seed=L)
    first = eos_positions(ids, EOS)
    assert first.tolist() == [0, L - 1, L // 2, 0, 0]
    assert (ids[3] != EOS).all() and int((ids[2] == EOS).sum()) > 1
    legacy = eos_positions(ids, 2)
    assert all(int(ids[b, legacy[b]]) == BIG and int((ids[b] == BIG).sum()) > 1 for b in (0, 1, 3)), "the largest id repeats"
    check_case(clip2_dev, 5, L, 64, torch.bfloat16, seed=L)


def test_a_selected_row_with_nan_reaches_out_and_no_other_does(clip2_dev):
    B, L, C, dtype = 5, 77, 192, torch.bfloat16
    ids = make_ids(B, L, seed=3)
    h, gamma, beta = operands(B, L, C, dtype, seed=4)
    want = eos_positions(ids, EOS)
    rows = torch.arange(B) * L + want
    h[rows[2], 5] = float("nan")
    out, _ = run_windowed(clip2_dev, ids, h, gamma, beta, rows, EOS, want_pos=False)  # (pos = NULL is taken)
    nan = torch.isnan(out.float())
    assert nan[2].all(), "the NaN of the selected row did not reach its output"
    assert not nan[[0, 1, 3, 4]].any()


def test_bad_arguments_are_refused_by_name(clip2_dev):
    dev = clip2_dev
    B, L, C = 2, 8, 64
    ids = make_ids(B, L, seed=1).to(dev)
    h, gamma, beta = (t.to(dev) for t in operands(B, L, C, torch.float32, seed=2))
    out, pos = torch.empty(B, C, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
    call = ops.pool_kernels().eos_pool
    good = dict(ids=ids, h=h, gamma=gamma, beta=beta, out=out, pos=pos, B=B, L=L, C=C, eos_id=EOS, eps=EPS)
    call(**good)
    bad = [dict(ids=None), dict(h=None, out=None), dict(gamma=None), dict(beta=None), dict(out=None, h=None), dict(B=0), dict(L=0),
           dict(C=0), dict(B=-1), dict(eos_id=-1), dict(h=h.half(), out=out.half())]
    for change in bad:
        with pytest.raises(RuntimeError, match="comat_eos_pool"):
            call(**{**good, **change})
    if dev.type == "cuda":
        torch.cuda.synchronize()


def test_the_operator(clip2_dev):
    dev = clip2_dev
    B, L, C = 3, 8, 64
    ids = make_ids(B, L, seed=5)
    h, gamma, beta = (t.to(dev) for t in operands(B, L, C, torch.float32, seed=6))
    got = ops.eos_pool(ids.to(dev), h, gamma, beta, L, EOS, EPS)
    with torch.no_grad():
        ref = ops.layer_norm(h, gamma, beta, eps=EPS)[torch.arange(B) * L + eos_positions(ids, EOS)]
    assert got.shape == (B, C) and not got.requires_grad and torch.equal(bits(got), bits(ref))
    with pytest.raises(NotImplementedError, match="not built"):
        ops.eos_pool(ids.to(dev), h.clone().requires_grad_(True), gamma, beta, L, EOS, EPS)
    with pytest.raises(ValueError, match="do not fit"):
        ops.eos_pool(ids.to(dev), h[:-1], gamma, beta, L, EOS, EPS)


def test_simulator_mirror_has_the_bindings_argument_list():
    names, differ = sim_matches_binding()
    assert names == ("eos_pool",) and not differ
    from comat_amd import _hip
    assert "comat_eos_pool" in _hip.SIGNATURES and _hip.ABI_VERSION == 8


def test_pool_kernels_hands_out_the_installed_backend(sim):
    from comat_amd import _hip
    assert ops.pool_kernels() is _hip  # the plain simulator lacks the entry point: the binding answers (and refuses CPU tensors)
    k = Clip2SimKernels()
    ops.set_kernel_backend(k)
    assert ops.pool_kernels() is k
