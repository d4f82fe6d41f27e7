"""The fused attention under a causal limit and a key-padding mask (comat_flash_attn_masked_fwd / _bwd; ops._MaskedFlashAttention,
ops.set_fused_masked_attention): parity against an fp64 reference, strided operands between NaN columns, operands whose answer is
known in closed form (bit for bit), routing of ops.attention, refusals.  Both legs of `masked_dev` (tests/masked_attn_sim.py): the
simulator's mirrors on the CPU, the kernels on the GPU.

Which kernels a case reaches (attention.hip, dispatch_masked): the one-tile forward, dQ and dK/dV kernels with MASK = true, bf16 on
the hardware transpose reads and fp32 on gathered fragments whatever flash_tr says; tile width by head dim as the unmasked kernels
(d <= 32: 32 | 33..48: 64 trimmed to 48 | 49..64: 64 | 65..80: 96 trimmed to 80 | ..96: 96 | else 160), flash_trim = 0 selects the
untrimmed 64- and 96-wide tiles.  flash_trim is the only option the masked path reads, so the variants are {default, flash_trim = 0}
at the head dims it moves (40, 80).

The exact cases.  Queries come in groups of G consecutive rows; group g owns head-dim column g: Q[q] = 32 e_g, and K[j, g] is 0 on
the group's HOT keys and -32 on its cold ones, so with scale = 1/8 a hot key scores 0 and a cold one -128 (exp(-128) = 0 in fp32).
The hot set is the last 1, 2 or 4 keys that EVERY query of the group sees, so its last member sits on the first query's diagonal;
keys no query of the group may see - beyond the last query's diagonal, or masked out - are hot too (K[j, g] = 0): a kernel that lets
one through gives it weight.  P is then 1 / |hot| on the hot set and 0 elsewhere; V holds small integers and dO one small integer
per row, the spare columns of K small integers: every product and partial sum of the forward and backward is an fp32 number, and
o, dQ, dK, dV are bf16 numbers (asserted per case), so the kernels must return them bit for bit in both storage types.
test_exact_values_reject_mutants shows on the CPU that these values tell the two mistakes a hard mask invites."""
import functools

import pytest
import torch

from comat_amd import ops
from helpers import _set_opts, restore_default_opts
from masked_attn_sim import MaskedAttnSimKernels, masked_dev, sim_matches_binding  # noqa: F401 - masked_dev is a fixture

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]


def tol(dtype):
    return 2e-4 if dtype == torch.float32 else 2e-2


def rnd(*shape, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype).double()  # value representable in `dtype`, held in fp64


def dv(x, dev, dtype, grad=False):
    t = x.detach().to(device=dev, dtype=dtype).contiguous()
    return t.clone().requires_grad_(True) if grad else t


def visible_of(B_, Nq, Nk, causal, key_mask, shift=0):
    vis = torch.ones(B_, 1, Nq, Nk, dtype=torch.bool)
    if causal:
        vis = vis & torch.ones(Nq, Nk, dtype=torch.bool).tril(diagonal=Nk - Nq + shift)
    if key_mask is not None:
        vis = vis & key_mask.bool()[:, None, None, :]
    return vis


def ref_attention(q, k, v, B_, Nq, Nk, H, d, vis):
    """test_ops.ref_attention on a visibility map; a row without a visible key is all zeros (there the softmax of the original is NaN)"""
    qh = q.reshape(B_, Nq, H, d).permute(0, 2, 1, 3)
    kh = k.reshape(B_, Nk, H, d).permute(0, 2, 1, 3)
    vh = v.reshape(B_, Nk, H, d).permute(0, 2, 1, 3)
    s = (qh @ kh.transpose(-1, -2)) * d ** -0.5
    some = vis.any(-1, keepdim=True)
    s = s.masked_fill(~vis, float("-inf")).masked_fill(~some, 0.0)
    p = torch.softmax(s, -1) * some
    o = (p @ vh).permute(0, 2, 1, 3).reshape(B_ * Nq, H * d)
    return o, p


def check(got, ref, dtype, what, factor=1.0):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    print(f"{what}: max err / scale = {err / scale:.3e} (bound {tol(dtype) * factor:.1e})")
    assert err / scale < tol(dtype) * factor, f"{what}: max err {err:.3e} vs scale {scale:.3e} ({dtype})"


@pytest.fixture
def options(masked_dev):
    """options(**kernel_selection) on the hip leg (the simulator has one mirror per entry point); the defaults come back afterwards"""
    used = []

    def f(**kw):
        if masked_dev.type == "cuda" and kw:
            restore_default_opts()
            _set_opts(**kw)
            used.append(True)
    yield f
    if used:
        restore_default_opts()


# ---- a. parity against the fp64 reference ----------------------------------------------------------------------------------------
def key_mask_for(name, B_, Nk):
    if name is None:
        return None
    km = torch.ones(B_, Nk, dtype=torch.int8)
    if name == "lengths":      # right padding: visible lengths Nk, 17 and 1
        for b, n in enumerate((Nk, 17, 1)[:B_]):
            km[b, n:] = 0
    elif name == "ragged":     # right padding and a hole
        km[0, Nk - 9:] = 0
        km[B_ - 1, 3:11] = 0
    elif name == "left":       # left padding of entry 0: under the causal limit queries 0..5 see nothing
        km[0, :6] = 0
    return km


# (B, Nq, Nk, H, d), causal, key mask; head dims 40 and 80 run trimmed and, on the GPU, untrimmed (flash_trim = 0)
PARITY = [
    ((2, 77, 77, 3, 64), True, None),         # the diagonal crosses every tile; 13-key tail
    ((3, 40, 40, 2, 64), True, "lengths"),    # causal + key mask, visible lengths 40, 17 and 1
    ((2, 33, 70, 2, 40), False, "ragged"),    # key mask only; trimmed head dim; Nq != Nk
    ((1, 5, 37, 2, 16), True, None),          # causal_offset = 32
    ((1, 300, 300, 1, 32), True, None),       # three query and key blocks: the block-uniform loop bounds at both ends
    ((2, 50, 50, 2, 80), True, None),         # the 96-wide kernels
    ((2, 20, 20, 2, 64), True, "left"),       # queries 0..5 of entry 0 have no visible key
]


def option_sets(d, dev):
    return ({}, dict(flash_trim=0)) if d in (40, 80) and dev.type == "cuda" else ({},)


@functools.lru_cache(maxsize=None)
def parity_case(shape, causal, mask_name, dtype):
    B_, Nq, Nk, H, d = shape
    q, k, v = (rnd(B_ * n, H * d, dtype=dtype, seed=s) for n, s in ((Nq, 1), (Nk, 2), (Nk, 3)))
    go = rnd(B_ * Nq, H * d, dtype=dtype, seed=4)
    km = key_mask_for(mask_name, B_, Nk)
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    o_ref, _ = ref_attention(qr, kr, vr, B_, Nq, Nk, H, d, visible_of(B_, Nq, Nk, causal, km))
    (o_ref * go).sum().backward()
    return q, k, v, go, km, o_ref.detach(), qr.grad, kr.grad, vr.grad


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", PARITY, ids=lambda c: "x".join(map(str, c[0])))
def test_parity(masked_dev, options, dtype, case):
    shape, causal, mask_name = case
    for opts in option_sets(shape[4], masked_dev):
        options(**opts)
        _parity(masked_dev, dtype, shape, causal, mask_name)


def _parity(masked_dev, dtype, shape, causal, mask_name):
    B_, Nq, Nk, H, d = shape
    q, k, v, go, km, o_ref, dq_ref, dk_ref, dv_ref = parity_case(shape, causal, mask_name, dtype)
    ops.set_fused_masked_attention(True)
    qd, kd, vd = (dv(t, masked_dev, dtype, grad=True) for t in (q, k, v))
    kmd = None if km is None else km.to(masked_dev)
    o, p = ops.attention(qd, kd, vd, B_, Nq, Nk, H, d, causal=causal, key_mask=kmd, need_probs=False)
    assert p is None
    (o.float() * dv(go, masked_dev, F32)).sum().backward()
    for t in (o, qd.grad, kd.grad, vd.grad):
        assert bool(torch.isfinite(t).all())
    if mask_name == "left":
        empty = slice(0, 6)  # rows of batch entry 0
        assert bool((o[empty] == 0).all()) and bool((qd.grad[empty] == 0).all()), "a query without a visible key must give O = 0 and dQ = 0"
    check(o, o_ref, dtype, "masked flash out")
    check(qd.grad, dq_ref, dtype, "masked flash dQ", factor=3)
    check(kd.grad, dk_ref, dtype, "masked flash dK", factor=3)
    check(vd.grad, dv_ref, dtype, "masked flash dV", factor=3)


# ---- b. strided operands ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_strided_operands(masked_dev, dtype):
    """q / k / v are column slices of one [M, 3D] buffer (ld = 3D), the gradients slices of another; the call covers the first H of
    HT heads, so the last head's columns of every slice - and of O and dO at ld = D - lie outside: NaN before, the same NaN after"""
    B_, N, HT, H, d = 2, 45, 3, 2, 16
    D, M = HT * d, B_ * N
    K = ops.masked_attn_kernels()
    km = key_mask_for("ragged", B_, N).to(masked_dev)
    inside = torch.zeros(D, dtype=torch.bool)
    inside[:H * d] = True
    qkv = torch.full((M, 3 * D), float("nan"), dtype=dtype)
    cols3 = inside.repeat(3)
    qkv[:, cols3] = rnd(M, 3 * H * d, dtype=dtype, seed=7).to(dtype)
    go = torch.full((M, D), float("nan"), dtype=dtype)
    go[:, inside] = rnd(M, H * d, dtype=dtype, seed=8).to(dtype)
    qkv, go = qkv.to(masked_dev), go.to(masked_dev)
    nan = lambda *s: torch.full(s, float("nan"), dtype=dtype, device=masked_dev)
    o, dqkv = nan(M, D), nan(M, 3 * D)
    lse, dbuf = (torch.empty((B_, H, N), dtype=F32, device=masked_dev) for _ in range(2))
    sl = lambda t, i: t[:, i * D:(i + 1) * D]
    args = (B_, H, N, N, d, 3 * D, 3 * D, 3 * D, D, d ** -0.5)
    K.flash_attn_masked_fwd(sl(qkv, 0), sl(qkv, 1), sl(qkv, 2), o, lse, *args, True, 0, km)
    K.flash_attn_masked_bwd(sl(qkv, 0), sl(qkv, 1), sl(qkv, 2), o, go, lse, dbuf, sl(dqkv, 0), sl(dqkv, 1), sl(dqkv, 2), *args, True, 0, km)
    # the same call on packed operands
    pk = lambda t: t[:, :H * d].contiguous()
    qc, kc, vc, gc = pk(sl(qkv, 0)), pk(sl(qkv, 1)), pk(sl(qkv, 2)), pk(go)
    oc, dqc, dkc, dvc = (torch.empty_like(qc) for _ in range(4))
    lse2, dbuf2 = torch.empty_like(lse), torch.empty_like(dbuf)
    argc = (B_, H, N, N, d, H * d, H * d, H * d, H * d, d ** -0.5)
    K.flash_attn_masked_fwd(qc, kc, vc, oc, lse2, *argc, True, 0, km)
    K.flash_attn_masked_bwd(qc, kc, vc, oc, gc, lse2, dbuf2, dqc, dkc, dvc, *argc, True, 0, km)
    assert bool(torch.isnan(o[:, H * d:]).all()), "O: a column outside the heads of the call was written"
    assert torch.equal(o[:, :H * d], oc) and bool(torch.isfinite(oc).all())
    for i, (name, ref) in enumerate((("dQ", dqc), ("dK", dkc), ("dV", dvc))):
        got = sl(dqkv, i)
        assert bool(torch.isnan(got[:, H * d:]).all()), f"{name}: a column outside the heads of the call was written"
        assert torch.equal(got[:, :H * d], ref) and bool(torch.isfinite(ref).all()), f"{name}: strided and packed calls differ"
    assert torch.equal(lse, lse2)


# ---- c. operands with a closed-form answer ---------------------------------------------------------------------------------------
SCALE = 0.125
# (B, Nq, Nk, H, d), causal, key mask: Nk no multiple of 32 everywhere; the second combines both masks
EXACT = [
    ((1, 40, 77, 1, 64), True, None),        # causal_offset 37; 13-key tail
    ((2, 45, 45, 2, 32), True, "ragged"),    # causal + key mask
    ((2, 20, 20, 2, 16), True, "left"),      # rows without a visible key
    ((1, 33, 70, 2, 40), False, "ragged"),   # key mask only, trimmed head dim
    ((1, 50, 50, 1, 80), True, None),        # the 96-wide kernels
]


@functools.lru_cache(maxsize=None)
def exact_case(shape, causal, mask_name):
    B_, Nq, Nk, H, d = shape
    km = key_mask_for(mask_name, B_, Nk)
    vis = visible_of(B_, Nq, Nk, causal, km)[:, 0]  # [B, Nq, Nk]
    ngroups = d // 2
    G = -(-Nq // ngroups)
    g = torch.Generator().manual_seed(sum(shape))
    Q = torch.zeros(B_, H, Nq, d, dtype=torch.float64)
    K = torch.randint(-2, 3, (B_, H, Nk, d), generator=g).double()  # spare columns: small integers no query reads
    P = torch.zeros(B_, H, Nq, Nk, dtype=torch.float64)
    for b in range(B_):
        for gi in range(-(-Nq // G)):
            rows = range(gi * G, min(Nq, (gi + 1) * G))
            common = torch.nonzero(vis[b, rows.start]).flatten()  # what the first query sees, every query of the group sees
            assert all(bool(vis[b, r, common].all()) for r in rows)
            n = 4 if len(common) >= 4 else 2 if len(common) >= 2 else len(common)
            hot = common[len(common) - n:]
            if n == 0:
                assert not bool(vis[b, list(rows)].any()), "a group without a hot key must be a group of empty rows"
            unseen = ~vis[b, list(rows)].any(0)  # keys no query of the group may see: hot, so that letting one in shows
            col = torch.full((Nk,), -32.0, dtype=torch.float64)
            col[hot] = 0.0
            col[unseen] = 0.0
            K[b, :, :, gi] = col
            for r in rows:
                Q[b, :, r, gi] = 32.0
                if n:
                    P[b, :, r, hot] = 1.0 / n
    V = torch.randint(-3, 4, (B_, H, Nk, d), generator=g).double()
    dO = torch.zeros(B_, H, Nq, d, dtype=torch.float64)
    cols = torch.randint(0, d, (B_, H, Nq), generator=g)
    vals = (torch.randint(1, 3, (B_, H, Nq), generator=g) * (torch.randint(0, 2, (B_, H, Nq), generator=g) * 2 - 1)).double()
    dO.scatter_(-1, cols[..., None], vals[..., None])
    O = P @ V
    Dq = (dO * O).sum(-1, keepdim=True)
    dS = P * (dO @ V.transpose(-1, -2) - Dq)
    exp = dict(o=O, dq=SCALE * dS @ K, dk=SCALE * dS.transpose(-1, -2) @ Q, dv=P.transpose(-1, -2) @ dO)
    for name, t in exp.items():
        assert torch.equal(t.to(BF16).double(), t), f"{name} of the exact case is not a bf16 number everywhere"
    assert torch.equal(dS.to(BF16).double(), dS), "dS is not a bf16 number: the bf16 pack in front of the dQ / dK products would round"
    return dict(Q=Q, K=K, V=V, dO=dO, km=km, vis=vis, P=P, **exp)


def flat(x):
    """[B, H, N, d] -> the [B * N, H * d] matrix the kernels address heads in"""
    B_, H, N, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(B_ * N, H * d)


def softmax_attention64(c, vis):
    """plain fp64 softmax attention and its gradients under the visibility map `vis` [B, Nq, Nk]"""
    B_, H, Nq, d = c["Q"].shape
    Nk = c["K"].shape[2]
    q, k, v = (flat(c[n]).clone().requires_grad_(True) for n in ("Q", "K", "V"))
    qh, kh, vh = (t.reshape(B_, -1, H, d).permute(0, 2, 1, 3) for t in (q, k, v))
    some = vis[:, None].any(-1, keepdim=True)
    s = (qh @ kh.transpose(-1, -2) * SCALE).masked_fill(~vis[:, None], float("-inf")).masked_fill(~some, 0.0)
    o = flat((torch.softmax(s, -1) * some) @ vh)
    (o * flat(c["dO"])).sum().backward()
    return dict(o=o.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


@pytest.mark.parametrize("case", EXACT, ids=lambda c: "x".join(map(str, c[0])))
def test_exact_values_reject_mutants(case):
    """CPU only.  The closed form IS the softmax answer (1e-12), and is not the answer of a kernel that moves the diagonal by one
    (j < q + offset) or lets one masked key through - a key that is hot for the query's group, which is every padded key and every
    key beyond the diagonal of the group's last query (a key that a later query of the same group sees is cold, exp(-128) = 0, for
    the whole group: G - 1 keys per row at most)"""
    shape, causal, mask_name = case
    c = exact_case(*case)
    differs = lambda got: any(not torch.allclose(got[n], flat(c[n]), rtol=0, atol=1e-3) for n in ("o", "dq", "dk", "dv"))
    good = softmax_attention64(c, c["vis"])
    for n in ("o", "dq", "dk", "dv"):
        assert torch.allclose(good[n], flat(c[n]), rtol=0, atol=1e-12), n
    B_, Nq, Nk = c["vis"].shape
    if causal:
        assert differs(softmax_attention64(c, visible_of(B_, Nq, Nk, True, c["km"], shift=-1)[:, 0])), "diagonal moved by one: not seen"
    G = -(-Nq // (shape[4] // 2))
    hot_col = c["K"][:, 0].transpose(-1, -2)[:, torch.arange(Nq) // G] == 0  # [B, Nq, Nk]: key j is hot for query r's group
    hidden = torch.nonzero(~c["vis"] & c["vis"].any(-1, keepdim=True) & hot_col)  # masked, hot entries of rows that see something
    assert len(hidden) >= 3
    for b, r, j in (hidden[0].tolist(), hidden[len(hidden) // 2].tolist(), hidden[-1].tolist()):
        leak = c["vis"].clone()
        leak[b, r, j] = True
        assert differs(softmax_attention64(c, leak)), f"masked key {j} visible to query {r} of entry {b}: not seen"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", EXACT, ids=lambda c: "x".join(map(str, c[0])))
def test_exact(masked_dev, options, dtype, case):
    (B_, Nq, Nk, H, d), causal, mask_name = case
    c = exact_case(*case)
    for opts in option_sets(d, masked_dev):
        options(**opts)
        ops.set_fused_masked_attention(True)
        qd, kd, vd = (dv(flat(c[n]), masked_dev, dtype, grad=True) for n in ("Q", "K", "V"))
        kmd = None if c["km"] is None else c["km"].to(masked_dev)
        o, p = ops.attention(qd, kd, vd, B_, Nq, Nk, H, d, scale=SCALE, causal=causal, key_mask=kmd, need_probs=False)
        assert p is None
        (o.float() * dv(flat(c["dO"]), masked_dev, F32)).sum().backward()
        for name, got in (("o", o), ("dq", qd.grad), ("dk", kd.grad), ("dv", vd.grad)):
            got, ref = got.detach().double().cpu(), flat(c[name])
            bad = torch.nonzero(got != ref)
            assert len(bad) == 0, (f"{name} {opts}: {len(bad)} elements differ from the closed form, first at row {bad[0][0].item()} column "
                                   f"{bad[0][1].item()}: got {got[tuple(bad[0])].item()!r}, exact {ref[tuple(bad[0])].item()!r}")


# ---- d. routing and refusals ------------------------------------------------------------------------------------------------------
def test_routing(masked_dev):
    B_, N, H, d = 2, 12, 2, 16
    dtype = F32
    q, k, v = (rnd(B_ * N, H * d, seed=s).float() for s in (1, 2, 3))
    km = key_mask_for("ragged", B_, N).to(masked_dev)
    sim = ops.kernels() if isinstance(ops.kernels(), MaskedAttnSimKernels) else None
    counts = lambda: dict(sim.masked_calls) if sim else None

    def run(need_probs):
        qd, kd, vd = (dv(t, masked_dev, dtype, grad=True) for t in (q, k, v))
        o, p = ops.attention(qd, kd, vd, B_, N, N, H, d, causal=True, key_mask=km, need_probs=need_probs)
        o.sum().backward()
        return o.detach(), p, qd.grad, kd.grad, vd.grad

    assert ops.fused_masked_attention() is False, "the switch is off by default"
    base = run(True)  # today's _Attention
    assert base[1] is not None
    off = run(False)
    assert off[1] is not None and all(torch.equal(a, b) for a, b in zip(off, base)), "switch off: need_probs=False must change nothing"
    assert counts() in (None, dict(fwd=0, bwd=0))
    ops.set_fused_masked_attention(True)
    assert ops.fused_masked_attention() is True
    probs = run(True)
    assert probs[1] is not None and all(torch.equal(a, b) for a, b in zip(probs, base)), "need_probs=True always materialises"
    assert counts() in (None, dict(fwd=0, bwd=0))
    fused = run(False)
    assert fused[1] is None
    assert counts() in (None, dict(fwd=1, bwd=1))
    for a, b in zip(fused[:1] + fused[2:], base[:1] + base[2:]):
        assert (a - b).abs().max().item() < 2e-4 * (b.abs().max().item() + 1e-6)
    # a head dim the fused kernels do not take stays on the materialised path
    q2, k2, v2 = (rnd(B_ * N, H * 6, seed=s).float().to(masked_dev) for s in (1, 2, 3))
    o2, p2 = ops.attention(q2, k2, v2, B_, N, N, H, 6, causal=True, need_probs=False)
    assert p2 is not None
    ops.set_fused_masked_attention(False)
    assert run(False)[1] is not None


def test_refusals(masked_dev):
    """null pointers and an unsupported head dim are refused by name, before anything is launched"""
    K = ops.masked_attn_kernels()
    B_, N, H, d = 1, 8, 1, 16
    t = lambda *s: torch.zeros(s, dtype=F32, device=masked_dev)
    q, k, v, o, go, dq, dk, dv_ = (t(B_ * N, H * d) for _ in range(8))
    lse, dbuf = t(B_, H, N), t(B_, H, N)
    shp = (B_, H, N, N, d, H * d, H * d, H * d, H * d, 0.25)
    with pytest.raises(RuntimeError, match="comat_flash_attn_masked_fwd.*null"):
        K.flash_attn_masked_fwd(q, None, v, o, lse, *shp, True, 0, None)
    with pytest.raises(RuntimeError, match="comat_flash_attn_masked_fwd.*null"):
        K.flash_attn_masked_fwd(q, k, v, o, None, *shp, True, 0, None)
    with pytest.raises(RuntimeError, match="comat_flash_attn_masked_bwd.*null"):
        K.flash_attn_masked_bwd(q, k, v, o, go, lse, dbuf, dq, None, dv_, *shp, True, 0, None)
    bad = (B_, H, N, N, 6, H * d, H * d, H * d, H * d, 0.25)
    with pytest.raises(RuntimeError, match="comat_flash_attn_masked_fwd.*head dim"):
        K.flash_attn_masked_fwd(q, k, v, o, lse, *bad, True, 0, None)
    with pytest.raises(RuntimeError, match="comat_flash_attn_masked_bwd.*head dim"):
        K.flash_attn_masked_bwd(q, k, v, o, go, lse, dbuf, dq, dk, dv_, *bad, True, 0, None)
    big = (40000, 2, N, N, d, H * d, H * d, H * d, H * d, 0.25)  # B * H > 65535
    with pytest.raises(RuntimeError, match="comat_flash_attn_masked_fwd.*bad shape"):
        K.flash_attn_masked_fwd(q, k, v, o, lse, *big, True, 0, None)
    assert bool((o == 0).all()) and bool((dq == 0).all())


# ---- e. the simulator carries the binding's argument lists ----------------------------------------------------------------------
def test_sim_matches_binding():
    names, mismatches = sim_matches_binding()
    assert len(names) == 2 and mismatches == []
