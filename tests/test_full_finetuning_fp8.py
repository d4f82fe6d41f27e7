"""The fp8 forward of a fully trained UNet: `UNetBank(..., fp8=True)` + `UNet(..., bank=bank, fp8_forward=True)`.

The bank owns the e4m3 bytes and the scale of every fp8-eligible weight; the refresh launch behind an optimizer update rewrites
them from the master (comat_weights_refresh_q8).  Exact statements: the bytes / scales are the CPU oracle's quantiser on the
forward copy and those of a frozen fp8 UNet built from the same weights (U1), the no-grad forward has the frozen fp8 UNet's bits
before and after an update (U2), and at operator level the output is the frozen holder's while every gradient is the unquantised
trained holder's (U3).  Network and step level are held to the oracle's fp8 emulation (oracle/sd.py fp8=True: value of the
quantised product, gradient of the unquantised one, for every leaf) under the noise-level bounds of tests/test_fp8.py.

Operator level, the GEGLU feed-forward pair: its backward reads the pre-activations and the GEGLU output its own forward saved, so
under fp8 only `ff.net.2`'s bias gradient is bitwise that of the fp8-off pair; y and dx are bitwise the frozen pair's under fp8 and the
weight gradients are held to fp64 sums of the saved tensors (see the test).  Measured distances: the docstrings of the U5 / U6 tests.
"""
import dataclasses

import numpy as np
import pytest
import torch

from comat_amd import checkpoint, config, ops, weights
from comat_amd.unet import UNet, UNetBank, _Mods
from helpers import fp8_state, rel_l2, tok
from oracle import fp8 as OF
from oracle import sd as O
from test_fp8 import FP8_DRAWS, FP8_UNET, _fp8_world, rnd
from test_full_finetuning import BF16_UNET_GRAD_LIMIT, bank_grads, bank_vec, oracle_vec

F32, BF16 = torch.float32, torch.bfloat16
T = 417


@pytest.fixture
def dev(dev):
    with fp8_state():
        yield dev


@pytest.fixture
def sim(sim):
    with fp8_state():
        yield sim


@pytest.fixture
def hip(hip):
    with fp8_state():
        yield hip


def k_inner(h):
    return h.cin if hasattr(h, "cin") else h.in_features


def eligible_name(name, h):
    return k_inner(h) % 64 == 0 and not any(f in name for f in _Mods.NO_FP8)


def forward(unet, dev, dtype, x, ctx, added, B, h, w, L):
    return unet(tok(x).to(dev, dtype), B, h, w, T, ctx.reshape(B * L, -1).to(dev, dtype).contiguous(), L,
                added=(added[0].to(dev), added[1].tolist()))[0]


def check_bank_bytes(bank, what):
    """every eligible holder: bytes and scale of the oracle's quantiser on the holder's own forward copy -> their number"""
    n = 0
    for name, (_, h) in bank._made.items():
        if not hasattr(h, "w"):
            continue
        w8 = getattr(h, "_w8", None)
        if not eligible_name(name, h):
            assert w8 is None, f"{what}: {name} is not eligible and carries bytes"
            continue
        assert w8 is not None, f"{what}: {name} is eligible and carries no bytes"
        q, s = OF.quantize(h.w.detach().cpu())
        assert w8[0].shape == h.w.shape and w8[0].dtype == torch.uint8 and w8[1].shape == (1,)
        assert torch.equal(w8[1].cpu().view(torch.int32).reshape(()), s.view(torch.int32)), f"{what}: scale of {name}"
        assert torch.equal(w8[0].cpu(), q), f"{what}: bytes of {name}"
        n += 1
    return n


# ---- U1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_bank_weight_bytes_follow_the_master(dev, dtype):
    ucfg, _, usd, _, _, _, _, _, _ = _fp8_world(dev, dtype)
    bank = UNetBank(ucfg, usd, dtype, dev, fp8=True)
    UNet(ucfg, usd, dtype, dev, bank=bank, fp8_forward=True)
    frozen = UNet(ucfg, usd, dtype, dev, fp8_forward=True)
    bank.ensure_compute_copy()
    n = check_bank_bytes(bank, "after construction")
    assert n > 100 and n == len(bank._slot)
    by_name, stack, seen = {}, [frozen], set()  # the frozen UNet keeps no list of its holders: walk its layers
    while stack:
        o = stack.pop()
        if id(o) in seen:
            continue
        seen.add(id(o))
        if hasattr(o, "_fp8_name") and hasattr(o, "w"):
            by_name[o._fp8_name] = o
        elif isinstance(o, (list, tuple)):
            stack += list(o)
        elif isinstance(o, dict):
            stack += list(o.values())
        elif hasattr(o, "__dict__") and type(o).__module__.startswith("comat_amd"):
            stack += list(vars(o).values())
    m = 0
    for name, (_, h) in bank._made.items():
        if getattr(h, "_w8", None) is None:
            continue
        f = by_name[name]
        assert torch.equal(h._w8[0].cpu(), f._w8[0].cpu().reshape(h._w8[0].shape)), f"{name}: bytes differ from the frozen UNet's"
        assert torch.equal(h._w8[1].cpu().reshape(()), f._w8[1].cpu().reshape(())), f"{name}: scale differs from the frozen UNet's"
        m += 1
    assert m == n
    ptrs = {name: (h._w8[0].data_ptr(), h._w8[1].data_ptr()) for name, (_, h) in bank._made.items() if getattr(h, "_w8", None)}
    with torch.no_grad():
        bank.flat.mul_(1.25).add_(0.01)
    bank.mark_updated()
    bank.ensure_compute_copy()
    assert check_bank_bytes(bank, "after the update") == n
    assert ptrs == {name: (h._w8[0].data_ptr(), h._w8[1].data_ptr()) for name, (_, h) in bank._made.items()
                    if getattr(h, "_w8", None)}


# ---- U2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_no_grad_forward_has_the_frozen_fp8_bits(dev, dtype):
    ops.set_fp8_scaling("jit")
    ucfg, _, usd, _, (B, h, w, L), x, ctx, added, _ = _fp8_world(dev, dtype)
    bank = UNetBank(ucfg, usd, dtype, dev, fp8=True)
    unet = UNet(ucfg, usd, dtype, dev, bank=bank, fp8_forward=True)
    plain = UNet(ucfg, usd, dtype, dev, bank=bank)  # the same holders, no fp8 context
    args = (dev, dtype, x, ctx, added, B, h, w, L)
    with torch.no_grad():
        got = forward(unet, *args).clone()
        want = forward(UNet(ucfg, usd, dtype, dev, fp8_forward=True), *args)
        exact = forward(plain, *args)
        assert torch.equal(got, want), f"before the update: rel-L2 {rel_l2(got, want):.3e}"
        assert rel_l2(got, exact) > 1e-2, "the quantiser is not on"
        for n_ in ("time_embedding.linear_2.weight", "down_blocks.0.resnets.0.time_emb_proj.bias", "mid_block.resnets.0.conv1.weight"):
            bank.params[n_].add_(0.05)
        bank.mark_updated()
        after = forward(unet, *args)
        # (the fp32 master as it is: the frozen constructor rounds the weights once, as the refresh does, and keeps biases fp32)
        fresh = forward(UNet(ucfg, bank.state_dict(), dtype, dev, fp8_forward=True), *args)
    assert not torch.equal(after, got)
    assert torch.equal(after, fresh), f"after the update: rel-L2 {rel_l2(after, fresh):.3e}"


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_no_grad_forward_has_the_frozen_fp8_bits_under_delayed_scaling(sim, dtype):
    """the same statement with delayed activation scales: after a calibration pass, two forwards with an update of the scales in
    between have the bits of the frozen fp8 UNet put through the same sequence (each in a site table of its own)"""
    ops.set_fp8_scaling("delayed")
    ucfg, _, usd, _, (B, h, w, L), x, ctx, added, _ = _fp8_world(sim, dtype)
    outs = []
    for banked in (True, False):
        ops.fp8_reset()
        kw = dict(bank=UNetBank(ucfg, usd, dtype, sim, fp8=True)) if banked else {}
        unet = UNet(ucfg, usd, dtype, sim, fp8_forward=True, **kw)
        with torch.no_grad():
            with ops.fp8_calibration():
                forward(unet, sim, dtype, x, ctx, added, B, h, w, L)
            ops.fp8_end_of_step()
            a = forward(unet, sim, dtype, x * 1.1, ctx, added, B, h, w, L).clone()  # beyond the calibrated maxima: some values saturate
            ops.fp8_end_of_step()
            outs.append((a, forward(unet, sim, dtype, x, ctx, added, B, h, w, L).clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], outs[0][1])


# ---- U3 -------------------------------------------------------------------------------------------------------------------------
def _own(holder, dev):
    """what the bank does for a holder, on buffers of the test's own: bytes and scale through the refresh launch"""
    from comat_amd import refresh
    holder.allow_fp8 = True
    w = holder.w
    n = w.numel()
    if w.dim() == 4:
        problems = refresh.conv_problems(0, 0, 0, *w.shape)
        wt = holder.wd
    else:
        problems = refresh.linear_problem(0, 0, 0, *w.shape)
        wt = holder.wt
    q8 = torch.zeros(n, dtype=torch.uint8, device=dev)
    sc, am = torch.zeros(1, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    master = w.detach().float().reshape(-1).contiguous()
    plan = refresh.RefreshPlan(problems, dev, slots=[0] * len(problems))
    plan.run(master, None if w.dtype == F32 else w.reshape(-1), wt.reshape(-1), q8, sc, am)
    holder._w8 = (q8.view(w.shape), sc)
    return holder


def _trainable_linear(W, b, dtype, dev, cls=ops.TrainableLinear):
    w = W.to(dev, dtype).contiguous()
    lin = cls(w, torch.zeros(W.shape, device=dev), b.to(dev), torch.zeros(b.shape, device=dev))
    lin.refresh()
    return lin


def test_operators_forward_of_the_frozen_backward_of_the_trained(dev):
    dtype = F32
    # ops.linear
    M, K, N = 96, 128, 192
    x, W, b, g = rnd(M, K, seed=1), rnd(N, K, seed=2) * 0.1, rnd(N, seed=3), rnd(M, N, seed=5)

    def lin_run(holder, fp8):
        xd = x.clone().to(dev).requires_grad_(True)
        with ops.fp8_forward(fp8):
            y = ops.linear(xd, holder)
        (y * g.to(dev)).sum().backward()
        ops.flush_weight_grads()
        return y.detach(), xd.grad

    frozen = ops.FrozenLinear(W, b, dtype, dev)
    frozen.allow_fp8 = True
    t8, t0 = _own(_trainable_linear(W, b, dtype, dev), dev), _trainable_linear(W, b, dtype, dev)
    (y8, dx8), (yf, _), (y0, dx0) = lin_run(t8, True), lin_run(frozen, True), lin_run(t0, False)
    assert torch.equal(y8, yf) and not torch.equal(y8, y0)
    assert torch.equal(dx8, dx0) and torch.equal(t8.w_grad, t0.w_grad) and torch.equal(t8.bias_grad, t0.bias_grad)
    assert float(t8.w_grad.abs().max()) > 0
    # ops.conv2d: stride 1, stride 2, fused 2x upsample
    for B, H, Cin, Cout, stride, ups in ((2, 8, 64, 128, 1, 1), (1, 8, 128, 64, 2, 1), (2, 4, 64, 64, 1, 2)):
        xc, Wc, bc = rnd(B * H * H, Cin, seed=11), rnd(Cout, Cin, 3, 3, seed=12) * 0.05, rnd(Cout, seed=13)

        def conv_holder():
            w = Wc.permute(0, 2, 3, 1).contiguous().to(dev)
            c = ops.TrainableConv(w, torch.zeros_like(w), bc.to(dev), torch.zeros(Cout, device=dev), stride=stride, pad=1)
            c.refresh()
            return c

        def conv_run(holder, fp8):
            xd = xc.clone().to(dev).requires_grad_(True)
            with ops.fp8_forward(fp8):
                y = ops.conv2d(xd, holder, B, H, H, ups=ups)
            gc = rnd(*y.shape, seed=14).to(dev)
            (y * gc).sum().backward()
            ops.flush_weight_grads()
            return y.detach(), xd.grad

        fz = ops.FrozenConv(Wc, bc, dtype, dev, stride=stride, pad=1)
        fz.allow_fp8 = True
        c8, c0 = _own(conv_holder(), dev), conv_holder()
        (y8, dx8), (yf, _), (y0, dx0) = conv_run(c8, True), conv_run(fz, True), conv_run(c0, False)
        assert torch.equal(y8, yf) and not torch.equal(y8, y0), (stride, ups)
        assert torch.equal(dx8, dx0) and torch.equal(c8.w_grad, c0.w_grad) and torch.equal(c8.bias_grad, c0.bias_grad), (stride, ups)
    if dev.type == "cuda":
        torch.cuda.synchronize()


@pytest.mark.parametrize("case", [(F32, "jit"), (BF16, "jit"), (BF16, "delayed")], ids=["fp32-jit", "bf16-jit", "bf16-delayed"])
def test_geglu_pair_forward_of_the_frozen_backward_from_its_own_saved_tensors(dev, case):
    """The GEGLU feed-forward pair with bank-owned bytes.  Its backward reads the pre-activations and the GEGLU output its own forward
    saved, and under fp8 those are the quantised products' values, so the gradients cannot be those of the fp8-off pair (only db2, the
    column sums of g, is: bitwise).  The exact statements instead:
      * y and dx are bitwise those of the FROZEN pair under fp8 (both save the same pre-activations);
      * dW2 = g^T f and db2 = colsum g, dW1 = d pre^T x and db1 = colsum d pre, with f and pre those of the fp8 forward
        (ops._geglu_linear_fwd on the same holders) and d pre produced from them by the backward's own two kernels: held to fp64
        sums of those operands under helpers.check, the bound of every weight-gradient test;
      * bf16 under delayed scaling, where the GEMM epilogue emits `ff.net.2`'s bytes AND (for the trained pair) the bf16 product:
        every output and gradient is bitwise that of the two-launch form (ops.set_geglu_fused(False)), and the fused form
        quantises only x by a launch of its own."""
    from helpers import check
    dtype, scaling = case
    ops.set_fp8_scaling(scaling)
    M, K, D, N = 200, 128, 256, 128
    q = lambda t: t.to(dtype).float()
    x, W1, b1 = q(rnd(M, K, seed=21)), q(rnd(2 * D, K, seed=22) * 0.1), rnd(2 * D, seed=23) * 0.1
    W2, b2, g = q(rnd(N, D, seed=24) * 0.1), rnd(N, seed=25) * 0.1, q(rnd(M, N, seed=26))
    perm = ops.geglu_perm(2 * D)
    k = ops.kernels()

    def trained(own):
        a = _trainable_linear(W1[perm], b1[perm], dtype, dev, cls=ops.TrainableGegluLinear)
        c = _trainable_linear(W2, b2, dtype, dev)
        return (_own(a, dev), _own(c, dev)) if own else (a, c)

    def frozen():
        f1, f2 = ops.FrozenGegluLinear(W1, b1, dtype, dev), ops.FrozenLinear(W2, b2, dtype, dev)
        f1.allow_fp8 = f2.allow_fp8 = True
        return f1, f2

    def calibrate(pair):
        if scaling == "delayed":
            with ops.fp8_forward(True), torch.no_grad(), ops.fp8_calibration():
                ops.geglu_feed_forward(x.to(dev, dtype), *pair)

    def run(pair, fp8):
        xd = x.clone().to(dev, dtype).requires_grad_(True)
        with ops.fp8_forward(fp8):
            y = ops.geglu_feed_forward(xd, *pair, residual=xd)
        (y.float() * g.to(dev)).sum().backward()
        ops.flush_weight_grads()
        return y.detach().clone(), xd.grad.clone()

    p8, pf, p0, pu, pr = trained(True), frozen(), trained(False), trained(True), trained(True)
    for pair in (p8, pf, pu, pr):
        calibrate(pair)
    ops.fp8_end_of_step()
    n_scaled, orig = [0], k.fp8_quantize_scaled
    k.fp8_quantize_scaled = lambda *a_, **kw: (n_scaled.__setitem__(0, n_scaled[0] + 1), orig(*a_, **kw))[1]
    try:
        y8, dx8 = run(p8, True)
        n_fused = n_scaled[0]
        yf, dxf = run(pf, True)
        y0, dx0 = run(p0, False)
        ops.set_geglu_fused(False)
        n_scaled[0] = 0
        yu, dxu = run(pu, True)
        n_unfused = n_scaled[0]
    finally:
        ops.set_geglu_fused(True)
        del k.fp8_quantize_scaled
    assert torch.equal(y8, yf) and torch.equal(dx8, dxf), "the trained pair under fp8 differs from the frozen pair under fp8"
    assert not torch.equal(y8, y0) and torch.equal(p8[1].bias_grad, p0[1].bias_grad)
    # the two-launch form: the same bits everywhere (under delayed scaling the fused form's bytes come from the epilogue)
    assert torch.equal(y8, yu) and torch.equal(dx8, dxu)
    for a_, b_ in zip(p8, pu):
        assert torch.equal(a_.w_grad, b_.w_grad) and torch.equal(a_.bias_grad, b_.bias_grad)
    if scaling == "delayed":
        fused_path = dtype == BF16 and k.geglu_gemm_ok(x.to(dev, dtype), p8[0].w, M, 2 * D, K)
        assert (n_fused, n_unfused) == ((1, 2) if fused_path else (2, 2)), (n_fused, n_unfused)
    # the weight gradients from the tensors the fp8 forward saves
    with ops.fp8_forward(True), torch.no_grad():
        f, pre, _ = ops._geglu_linear_fwd(x.to(dev, dtype), pr[0], True, fp8_for=pr[1], keep_y=True)
    gd = g.to(dev, dtype)
    df, dpre = pre.new_empty((M, D)), torch.empty_like(pre)
    k.gemm(gd, pr[1].wt, df, M, D, N, N, N, D)
    k.geglu_il_bwd(df, pre, dpre, M, D)
    dd, xx, ff, gg = dpre.double().cpu(), x.double(), f.double().cpu(), gd.double().cpu()
    check(p8[1].w_grad, gg.t() @ ff, dtype, "dW2 = g^T f")
    check(p8[1].bias_grad, gg.sum(0), dtype, "db2 = colsum g")
    check(p8[0].w_grad, dd.t() @ xx, dtype, "dW1 = d pre^T x")
    check(p8[0].bias_grad, dd.sum(0), dtype, "db1 = colsum d pre")
    if dev.type == "cuda":
        torch.cuda.synchronize()


# ---- U4 -------------------------------------------------------------------------------------------------------------------------
def test_constructor_protocol(sim):
    ucfg, _, usd, _, (B, h, w, L), x, ctx, added, _ = _fp8_world(sim)
    plain_bank = UNetBank(ucfg, usd, F32, sim)
    with pytest.raises(ValueError, match="fp8"):
        UNet(ucfg, usd, F32, sim, fp8_forward=True, bank=plain_bank)
    k = ops.kernels()
    calls = []
    spies = {}
    for name in ("fp8_quantize", "fp8_quantize_scaled"):
        orig = getattr(k, name)
        spies[name] = orig
        setattr(k, name, (lambda o, nm: lambda *a, **kw: (calls.append(nm), o(*a, **kw))[1])(orig, name))
    try:
        bank = UNetBank(ucfg, usd, F32, sim, fp8=True)
        unet0 = UNet(ucfg, usd, F32, sim, bank=bank)  # no flag on an fp8 bank: allowed, never quantises, no slot
        with torch.no_grad():
            e0 = forward(unet0, sim, F32, x, ctx, added, B, h, w, L)
        assert calls == [] and len(bank._slot) == 0 and bank._plan.d_slots is None
        refreshes = []
        orig_q8 = k.weights_refresh_q8
        k.weights_refresh_q8 = lambda *a: (refreshes.append(1), orig_q8(*a))[1]
        unet8 = UNet(ucfg, usd, F32, sim, bank=bank, fp8_forward=True)
        n = len(bank._slot)
        assert n > 100 and calls == []  # no weight is quantised by the per-tensor kernels
        unet8b = UNet(ucfg, usd, F32, sim, bank=bank, fp8_forward=True)  # a second one: the same holders, no new slot
        assert len(bank._slot) == n and unet8b.conv_in is unet8.conv_in
        with torch.no_grad():
            e8 = forward(unet8, sim, F32, x, ctx, added, B, h, w, L)
            e8b = forward(unet8b, sim, F32, x, ctx, added, B, h, w, L)
            assert torch.equal(forward(unet0, sim, F32, x, ctx, added, B, h, w, L), e0)  # the plain UNet still reads no bytes
        assert len(refreshes) == 1 and torch.equal(e8, e8b) and not torch.equal(e8, e0)
        assert calls and set(calls) == {"fp8_quantize"}  # activations only (jit scaling)
        del k.weights_refresh_q8
    finally:
        for name in spies:
            delattr(k, name)
    lone = ops.TrainableLinear(torch.zeros(64, 64), torch.zeros(64, 64), None, None)
    lone.allow_fp8 = True
    with pytest.raises(RuntimeError, match="bank"):
        ops.fp8_weight(lone)
    with pytest.raises(RuntimeError, match="bank"), ops.fp8_forward(True):
        ops.linear(torch.zeros(4, 64), lone)
    # a fragment tuple quantises only the named layers
    bank2 = UNetBank(ucfg, usd, F32, sim, fp8=True)
    UNet(ucfg, usd, F32, sim, bank=bank2, fp8_forward=("ff.net",))
    assert bank2._slot and all("ff.net" in n_ for n_ in bank2._slot)
    # the tags live on the bank's holders: a second UNet may repeat the bank's selection or ask for none, not for another
    n2 = len(bank2._slot)
    UNet(ucfg, usd, F32, sim, bank=bank2, fp8_forward=("ff.net",))
    UNet(ucfg, usd, F32, sim, bank=bank2)
    for other in (True, ("attn",)):
        with pytest.raises(ValueError, match="fp8"):
            UNet(ucfg, usd, F32, sim, bank=bank2, fp8_forward=other)
    assert len(bank2._slot) == n2 and all("ff.net" in n_ for n_ in bank2._slot)
    assert all((getattr(h_, "_w8", None) is not None) == (n_ in bank2._slot) for n_, (_, h_) in bank2._made.items() if hasattr(h_, "w"))


# ---- U5 -------------------------------------------------------------------------------------------------------------------------
def test_every_parameter_gradient_against_emulation(dev):
    """Every parameter's gradient under the fp8 forward against the oracle's emulation (fp8=True: value of the quantised product,
    gradient of the unquantised one, for every leaf), root mean square over FP8_DRAWS inputs; the yardstick is the emulation's own
    distance to the exact network.  Factors: eps product-vs-emulation < 1.2 x, concatenated gradient < 1.5 x, product-vs-exact
    within a factor two of emulation-vs-exact both ways.
    Measured (rms over the 8 inputs; emulation-vs-exact, product-vs-exact, product-vs-emulation): simulator eps 0.180, 0.189, 0.135,
    gradient 0.282, 0.282, 0.183; MI355X eps 0.184, 0.185, 0.154, gradient 0.280, 0.271, 0.226.  First input on the CPU: 0.161 on
    eps and 0.262 on the gradient; 157 of the 174 matrices are eligible."""
    ucfg, ocfg, usd, _, (B, h, w, L), x, ctx, added, gout = _fp8_world(dev)
    bank = UNetBank(ucfg, usd, F32, dev, fp8=True)
    unet = UNet(ucfg, usd, F32, dev, bank=bank, fp8_forward=True)
    assert len(bank._slot) == 157

    def oracle(fp8, x, ctx, added):
        leaves = {k_: v.clone().requires_grad_(True) for k_, v in usd.items()}
        eps = O.unet_forward(leaves, ocfg, x, T, ctx, None, None, added, fp8=fp8)
        (eps * gout).sum().backward()
        assert all(v.grad is not None for v in leaves.values())
        return eps.detach(), oracle_vec(bank, {k_: v.grad for k_, v in leaves.items()})

    sq = np.zeros(6)
    for d in range(FP8_DRAWS):
        if d > 0:
            x, ctx = rnd(B, 4, h, w, seed=10 * d + 1), rnd(B, L, ucfg.cross_attention_dim, seed=10 * d + 2)
            added = (rnd(B, ucfg.pooled_dim, seed=10 * d + 3), added[1])
        e8, g8 = oracle(True, x, ctx, added)
        ex, gx = oracle(False, x, ctx, added)
        bank.zero_grad()
        e = forward(unet, dev, F32, x, ctx, added, B, h, w, L)
        (e * tok(gout).to(dev)).sum().backward()
        ops.flush_weight_grads()
        g = bank_vec(bank, bank.flat_grad)
        if d == 0:
            got = bank_grads(bank)
            assert all(float(v.abs().max()) > 0 for v in got.values()), "a parameter is left without a gradient"
        row = [rel_l2(tok(e8), tok(ex)), rel_l2(e, tok(ex)), rel_l2(e, tok(e8)), rel_l2(g8, gx), rel_l2(g, gx), rel_l2(g, g8)]
        print(f"fp8 full fine-tuning, input {d}: eps emulation-vs-exact {row[0]:.3e}, product-vs-exact {row[1]:.3e}, "
              f"product-vs-emulation {row[2]:.3e}; gradient {row[3]:.3e}, {row[4]:.3e}, {row[5]:.3e}")
        assert row[0] > 1e-2 and row[3] > 1e-2
        sq += np.array(row) ** 2
    eo, ep, em, go, gp, gm = np.sqrt(sq / FP8_DRAWS)
    print(f"fp8 full fine-tuning, rms over {FP8_DRAWS} inputs: eps {eo:.3e} {ep:.3e} {em:.3e}; gradient {go:.3e} {gp:.3e} {gm:.3e}")
    assert em < 1.2 * eo and 0.5 * eo < ep < 2.0 * eo
    assert gm < 1.5 * go and 0.5 * go < gp < 2.0 * go


# =================================================================================================================================
# The step: CoMatTrainer(pipe, ubank, ...) with the fp8 forward
# =================================================================================================================================
from comat_amd.blip import Blip  # noqa: E402
from comat_amd.gan import D_sd  # noqa: E402
from comat_amd.segments import SegmentedStep  # noqa: E402
from comat_amd.step import CoMatTrainer, GraphedStep  # noqa: E402
from comat_amd.unet import LoRABank, VAEDecoder  # noqa: E402
from oracle import step as OS  # noqa: E402

import test_tune_vae as TV  # noqa: E402
from comat_amd.pipeline import TrainableSDPipeline  # noqa: E402
from helpers import tiny_weights  # noqa: E402

TS, CROP = TV.TS, TV.CROP
# the generator of the step tests: TINY_UNET with the channels of FP8_UNET, so that the contraction length of every block layer but the
# text key / value projections (the world's 24-wide prompt embeddings) is a multiple of 64
STEP_UNET = dataclasses.replace(config.TINY_UNET, block_out_channels=FP8_UNET.block_out_channels)


def fp8_step_world(dtype, dev, gan=True, **cfg_kw):
    """the world of tests/test_full_finetuning.make_step_world - the configuration, batch, VAE, BLIP and discriminator of
    tests/test_tune_vae.make_inputs, unchanged - with a generator that has fp8-eligible layers (STEP_UNET): UNetBank(fp8=True),
    UNet(bank=bank, fp8_forward=True), CoMatTrainer(pipe, ubank, ...) -> (cfg, batch, oracle_world(fp8) -> W, trainer)"""
    cfg, batch, W0, (tcfg, _, vsd, _, bsd, dsd, dl, head_w, head_b) = TV.make_inputs(dtype, False, gan, full_finetuning=True, **cfg_kw)
    usd = tiny_weights(dtype, STEP_UNET)[0]

    def oracle_world(fp8):
        W = dict(W0, unet={k_: v.clone().requires_grad_(True) for k_, v in usd.items()}, lora={}, fp8_unet=fp8,
                 ucfg=O.UNetConfig(**dataclasses.asdict(STEP_UNET)), d_ucfg=O.UNetConfig(**dataclasses.asdict(tcfg)))
        for k_ in ("d_lora", "head_w", "head_b"):
            W[k_] = ({n: v.detach().clone().requires_grad_(True) for n, v in W0[k_].items()} if isinstance(W0[k_], dict)
                     else W0[k_].detach().clone().requires_grad_(True))
        return W
    bank = UNetBank(STEP_UNET, usd, dtype, dev, fp8=True)
    pipe = TrainableSDPipeline(UNet(STEP_UNET, usd, dtype, dev, bank=bank, fp8_forward=True), VAEDecoder(config.TINY_VAE, vsd, dtype, dev))
    dbank = LoRABank(tcfg, dl, dtype, dev)
    disc = D_sd(UNet(tcfg, dsd, dtype, dev, dbank), dbank, head_w, head_b)
    trainer = CoMatTrainer(pipe, bank, Blip(config.TINY_BLIP, bsd, dtype, dev), disc, cfg, seed=0)
    return cfg, batch, oracle_world, trainer


_ORACLE = {}


def oracle_terms(dtype, oracle_world, batch, cfg):
    """the oracle's losses and UNet gradient with and without its fp8 emulation; once per dtype of the weights, never written"""
    if dtype not in _ORACLE:
        res = {}
        for fp8 in (True, False):
            W = oracle_world(fp8)
            out = OS.g_loss_terms(W, batch, cfg, TS, CROP)
            out["loss"].backward()
            assert all(v.grad is not None for v in W["unet"].values())
            res[fp8] = dict(out={k_: float(out[k_].detach()) for k_ in ("Blip", "G_loss", "loss")}, g={k_: v.grad for k_, v in W["unet"].items()})
        _ORACLE[dtype] = res
    return _ORACLE[dtype]


# ---- U6 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaling", ["delayed", "jit"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_step_against_oracle_emulation(dev, dtype, scaling):
    """One whole step, every UNet parameter trained, forward on fp8: losses and the UNet gradient against the oracle step with its
    fp8 emulation.  Bound: the form and constants of tests/test_fp8.test_fp8_step_against_oracle_emulation - every loss term
    within 1.5 x the emulation's own distance to the exact step (+ 5e-3 of its scale; bf16 storage: + 0.1), the gradient within
    1.5 x the emulation-vs-exact gradient distance (bf16 storage: + BF16_UNET_GRAD_LIMIT).  After the step the bank's bytes and
    scales are the oracle quantiser's on the UPDATED weights: the refresh ran behind the optimizer.
    World: that of tests/test_full_finetuning.make_step_world (batch 2, SD1.5 layout, GAN loss on) with the generator STEP_UNET.
    Measured on the simulator (CPU), gradient product-vs-emulation / emulation-vs-exact: fp32 delayed 0.870 / 0.696, jit 0.743 /
    0.696; bf16 delayed 0.854 / 0.864, jit 0.729 / 0.864.  The tightest loss term is G_loss in fp32 under delayed scaling: product
    0.71706, emulation 0.71143, exact 0.70957 - 0.0056 against a bound of 1.5 x 0.0019 + 5e-3 = 0.0078.  MI355X: fp32
    delayed 0.906 / 0.768, jit 0.943 / 0.768; bf16 delayed 0.775 / 0.779, jit 0.816 / 0.779; tightest loss term there: the reward in
    fp32 under jit scaling, product -4.48282, emulation -4.45911, exact -4.45715 - 0.0237 against 1.5 x 0.0020 + 5e-3 x 4.459 = 0.0252."""
    ops.set_fp8_scaling(scaling)
    cfg, batch, oracle_world, trainer = fp8_step_world(dtype, dev)
    ref = oracle_terms(dtype, oracle_world, batch, cfg)
    bank = trainer.bank
    if scaling == "delayed":
        assert trainer.fp8_calibrate(batch)
    p0 = bank.flat.clone()
    logs = trainer.train_step(batch, training_steps=TS, crop=CROP)
    g8, gx = oracle_vec(bank, ref[True]["g"]), oracle_vec(bank, ref[False]["g"])
    own = rel_l2(g8, gx)
    got = rel_l2(bank_vec(bank, bank.flat_grad), g8)
    line = [f"fp8 full fine-tuning step ({dtype}, {scaling}, {dev.type}): grads emulation-vs-exact {own:.3e}, product-vs-emulation {got:.3e}"]
    slack = 0.0 if dtype == F32 else BF16_UNET_GRAD_LIMIT
    for key, rk in (("Blip", "Blip"), ("G_loss", "G_loss"), ("step_loss", "loss")):
        a, b8, bx = float(logs[key]), ref[True]["out"][rk], ref[False]["out"][rk]
        line.append(f"{key}: product {a:.5f} emulation {b8:.5f} exact {bx:.5f}")
    print("\n".join(line))
    assert own > 1e-3 and got < 1.5 * own + slack, line
    for key, rk in (("Blip", "Blip"), ("G_loss", "G_loss"), ("step_loss", "loss")):
        a, b8, bx = float(logs[key]), ref[True]["out"][rk], ref[False]["out"][rk]
        assert abs(a - b8) <= 1.5 * abs(b8 - bx) + (5e-3 if dtype == F32 else 1e-1) * max(1.0, abs(b8)), line
    assert not torch.equal(bank.flat, p0) and bank._fresh
    assert check_bank_bytes(bank, "after the step") == len(bank._slot) > 100


# ---- U7 -------------------------------------------------------------------------------------------------------------------------
def test_gradient_checkpointing_same_bits(dev):
    ops.set_fp8_scaling("delayed")
    _, batch, _, plain = fp8_step_world(F32, dev, gan=False)
    plain.pipe.share_text_kv = False
    assert plain.fp8_calibrate(batch)
    la = plain.train_step(batch, training_steps=TS, crop=CROP)
    res = (la["step_loss"].clone(), plain.bank.flat_grad.clone(), plain.bank.flat.clone())
    ops.fp8_reset()
    _, batch2, _, ck = fp8_step_world(F32, dev, gan=False, gradient_checkpointing=True)
    assert ck.fp8_calibrate(batch2)
    lb = ck.train_step(batch2, training_steps=TS, crop=CROP)
    assert torch.equal(res[0], lb["step_loss"])
    assert torch.equal(res[1], ck.bank.flat_grad)
    assert torch.equal(res[2], ck.bank.flat)


# ---- U8 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_segmented_step_matches_eager(hip):
    """three calls of SegmentedStep = three eager steps, bit for bit, on master, moments, bytes and scales; bf16, delayed scaling,
    calibrated before the first capture.  (Two worlds in one process: each has its own activation sites in the device's table.)"""
    ops.set_fp8_scaling("delayed")
    _, batch, _, eager = fp8_step_world(BF16, hip)
    _, batch2, _, tr = fp8_step_world(BF16, hip)
    assert GraphedStep(tr).supported(batch2) is False
    eager.pipe.share_text_kv = False
    assert eager.fp8_calibrate(batch) and tr.fp8_calibrate(batch2)
    stepper = SegmentedStep(tr)
    for i in range(3):
        eager.train_step(batch, training_steps=TS, crop=CROP)
        stepper(batch2, training_steps=TS, crop=CROP)
        torch.cuda.synchronize()
        assert stepper.failed is None, stepper.failed
        assert torch.equal(eager.bank.flat, tr.bank.flat), i
        assert torch.equal(eager.opt.m[0], tr.opt.m[0]) and torch.equal(eager.opt.v[0], tr.opt.v[0]), i
        n = len(tr.bank._slot)
        assert torch.equal(eager.bank.flat_q8, tr.bank.flat_q8) and torch.equal(eager.bank.w_scale[:n], tr.bank.w_scale[:n]), i


# ---- U9 -------------------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip(sim, tmp_path):
    """weight scales are derived state: not saved; load -> mark_updated -> the next refresh restores bytes and scales, and with the
    activation sites' state (fp8_device=) the next step's logs are the uninterrupted run's"""
    ops.set_fp8_scaling("delayed")
    d = str(tmp_path)
    _, batch, _, tr = fp8_step_world(F32, sim, gan=False)
    assert tr.fp8_calibrate(batch)
    tr.train_step(batch, training_steps=TS, crop=CROP)
    checkpoint.save_checkpoint(d, tr.bank, fp8_device=sim, optim=dict(G=tr.opt))
    saved = {k_: set(v.keys()) if isinstance(v, dict) else None for k_, v in
             ((f, torch.load(str(tmp_path / f), map_location="cpu")) for f in ("unet.pt", "fp8_state.pt"))}
    assert not any("w_scale" in k_ or "q8" in k_ for keys in saved.values() if keys for k_ in keys)
    n = len(tr.bank._slot)
    want_q, want_s = tr.bank.flat_q8.clone(), tr.bank.w_scale[:n].clone()
    logs = tr.train_step(batch, training_steps=TS, crop=CROP)
    want = {k_: logs[k_].clone() for k_ in ("Blip", "step_loss")}
    want_flat = tr.bank.flat.clone()
    ops.fp8_reset()
    _, batch2, _, fresh = fp8_step_world(F32, sim, gan=False)
    checkpoint.load_checkpoint(d, fresh.bank, fp8_device=sim, optim=dict(G=fresh.opt))
    assert not fresh.bank._fresh
    fresh.bank.ensure_compute_copy()
    assert torch.equal(fresh.bank.flat_q8, want_q) and torch.equal(fresh.bank.w_scale[:n], want_s)
    logs2 = fresh.train_step(batch2, training_steps=TS, crop=CROP)
    for k_ in want:
        assert torch.equal(logs2[k_], want[k_]), k_
    assert torch.equal(fresh.bank.flat, want_flat)
