"""comat_denoise_prepare, comat_mse_fwd and comat_mse_bwd (include/comat_hip.h) on the simulator (tests/denoise_sim.py) and on the real
kernels, entry point by entry point.

What is held without a tolerance: the noised UNet input against comat_add_noise_fwd of the SAME backend (called per sample with that
sample's coefficients), the table rows, `scaling * mean`, the MSE of integer operands, the bf16 gradient as the once-rounded fp32
one, two runs against each other.  What is held under a bound worked out from the arithmetic, not from the code under test: the
sampled latent against float64 (8 * 2^-24: 4 ulp for expf, one rounding for each of the four other operations), the per-sample MSE
(n * 2^-24 relative: any summation order of n non-negative once-rounded terms), the loss ((B + 2) * 2^-24 on top) and the fp32
gradient (4 * 2^-24 relative per element).  References are computed HERE, not by the simulator.  Operands are windowed
(helpers.Window): NaN all around the inputs, armed guard bands around every output."""
import ctypes as C

import numpy as np
import pytest
import torch

from comat_amd import _hip, ops
from denoise_sim import DenoiseSimKernels, denoise_dev, sim_matches_binding  # noqa: F401 - fixture
from helpers import Window

f32 = np.float32
U = 2.0 ** -24
T = 11  # rows of the tables
SCALING = 0.18215
DT = [torch.float32, torch.bfloat16]
ids_dt = lambda d: "fp32" if d == torch.float32 else "bf16"


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def tables(C0, seed=0):
    g = gen(seed)
    sab = torch.rand(T, 2, generator=g) * 0.98 + 0.01
    return sab, torch.randn(T, C0, generator=g), torch.rand(T, generator=g) + 0.25


def run_prepare(dev, B, P, Cn, C0, tvec, xdt, mdt, mode, m_off=0, seed=0, want=True):
    """one call on windowed operands.  mode: 'latents', 'mean' (moments, z = NULL) or 'sample'.  -> dict of host tensors"""
    g = gen(seed + 17 * B + P)
    n = B * P
    sab, sinus, wtab = tables(C0, seed)
    mom = torch.cat([torch.randn(n, Cn, generator=g), torch.rand(n, Cn, generator=g) * 8 - 6], dim=1).to(mdt)
    if mode == "sample" and n * Cn >= 4:  # both clamps act
        mom[0, Cn], mom[-1, 2 * Cn - 1] = -40.0, 25.0
    z, lat, noise = (torch.randn(n, Cn, generator=g) for _ in range(3))
    W = lambda rows, cols, dt=torch.float32, left=8: Window(rows, cols, dtype=dt, device=dev, left=left)
    mw = W(n, 2 * Cn, mdt, 8 + m_off).put(mom)
    zw, lw, nw = W(n, Cn).put(z), W(n, Cn).put(lat), W(n, Cn).put(noise)
    sw, iw, ww = W(T, 2).put(sab), W(T, C0).put(sinus), W(1, T).put(wtab)
    tw = W(1, B, torch.int32).put(torch.tensor(tvec, dtype=torch.int32))
    xw, x0w, ew, pw = W(n, Cn, xdt).arm(), W(n, Cn).arm(), W(B, C0).arm(), W(1, B).arm()
    ow = W(1, 1, torch.int32)
    ow.flat.zero_()
    ow.arm()
    ops.denoise_kernels().denoise_prepare(mw.view if mode != "latents" else None, zw.view if mode == "sample" else None,
                                          lw.view if mode == "latents" else None, nw.view, tw.flat, sw.view, iw.view, ww.flat, xw.view,
                                          x0w.view if want else None, ew.view, pw.flat, ow.flat if want else None, SCALING, T, B, P,
                                          Cn, C0)
    sync(dev)
    for win, what in ((xw, "xin"), (x0w, "x0"), (ew, "temb"), (pw, "w"), (ow, "oob")):
        win.assert_guard_intact(what)
    out = dict(xin=xw.get().cpu(), temb=ew.get().cpu(), w=pw.flat.clone().cpu(), oob=int(ow.flat.cpu()[0]), mom=mom.float(), z=z,
               lat=lat, noise=noise, sab=sab, sinus=sinus, wtab=wtab)
    if want:
        x0w.assert_written("x0")
        out["x0"] = x0w.get().cpu()
    else:
        assert bool(torch.isnan(x0w.view).all()), "x0 = NULL was written"
    return out


def add_noise_bits(dev, x0, noise, sa, sb, xdt):
    """comat_add_noise_fwd (copies 1) of the installed backend on one sample -> xin on the host"""
    x, nz = x0.reshape(-1).to(dev).contiguous(), noise.reshape(-1).to(dev).contiguous()
    noisy, xin = torch.empty_like(x), torch.empty(x.numel(), dtype=xdt, device=dev)
    ops.kernels().add_noise_fwd(x, nz, noisy, xin, x.numel(), sa, sb, 1)
    sync(dev)
    return xin.cpu()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def check_prepare(dev, r, B, P, Cn, tvec, xdt, mode):
    tc = [min(max(t, 0), T - 1) for t in tvec]
    assert r["oob"] == int(any(t != c for t, c in zip(tvec, tc))), (tvec, r["oob"])
    assert torch.equal(bits(r["temb"]), bits(r["sinus"][tc])), "temb is not the table's rows"
    assert torch.equal(bits(r["w"]), bits(r["wtab"][tc])), "w is not the table's entries"
    mean, lv = r["mom"][:, :Cn], r["mom"][:, Cn:]
    if mode == "latents":
        assert torch.equal(bits(r["x0"]), bits(r["lat"]))
    elif mode == "mean":
        want = torch.from_numpy((f32(SCALING) * mean.numpy()).astype(f32))
        assert torch.equal(bits(r["x0"]), bits(want)), "scaling * mean is not one rounding"
    else:
        std = torch.exp(0.5 * lv.double().clamp(-30, 20))
        ref = SCALING * (mean.double() + std * r["z"].double())
        bound = 8 * U * SCALING * (mean.double().abs() + (std * r["z"].double()).abs())
        err = (r["x0"].double() - ref).abs()
        worst = float((err / bound).max())
        print(f"posterior: worst |x0 - ref| / (2^-24 scaling (|mean| + |std z|)) = {8 * worst:.3f} (allowed 8)")
        assert bool((err <= bound).all()), f"posterior beyond the bound: worst ratio {8 * worst:.3f} of 8"
    for b in range(B):  # the noising: comat_add_noise_fwd's bits, sample by sample with that sample's coefficients
        sl = slice(b * P, (b + 1) * P)
        sa, sb = float(r["sab"][tc[b], 0]), float(r["sab"][tc[b], 1])
        want = add_noise_bits(dev, r["x0"][sl], r["noise"][sl], sa, sb, xdt)
        assert torch.equal(bits(r["xin"][sl].reshape(-1)), bits(want)), f"sample {b}: xin differs from comat_add_noise_fwd's bits"


TVECS = {1: [(0,), (T - 1,), (T + 7,)], 3: [(0, T - 1, T - 1), (4, 4, 4), (3, -1, 3), (T, 0, 5)]}


@pytest.mark.parametrize("mdt", DT, ids=lambda d: "m" + ids_dt(d))
@pytest.mark.parametrize("xdt", DT, ids=lambda d: "x" + ids_dt(d))
@pytest.mark.parametrize("P", [1, 5, 257, 1025])
@pytest.mark.parametrize("B", [1, 3])
def test_prepare_shapes_and_contracts(denoise_dev, B, P, xdt, mdt):
    """P * C = 4 (one vector), 20 (a ragged block), 4 * 257 (just past one block) and 4 * 1024 + 4 (past several); timesteps 0, T - 1,
    equal ones, all equal, one out of range on either side"""
    k = 0
    for C0 in (32, 320):
        for mode in ("latents", "mean", "sample"):
            tvec = TVECS[B][k % len(TVECS[B])]
            k += 1
            r = run_prepare(denoise_dev, B, P, 4, C0, tvec, xdt, mdt, mode, seed=k)
            check_prepare(denoise_dev, r, B, P, 4, tvec, xdt, mode)


@pytest.mark.parametrize("B", [1, 3])
def test_prepare_every_timestep_vector(denoise_dev, B):
    for tvec in TVECS[B]:
        for mode in ("latents", "sample"):
            r = run_prepare(denoise_dev, B, 5, 4, 32, tvec, torch.float32, torch.float32, mode)
            check_prepare(denoise_dev, r, B, 5, 4, tvec, torch.float32, mode)


def test_prepare_out_of_range_changes_nothing_else(denoise_dev):
    """t = T + 7 reads row T - 1 and t = -1 row 0; the samples in range have the bits of a call whose vector is in range"""
    a = run_prepare(denoise_dev, 3, 257, 4, 32, (T + 7, 2, -1), torch.bfloat16, torch.float32, "sample")
    b = run_prepare(denoise_dev, 3, 257, 4, 32, (T - 1, 2, 0), torch.bfloat16, torch.float32, "sample")
    assert (a["oob"], b["oob"]) == (1, 0)
    for key in ("xin", "x0", "temb", "w"):
        assert torch.equal(bits(a[key]), bits(b[key])), key


@pytest.mark.parametrize("mdt", DT, ids=ids_dt)
@pytest.mark.parametrize("case", ["moments one element off", "three channels"])
def test_prepare_element_path_has_the_vector_paths_bits(denoise_dev, case, mdt):
    """a moments base that is not 16-byte aligned, and a channel count that is no multiple of 4, take the element accesses"""
    B, P, tvec = 3, 257, (0, T - 1, 6)
    for mode in ("mean", "sample"):
        for xdt in DT:
            if case == "three channels":
                r = run_prepare(denoise_dev, B, P, 3, 32, tvec, xdt, mdt, mode)
                check_prepare(denoise_dev, r, B, P, 3, tvec, xdt, mode)
            else:
                r = run_prepare(denoise_dev, B, P, 4, 32, tvec, xdt, mdt, mode, m_off=1)
                check_prepare(denoise_dev, r, B, P, 4, tvec, xdt, mode)
                v = run_prepare(denoise_dev, B, P, 4, 32, tvec, xdt, mdt, mode)
                assert torch.equal(bits(r["xin"]), bits(v["xin"])) and torch.equal(bits(r["x0"]), bits(v["x0"]))


def test_prepare_optional_outputs_and_nonfinite(denoise_dev):
    """x0 = NULL and oob = NULL are taken and nothing is stored there; a NaN logvar and an Inf mean stay where they are"""
    r = run_prepare(denoise_dev, 3, 5, 4, 32, (1, T + 1, 2), torch.float32, torch.bfloat16, "sample", want=False)
    full = run_prepare(denoise_dev, 3, 5, 4, 32, (1, T + 1, 2), torch.float32, torch.bfloat16, "sample")
    assert torch.equal(bits(r["xin"]), bits(full["xin"])) and r["oob"] == 0 and full["oob"] == 1
    dev = denoise_dev
    sab, sinus, wtab = (a.to(dev) for a in tables(32))
    mom = torch.zeros(8, 8)
    mom[2, 4], mom[5, 1] = float("nan"), float("inf")  # a logvar of pixel 2, a mean of pixel 5
    z = torch.ones(8, 4)
    xin, x0 = torch.empty(8, 4, device=dev), torch.empty(8, 4, device=dev)
    temb, w = torch.empty(2, 32, device=dev), torch.empty(2, device=dev)
    ops.denoise_kernels().denoise_prepare(mom.to(dev), z.to(dev), None, z.to(dev), torch.tensor([1, 2], dtype=torch.int32, device=dev),
                                          sab, sinus, wtab, xin, x0, temb, w, None, 1.0, T, 2, 4, 4, 32)
    sync(dev)
    bad = ~torch.isfinite(xin.cpu())
    want = torch.zeros(8, 4, dtype=torch.bool)
    want[2, 0] = want[5, 1] = True
    assert torch.equal(bad, want) and torch.equal(~torch.isfinite(x0.cpu()), want)


PREPARE_BAD = [(dict(moments=None), "exactly one"), (dict(latents="LAT"), "exactly one"), (dict(moments=None, latents="LAT"), "z goes with moments"),
               (dict(noise=None), "null pointer"), (dict(t=None), "null pointer"), (dict(sab=None), "null pointer"),
               (dict(sinus=None), "null pointer"), (dict(wtab=None), "null pointer"), (dict(xin=None), "null pointer"),
               (dict(temb=None), "null pointer"), (dict(w=None), "null pointer"), (dict(B=0), "bad shape"), (dict(P=0), "bad shape"),
               (dict(C=-4), "bad shape"), (dict(C0=0), "bad shape"), (dict(T=0), "bad shape"), (dict(B=65536), "65535"),
               (dict(P=2 ** 30), "beyond 2")]


def test_prepare_bad_arguments_are_refused_by_name(denoise_dev):
    dev = denoise_dev
    B, P, Cn, C0 = 2, 3, 4, 8
    sab, sinus, wtab = (a.to(dev) for a in tables(C0))
    f = lambda *s: torch.zeros(*s, device=dev)
    lat = f(B * P, Cn)
    good = dict(moments=f(B * P, 2 * Cn), z=f(B * P, Cn), latents=None, noise=f(B * P, Cn), t=torch.zeros(B, dtype=torch.int32, device=dev),
                sab=sab, sinus=sinus, wtab=wtab, xin=torch.full((B * P, Cn), 7.0, device=dev), x0=None, temb=f(B, C0), w=f(B), oob=None,
                scaling=1.0, T=T, B=B, P=P, C=Cn, C0=C0)
    call = ops.denoise_kernels().denoise_prepare
    swap = lambda d: {k: (lat if isinstance(v, str) else v) for k, v in d.items()}
    for change, words in PREPARE_BAD + [(dict(moments=good["moments"].half()), "bad dtype"), (dict(xin=good["xin"].half()), "bad dtype")]:
        with pytest.raises(RuntimeError, match=f"comat_denoise_prepare.*{words}"):
            call(**{**good, **swap(change)})
    sync(dev)
    assert bool((good["xin"] == 7.0).all()), "a refused call wrote"
    call(**good)
    call(**{**good, "moments": None, "z": None, "latents": lat})
    sync(dev)


def test_library_refuses_without_launching():
    """the cross-compiled library's own checks, without a GPU (as tests/test_image_u8.py)"""
    lib = _hip.load_library()
    buf = C.create_string_buffer(4096)
    p = C.addressof(buf)
    good = dict(moments=p, z=p, latents=None, noise=p, t=p, sab=p, sinus=p, wtab=p, xin=p, x0=None, temb=p, w=p, oob=None, scaling=1.0,
                T=T, B=2, P=3, C=4, C0=8, moments_dtype=_hip.F32, xin_dtype=_hip.BF16, stream=None)
    swap = lambda d: {k: (p if isinstance(v, str) else v) for k, v in d.items()}
    for change, words in PREPARE_BAD + [(dict(moments_dtype=_hip.FP8), "bad dtype"), (dict(xin_dtype=-1), "bad dtype")]:
        assert lib.comat_denoise_prepare(*{**good, **swap(change)}.values()) == -1, change
        msg = lib.comat_last_error().decode()
        assert "comat_denoise_prepare" in msg and words in msg, (change, msg)
    fwd = dict(pred=p, target=p, w=None, per_sample=p, loss=p, B=2, n=8, dtype=_hip.F32, stream=None)
    bwd = dict(pred=p, target=p, w=None, g=None, dpred=p, B=2, n=8, dtype=_hip.BF16, stream=None)
    for fn, good, nulls in ((lib.comat_mse_fwd, fwd, ("pred", "target", "per_sample", "loss")),
                            (lib.comat_mse_bwd, bwd, ("pred", "target", "dpred"))):
        cases = [({k: None}, "null pointer") for k in nulls] + [(dict(B=0), "bad shape"), (dict(n=0), "bad shape"), (dict(n=-1), "bad shape"),
                                                              (dict(B=65536), "65535"), (dict(dtype=_hip.FP8), "bad dtype")]
        for change, words in cases:
            assert fn(*{**good, **change}.values()) == -1, change
            msg = lib.comat_last_error().decode()
            assert fn.__name__ in msg and words in msg, (change, msg)
    assert buf.raw == bytes(4096)


# ---- the MSE pair ----------------------------------------------------------------------------------------------------------------
def run_mse(dev, pred, target, w=None, g=None, left=8):
    """pred [B, n] of its dtype, target fp32 - windowed; -> (per_sample, loss, dpred) on the host"""
    B, n = pred.shape
    Wn = lambda rows, cols, dt=torch.float32, lf=8: Window(rows, cols, dtype=dt, device=dev, left=lf)
    pw, tw = Wn(B, n, pred.dtype, left).put(pred), Wn(B, n).put(target)
    ww = None if w is None else Wn(1, B).put(w)
    gw = None if g is None else Wn(1, 1).put(torch.tensor([g]))
    sw, lw, dw = Wn(1, B).arm(), Wn(1, 1).arm(), Wn(B, n, pred.dtype, left).arm()
    k = ops.denoise_kernels()
    k.mse_fwd(pw.view, tw.view, None if ww is None else ww.flat, sw.flat, lw.flat, B, n)
    k.mse_bwd(pw.view, tw.view, None if ww is None else ww.flat, None if gw is None else gw.flat, dw.view, B, n)
    sync(dev)
    for win, what in ((sw, "per_sample"), (lw, "loss"), (dw, "dpred")):
        win.assert_guard_intact(what)
    return sw.flat.clone().cpu(), lw.flat.clone().cpu(), dw.get().cpu()


def draw_mse(B, n, dtype, seed):
    g = gen(seed)
    return (torch.randn(B, n, generator=g) * 1.5).to(dtype), torch.randn(B, n, generator=g), torch.rand(B, generator=g) * 1.9 + 0.1


@pytest.mark.parametrize("dtype", DT, ids=ids_dt)
@pytest.mark.parametrize("n", [1, 4, 1000, 4100])
@pytest.mark.parametrize("B", [1, 3, 4])
def test_mse_against_float64(denoise_dev, B, n, dtype):
    pred, target, w = draw_mse(B, n, dtype, seed=B * 10000 + n)
    d64 = pred.double() - target.double()
    ps_ref = (d64 * d64).mean(dim=1)
    for wv, g in ((None, None), (w, None), (w, 0.75)):
        ps, loss, dp = run_mse(denoise_dev, pred, target, wv, g)
        wd = torch.ones(B, dtype=torch.float64) if wv is None else wv.double()
        err = (ps.double() - ps_ref).abs()
        print(f"B {B} n {n} {ids_dt(dtype)}: per_sample worst |err| / (2^-24 ref) = {float((err / (U * ps_ref)).max()):.3f} (allowed {n})")
        assert bool((err <= n * U * ps_ref).all()), "per_sample beyond n * 2^-24"
        loss_ref = float((wd * ps_ref).mean())
        assert abs(float(loss.double()) - loss_ref) <= (n + B + 2) * U * loss_ref, (float(loss), loss_ref)
        ref = (1.0 if g is None else g) * wd[:, None] * (2.0 / (B * n)) * d64
        ps32, _, dp32 = run_mse(denoise_dev, pred.float(), target, wv, g)
        assert bool(((dp32.double() - ref).abs() <= 4 * U * ref.abs()).all()), "fp32 gradient beyond 4 * 2^-24 per element"
        if dtype == torch.bfloat16:  # the fp32 value rounded once
            assert torch.equal(bits(dp), bits(dp32.to(torch.bfloat16))) and torch.equal(bits(ps), bits(ps32))
        again = run_mse(denoise_dev, pred, target, wv, g)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip((ps, loss, dp), again)), "two runs differ"
        off = run_mse(denoise_dev, pred, target, wv, g, left=9)  # the element path: the same order, the same bits
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip((ps, loss, dp), off)), "the element path gives other bits"


@pytest.mark.parametrize("dtype", DT, ids=ids_dt)
@pytest.mark.parametrize("n", [4, 1024, 8192])
@pytest.mark.parametrize("B", [1, 2, 4])
def test_mse_of_integers_is_exact(denoise_dev, B, n, dtype):
    """integer pred and target in [-8, 8], B and n powers of two, w = 1: every partial sum is an integer below 2^24 and every
    quotient a power of two away from one - per_sample, loss and the gradient are the exact values, bit for bit"""
    g = gen(B + n)
    pred = torch.randint(-8, 9, (B, n), generator=g).to(dtype)
    target = torch.randint(-8, 9, (B, n), generator=g).float()
    d64 = pred.double() - target.double()
    assert float((d64 * d64).sum(dim=1).max()) < 2 ** 24
    for wv in (None, torch.ones(B)):
        ps, loss, dp = run_mse(denoise_dev, pred, target, wv)
        assert torch.equal(ps.double(), (d64 * d64).mean(dim=1))
        assert float(loss.double()) == float((d64 * d64).mean())
        assert dp.dtype == dtype and torch.equal(dp.double(), d64 * (2.0 / (B * n)))


@pytest.mark.parametrize("dtype", DT, ids=ids_dt)
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_mse_nonfinite_stays_in_its_sample(denoise_dev, value, dtype):
    B, n = 3, 1000
    pred, target, w = draw_mse(B, n, dtype, seed=5)
    clean = run_mse(denoise_dev, pred, target, w)
    pred[1, 333] = value
    ps, loss, dp = run_mse(denoise_dev, pred, target, w)
    assert not bool(torch.isfinite(ps[1])) and not bool(torch.isfinite(loss[0])) and not bool(torch.isfinite(dp[1, 333].float()))
    keep = torch.ones(B, n, dtype=torch.bool)
    keep[1, 333] = False
    assert torch.equal(bits(ps[[0, 2]]), bits(clean[0][[0, 2]])), "another sample's per_sample changed"
    assert torch.equal(bits(dp)[keep], bits(clean[2])[keep]), "another gradient element changed"


def test_mse_bad_arguments_are_refused_by_name(denoise_dev):
    dev = denoise_dev
    f = lambda *s: torch.zeros(*s, device=dev)
    k = ops.denoise_kernels()
    fwd = dict(pred=f(2, 8), target=f(2, 8), w=None, per_sample=f(2), loss=f(1), B=2, n=8)
    bwd = dict(pred=f(2, 8), target=f(2, 8), w=None, g=None, dpred=f(2, 8), B=2, n=8)
    for fn, name, good in ((k.mse_fwd, "comat_mse_fwd", fwd), (k.mse_bwd, "comat_mse_bwd", bwd)):
        ptrs = [a for a in good if a not in ("w", "g", "B", "n")]
        half = {"pred": good["pred"].half()} if "dpred" not in good else {"pred": good["pred"].half(), "dpred": good["dpred"].half()}
        for change, words in [({a: None}, "null pointer") for a in ptrs] + [(dict(B=0), "bad shape"), (dict(n=0), "bad shape"),
                                                                         (dict(B=65536), "65535"), (half, "bad dtype")]:
            with pytest.raises(RuntimeError, match=f"{name}.*{words}"):
                fn(**{**good, **change})
        fn(**good)
    sync(dev)


def test_launch_counts_on_the_simulators_log(sim):
    k = DenoiseSimKernels()
    ops.set_kernel_backend(k)
    r = run_prepare(sim, 3, 5, 4, 32, (0, 1, 2), torch.float32, torch.float32, "sample")
    assert r["oob"] == 0
    pred, target, w = draw_mse(3, 20, torch.float32, seed=1)
    run_mse(sim, pred, target, w)
    count = lambda name: [c for n_, c in k.launches if n_ == name]
    assert count("comat_denoise_prepare") == [1] and count("comat_mse_bwd") == [1]
    assert len(count("comat_mse_fwd")) == 1 and count("comat_mse_fwd")[0] <= 2


def test_the_operator(denoise_dev):
    """ops.mse_loss under autograd against F.mse_loss; the upstream gradient is read on the device"""
    dev = denoise_dev
    pred, target, w = draw_mse(3, 40, torch.float32, seed=3)
    p = pred.clone().to(dev).requires_grad_(True)
    loss, ps = ops.mse_loss(p.reshape(30, 4), target.to(dev).reshape(30, 4), 3, w.to(dev))
    (loss * 0.5).sum().backward()
    pr = pred.detach().double().requires_grad_(True)
    ref = (((pr - target.double()) ** 2).mean(dim=1) * w.double()).mean()
    (ref * 0.5).backward()
    assert abs(float(loss.detach()) - float(ref.detach())) < 1e-6 * float(ref.detach()) and not ps.requires_grad
    assert float((p.grad.cpu().double() - pr.grad).abs().max()) <= 1e-6 * float(pr.grad.abs().max())
    with pytest.raises(ValueError, match="do not fit"):
        ops.mse_loss(p, target.to(dev)[:2], 3)


def test_simulator_mirrors_have_the_bindings_argument_lists():
    names, differ = sim_matches_binding()
    assert names == ("denoise_prepare", "mse_fwd", "mse_bwd") and not differ
    assert all(f"comat_{n}" in _hip.SIGNATURES for n in names) and _hip.ABI_VERSION == 8


def test_denoise_kernels_hands_out_the_installed_backend(sim):
    assert ops.denoise_kernels() is _hip  # the plain simulator lacks the entry points: the binding answers (and refuses CPU tensors)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.mse_loss(torch.zeros(2, 4), torch.zeros(2, 4), 2)
    k = DenoiseSimKernels()
    ops.set_kernel_backend(k)
    assert ops.denoise_kernels() is k
