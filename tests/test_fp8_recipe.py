"""The delayed-scaling RECIPE of the fp8 forward: comat_fp8_scales_update_hist (abs-max history window, margin, step-level clip
accounting) from the kernel to CoMatTrainer - self-calibrating sites, the stale-byte guard, save / restore, graphs.

Every case runs on the simulator (tests/sim_backend.py restates the header) and, marked `gpu`, on libcomat_hip.so.  Expected
values come from `_ref_update` below: the header text once more, in plain torch, every value fp32 and in the header's order."""
import warnings

import pytest
import torch

from comat_amd import checkpoint, ops
from helpers import fp8_state, rel_l2
from oracle import fp8 as OF
from test_fp8 import _fp8_step_world, _tagged, rnd

F32 = torch.float32
TINY = torch.tensor(2.0 ** -100, dtype=F32)
E4M3_MAX = torch.tensor(448.0, dtype=F32)


@pytest.fixture
def dev(dev):
    with fp8_state():
        yield dev


@pytest.fixture
def hip(hip):
    with fp8_state():
        yield hip


def _scale_of(a, margin=1.0):
    """fl(fl(max(a, 2^-100) * margin) / 448), fp32"""
    return torch.maximum(torch.as_tensor(a, dtype=F32), TINY) * torch.tensor(margin, dtype=F32) / E4M3_MAX


def _ref_update(t, hist_len, margin, account):
    """include/comat_hip.h, comat_fp8_scales_update_hist, on host tables t = dict(amax int32, scale, hist [n, hist_len], count,
    clip_steps, worst, clip_now)"""
    seen = t["amax"] != 0
    a = t["amax"].view(F32).clone()
    s_a = torch.maximum(a, TINY) / E4M3_MAX
    s = t["scale"].clone()
    clipped = seen & (s > 0) & (s_a > s) if account else torch.zeros_like(seen)
    t["clip_steps"] += clipped.int()
    over = s_a / torch.where(clipped, s, torch.ones_like(s))
    t["worst"].copy_(torch.where(clipped, torch.maximum(t["worst"], over), t["worst"]))
    t["clip_now"].copy_(clipped.int())
    for j in range(hist_len):  # the ring slot count % hist_len takes this step's abs-max
        put = seen & (t["count"] % hist_len == j)
        t["hist"][:, j] = torch.where(put, a, t["hist"][:, j])
    t["count"] += seen.int()
    m = torch.zeros_like(a)
    for j in range(hist_len):  # maximum over the first min(count, hist_len) slots
        m = torch.where(t["count"] > j, torch.maximum(m, t["hist"][:, j]), m)
    t["scale"].copy_(torch.where(seen, torch.maximum(m, TINY) * torch.tensor(margin, dtype=F32) / E4M3_MAX, s))
    t["amax"].zero_()


def _tables(n, hist_len, dev):
    z = lambda dt, *shape: torch.zeros(*shape, dtype=dt, device=dev)
    return dict(amax=z(torch.int32, n), scale=z(F32, n), hist=z(F32, n, hist_len), count=z(torch.int32, n),
                clip_steps=z(torch.int32, n), worst=z(F32, n), clip_now=z(torch.int32, n))


def _launch(k, t, n, hist_len, margin, account):
    k.fp8_scales_update_hist(t["amax"], t["scale"], t["hist"], t["count"], t["clip_steps"], t["worst"], t["clip_now"], n, hist_len,
                             margin, account)


def _draw_amax(n, g):
    """abs-maxima over ~30 binades, some below the 2^-100 floor, about a third of the sites unseen (bits 0)"""
    a = (torch.randn(n, generator=g).abs() * torch.exp2(torch.randint(-12, 18, (n,), generator=g).float())).to(F32)
    a = torch.where(torch.rand(n, generator=g) < 0.02, torch.full_like(a, 1e-35), a)
    a = torch.where(torch.rand(n, generator=g) < 1 / 3, torch.zeros_like(a), a)
    return a.view(torch.int32).clone()


# ---- 1. the kernel, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("margin", [1.0, 1.25, 2.0])
@pytest.mark.parametrize("hist_len", [1, 2, 4, 16])
@pytest.mark.parametrize("n", [1, 255, 256, 1000, 4096])
def test_update_kernel_matches_the_header_bit_for_bit(dev, n, hist_len, margin):
    """random tables, 20 updates in a row, every table compared after every one of them (0 .. 20 updates); the first update has no
    scale to compare against, one in five runs without accounting.  hist_len = 1, margin = 1: the scale words of
    comat_fp8_scales_update on the same inputs."""
    k = ops.kernels()
    g = torch.Generator().manual_seed(1000 * n + 10 * hist_len + int(margin * 4))
    ref, got = _tables(n, hist_len, "cpu"), _tables(n, hist_len, dev)
    plain = (torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=F32, device=dev))
    for step in range(20):
        bits = _draw_amax(n, g)
        account = step % 5 != 3
        ref["amax"].copy_(bits)
        got["amax"].copy_(bits)
        _ref_update(ref, hist_len, margin, account)
        _launch(k, got, n, hist_len, margin, account)
        for key in ("scale", "hist", "count", "clip_steps", "worst", "clip_now", "amax"):
            assert torch.equal(got[key].cpu(), ref[key]), f"update {step + 1}: {key}"
        if hist_len == 1 and margin == 1.0:
            plain[0].copy_(bits)
            k.fp8_scales_update(plain[0], plain[1], n)
            assert torch.equal(got["scale"].cpu(), plain[1].cpu()), f"update {step + 1}: differs from comat_fp8_scales_update"
    assert n < 200 or int(ref["clip_steps"].sum()) > 0  # the accounting branch really ran


def test_update_kernel_rejects_bad_arguments(dev):
    """COMAT_EINVAL (-1) with a message, and nothing launched: the tables keep their contents"""
    k = ops.kernels()
    n = 8
    t = _tables(n, 32, dev)  # room for any hist_len tried below
    t["amax"].copy_(torch.full((n,), 3.0).view(torch.int32))
    before = {key: v.clone() for key, v in t.items()}
    bad = [dict(hist_len=0), dict(hist_len=17), dict(margin=0.5), dict(margin=float("inf")), dict(margin=float("nan")), dict(n=0),
           dict(amax=None), dict(scale=None), dict(hist=None), dict(count=None), dict(worst=None), dict(clip_steps=None, clip_now=None)]
    for change in bad:
        a = dict(t, n=n, hist_len=4, margin=1.0)
        a.update(change)
        with pytest.raises(RuntimeError, match=r"rc=-1\): \S"):
            k.fp8_scales_update_hist(a["amax"], a["scale"], a["hist"], a["count"], a["clip_steps"], a["worst"], a["clip_now"], a["n"],
                                     a["hist_len"], a["margin"], True)
        for key, v in t.items():
            assert torch.equal(v, before[key]), (change, key)
    k.fp8_scales_update_hist(t["amax"], t["scale"], t["hist"], t["count"], None, None, None, n, 4, 1.0, True)  # no accounting: fine
    assert torch.equal(t["scale"].cpu(), _scale_of(torch.full((n,), 3.0)))


# ---- 2. no false clip in the steady state ---------------------------------------------------------------------------------
@pytest.mark.parametrize("hist_len", [1, 4])
@pytest.mark.parametrize("margin", [1.0, 1.0000001, 1.25, 2.0, 7.3])
def test_steady_state_is_never_flagged(dev, hist_len, margin):
    """the same abs-max for 10 updates: the comparison is made between SCALES and fp32 division is monotone, so no site is flagged
    for any margin >= 1 (a comparison against 448 * scale would flag through rounding)"""
    k = ops.kernels()
    n = 1000
    g = torch.Generator().manual_seed(7)
    a = (torch.rand(n, generator=g) + 0.01) * torch.exp2(torch.randint(-10, 14, (n,), generator=g).float())
    t = _tables(n, hist_len, dev)
    for _ in range(10):
        t["amax"].copy_(a.to(F32).view(torch.int32))
        _launch(k, t, n, hist_len, margin, True)
    assert int(t["clip_steps"].sum()) == 0 and int(t["clip_now"].sum()) == 0 and float(t["worst"].max()) == 0.0


def test_one_ulp_above_the_window_maximum_is_flagged_once(dev):
    """margin 1: an abs-max one ulp above the scale's is flagged exactly once (it then IS the window maximum).
    The cases: significands in [1, 1.75).  a / 448 = (a / 7) / 64; for a significand m < 1.75, m / 7 lies in [1/8, 1/4), where the
    quotient's ulp (2^-26) is below the 2^-23 / 7 by which the quotients of neighbouring a differ - neighbours never round to the
    same scale.  (For m in [1.75, 2) the quotient's ulp is 2^-25 and two neighbours may share a scale: an overshoot below the
    resolution of the scale word cannot be seen in the scale domain, by design.)"""
    k = ops.kernels()
    n = 1000
    g = torch.Generator().manual_seed(8)
    m = 1.0 + 0.75 * torch.rand(n, generator=g).clamp(max=0.999)
    a = (m * torch.exp2(torch.randint(-10, 14, (n,), generator=g).float())).to(F32)
    up = torch.nextafter(a, torch.full_like(a, float("inf")))
    t = _tables(n, 1, dev)
    for v in (a, a, up, up, up):
        t["amax"].copy_(v.view(torch.int32))
        _launch(k, t, n, 1, 1.0, True)
    assert torch.equal(t["clip_steps"].cpu(), torch.ones(n, dtype=torch.int32))
    assert torch.equal(t["worst"].cpu(), (up / E4M3_MAX) / (a / E4M3_MAX)) and int(t["clip_now"].sum()) == 0


# ---- 3. the site protocol under a recipe ----------------------------------------------------------------------------------
def _site_world(dev):
    lin = _tagged(ops.FrozenLinear(rnd(96, 128, seed=1) * 0.1, rnd(96, seed=2) * 0.1, F32, dev))
    lin._fp8_name = "blocks.0.ff.net.2"
    wq = OF.dequantize(*OF.quantize(lin.w.cpu().float()))

    def ref(x, s):
        return OF.dequantize(OF.quantize_with_scale(x, s), s) @ wq.t() + lin.bias.cpu()
    return lin, ref


def test_history_window_of_three_steps(dev):
    """maxima a1 < a2 > a3 > a4 > a5: the scale in force is the maximum of the last three; a2 leaves after its third successor"""
    ops.set_fp8_scaling("delayed")
    ops.set_fp8_recipe(history=3, margin=1.0)
    lin, ref = _site_world(dev)
    base = rnd(40, 128, seed=3)
    xs = [base * f for f in (1.0, 3.0, 2.0, 1.5, 1.2)]
    am = [x.abs().max() for x in xs]
    window = [am[0], am[1], am[1], am[1], am[2]]  # max of the last three after steps 1 .. 5
    with torch.no_grad(), ops.fp8_forward(True):
        with ops.fp8_calibration():
            ops.linear(xs[0].to(dev), lin)
        ops.fp8_end_of_step()
        assert torch.equal(lin._fp8_site[0].cpu(), _scale_of(am[0]).reshape(1))
        for i in range(1, 5):
            s_in_force = lin._fp8_site[0].cpu()[0].clone()
            y = ops.linear(xs[i].to(dev), lin)
            assert rel_l2(y, ref(xs[i], s_in_force)) < 1e-4
            ops.fp8_end_of_step()
            assert torch.equal(lin._fp8_site[0].cpu(), _scale_of(window[i]).reshape(1)), f"after step {i + 1}"
    assert float(window[3]) > float(window[4])  # a2 really dropped out


def test_margin_and_the_clip_report(dev):
    """margin 2: 1.9x the window maximum is inside the scale (output = the oracle quantiser's under the margined scale, nothing
    reported); 2.5x the then maximum is not, and fp8_report names the site with worst = fl(s_a / scale)"""
    ops.set_fp8_scaling("delayed")
    ops.set_fp8_recipe(history=1, margin=2.0)
    lin, ref = _site_world(dev)
    x1 = rnd(40, 128, seed=3)
    x2, x3 = x1 * 1.9, x1 * (1.9 * 2.5)
    with torch.no_grad(), ops.fp8_forward(True):
        with ops.fp8_calibration():
            ops.linear(x1.to(dev), lin)
        ops.fp8_end_of_step()
        s1 = _scale_of(x1.abs().max(), 2.0)
        assert torch.equal(lin._fp8_site[0].cpu(), s1.reshape(1))
        y2 = ops.linear(x2.to(dev), lin)
        assert rel_l2(y2, ref(x2, s1)) < 1e-4
        assert rel_l2(ref(x2, s1), x2 @ lin.w.cpu().float().t() + lin.bias.cpu()) < 0.1  # unsaturated: close to the exact product
        ops.fp8_end_of_step()
        rep = ops.fp8_report(dev)
        assert rep["sites"] == 1 and rep["clipped_now"] == [] and rep["clip_steps"] == 0 and rep["top"] == []
        s2 = _scale_of(x2.abs().max(), 2.0)
        assert torch.equal(lin._fp8_site[0].cpu(), s2.reshape(1))
        y3 = ops.linear(x3.to(dev), lin)
        assert rel_l2(y3, ref(x3, s2)) < 1e-4  # saturated, as the oracle's quantiser under that scale
        ops.fp8_end_of_step()
    rep = ops.fp8_report(dev)
    worst = float(_scale_of(x3.abs().max()) / s2)
    assert rep["clip_steps"] == 1 and [e["name"] for e in rep["clipped_now"]] == ["blocks.0.ff.net.2"]
    assert rep["top"] == [dict(site=0, name="blocks.0.ff.net.2", worst=worst, clip_steps=1, clipped_now=True)]
    assert 1.2 < worst < 1.3


# ---- 4. a trainer that never calibrates -----------------------------------------------------------------------------------
STEP = dict(training_steps=[1, 2], crop=(1, 0, 63, 63), attrcon_steps=[2])


def _record_launches(k):
    """every public method of the backend, wrapped to note its name -> (log, undo)"""
    log, saved = [], {}
    for name in dir(k):
        fn = getattr(k, name)
        if name.startswith("_") or not callable(fn):
            continue
        saved[name] = fn

        def wrapped(*a, _n=name, _f=fn, **kw):
            log.append(_n)
            return _f(*a, **kw)
        setattr(k, name, wrapped)

    def undo():
        for name in saved:
            delattr(k, name) if name in k.__dict__ else None
    return log, undo


def test_trainer_without_calibration_is_the_jit_step(dev):
    """delayed scaling, no fp8_calibrate: the first step runs every site just in time - the gradients of the jit step, bit for bit,
    and its launches (the jit pair also records the abs-max) - the second one never does.
    (Before the self-calibrating sites the first step quantised with 1 / 0 and multiplied by scale 0: bias-only layers.)"""
    ops.set_fp8_scaling("jit")
    trainer, bank, batch, cfg, _ = _fp8_step_world(dev, F32)
    trainer.pipe.graphed = None  # launches are compared: every call eager (graphs: test_graphs_prepared_before_any_scale_exists_..)
    log_j, undo = _record_launches(ops.kernels())
    trainer.train_step(batch, **STEP)
    undo()
    g_jit = bank.flat_grad.detach().clone()
    ops.fp8_reset()
    ops.set_fp8_scaling("delayed")
    trainer, bank, batch, cfg, _ = _fp8_step_world(dev, F32)
    trainer.pipe.graphed = None
    log_d, undo = _record_launches(ops.kernels())
    logs = trainer.train_step(batch, **STEP)
    n1 = len(log_d)
    g1 = bank.flat_grad.detach().clone()
    trainer.train_step(batch, **STEP)
    undo()
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    assert torch.equal(g1, g_jit)
    assert log_d[:n1] == log_j + ["fp8_scales_update"] and log_j.count("fp8_quantize") > 40
    assert "fp8_clipped_sites" not in logs  # no recipe: the default keys
    second = log_d[n1:]
    assert second.count("fp8_quantize") == 0 and second.count("fp8_quantize_scaled") > 0 and second.count("layernorm_fwd_q") > 0


# ---- 5. the default path ---------------------------------------------------------------------------------------------------
def test_default_path_is_unchanged_and_the_unit_recipe_reproduces_it(dev):
    """no recipe: fp8_end_of_step launches comat_fp8_scales_update, never the new kernel; history 1 / margin 1 gives the same
    losses and gradients bit for bit"""
    ops.set_fp8_scaling("delayed")
    runs = {}
    for name in ("default", "unit"):
        ops.fp8_reset()
        if name == "unit":
            ops.set_fp8_recipe(history=1, margin=1.0)
        trainer, bank, batch, cfg, _ = _fp8_step_world(dev, F32)
        log, undo = _record_launches(ops.kernels())
        assert trainer.fp8_calibrate(batch)
        out = []
        for _ in range(3):
            logs = trainer.train_step(batch, **STEP)
            out.append((float(logs["step_loss"]), float(logs["Blip"]), float(logs["G_loss"]), float(logs["D_loss"]),
                        bank.flat_grad.detach().cpu().clone(), "fp8_clipped_sites" in logs))
        undo()
        runs[name] = (out, log)
    (d_out, d_log), (u_out, u_log) = runs["default"], runs["unit"]
    assert d_log.count("fp8_scales_update") == 4 and d_log.count("fp8_scales_update_hist") == 0  # calibration + three steps
    assert u_log.count("fp8_scales_update") == 0 and u_log.count("fp8_scales_update_hist") == 4
    for a, b in zip(d_out, u_out):
        assert a[:4] == b[:4] and torch.equal(a[4], b[4])
        assert not a[5] and b[5]
    assert not torch.equal(d_out[0][4], d_out[1][4])  # the steps really moved


# ---- 6. stale bytes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["untouched", "written in place", "held across the update"])
def test_producer_bytes_are_used_only_while_they_are_current(dev, case):
    """LayerNorm emits the bytes for the layer it feeds; they are used when the tensor still is what was quantised, under the
    scales of this step - else the consumer quantises the tensor as it then is (one launch)"""
    ops.set_fp8_scaling("delayed")
    lin, _ = _site_world(dev)
    x = rnd(40, 128, seed=3).to(dev)
    gamma, beta = (1 + 0.1 * rnd(128, seed=4)).to(dev), (0.1 * rnd(128, seed=5)).to(dev)
    k = ops.kernels()
    n_scaled, orig = [0], k.fp8_quantize_scaled

    def counted(*a, **kw):
        n_scaled[0] += 1
        return orig(*a, **kw)
    with torch.no_grad(), ops.fp8_forward(True):
        with ops.fp8_calibration():
            ops.linear(ops.layer_norm(x, gamma, beta, fp8_for=lin), lin)
        ops.fp8_end_of_step()
        y = ops.layer_norm(x, gamma, beta, fp8_for=lin)
        assert getattr(y, "_fp8", None) is not None  # the producer did emit the bytes
        if case == "written in place":
            y.mul_(0.5)
        elif case == "held across the update":
            ops.linear((y * 4).contiguous(), lin)  # a 4x larger tensor passes the site: the update really changes the scale
            ops.fp8_end_of_step()
        k.fp8_quantize_scaled = counted
        try:
            out = ops.linear(y, lin)
            cost = n_scaled[0]
            expect = ops.linear(y.clone(), lin)  # a tensor without bytes: quantised as it is, under the scale in force
        finally:
            del k.fp8_quantize_scaled
    assert cost == (0 if case == "untouched" else 1) and n_scaled[0] == cost + 1
    assert torch.equal(out, expect)


# ---- 7. save and restore ---------------------------------------------------------------------------------------------------
def test_checkpoint_carries_the_fp8_state(dev, tmp_path):
    """two steps, save, a fresh process in miniature, load, a third step: the gradients and the scale table of the uninterrupted
    third step, without a just-in-time launch"""
    ops.set_fp8_scaling("delayed")
    ops.set_fp8_recipe(history=2, margin=1.25)
    trainer, bank, batch, cfg, _ = _fp8_step_world(dev, F32)
    assert trainer.fp8_calibrate(batch)
    for _ in range(3):
        trainer.train_step(batch, **STEP)
    st = ops.fp8_state(dev)
    want = (bank.flat_grad.detach().cpu().clone(), st.scale[:st.n].cpu().clone(), st.n)

    ops.fp8_reset()
    trainer, bank, batch, cfg, _ = _fp8_step_world(dev, F32)
    assert trainer.fp8_calibrate(batch)
    for _ in range(2):
        trainer.train_step(batch, **STEP)
    checkpoint.save_checkpoint(str(tmp_path), bank, trainer.D, fp8_device=dev)
    plain = tmp_path / "plain"
    checkpoint.save_checkpoint(str(plain), bank, trainer.D)
    assert not (plain / "fp8_state.pt").exists() and (tmp_path / "fp8_state.pt").exists()

    ops.fp8_reset()
    ops.clear_fp8_recipe()
    trainer, bank, batch, cfg, _ = _fp8_step_world(dev, F32)
    checkpoint.load_checkpoint(str(tmp_path), bank, trainer.D, fp8_device=dev)
    assert ops.fp8_recipe() == dict(history=2, margin=1.25, account=True, reduce_amax=False)
    st = ops.fp8_state(dev)
    addresses = (st.scale.data_ptr(), st.hist.data_ptr(), st.count.data_ptr())
    log, undo = _record_launches(ops.kernels())
    trainer.train_step(batch, **STEP)
    undo()
    assert log.count("fp8_quantize") == 0
    assert addresses == (st.scale.data_ptr(), st.hist.data_ptr(), st.count.data_ptr())
    assert st.n == want[2] and torch.equal(st.scale[:st.n].cpu(), want[1])
    assert torch.equal(bank.flat_grad.detach().cpu(), want[0])
    sd = ops.fp8_state_dict(dev)
    sd["n"] += 1
    with pytest.raises(ValueError, match="sites"):
        ops.fp8_load_state_dict(dev, sd)


# ---- 8. graphs -------------------------------------------------------------------------------------------------------------
def _fp8_sd15_world(dev):
    """the SD1.5-layout miniature of tests/test_step.py with the fp8 forward on its generator: the layout GraphedStep captures (the
    SDXL layout builds its added time embedding on the host in every call)"""
    from comat_amd import config
    from comat_amd.pipeline import TrainableSDPipeline
    from comat_amd.unet import UNet
    from helpers import tiny_weights
    from test_step import make_world
    cfg, batch, _, trainer = make_world(F32, dev, False)
    usd, _, _ = tiny_weights(F32, config.TINY_UNET)
    unet = UNet(config.TINY_UNET, usd, F32, dev, trainer.bank, fp8_forward=True)
    trainer.pipe = TrainableSDPipeline(unet, trainer.pipe.vae)
    return trainer, batch


def _recipe_steps(trainer, batch, step, sync):
    assert trainer.fp8_calibrate(batch)
    gen = torch.Generator().manual_seed(11)
    dev = trainer.device
    out = []
    for it in range(3):
        b = dict(batch)
        b["latents"] = torch.randn(batch["latents"].shape, generator=gen) * (1.0 + it)
        b["noises"] = [torch.randn(n.shape, generator=gen) for n in batch["noises"]]
        logs = step(b, training_steps=[1, 2], crop=(1, 0, 63, 63))
        sync()
        st = ops.fp8_state(dev)
        assert st.n > 5
        out.append((float(logs["step_loss"]), int(logs["fp8_clipped_sites"]), trainer.bank.flat_grad.detach().cpu().clone(),
                    st.scale[:st.n].cpu().clone(), trainer.bank.flat.detach().cpu().clone()))
    return out


def test_recipe_steps_on_the_sd15_layout_log_the_clipped_sites(dev):
    """the world of the graph test below, eagerly (simulator and library): growing latents clip some sites, and the log says so"""
    ops.set_fp8_scaling("delayed")
    ops.set_fp8_recipe(history=4, margin=1.25)
    trainer, batch = _fp8_sd15_world(dev)
    out = _recipe_steps(trainer, batch, trainer.train_step, (lambda: None) if dev.type == "cpu" else torch.cuda.synchronize)
    rep = ops.fp8_report(dev)
    assert sum(o[1] for o in out) == rep["clip_steps"] and out[-1][1] == len(rep["clipped_now"])
    assert all(torch.isfinite(o[2]).all() for o in out)


@pytest.mark.gpu
def test_graphed_step_under_a_recipe_matches_eager(hip):
    """GraphedStep under history 4 / margin 1.25 with accounting: three steps (one eager + capture, two replays) against three
    eager steps of a second world - gradients, scale table and logs["fp8_clipped_sites"] bit for bit.
    Like for like: the whole-step graph holds the no-grad denoise calls as the launches of UNet.__call__, so both worlds run them
    that way (`pipe.graphed = None`).  GraphedUNetForward is another form of those calls under the fp8 forward, with or without a
    recipe: it projects the text keys / values outside ops.fp8_forward, where the no-grad LoRA projections take their merged-weight
    form (measured on MI355X, step losses of this world: 5.221705 with its graphs, 5.221770 without, eager and graphed alike)."""
    from comat_amd.step import GraphedStep
    ops.set_fp8_scaling("delayed")
    ops.set_fp8_recipe(history=4, margin=1.25)
    runs = []
    for graphed in (False, True):
        ops.fp8_reset()
        trainer, batch = _fp8_sd15_world(hip)
        trainer.pipe.graphed = None
        step = GraphedStep(trainer) if graphed else trainer.train_step
        assert not graphed or step.supported(batch)
        runs.append(_recipe_steps(trainer, batch, step, torch.cuda.synchronize))
        if graphed:
            assert step.failed is None and len(step.graphs) == 1
    for it, (e, g) in enumerate(zip(*runs)):
        assert e[:2] == g[:2], f"step {it}: (loss, clipped sites) {e[:2]} eager vs {g[:2]} graph"
        for a, b, what in zip(e[2:], g[2:], ("gradients", "scale table", "parameters")):
            assert torch.equal(a, b), f"step {it}: {what} differ"
    print("fp8 recipe, graphed step: clipped sites per step", [e[1] for e in runs[0]])


@pytest.mark.gpu
def test_capturing_a_site_without_a_scale_warns_once(hip):
    """an unready site inside a capture keeps the two-launch just-in-time form - right, but worth a calibration: one warning"""
    ops.set_fp8_scaling("delayed")
    lins = [_site_world(hip)[0] for _ in range(2)]
    x = rnd(40, 128, seed=3).to(hip)
    with torch.no_grad(), ops.fp8_forward(True):
        ops.set_fp8_scaling("jit")
        want = ops.linear(x, lins[0])
        ops.set_fp8_scaling("delayed")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            with ops.graph_capture(g, stream=ops.capture_stream(hip)):
                y0 = ops.linear(x, lins[0])
                y1 = ops.linear(x, lins[1])
        assert len([w for w in seen if "without a scale" in str(w.message)]) == 1
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(y0, want) and torch.equal(y1, want)


@pytest.mark.gpu
def test_graphs_prepared_before_any_scale_exists_wait_for_the_scales(hip):
    """prepare_graphs() before any calibration (the order bench.py uses): the no-grad forward graphs hold the delayed launches, no
    warning; without a calibration the first step does not replay them (every site just in time: the jit step's gradients), the
    second one does, and never quantises just in time"""
    ops.set_fp8_scaling("jit")
    trainer, bank, batch, cfg, _ = _fp8_step_world(hip, F32)
    trainer.train_step(batch, **STEP)
    torch.cuda.synchronize()
    g_jit = bank.flat_grad.detach().clone()
    ops.fp8_reset()
    ops.set_fp8_scaling("delayed")
    trainer, bank, batch, cfg, _ = _fp8_step_world(hip, F32)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        assert trainer.pipe.prepare_graphs(1, cfg.resolution, cfg.resolution, 7, cfg.total_step) == cfg.total_step
    assert not [w for w in seen if "without a scale" in str(w.message)]
    graphed = trainer.pipe.graphed
    graphed.timing = []
    trainer.train_step(batch, **STEP)
    torch.cuda.synchronize()
    assert graphed.timing == [] and torch.equal(bank.flat_grad, g_jit)
    k = ops.kernels()
    n_jit, kq = [0], k.fp8_quantize
    k.fp8_quantize = lambda t, **kw: (n_jit.__setitem__(0, n_jit[0] + 1), kq(t, **kw))[1]
    try:
        trainer.train_step(batch, **STEP)
        torch.cuda.synchronize()
    finally:
        del k.fp8_quantize
    assert len(graphed.timing) == cfg.total_step - len(STEP["training_steps"]) and n_jit[0] == 0
    assert torch.isfinite(bank.flat_grad).all()


def test_capture_on_trust_takes_the_delayed_form_and_remembers_the_sites(dev):
    """ops.fp8_capture_on_trust (what GraphedUNetForward wraps its captures in): a site without a scale gets the delayed launches
    all the same and is handed to the owner, who must not run them while fp8_pending says a scale is missing"""
    ops.set_fp8_scaling("delayed")
    lin, _ = _site_world(dev)
    x = rnd(40, 128, seed=3).to(dev)
    k = ops.kernels()
    ops.fp8_weight(lin)  # the frozen weight's own (one-time) quantisation, out of the count
    log, undo = _record_launches(k)
    with torch.no_grad(), ops.fp8_forward(True):
        with ops.fp8_capture_on_trust() as trust:
            ops.linear(x, lin)
        assert log.count("fp8_quantize_scaled") == 1 and log.count("fp8_quantize") == 0
        assert len(trust.sites) == 1 and ops.fp8_pending(trust.sites) and ops.fp8_unready(dev)
        ops.linear(x, lin)  # outside: just in time
        assert log.count("fp8_quantize") == 1
        ops.fp8_end_of_step()
        assert not ops.fp8_pending(trust.sites) and not trust.sites and not ops.fp8_unready(dev)
        ops.linear(x, lin)
        assert log.count("fp8_quantize") == 1 and log.count("fp8_quantize_scaled") == 2
    undo()
