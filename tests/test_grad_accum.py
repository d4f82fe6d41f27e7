"""Gradient accumulation with its window decided on the device (`--gradient_accumulation_steps`; training_script.py:556,680
`accelerator.accumulate`, :293-294 the schedule's lengths, :655,702 train_loss, :698,710 logging / saving under sync_gradients):
the three entry points (comat_accum_zero, comat_adamw_window, comat_window_tick), the optimizer against tests/golden/grad_accum.json
(recorded from the installed accelerate by tests/golden/make_grad_accum_golden.py), the trainer against the CPU oracle, the graph
steppers against eager micro-steps bit for bit, two ranks over gloo, and the checkpoint.

Bounds: a learning rate as in tests/test_lr_schedule.py (`assert_rate`: exact for constant / linear); the optimizer against torch
as tests/test_lr_schedule.py::test_flat_adamw_with_schedule_matches_torch (`check(..., factor=0.5)`); the trainer against the oracle
as tests/test_step.py::test_train_step_matches_oracle for the dtype."""
import dataclasses
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from comat_amd import _hip, checkpoint
from comat_amd.step import CoMatTrainer, FlatAdamW, GraphedStep, StepConfig, lr_schedule
from helpers import Window, check, rel_l2
from test_lr_schedule import PLAN, STEP, assert_rate, fresh_inputs
from test_step import BF16_D_GRAD_LIMIT, BF16_GRAD_LIMIT, BF16_HEAD_GRAD_LIMIT, make_world

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "grad_accum.json")))
HYPER = FIX["hyper"]
F32 = torch.float32
I32 = torch.int32
# below one vector, one vector, tails, several blocks, and a second trip of the grid-stride loop past the 4096-block cap
SIZES = [1, 3, 4, 5, 1023, 4099, 4 * 256 * 4096 + 4099]


def kernels():
    from comat_amd import ops
    return ops.kernels()


def window_of(n, dev, left):
    """a vector of n floats in a poisoned buffer: `left` guard elements before it (8: 16-byte aligned, 1: not), 32 after"""
    w = Window(1, n, ld=n + 32, dtype=F32, device=dev, lead=0, trail=0, left=left)
    assert (w.flat.data_ptr() % 16 == 0) == (left == 8)
    return w


def word(v, dev, dtype=I32):
    return torch.tensor([v], dtype=dtype, device=dev)


# ---- 1. comat_accum_zero ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("left", [8, 1])
@pytest.mark.parametrize("n", SIZES)
def test_accum_zero(dev, n, left):
    k = kernels()
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen) + 3.0
    g = window_of(n, dev, left).put(x).arm()
    k.accum_zero(g.flat, n, word(1, dev))  # inside a window: every byte as before
    assert torch.equal(g.buf.view(I32), g._snap), "window[0] = 1: the buffer changed"
    k.accum_zero(g.flat, n, word(0, dev))
    assert int(torch.count_nonzero(g.get().view(I32))) == 0, "window[0] = 0: not all elements are +0"
    g.assert_guard_intact(f"accum_zero n={n} left={left}")


def test_accum_zero_refusals(dev):
    k = kernels()
    x, w = torch.ones(8, dtype=F32, device=dev), word(0, dev)
    for args in ((None, 8, w), (x, 8, None), (x, 0, w), (x, -1, w)):
        with pytest.raises(RuntimeError, match="comat_accum_zero"):
            k.accum_zero(*args)
    assert torch.equal(x.cpu(), torch.ones(8))


# ---- 2. comat_adamw_window --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("left", [8, 1])
@pytest.mark.parametrize("n", SIZES)
def test_adamw_window(dev, n, left):
    """closing: p, m, v bit-identical to comat_adamw_lr on copies (with a clipping norm, and a non-finite one: nothing written);
    not closing: p, m, v are their inputs bit for bit"""
    k = kernels()
    gen = torch.Generator().manual_seed(200 + n % 1000)
    hp = (0.9, 0.999, 1e-8, 1e-2)
    init = [torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 0.01]
    gw = window_of(n, dev, left).put((torch.rand(n, generator=gen) + 0.5) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1))
    A, B = [window_of(n, dev, left).put(x) for x in init], [window_of(n, dev, left).put(x) for x in init]
    lr, counters, nsq = word(5e-3, dev, F32), torch.tensor([2, 0], dtype=I32, device=dev), torch.zeros(1, dtype=F32, device=dev)
    k.sumsq(gw.flat, n, nsq)  # |g|_2 >= 0.5 sqrt(n) > max_norm: the clip acts
    assert float(nsq[0]) > 0.1 ** 2
    for N in (1, 2, 3):
        for w in A + B:
            w.arm()
        k.adamw_lr(A[0].flat, gw.flat, A[1].flat, A[2].flat, n, lr, *hp, counters, nsq, 0.1, grad_scale=0.5)
        for idx in range(N - 1):  # not closing
            k.adamw_window(B[0].flat, gw.flat, B[1].flat, B[2].flat, n, lr, *hp, counters, nsq, 0.1, word(idx, dev), N, grad_scale=0.5)
            for w, name in zip(B, "pmv"):
                assert torch.equal(w.buf.view(I32), w._snap), f"N={N} window={idx}: {name} was written"
        k.adamw_window(B[0].flat, gw.flat, B[1].flat, B[2].flat, n, lr, *hp, counters, nsq, 0.1, word(N - 1, dev), N, grad_scale=0.5)
        for a, b, name in zip(A, B, "pmv"):
            assert torch.equal(a.get().view(I32), b.get().view(I32)), f"N={N} closing: {name} differs from comat_adamw_lr's"
            assert not torch.equal(b.buf.view(I32), b._snap), f"N={N} closing: {name} did not move"
            b.assert_guard_intact(f"adamw_window n={n} left={left} N={N}")
    for w in B:  # a closing launch under a non-finite norm writes nothing
        w.arm()
    k.adamw_window(B[0].flat, gw.flat, B[1].flat, B[2].flat, n, lr, *hp, counters, word(float("inf"), dev, F32), 0.1, word(1, dev), 2)
    for w, name in zip(B, "pmv"):
        assert torch.equal(w.buf.view(I32), w._snap), f"non-finite norm: {name} was written"


def test_adamw_window_refusals(dev):
    k = kernels()
    x, lr, c, w = torch.ones(8, dtype=F32, device=dev), word(1e-3, dev, F32), torch.zeros(2, dtype=I32, device=dev), word(0, dev)
    nsq = torch.ones(1, dtype=F32, device=dev)
    good = dict(p=x, g=x, m=x, v=x, n=8, lr_dev=lr, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0, step_dev=c, gnorm_sq=nsq, max_norm=0.1,
                window=w, accum_steps=1)
    for change in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(lr_dev=None), dict(step_dev=None), dict(window=None),
                   dict(n=0), dict(accum_steps=0), dict(accum_steps=-2)):
        with pytest.raises(RuntimeError, match="comat_adamw_window"):
            k.adamw_window(**{**good, **change})
    assert torch.equal(x.cpu(), torch.ones(8))


# ---- 3. comat_window_tick against the fixture traces ------------------------------------------------------------------------
def traces():
    return [(f"N={c['accum_steps']} {c['kind']}", c) for c in FIX["cases"]] + [("nonfinite", FIX["nonfinite"]), ("stride", FIX["stride"])]


def sched_of(c):
    return lr_schedule(c["kind"], c["lr0"], warmup=c["warmup"], total=c["total"], steps_per_update=c["num_processes"])


def test_fixture_covers_what_it_should():
    assert {(c["accum_steps"], c["kind"]) for c in FIX["cases"]} == {(N, kd) for N in (1, 2, 3) for kd in ("constant", "linear")}
    for _, c in traces():
        assert len(c["trace"]) == 7 and c["order"] == "documented"
        N = c["accum_steps"]
        assert [t["sync_gradients"] for t in c["trace"]] == [(i + 1) % N == 0 for i in range(7)]
    nf = FIX["nonfinite"]["trace"]
    assert [t["skipped"] for t in nf] == [False, False, False, True, False, False, False] and nf[3]["sync_gradients"]
    assert FIX["stride"]["num_processes"] == 2
    ev = FIX["evidence"]  # what INTEGRATION.md says about the reference's loop as written
    assert ev["sgd_probe"] == dict(documented=-0.5, reference=0.0)
    assert not any(ev["two_contexts"]["2"]["G"]) and sum(ev["two_contexts"]["3"]["G"]) == 3


def test_window_tick_follows_the_traces(dev):
    k = kernels()
    gen = torch.Generator().manual_seed(7)
    for name, c in traces():
        N, s = c["accum_steps"], sched_of(c)
        for with_sched in ((True, False) if c["kind"] == "constant" else (True,)):  # a constant rate also without the struct
            window, counters = word(0, dev), torch.zeros(2, dtype=I32, device=dev)
            lr, nsq = torch.zeros(1, dtype=F32, device=dev), torch.zeros(1, dtype=F32, device=dev)
            k.lr_schedule_eval(s, counters, lr)
            tl, loss = torch.full((2,), 77.0, dtype=F32, device=dev), torch.zeros(1, dtype=F32, device=dev)
            applied = skipped = 0
            run, closed = np.float32(0), np.float32(77.0)
            for i, t in enumerate(c["trace"]):
                loss_i = np.float32(float(torch.randn(1, generator=gen)) * 3)
                loss.fill_(float(loss_i))
                nsq.fill_(float("inf") if t["skipped"] else 1.0)
                k.window_tick(window, N, counters, nsq, s if with_sched else None, lr, loss, tl)
                run = (np.float32(0) if i % N == 0 else run) + loss_i / np.float32(N)
                if t["sync_gradients"]:
                    applied, skipped, closed = applied + (not t["skipped"]), skipped + t["skipped"], run
                what = f"{name} sched={with_sched} micro-step {i}"
                assert window.tolist() == [(i + 1) % N], what
                assert counters.tolist() == [applied, skipped], what
                assert_rate(float(lr[0]), t["lr"], c["kind"], what)
                assert tl.cpu().numpy().tolist() == [float(run), float(closed)], what
            # the discriminator's optimizer: no loss words
            window.zero_(), counters.zero_()
            for i in range(N):
                k.window_tick(window, N, counters, nsq.fill_(1.0), None, None)
            assert window.tolist() == [0] and counters.tolist() == [1, 0]


def test_window_tick_refusals(dev):
    k = kernels()
    window, counters = word(1, dev), torch.zeros(2, dtype=I32, device=dev)
    lr, nsq = torch.full((1,), 7.0, dtype=F32, device=dev), torch.ones(1, dtype=F32, device=dev)
    loss, tl = torch.ones(1, dtype=F32, device=dev), torch.zeros(2, dtype=F32, device=dev)
    ok = lr_schedule("linear", 1e-3, warmup=1, total=8)
    good = dict(window=window, accum_steps=2, counters=counters, gnorm_sq=nsq, sched=ok, lr_out=lr, step_loss=loss, train_loss=tl)
    bad_scheds = [_hip.LrSchedule(9, 1, 0, 10, 1e-3, 0.5, 1.0, 1e-7), _hip.LrSchedule(2, 0, 0, 10, 1e-3, 0.5, 1.0, 1e-7),
                  _hip.LrSchedule(2, 1, -1, 10, 1e-3, 0.5, 1.0, 1e-7), _hip.LrSchedule(3, 1, 0, 0, 1e-3, 0.5, 1.0, 1e-7),
                  _hip.LrSchedule(5, 1, 0, 10, 1e-8, 0.5, 1.0, 1e-7)]
    for change in [dict(window=None), dict(counters=None), dict(gnorm_sq=None), dict(lr_out=None), dict(accum_steps=0),
                   dict(step_loss=None), dict(train_loss=None)] + [dict(sched=s) for s in bad_scheds]:
        with pytest.raises(RuntimeError, match="comat_window_tick"):
            k.window_tick(**{**good, **change})
    assert window.tolist() == [1] and counters.tolist() == [0, 0] and float(lr[0]) == 7.0 and tl.tolist() == [0.0, 0.0]
    k.window_tick(**{**good, "sched": None, "lr_out": None})  # without a schedule the rate word is not needed
    assert window.tolist() == [0] and counters.tolist() == [1, 0]


def test_library_refuses_without_launching():
    """the cross-compiled library's own argument checks, without a GPU (as tests/test_abi.py does for the other entry points)"""
    import ctypes as C
    lib = _hip.load_library()
    assert lib.comat_accum_zero(None, 4, None, None) == -1 and b"comat_accum_zero" in lib.comat_last_error()
    assert lib.comat_adamw_window(None, None, None, None, 4, None, 0.9, 0.999, 1e-8, 0.0, None, None, 0.1, 1.0, None, 2, None) == -1
    assert b"comat_adamw_window" in lib.comat_last_error()
    bad = _hip.LrSchedule(9, 1, 0, 10, 1e-3, 0.5, 1.0, 1e-7)
    assert lib.comat_window_tick(None, 2, None, None, C.byref(bad), None, None, None, None) == -1
    assert b"comat_window_tick: unknown schedule kind 9" in lib.comat_last_error()
    assert lib.comat_window_tick(None, 2, None, None, None, None, None, None, None) == -1 and b"null pointer" in lib.comat_last_error()


# ---- 4. FlatAdamW(accum_steps=N) against the fixture ------------------------------------------------------------------------
def grad_of(row):
    return torch.tensor([float("inf") if x == "inf" else x for x in row], dtype=F32)


@pytest.mark.parametrize("name", [n for n, _ in traces()])
def test_flat_adamw_follows_accelerate(dev, name):
    c = dict(traces())[name]
    N = c["accum_steps"]
    p, g = torch.tensor(FIX["w0"], dtype=F32, device=dev), torch.zeros(6, dtype=F32, device=dev)
    opt = FlatAdamW([(p, g)], HYPER["lr"], tuple(HYPER["betas"]), HYPER["eps"], HYPER["weight_decay"], HYPER["max_norm"],
                    schedule=sched_of(c), accum_steps=N)
    applied = skipped = 0
    for i, (row, t) in enumerate(zip(c["grads"], c["trace"])):
        assert opt.closing == t["sync_gradients"], f"{name}: micro-step {i}"
        opt.zero_grad()
        g.add_(grad_of(row).to(dev) / N)  # what backward of loss / N adds
        opt.step()
        applied, skipped = applied + (t["sync_gradients"] and not t["skipped"]), skipped + t["skipped"]
        assert opt.counters.tolist() == [applied, skipped]
        check(p, torch.tensor(t["params"], dtype=F32), F32, f"{name}: parameters after micro-step {i}", factor=0.5)
        if opt.lr_now is not None:
            assert_rate(float(opt.lr_now[0]), t["lr"], c["kind"], f"{name}: rate after micro-step {i}")
        if N > 1:
            assert opt.window.tolist() == [(i + 1) % N]
    assert applied >= 2 and not torch.equal(p.cpu(), torch.tensor(FIX["w0"], dtype=F32))


def test_accum_steps_one_keeps_todays_launches(dev):
    from comat_amd import ops
    calls = []

    class Spy:
        def __init__(self, b):
            self.b = b

        def __getattr__(self, name):
            calls.append(name)
            return getattr(self.b, name)
    ops.set_kernel_backend(Spy(ops.kernels()))
    seen = {}
    for sched in (None, lr_schedule("cosine", 1e-2, warmup=1, total=6)):
        for kw in ({}, dict(accum_steps=1), dict(accum_steps=2)):
            gen = torch.Generator().manual_seed(1)
            p, g = torch.randn(300, generator=gen).to(dev), torch.randn(300, generator=gen).to(dev)
            calls.clear()
            opt = FlatAdamW([(p, g)], 1e-2, (0.9, 0.999), 1e-8, 1e-2, 0.1, schedule=sched, **kw)
            opt.step()
            opt.step()
            seen[(sched is None, kw.get("accum_steps"))] = (list(calls), p.clone())
    for plain in (True, False):
        assert seen[(plain, None)][0] == seen[(plain, 1)][0] and torch.equal(seen[(plain, None)][1], seen[(plain, 1)][1])
        assert not {"accum_zero", "adamw_window", "window_tick"} & set(seen[(plain, 1)][0])
    assert seen[(True, 1)][0] == ["sumsq", "adamw", "adamw_tick"] * 2
    assert seen[(True, 2)][0] == ["lr_schedule_eval"] + ["sumsq", "adamw_window", "window_tick"] * 2
    assert seen[(False, 2)][0] == ["lr_schedule_eval"] + ["sumsq", "adamw_window", "window_tick"] * 2
    with pytest.raises(ValueError, match="accum_steps"):
        FlatAdamW([(p, g)], 1e-2, (0.9, 0.999), 1e-8, 1e-2, 0.1, accum_steps=0)


# ---- 5. the trainer against the CPU oracle ----------------------------------------------------------------------------------
def world(dtype, dev, gan=True, **fields):
    cfg, batch, W, tr = make_world(dtype, dev, False, gan=gan)
    cfg = dataclasses.replace(cfg, **fields)
    return cfg, batch, W, CoMatTrainer(tr.pipe, tr.bank, tr.blip, tr.D, cfg, seed=0)


@pytest.fixture(params=[("sim", torch.float32), pytest.param(("hip", torch.float32), marks=pytest.mark.gpu),
                        pytest.param(("hip", torch.bfloat16), marks=pytest.mark.gpu)], ids=["sim-fp32", "hip-fp32", "hip-bf16"])
def dev_dtype(request):
    backend, dtype = request.param
    return request.getfixturevalue(backend), dtype  # the `sim` / `hip` fixture installs the backend and releases it


def test_trainer_accumulates_like_the_oracle(dev_dtype):
    """N = 2 over two different micro-batches: nothing moves after the first; after the second the flat gradients are the mean of
    the oracle's two and the parameters torch AdamW's on the clipped mean, within the limits of
    tests/test_step.py::test_train_step_matches_oracle for the dtype"""
    from oracle import step as OS
    dev, dtype = dev_dtype
    cfg, A, W, tr = world(dtype, dev, gradient_accumulation_steps=2)
    B = fresh_inputs(A, torch.Generator().manual_seed(21), dtype)
    stepA, stepB = dict(training_steps=[1, 2], crop=(1, 0, 63, 63)), dict(training_steps=[0, 1], crop=(0, 1, 63, 63))
    refs = [OS.train_step(W, b, cfg, s["training_steps"], s["crop"]) for b, s in ((A, stepA), (B, stepB))]
    mean = lambda get: [(a + b) / 2 for a, b in zip(get(refs[0]), get(refs[1]))]
    bank, dbank = tr.bank, tr.D.bank
    g_params, d_params = [W["lora"][n] for n in bank.names], [W["d_lora"][n] for n in dbank.names] + [W["head_w"], W["head_b"]]
    g_mean = mean(lambda r: [r["g_grads"][n] for n in bank.names])
    d_mean = mean(lambda r: [r["d_grads"][n] for n in dbank.names] + list(r["head_grads"]))
    for params, grads, lr, betas, clip in ((g_params, g_mean, cfg.lr, (cfg.adam_beta1, cfg.adam_beta2), cfg.max_grad_norm),
                                           (d_params, d_mean, cfg.lr_D, (cfg.adam_beta1_D, cfg.adam_beta2_D), cfg.max_grad_norm_D)):
        for p, g in zip(params, grads):
            p.grad = g.clone()
        topt = torch.optim.AdamW(params, lr=lr, betas=betas, eps=cfg.adam_epsilon, weight_decay=cfg.adam_weight_decay)
        torch.nn.utils.clip_grad_norm_(params, clip)
        topt.step()
    start = [t.clone() for t in (bank.flat, dbank.flat, tr.D.head)]
    la = tr.train_step(A, **stepA)
    loss_a = float(la["step_loss"])
    assert la["sync_gradients"] is False
    for t, s, name in zip((bank.flat, dbank.flat, tr.D.head), start, ("G LoRA", "D LoRA", "D head")):
        assert torch.equal(t, s), f"{name} parameters moved on a micro-step that does not close"
    assert tr.opt.counters.tolist() == [0, 0] and tr.opt.window.tolist() == [1] and tr.opt_D.window.tolist() == [1]
    lb = tr.train_step(B, **stepB)
    assert lb["sync_gradients"] is True
    f = 1.0 if dtype == torch.float32 else 4.0
    check(lb["step_loss"], refs[1]["loss"], dtype, "step loss of B is logged unscaled", factor=f)
    check(lb["D_loss"], refs[1]["D_loss"], dtype, "D_loss of B is logged unscaled", factor=f)
    check(lb["train_loss"], (torch.tensor([loss_a]) + lb["step_loss"].detach().cpu().float().reshape(1)) / 2, F32, "train_loss")
    check(lb["train_loss"], ((refs[0]["loss"] + refs[1]["loss"]) / 2).reshape(1), dtype, "train_loss against the oracle", factor=f)
    cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])
    fp32 = dtype == torch.float32
    lim, lim_d, lim_h, lim_p = (1e-3, 1e-3, 3e-3, 3e-4) if fp32 else (BF16_GRAD_LIMIT, BF16_D_GRAD_LIMIT, BF16_HEAD_GRAD_LIMIT, 2e-2)
    errs = dict(g=rel_l2(bank.flat_grad, cat(g_mean)), d=rel_l2(dbank.flat_grad, cat(d_mean[:-2])),
                head=rel_l2(tr.D.head_grad, cat(d_mean[-2:])), p=rel_l2(bank.flat, cat(g_params)),
                pd=rel_l2(dbank.flat, cat(d_params[:-2])))
    print(f"accumulated step {dtype} {dev.type}: " + " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    assert errs["g"] < lim and errs["d"] < lim_d and errs["head"] < lim_h, errs
    assert errs["p"] < lim_p and errs["pd"] < lim_p, errs
    assert tr.opt.counters.tolist() == [1, 0] and tr.opt_D.counters.tolist() == [1, 0] and tr.opt.window.tolist() == [0]
    assert not torch.equal(bank.flat, start[0]) and not torch.equal(dbank.flat, start[1])


def test_schedule_lengths_are_counted_in_micro_steps(dev):
    _, _, _, tr = world(F32, dev, gan=False, gradient_accumulation_steps=3, lr_scheduler="linear", lr_warmup_steps=2,
                        max_train_steps=5)
    assert (tr.opt.schedule.warmup, tr.opt.schedule.total) == (6, 15) and tr.opt.accum_steps == 3


def test_config_refuses_less_than_one_micro_step():
    for bad in (0, -1):
        with pytest.raises(ValueError, match="gradient_accumulation_steps"):
            StepConfig(gradient_accumulation_steps=bad)
    assert StepConfig().gradient_accumulation_steps == 1 and StepConfig.sdxl().gradient_accumulation_steps == 1


# ---- 6. the graph steppers ---------------------------------------------------------------------------------------------------
ACCUM3 = dict(gradient_accumulation_steps=3, lr_scheduler="linear", lr_warmup_steps=1, max_train_steps=4)
CALLS = PLAN + [PLAN[0]]  # 7 calls: two windows and a bit


def assert_same_state(tr_e, tr_g, what):
    for a, b, name in ((tr_e.bank.flat, tr_g.bank.flat, "G LoRA"), (tr_e.D.bank.flat, tr_g.D.bank.flat, "D LoRA"),
                       (tr_e.D.head, tr_g.D.head, "D head"), (tr_e.bank.flat_grad, tr_g.bank.flat_grad, "G gradient"),
                       (tr_e.D.bank.flat_grad, tr_g.D.bank.flat_grad, "D gradient")):
        assert torch.equal(a, b), f"{what}: {name} differs"
    for oe, og in ((tr_e.opt, tr_g.opt), (tr_e.opt_D, tr_g.opt_D)):
        for a, b in zip(oe.m + oe.v, og.m + og.v):
            assert torch.equal(a, b), f"{what}: optimizer moments differ"
        assert oe.counters.tolist() == og.counters.tolist() and oe.window.tolist() == og.window.tolist(), what
        assert oe._index == og._index == int(og.window[0]), f"{what}: the host's copy of the window index"
    assert tr_e.opt.train_loss.tolist() == tr_g.opt.train_loss.tolist(), what
    assert float(tr_e.opt.lr_now[0]) == float(tr_g.opt.lr_now[0]), what


def record_exchanges(monkeypatch, trainer, log, call):
    from comat_amd.dist import GradReducer
    real = GradReducer.start

    def start(self, *flats):
        if self is trainer.reducer:
            log.append((call[0], len(flats)))
        return real(self, *flats)
    monkeypatch.setattr(GradReducer, "start", start)


@pytest.mark.gpu
@pytest.mark.parametrize("stepper", ["graph", "graph_split", "segments"])
def test_steppers_run_whole_windows_from_their_graphs(hip, stepper, monkeypatch):
    """N = 3, 7 calls: the graph steppers against eager micro-steps, bit for bit after every call, with the graphs they have (one
    per key).  The exchange is started on the closing calls only; a whole-step graph on one rank holds no exchange at all, so
    there only the eager first use of a key (call 3 here) can start one."""
    from comat_amd.segments import SegmentedStep
    if stepper == "graph_split":
        monkeypatch.setenv("COMAT_GRAPH_SPLIT", "1")
    else:
        monkeypatch.delenv("COMAT_GRAPH_SPLIT", raising=False)
    dtype = torch.bfloat16
    _, batch, _, tr_e = world(dtype, hip, **ACCUM3)
    _, _, _, tr_g = world(dtype, hip, **ACCUM3)
    if stepper == "segments":
        tr_e.pipe.share_text_kv = False  # as tests/test_lr_schedule.py::test_segmented_step_runs_the_schedule
        st = SegmentedStep(tr_g)
    else:
        st = GraphedStep(tr_g)
        assert st.supported(batch)
    log, call = [], [0]
    record_exchanges(monkeypatch, tr_g, log, call)
    gen = torch.Generator().manual_seed(31)
    for it, (ts, crop) in enumerate(CALLS):
        call[0] = it + 1
        b = fresh_inputs(batch, gen, dtype)
        le = tr_e.train_step(b, training_steps=ts, crop=crop)
        lg = st(b, training_steps=ts, crop=crop)
        torch.cuda.synchronize()
        assert st.failed is None, st.failed
        for k in ("step_loss", "Blip", "G_loss", "D_loss", "train_loss"):
            assert float(le[k]) == float(lg[k]), f"call {it + 1}: {k} {float(le[k])} (eager) vs {float(lg[k])} ({stepper})"
        assert le["sync_gradients"] is lg["sync_gradients"] is ((it + 1) % 3 == 0)
        assert_same_state(tr_e, tr_g, f"{stepper}, call {it + 1}")
    assert tr_g.opt.counters.tolist() == [2, 0] and tr_g.opt_D.counters.tolist() == [2, 0] and tr_g.opt.window.tolist() == [1]
    if stepper != "segments":
        assert len(st.graphs) == 2
    assert {c for c, _ in log} == ({3} if stepper == "graph" else {3, 6}), log
    assert all(sum(n for c, n in log if c == cl) == 3 for cl in {c for c, _ in log}), log  # G, D LoRA, D head: once each


# ---- 7. two ranks over gloo ---------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world_size, port, out_dir):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world_size), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(2)
    from comat_amd import dist as cdist
    from comat_amd import ops
    from sim_backend import SimKernels
    ops.set_kernel_backend(SimKernels())  # (the worker process ends with it installed)
    dev = torch.device("cpu")
    cdist.init(backend="gloo")
    _, batch, _, tr = world(F32, dev, gradient_accumulation_steps=2)
    bufs = dict(G=tr.bank.flat_grad, D=tr.D.bank.flat_grad, head=tr.D.head_grad)
    reduced = {k: 0 for k in bufs}
    real = dist.all_reduce

    def counting(t, *a, **kw):
        for k, b in bufs.items():
            reduced[k] += t.data_ptr() == b.data_ptr()
        return real(t, *a, **kw)
    dist.all_reduce = counting
    p0 = {k: t.clone() for k, t in dict(G=tr.bank.flat, D=tr.D.bank.flat, head=tr.D.head).items()}
    gen = torch.Generator().manual_seed(100 + rank)  # each rank: its own micro-batches
    windows, local = [], None
    for it in range(4):
        closing = tr.opt.closing
        real_start = tr.reducer.start
        if closing:  # what this rank hands to the exchange: its own window sum
            def start(*flats, _real=real_start):
                for k, b in bufs.items():
                    if any(f.data_ptr() == b.data_ptr() for f in flats):
                        local[k] = b.clone()
                return _real(*flats)
            local = {}
            tr.reducer.start = start
        logs = tr.train_step(fresh_inputs(batch, gen, F32), **STEP)
        tr.reducer.start = real_start
        assert logs["sync_gradients"] is closing
        if closing:
            windows.append(local)
    dist.all_reduce = real
    gathered = tr.gather_logs(logs)
    mine = {k: float(v.reshape(-1)[0]) for k, v in logs.items() if torch.is_tensor(v)}
    torch.save(dict(reduced=reduced, windows=windows, p0=p0, gathered=gathered, mine=mine,
                    params=dict(G=tr.bank.flat.clone(), D=tr.D.bank.flat.clone(), head=tr.D.head.clone())),
               os.path.join(out_dir, f"rank{rank}.pt"))
    cdist.barrier()
    dist.destroy_process_group()


def test_two_ranks_exchange_once_per_window(tmp_path, sim):
    """N = 2, 4 micro-steps on 2 ranks (gloo, simulated kernels): each gradient buffer is all-reduced exactly twice, the replicas
    stay equal, and equal to one process stepping on the mean of the ranks' window sums; gather_logs gives the rank mean of the
    gathered names and the local value of the others"""
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [torch.load(os.path.join(tmp_path, f"rank{i}.pt"), weights_only=False) for i in range(2)]
    cfg = StepConfig(lr=1e-2, lr_D=1e-2)  # the rates of make_world
    for i in range(2):
        assert r[i]["reduced"] == dict(G=2, D=2, head=2), r[i]["reduced"]
        assert len(r[i]["windows"]) == 2
    assert not torch.equal(r[0]["windows"][0]["G"], r[1]["windows"][0]["G"])  # the ranks really saw different data
    for k in ("G", "D", "head"):
        assert torch.equal(r[0]["params"][k], r[1]["params"][k]), f"{k}: the replicas drifted apart"
        assert not torch.equal(r[0]["params"][k], r[0]["p0"][k])
    for names, lr, betas, clip in ((("G",), cfg.lr, (cfg.adam_beta1, cfg.adam_beta2), cfg.max_grad_norm),
                                   (("D", "head"), cfg.lr_D, (cfg.adam_beta1_D, cfg.adam_beta2_D), cfg.max_grad_norm_D)):
        segs = [(r[0]["p0"][k].clone(), torch.zeros_like(r[0]["p0"][k])) for k in names]
        opt = FlatAdamW(segs, lr, betas, cfg.adam_epsilon, cfg.adam_weight_decay, clip)
        for w in range(2):
            for (_, g), k in zip(segs, names):
                g.copy_((r[0]["windows"][w][k] + r[1]["windows"][w][k]) / 2)
            opt.step()
        for (p, _), k in zip(segs, names):
            assert torch.allclose(p, r[0]["params"][k], rtol=1e-5, atol=1e-7), f"{k}: not the update on the rank-mean gradient"
    for i in range(2):
        g = r[i]["gathered"]
        assert set(g) == {"Blip", "G_loss", "D_loss", "train_loss", "step_loss", "lr"}
        for k in ("Blip", "G_loss", "D_loss", "train_loss"):
            want = np.float32(np.float32(r[0]["mine"][k]) + np.float32(r[1]["mine"][k])) / np.float32(2)
            assert g[k] == pytest.approx(float(want), rel=1e-6), k
            assert r[0]["mine"][k] != r[1]["mine"][k]
        assert g["step_loss"] == r[i]["mine"]["step_loss"] and g["lr"] == r[i]["mine"]["lr"]


def test_gather_logs_with_one_process(dev):
    _, batch, _, tr = world(F32, dev, gan=False, reward_norm=True)
    logs = tr.train_step(batch, **STEP)
    g = tr.gather_logs(logs)
    assert set(g) == {"Blip", "train_loss", "step_loss", "lr", "reward_norm"}
    assert g["Blip"] == float(logs["Blip"]) and g["train_loss"] == g["step_loss"] == float(logs["step_loss"])
    assert g["lr"] == float(np.float32(tr.cfg.lr)) and g["reward_norm"] == float(logs["reward_norm"][0]) > 0
    assert all(type(v) is float for v in g.values()) and logs["sync_gradients"] is True


# ---- 8. checkpoint -----------------------------------------------------------------------------------------------------------
def test_checkpoint_at_a_closed_window(dev, tmp_path):
    gan = dev.type == "cuda"
    kw = dict(gradient_accumulation_steps=2, lr_scheduler="linear", lr_warmup_steps=1, max_train_steps=4)
    _, batch, _, tr_a = world(F32, dev, gan=gan, **kw)
    gen = torch.Generator().manual_seed(13)
    optim = lambda tr: dict(G=tr.opt, D=tr.opt_D) if gan else dict(G=tr.opt)
    for i, (ts, crop) in enumerate(PLAN[:4]):
        if i == 3:  # mid-window: the partial gradient is not part of the state
            with pytest.raises(ValueError, match="window"):
                tr_a.opt.state_dict()
            with pytest.raises(ValueError, match="window"):
                checkpoint.save_checkpoint(str(tmp_path / "mid"), tr_a.bank, tr_a.D, optim=optim(tr_a))
        tr_a.train_step(fresh_inputs(batch, gen, F32), training_steps=ts, crop=crop)
    assert tr_a.opt.state_dict()["accum"] == (2, 0)
    full = str(tmp_path / "full")
    checkpoint.save_checkpoint(full, tr_a.bank, tr_a.D, optim=optim(tr_a))
    _, _, _, tr_b = world(F32, dev, gan=gan, **kw)
    tr_b.train_step(fresh_inputs(batch, torch.Generator().manual_seed(99), F32), **STEP)  # leaves tr_b mid-window
    ptrs = [t.data_ptr() for t in (tr_b.opt.window, tr_b.opt.counters, tr_b.opt.lr_now, tr_b.opt.train_loss)]
    checkpoint.load_checkpoint(full, tr_b.bank, tr_b.D, optim=optim(tr_b))
    assert ptrs == [t.data_ptr() for t in (tr_b.opt.window, tr_b.opt.counters, tr_b.opt.lr_now, tr_b.opt.train_loss)]
    assert tr_b.opt.window.tolist() == [0] and tr_b.opt._index == 0 and tr_b.opt.counters.tolist() == [2, 0]
    assert tr_b.opt.train_loss.tolist() == tr_a.opt.train_loss.tolist()
    for ts, crop in PLAN[4:6]:  # one more window on both
        b = fresh_inputs(batch, gen, F32)
        la, lb = tr_a.train_step(b, training_steps=ts, crop=crop), tr_b.train_step(b, training_steps=ts, crop=crop)
        assert float(la["step_loss"]) == float(lb["step_loss"]) and la["sync_gradients"] is lb["sync_gradients"]
    assert torch.equal(tr_a.bank.flat, tr_b.bank.flat) and tr_a.opt.counters.tolist() == tr_b.opt.counters.tolist() == [3, 0]
    for a, b in zip(tr_a.opt.m + tr_a.opt.v + [tr_a.opt.lr_now, tr_a.opt.train_loss],
                    tr_b.opt.m + tr_b.opt.v + [tr_b.opt.lr_now, tr_b.opt.train_loss]):
        assert torch.equal(a, b)
    if gan:
        assert torch.equal(tr_a.D.bank.flat, tr_b.D.bank.flat) and torch.equal(tr_a.D.head, tr_b.D.head)
    # a state saved under another number of micro-steps is refused
    _, _, _, tr_c = world(F32, dev, gan=gan, **{**kw, "gradient_accumulation_steps": 3})
    with pytest.raises(ValueError, match="accum_steps"):
        checkpoint.load_checkpoint(full, tr_c.bank, tr_c.D, optim=optim(tr_c))


def test_state_from_before_the_feature_loads(dev):
    p, g = torch.ones(8, dtype=F32, device=dev), torch.ones(8, dtype=F32, device=dev)
    a = FlatAdamW([(p, g)], 1e-2, (0.9, 0.999), 1e-8, 1e-2, 0.1)
    a.step()
    old = {k: v for k, v in a.state_dict().items() if k != "accum"}  # what optim_state.pt held before the field existed
    assert set(old) == {"m", "v", "counters", "schedule"}
    b = FlatAdamW([(p.clone(), g.clone())], 1e-2, (0.9, 0.999), 1e-8, 1e-2, 0.1, accum_steps=1)
    b.load_state_dict(old)
    assert b.counters.tolist() == [1, 0] and torch.equal(b.m[0], a.m[0])
    with pytest.raises(ValueError, match="accum_steps"):
        FlatAdamW([(p.clone(), g.clone())], 1e-2, (0.9, 0.999), 1e-8, 1e-2, 0.1, accum_steps=2).load_state_dict(old)
