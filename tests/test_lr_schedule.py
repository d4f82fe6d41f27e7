"""Learning-rate schedules evaluated on the device (`--lr_scheduler`, `--lr_warmup_steps`, `--max_train_steps`;
training_script.py:290-295 get_scheduler, :664 `lr_scheduler.step()`, :667 `logs["lr"]`): the schedule kernels against
tests/golden/lr_schedules.json (recorded from the installed transformers / accelerate by tests/golden/make_lr_schedule_golden.py),
the device-rate AdamW pass against the by-value one bit for bit, the optimizer against torch + transformers, and the trainer,
its graph replays and its checkpoints with a schedule.

Bounds on a learning rate (the issue's "bound 1"):
  * constant, constant_with_warmup, linear: equal to float32(fixture).  Their evaluation is one IEEE double division and one
    multiplication in a fixed order, the same on the host and on the device.
  * cosine, cosine_with_restarts, polynomial: within 1 ulp of float32(fixture).  The device's double cos / pow may differ from
    the host's by a few double ulps, which after rounding to fp32 can flip the last bit only at a tie.
"""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

from comat_amd import _hip, checkpoint
from comat_amd.step import CoMatTrainer, FlatAdamW, GraphedStep, StepConfig, lr_schedule
from helpers import Window, check
from test_step import make_world

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "lr_schedules.json")))
BASE = FIX["base_lr"]
EXACT = ("constant", "constant_with_warmup", "linear")
F32 = torch.float32


def kernels():
    from comat_amd import ops
    return ops.kernels()


def assert_rate(got, ref, kind, what):
    """bound 1 of the module docstring; got: a float that came out of an fp32 word, ref: the fixture's double"""
    r32 = np.float32(ref)
    g32 = np.float32(got)
    assert float(g32) == float(got), (what, got)
    print(f"{what}: got {float(g32)!r} fixture {float(r32)!r}")
    if kind in EXACT:
        assert g32 == r32, f"{what}: {float(g32)!r} != float32(fixture) {float(r32)!r}"
    else:
        assert abs(float(g32) - float(r32)) <= float(np.spacing(np.abs(r32))), \
            f"{what}: {float(g32)!r} is more than 1 ulp from float32(fixture) {float(r32)!r}"


def sched_of(case, stride=1, base_lr=BASE):
    """the ABI struct of a fixture case, without the host-side refusals of step.lr_schedule (polynomial at W == T is recorded up
    to the clock at which the library raises)"""
    nc = case.get("num_cycles", 1.0 if case["kind"] == "cosine_with_restarts" else 0.5)
    return _hip.LrSchedule(_hip.LR_KINDS[case["kind"]], stride, case["warmup"], case["total"], base_lr, nc,
                           case.get("power", 1.0), 1e-7)


# ---- 1. the schedule against the fixture ----------------------------------------------------------------------------------
def test_fixture_covers_what_it_should():
    cases = FIX["cases"]
    for kind in _hip.LR_KINDS:
        assert {(c["warmup"], c["total"]) for c in cases if c["kind"] == kind} >= {(0, 10), (3, 10), (4, 4)}
    assert any(c["kind"] == "cosine_with_restarts" and c.get("num_cycles") == 2 for c in cases)
    assert any(c["kind"] == "polynomial" and c.get("power") == 2 for c in cases)
    for c in cases:  # every clock 0 .. T + 2, except where the library itself raised (polynomial, W == T, at clock T)
        if c["raises"]:
            assert c["kind"] == "polynomial" and c["warmup"] == c["total"] and len(c["lr"]) == c["total"]
        else:
            assert len(c["lr"]) == c["total"] + 3


@pytest.mark.parametrize("stride", [1, 3])
def test_schedule_eval_matches_the_fixture(dev, stride):
    """comat_lr_schedule_eval at every recorded clock of every case; stride 3: the counter k is read as clock 3 k"""
    k = kernels()
    jobs = [(c, n) for c in FIX["cases"] for n in range((len(c["lr"]) - 1) // stride + 1)]
    counters = torch.tensor([n for _, n in jobs], dtype=torch.int32, device=dev)
    out = torch.full((len(jobs),), float("nan"), dtype=F32, device=dev)
    for i, (c, n) in enumerate(jobs):
        k.lr_schedule_eval(sched_of(c, stride), counters[i:i + 1], out[i:i + 1])
    got = out.cpu().tolist()
    assert len(jobs) >= (250 if stride == 1 else 90)
    for (c, n), g in zip(jobs, got):
        assert_rate(g, c["lr"][n * stride], c["kind"],
                    f"{c['kind']} W={c['warmup']} T={c['total']} {c.get('num_cycles', '')}{c.get('power', '')} clock {n * stride}")


def test_tick_follows_the_accelerate_traces(dev):
    """the two rules of accelerate's AcceleratedScheduler, as recorded through it: a skipped optimizer step does not advance
    the schedule; without split_batches the schedule advances num_processes times per optimizer step"""
    k = kernels()
    for name, tr in FIX["accelerate_traces"].items():
        s = sched_of(tr, stride=tr.get("num_processes", 1))
        counters = torch.zeros(2, dtype=torch.int32, device=dev)
        word = torch.zeros(1, dtype=F32, device=dev)
        nsq = torch.zeros(1, dtype=F32, device=dev)
        k.lr_schedule_eval(s, counters, word)
        skipped = tr.get("skipped", [False] * (len(tr["lr"]) - 1))
        for i, skip in enumerate(skipped):
            assert_rate(float(word[0]), tr["lr"][i], tr["kind"], f"{name} before update {i}")
            nsq.fill_(float("inf") if skip else 1.0)
            k.adamw_tick_lr(counters, nsq, s, word)
        assert_rate(float(word[0]), tr["lr"][-1], tr["kind"], f"{name} after the last update")
        assert counters.tolist() == [len(skipped) - sum(skipped), sum(skipped)]


def test_contract_refusals(dev):
    k = kernels()
    counters = torch.zeros(2, dtype=torch.int32, device=dev)
    word = torch.full((1,), 7.0, dtype=F32, device=dev)
    nsq = torch.ones(1, dtype=F32, device=dev)
    good = dict(kind=3, stride=1, warmup=2, total=8, base_lr=BASE, num_cycles=0.5, power=1.0, lr_end=1e-7)
    bad = [dict(kind=6), dict(kind=-1), dict(stride=0), dict(warmup=-1), dict(kind=2, total=0), dict(kind=3, total=0),
           dict(kind=4, total=0), dict(kind=5, total=0), dict(kind=5, lr_end=BASE), dict(kind=5, base_lr=1e-8)]
    for change in bad:
        s = _hip.LrSchedule(**{**good, **change})
        with pytest.raises(RuntimeError, match="comat_lr_schedule_eval"):
            k.lr_schedule_eval(s, counters, word)
        with pytest.raises(RuntimeError, match="comat_adamw_tick_lr"):
            k.adamw_tick_lr(counters, nsq, s, word)
    for kind in (0, 1):  # the constant kinds do not read `total`
        k.lr_schedule_eval(_hip.LrSchedule(**{**good, "kind": kind, "total": 0}), counters, word)
    assert counters.tolist() == [0, 0]  # a refused tick launched nothing
    x = torch.zeros(8, dtype=F32, device=dev)
    with pytest.raises(RuntimeError, match="comat_adamw_lr"):
        k.adamw_lr(x, x, x, x, 8, None, 0.9, 0.999, 1e-8, 1e-2, counters, nsq, 0.1)
    with pytest.raises(RuntimeError, match="comat_adamw_lr"):
        k.adamw_lr(x, x, x, x, 8, word, 0.9, 0.999, 1e-8, 1e-2, None, nsq, 0.1)


def test_library_refuses_a_bad_schedule_without_launching():
    """the cross-compiled library's own argument check, without a GPU (as tests/test_abi.py does for the other entry points)"""
    import ctypes as C
    lib = _hip.load_library()
    bad = _hip.LrSchedule(9, 1, 0, 10, BASE, 0.5, 1.0, 1e-7)
    assert lib.comat_lr_schedule_eval(C.byref(bad), None, None, None) == -1
    assert b"unknown schedule kind 9" in lib.comat_last_error()
    ok = _hip.LrSchedule(3, 1, 0, 10, BASE, 0.5, 1.0, 1e-7)
    assert lib.comat_adamw_tick_lr(None, None, C.byref(ok), None, None) == -1 and b"null pointer" in lib.comat_last_error()
    assert lib.comat_adamw_lr(None, None, None, None, 0, None, 0.9, 0.999, 1e-8, 0.0, None, None, 0.1, 1.0, None) == -1
    assert C.sizeof(_hip.LrSchedule) == 4 * 8 + 4 * 8  # comat_lr_schedule


def test_host_side_refusals_name_the_field():
    with pytest.raises(ValueError, match="max_train_steps"):
        lr_schedule("cosine", BASE, warmup=2)
    with pytest.raises(ValueError, match="lr_scheduler"):
        lr_schedule("piecewise_constant", BASE)
    with pytest.raises(ValueError, match="max_train_steps != lr_warmup_steps"):
        lr_schedule("polynomial", BASE, warmup=4, total=4)  # transformers divides by zero at clock 4
    s = lr_schedule("cosine_with_restarts", BASE, warmup=1, total=9, steps_per_update=8)
    assert (s.kind, s.stride, s.warmup, s.total, s.num_cycles, s.lr_end) == (4, 8, 1, 9, 1.0, 1e-7)
    assert lr_schedule("cosine", BASE, total=9).num_cycles == 0.5
    c = StepConfig()
    assert (c.lr_scheduler, c.lr_warmup_steps, c.max_train_steps, c.lr_num_cycles, c.lr_power, c.lr_steps_per_update) == \
        ("constant", 0, None, None, 1.0, 1)


# ---- 2. adamw_lr against adamw, bit for bit -------------------------------------------------------------------------------
@pytest.mark.parametrize("left", [8, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 257, 4099])
def test_adamw_lr_matches_adamw_bit_for_bit(dev, n, left):
    """below one vector, one vector, tails, several blocks; left = 8: 16-byte aligned operands (the 16-byte path on the GPU),
    left = 1: misaligned (the 4-byte path).  Three consecutive steps with the clip active and a moving rate."""
    k = kernels()
    gen = torch.Generator().manual_seed(100 + n)
    hp = (0.9, 0.999, 1e-8, 1e-2)
    mk = lambda x: Window(1, n, dtype=F32, device=dev, lead=4, trail=4, left=left).put(x)  # lead 4: 16-byte aligned for odd n too
    init = [torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 0.01]
    A, B = [mk(x) for x in init], [mk(x) for x in init]
    gw = Window(1, n, dtype=F32, device=dev, lead=4, trail=4, left=left)
    for w in A + B + [gw]:
        assert (w.flat.data_ptr() % 16 == 0) == (left == 8)
    sched = _hip.LrSchedule(_hip.LR_KINDS["cosine"], 1, 2, 8, 5e-3, 0.5, 1.0, 1e-7)
    cA = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    cB = cA.clone()
    word = torch.zeros(1, dtype=F32, device=dev)
    nsq = torch.zeros(1, dtype=F32, device=dev)
    k.lr_schedule_eval(sched, cB, word)
    for step in range(3):
        g = (torch.rand(n, generator=gen) + 0.5) * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)  # |g|_2 >= 0.5 > max_norm
        gw.put(g)
        for w in A + B + [gw]:
            w.arm()
        nsq.zero_()
        k.sumsq(gw.flat, n, nsq)
        lr = float(word[0])
        assert lr > 0 and (step == 0 or lr != last), "the rate moves between the steps"
        last = lr
        k.adamw(A[0].flat, gw.flat, A[1].flat, A[2].flat, n, lr, *hp, 0, nsq, 0.1, step_dev=cA)
        k.adamw_tick(cA, nsq)
        k.adamw_lr(B[0].flat, gw.flat, B[1].flat, B[2].flat, n, word, *hp, cB, nsq, 0.1)
        k.adamw_tick_lr(cB, nsq, sched, word)
        for a, b, name in zip(A, B, "pmv"):
            assert torch.equal(a.get(), b.get()), f"step {step}: {name} differs from comat_adamw's"
            assert not torch.equal(b.get().cpu(), init["pmv".index(name)].reshape(1, n)), f"step {step}: {name} did not move"
        for w in A + B + [gw]:
            w.assert_guard_intact(f"n={n} left={left} step {step}")
        for w in A + B:
            w.assert_written(f"n={n} left={left} step {step}")
    assert cA.tolist() == cB.tolist() == [4, 0]
    # a non-finite norm: nothing moves but the count of skipped updates
    before = [w.get() for w in B]
    lr = float(word[0])
    for w in B:
        w.arm()
    nsq.fill_(float("inf"))
    k.adamw_lr(B[0].flat, gw.flat, B[1].flat, B[2].flat, n, word, *hp, cB, nsq, 0.1)
    k.adamw_tick_lr(cB, nsq, sched, word)
    for w, b in zip(B, before):
        assert torch.equal(w.get(), b)
        w.assert_guard_intact(f"n={n} left={left} skipped step")
    assert cB.tolist() == [4, 1] and float(word[0]) == lr


# ---- 3. the optimizer against torch + transformers ------------------------------------------------------------------------
def test_flat_adamw_with_schedule_matches_torch(dev):
    """FlatAdamW with cosine, W = 2, T = 8 over 8 steps (n = 4099 in two segments sharing the norm) against torch.optim.AdamW +
    clip_grad_norm_ + transformers.get_scheduler.  The 4th step's gradient holds an inf: the reference loop skips
    optimizer.step() AND scheduler.step() there (what accelerate does under a gradient scaler)."""
    from transformers import get_scheduler
    gen = torch.Generator().manual_seed(3)
    lr, betas, eps, wd, max_norm, n1, n2 = 5e-3, (0.9, 0.999), 1e-8, 1e-2, 0.1, 4000, 99
    p0 = [torch.randn(n1, generator=gen), torch.randn(n2, generator=gen)]
    ref_p = [torch.nn.Parameter(p.clone()) for p in p0]
    ropt = torch.optim.AdamW(ref_p, lr=lr, betas=betas, eps=eps, weight_decay=wd)
    rsched = get_scheduler("cosine", ropt, num_warmup_steps=2, num_training_steps=8)
    segs = [(p.clone().to(dev), torch.zeros(p.numel(), device=dev)) for p in p0]
    opt = FlatAdamW(segs, lr, betas, eps, wd, max_norm, schedule=lr_schedule("cosine", lr, warmup=2, total=8))
    assert opt.lr_now is not None
    word = opt.lr_now.data_ptr()
    assert_rate(float(opt.lr_now[0]), rsched.get_last_lr()[0], "cosine", "before the first update")
    for step in range(8):
        gs = [torch.randn(n1, generator=gen), torch.randn(n2, generator=gen)]
        if step == 3:
            gs[1][7] = float("inf")
        for (_, g), rp, x in zip(segs, ref_p, gs):
            g.copy_(x)
            rp.grad = x.clone()
        if all(bool(torch.isfinite(x).all()) for x in gs):
            torch.nn.utils.clip_grad_norm_(ref_p, max_norm)
            ropt.step()
            rsched.step()
        opt.step()
        assert_rate(float(opt.lr_now[0]), rsched.get_last_lr()[0], "cosine", f"after step {step + 1}")
    assert opt.counters.tolist() == [7, 1] and opt.lr_now.data_ptr() == word
    for (p, _), rp, name in zip(segs, ref_p, ("segment 0", "segment 1")):
        check(p, rp.detach(), F32, f"FlatAdamW with a cosine schedule, {name}", factor=0.5)
    assert not torch.equal(segs[0][0].cpu(), p0[0])


def test_constant_schedule_keeps_the_launches_of_no_schedule(dev):
    """schedule=None and `constant` at one scheduler step per update issue sumsq, adamw, adamw_tick with the host rate;
    `constant` at another stride owns the word (and holds the same rate)"""
    from comat_amd import ops
    calls = []

    class Spy:
        def __init__(self, b):
            self.b = b

        def __getattr__(self, name):
            calls.append(name)
            return getattr(self.b, name)
    ops.set_kernel_backend(Spy(ops.kernels()))
    res = []
    for sched in (None, lr_schedule("constant", 1e-2), lr_schedule("constant", 1e-2, steps_per_update=8)):
        gen = torch.Generator().manual_seed(1)
        p, g = torch.randn(300, generator=gen).to(dev), torch.randn(300, generator=gen).to(dev)
        calls.clear()
        opt = FlatAdamW([(p, g)], 1e-2, (0.9, 0.999), 1e-8, 1e-2, 0.1, schedule=sched)
        opt.step()
        opt.step()
        res.append((p.clone(), list(calls), opt.lr_now))
    assert res[0][1] == res[1][1] == ["sumsq", "adamw", "adamw_tick"] * 2 and res[0][2] is None and res[1][2] is None
    assert res[2][1] == ["lr_schedule_eval"] + ["sumsq", "adamw_lr", "adamw_tick_lr"] * 2
    assert float(res[2][2][0]) == float(np.float32(1e-2))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][0], res[2][0])


# ---- 4. the trainer -------------------------------------------------------------------------------------------------------
STEP = dict(training_steps=[1, 2], crop=(1, 0, 63, 63))


def world(dtype, dev, gan=True, **fields):
    """the miniature world of tests/test_step.py with StepConfig fields replaced.  gan=False: concept matching alone - a third of
    a step's cost on the CPU simulator, for the tests that are about the generator's optimizer only"""
    cfg, batch, W, tr = make_world(dtype, dev, False, gan=gan)
    if fields:
        cfg = dataclasses.replace(cfg, **fields)
        tr = CoMatTrainer(tr.pipe, tr.bank, tr.blip, tr.D, cfg, seed=0)
    return cfg, batch, tr


def test_trainer_warms_up(dev):
    cfg, batch, tr = world(F32, dev, gan=False, lr_scheduler="constant_with_warmup", lr_warmup_steps=2)
    flat0 = tr.bank.flat.clone()
    rates = []
    for i in range(3):
        logs = tr.train_step(batch, **STEP)
        rates.append(float(logs["lr"][0]))
        if i == 0:  # the first update runs at rate 0: nothing moves, weight decay included
            assert torch.equal(tr.bank.flat, flat0)
    assert rates == [float(np.float32(cfg.lr * 0.5)), float(np.float32(cfg.lr)), float(np.float32(cfg.lr))]
    assert not torch.equal(tr.bank.flat, flat0) and tr.opt.counters.tolist() == [3, 0]
    assert tr.opt_D.schedule is None and tr.opt_D.lr_now is None  # the discriminator's optimizer has no schedule


def test_default_trainer_is_the_trainer_without_a_schedule(dev):
    _, batch, tr_a = world(F32, dev, gan=False)
    cfg, _, tr_b = world(F32, dev, gan=False)
    assert tr_a.opt.schedule is None and tr_a.opt.lr_now is None
    tr_b.opt = FlatAdamW([(tr_b.bank.flat, tr_b.bank.flat_grad)], cfg.lr, (cfg.adam_beta1, cfg.adam_beta2), cfg.adam_epsilon,
                         cfg.adam_weight_decay, cfg.max_grad_norm, schedule=None)
    for _ in range(2):
        la = tr_a.train_step(batch, **STEP)
        tr_b.train_step(batch, **STEP)
        assert "lr" not in la
    assert torch.equal(tr_a.bank.flat, tr_b.bank.flat) and torch.equal(tr_a.opt.m[0], tr_b.opt.m[0])


# ---- 5. no host synchronisation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attrcon", [False, True])
def test_scheduled_step_has_no_host_synchronisation(attrcon):
    """tests/test_step.py::test_step_has_no_host_synchronisation with a cosine schedule: on the `meta` device with no-op
    kernels any read of a tensor's value raises"""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    from host_overhead import NullKernels
    from comat_amd import ops
    ops.set_kernel_backend(NullKernels())
    try:
        cfg, batch, W, tr = make_world(torch.bfloat16, torch.device("meta"), attrcon)
        cfg = dataclasses.replace(cfg, lr_scheduler="cosine", lr_warmup_steps=2, max_train_steps=6)
        tr = CoMatTrainer(tr.pipe, tr.bank, tr.blip, tr.D, cfg, seed=0)
        logs = tr.train_step(batch, training_steps=[1, 2], crop=(1, 0, 63, 63), attrcon_steps=[2])
        assert logs["lr"].device.type == "meta" and logs["step_loss"].device.type == "meta"
        assert tr.train_step(batch)["lr"] is logs["lr"]  # one word at a fixed address
    finally:
        ops.set_kernel_backend(None)


# ---- 6. graph replay ------------------------------------------------------------------------------------------------------
COSINE_2_6 = dict(lr_scheduler="cosine", lr_warmup_steps=2, max_train_steps=6, lr=BASE)
PLAN = [([1, 2], (1, 0, 63, 63)), ([1, 2], (0, 1, 63, 63)), ([0, 1], (1, 1, 63, 63)), ([1, 2], (0, 0, 63, 63)),
        ([0, 1], (0, 1, 63, 63)), ([1, 2], (1, 1, 63, 63))]


def fixture_2_6():
    return next(c for c in FIX["cases"] if (c["kind"], c["warmup"], c["total"]) == ("cosine", 2, 6))["lr"]


def fresh_inputs(batch, gen, dtype):
    b = dict(batch)
    b["latents"] = torch.randn(batch["latents"].shape, generator=gen)
    b["noises"] = [torch.randn(n.shape, generator=gen) for n in batch["noises"]]
    b["prompt_embeds"] = torch.randn(batch["prompt_embeds"].shape, generator=gen).to(dtype).float()
    return b


def assert_same_state(tr_e, tr_g, what):
    assert torch.equal(tr_e.bank.flat, tr_g.bank.flat), f"{what}: generator LoRA parameters differ"
    assert torch.equal(tr_e.D.bank.flat, tr_g.D.bank.flat), f"{what}: discriminator LoRA parameters differ"
    assert torch.equal(tr_e.D.head, tr_g.D.head), f"{what}: discriminator head differs"
    for oe, og in ((tr_e.opt, tr_g.opt), (tr_e.opt_D, tr_g.opt_D)):
        for a, b in zip(oe.m + oe.v, og.m + og.v):
            assert torch.equal(a, b), f"{what}: optimizer moments differ"
        assert oe.counters.tolist() == og.counters.tolist()
    assert float(tr_e.opt.lr_now[0]) == float(tr_g.opt.lr_now[0])


@pytest.mark.gpu
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_graphed_step_replays_with_the_moving_rate(hip, dtype, split, monkeypatch):
    """the plan of tests/test_step.py::test_graphed_step_matches_eager under cosine, W = 2, T = 6: the whole-step graph bakes
    the schedule and reads the counter and the word, so its replays run at the moving rate without a new capture"""
    if split:
        monkeypatch.setenv("COMAT_GRAPH_SPLIT", "1")
    _, batch, tr_e = world(dtype, hip, **COSINE_2_6)
    _, _, tr_g = world(dtype, hip, **COSINE_2_6)
    gs = GraphedStep(tr_g)
    assert gs.supported(batch)
    gen = torch.Generator().manual_seed(11)
    want = fixture_2_6()
    word = tr_g.opt.lr_now.data_ptr()
    for it, (ts, crop) in enumerate(PLAN):
        b = fresh_inputs(batch, gen, dtype)
        le = tr_e.train_step(b, training_steps=ts, crop=crop)
        lg = gs(b, training_steps=ts, crop=crop)
        torch.cuda.synchronize()
        assert gs.failed is None, gs.failed
        for k in ("step_loss", "Blip", "G_loss", "D_loss"):
            assert float(le[k]) == float(lg[k]), f"step {it}: {k} {float(le[k])} (eager) vs {float(lg[k])} (graph)"
        assert_same_state(tr_e, tr_g, f"step {it}")
        assert lg["lr"].data_ptr() == word
        assert_rate(float(lg["lr"][0]), want[it + 1], "cosine", f"graph, after step {it + 1}")
        assert_rate(float(le["lr"][0]), want[it + 1], "cosine", f"eager, after step {it + 1}")
    assert len(gs.graphs) == 2 and tr_g.opt.t == 6 and tr_g.opt_D.t == 6


@pytest.mark.gpu
def test_segmented_step_runs_the_schedule(hip):
    from comat_amd.segments import SegmentedStep
    dtype = torch.bfloat16
    _, batch, tr_e = world(dtype, hip, **COSINE_2_6)
    _, _, tr_s = world(dtype, hip, **COSINE_2_6)
    tr_e.pipe.share_text_kv = False  # replayed segments project the text keys / values once per call (tests/test_segments.py)
    st = SegmentedStep(tr_s)
    gen = torch.Generator().manual_seed(12)
    want = fixture_2_6()
    for it in range(3):
        b = fresh_inputs(batch, gen, dtype)
        le = tr_e.train_step(b, **STEP)
        ls = st(b, **STEP)
        torch.cuda.synchronize()
        assert st.failed is None, st.failed
        assert float(le["step_loss"]) == float(ls["step_loss"])
        assert_same_state(tr_e, tr_s, f"step {it}")
        assert_rate(float(ls["lr"][0]), want[it + 1], "cosine", f"segments, after step {it + 1}")


# ---- 7. checkpoint --------------------------------------------------------------------------------------------------------
def test_checkpoint_resumes_the_schedule(dev, tmp_path):
    gan = dev.type == "cuda"  # the discriminator's optimizer state too where a step is cheap
    _, batch, tr_a = world(F32, dev, gan=gan, **COSINE_2_6)
    gen = torch.Generator().manual_seed(13)
    for ts, crop in PLAN[:3]:
        tr_a.train_step(fresh_inputs(batch, gen, F32), training_steps=ts, crop=crop)
    plain, full = str(tmp_path / "plain"), str(tmp_path / "full")
    checkpoint.save_checkpoint(plain, tr_a.bank, tr_a.D)
    assert not os.path.exists(os.path.join(plain, checkpoint.OPTIM_STATE_NAME))
    checkpoint.save_checkpoint(full, tr_a.bank, tr_a.D, optim=dict(G=tr_a.opt, D=tr_a.opt_D))
    files = lambda d: sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)
    assert files(full) == sorted(files(plain) + [checkpoint.OPTIM_STATE_NAME])
    _, _, tr_b = world(F32, dev, gan=gan, **COSINE_2_6)
    ptrs = [t.data_ptr() for t in tr_b.opt.m + tr_b.opt.v + [tr_b.opt.counters, tr_b.opt.lr_now]]
    checkpoint.load_checkpoint(full, tr_b.bank, tr_b.D, optim=dict(G=tr_b.opt, D=tr_b.opt_D))
    assert ptrs == [t.data_ptr() for t in tr_b.opt.m + tr_b.opt.v + [tr_b.opt.counters, tr_b.opt.lr_now]]
    assert tr_b.opt.counters.tolist() == [3, 0] and tr_b.opt_D.counters.tolist() == [3 * gan, 0]
    assert_rate(float(tr_b.opt.lr_now[0]), fixture_2_6()[3], "cosine", "the word after the load")
    assert_same_state(tr_a, tr_b, "after the load")
    b4 = fresh_inputs(batch, gen, F32)
    ts, crop = PLAN[3]
    la = tr_a.train_step(b4, training_steps=ts, crop=crop)
    lb = tr_b.train_step(b4, training_steps=ts, crop=crop)
    assert float(la["step_loss"]) == float(lb["step_loss"])
    assert_same_state(tr_a, tr_b, "step 4")
    # a state saved under another schedule is refused: captured graphs bake the schedule
    _, _, tr_c = world(F32, dev, gan=gan, lr_scheduler="linear", lr_warmup_steps=2, max_train_steps=6, lr=BASE)
    with pytest.raises(ValueError, match="schedule"):
        checkpoint.load_checkpoint(full, tr_c.bank, tr_c.D, optim=dict(G=tr_c.opt, D=tr_c.opt_D))
