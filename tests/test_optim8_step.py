"""`StepConfig.use_8bit_adam` (training_script.py:216-223) through the trainer on the tiny configuration: the first update against
the trainer without the flag (bit-identical: both run the same element arithmetic on the same gradients from zero moments), three
steps, the segment graphs against eager steps, gradient accumulation, and the optimizer state through a checkpoint in both formats."""
import os

import pytest
import torch

import optim8_reference as R
from comat_amd import checkpoint, optim8
from comat_amd.segments import SegmentedStep
from comat_amd.step import FlatAdamW
from test_full_finetuning import CROP, TS, make_step_world
from test_lr_schedule import PLAN, STEP, fresh_inputs, world

pytestmark = pytest.mark.gpu

F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32


def make(kind, dev, flag, dtype, **fields):
    """(batch, trainer, the fixed step arguments): the LoRA world of tests/test_step.py or the fully trained UNet of
    tests/test_full_finetuning.py, both with the GAN leg"""
    if kind == "lora":
        _, batch, tr = world(dtype, dev, use_8bit_adam=flag, **fields)
        return batch, tr, STEP
    _, batch, _, tr = make_step_world(dtype, dev, use_8bit_adam=flag, **fields)
    return batch, tr, dict(training_steps=TS, crop=CROP)


def params(tr):
    return dict(G=tr.bank.flat, D=tr.D.bank.flat, head=tr.D.head)


def state8(opt):
    """every tensor of an 8-bit optimizer's state, by name"""
    out = {}
    for name in ("m", "v", "m8", "v8", "absmax_m", "absmax_v"):
        out.update({f"{name}[{i}]": t for i, t in enumerate(getattr(opt, name)) if t is not None})
    return out


def assert_same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
        same = torch.equal(x.view(I32), y.view(I32)) if x.dtype == F32 else torch.equal(x, y)
        assert same, f"{what}: {k} differs"


@pytest.mark.parametrize("kind,dtype", [("lora", F32), ("full", BF16)], ids=["lora-fp32", "full-bf16"])
def test_first_update_is_exact_and_three_steps_run(hip, kind, dtype):
    batch, plain, step = make(kind, hip, False, dtype)
    _, tr, _ = make(kind, hip, True, dtype)
    assert isinstance(tr.opt, optim8.FlatAdamW8bit) and isinstance(tr.opt_D, optim8.FlatAdamW8bit)
    assert type(plain.opt) is FlatAdamW
    assert tr.opt.seg8 == [True] and tr.opt_D.seg8 == [True, False]
    assert tr.opt.m == [None] and tr.opt.m8[0].dtype == torch.uint8 and tr.opt.absmax_m[0].numel() == -(-tr.bank.flat.numel() // 256)
    head_m = tr.opt_D.m[1]  # under 4096 elements: fp32 moments and the fp32 kernel
    assert tr.opt_D.m8[1] is None and head_m.dtype == F32 and head_m.shape == tr.D.head.shape
    start = {k: v.clone() for k, v in params(tr).items()}
    plain.train_step(batch, **step)
    logs = tr.train_step(batch, **step)
    assert_same_bits(params(plain), params(tr), f"{kind}: parameters after the first update")
    assert all(not torch.equal(v, start[k]) for k, v in params(tr).items())
    assert torch.equal(head_m, plain.opt_D.m[1]) and float(head_m.abs().max()) > 0
    for _ in range(2):
        logs = tr.train_step(batch, **step)
    for k in ("step_loss", "Blip", "G_loss", "D_loss", "grad_norm_sq", "lr"):
        assert bool(torch.isfinite(logs[k].float()).all()), k
    assert tr.opt.t == 3 and tr.opt_D.t == 3 and tr.opt.counters.tolist() == [3, 0]
    fp32_bytes = sum(t.numel() * t.element_size() for t in plain.opt.m + plain.opt.v)
    ratio = tr.opt.state_bytes() / fp32_bytes
    print(f"{kind}: 8-bit generator state {tr.opt.state_bytes()} bytes, fp32 {fp32_bytes}: {ratio:.4f}")
    assert ratio < 0.27  # 2 + 8 / 256 bytes over 8 is 0.254


def test_segment_graphs_replay_bit_for_bit(hip):
    """three calls of SegmentedStep under the flag = three eager steps: parameters, codes and scales"""
    dtype = BF16
    batch, tr_e, _ = make("lora", hip, True, dtype)
    _, tr_s, _ = make("lora", hip, True, dtype)
    tr_e.pipe.share_text_kv = False  # as tests/test_lr_schedule.py::test_segmented_step_runs_the_schedule
    st = SegmentedStep(tr_s)
    gen = torch.Generator().manual_seed(12)
    for it in range(3):
        b = fresh_inputs(batch, gen, dtype)
        le, ls = tr_e.train_step(b, **STEP), st(b, **STEP)
        torch.cuda.synchronize()
        assert st.failed is None, st.failed
        assert float(le["step_loss"]) == float(ls["step_loss"])
        assert_same_bits(params(tr_e), params(tr_s), f"call {it + 1}: parameters")
        for oe, os_ in ((tr_e.opt, tr_s.opt), (tr_e.opt_D, tr_s.opt_D)):
            assert_same_bits(state8(oe), state8(os_), f"call {it + 1}: optimizer state")
            assert oe.counters.tolist() == os_.counters.tolist() == [it + 1, 0]
    assert float(tr_s.opt.absmax_m[0].max()) > 0


def test_gradient_accumulation(hip):
    """N = 2: nothing of the state moves on the opening micro-step, one update per two calls"""
    batch, tr, _ = make("lora", hip, True, F32, gradient_accumulation_steps=2)
    gen = torch.Generator().manual_seed(21)
    snap = lambda: {**{k: v.clone() for k, v in params(tr).items()},
                    **{f"G {k}": v.clone() for k, v in state8(tr.opt).items()},
                    **{f"D {k}": v.clone() for k, v in state8(tr.opt_D).items()}}
    before = snap()
    logs = tr.train_step(fresh_inputs(batch, gen, F32), **STEP)
    assert logs["sync_gradients"] is False
    assert_same_bits(before, snap(), "opening micro-step")
    assert tr.opt.counters.tolist() == [0, 0] and tr.opt.window.tolist() == [1]
    logs = tr.train_step(fresh_inputs(batch, gen, F32), **STEP)
    assert logs["sync_gradients"] is True
    after = snap()
    assert all(not torch.equal(before[k], after[k]) for k in after), [k for k in after if torch.equal(before[k], after[k])]
    assert tr.opt.counters.tolist() == [1, 0] and tr.opt_D.counters.tolist() == [1, 0] and tr.opt.window.tolist() == [0]
    for _ in range(2):
        tr.train_step(fresh_inputs(batch, gen, F32), **STEP)
    assert tr.opt.t == 2 and tr.opt_D.t == 2


def test_checkpoint_in_both_formats(hip, tmp_path):
    optim = lambda tr: dict(G=tr.opt, D=tr.opt_D)
    gen = torch.Generator().manual_seed(13)
    batch, tr_a, _ = make("lora", hip, True, F32)
    _, tr_f, _ = make("lora", hip, False, F32)
    for ts, crop in PLAN[:2]:
        b = fresh_inputs(batch, gen, F32)
        tr_a.train_step(b, training_steps=ts, crop=crop)
        tr_f.train_step(b, training_steps=ts, crop=crop)
    d8, d32 = str(tmp_path / "bits8"), str(tmp_path / "bits32")
    checkpoint.save_checkpoint(d8, tr_a.bank, tr_a.D, optim=optim(tr_a))
    checkpoint.save_checkpoint(d32, tr_f.bank, tr_f.D, optim=optim(tr_f))
    file8 = torch.load(os.path.join(d8, checkpoint.OPTIM_STATE_NAME), weights_only=False)
    file32 = torch.load(os.path.join(d32, checkpoint.OPTIM_STATE_NAME), weights_only=False)
    assert file8["G"]["state_bits"] == 8 and file8["G"]["seg8"] == (True,) and file8["D"]["seg8"] == (True, False)
    assert "state_bits" not in file32["G"] and all(t.device.type == "cpu" for t in file8["D"]["m8"] + file8["D"]["m"])
    # 1. resume: load into a fresh 8-bit trainer, one more step on both - the uninterrupted run's bits
    _, tr_b, _ = make("lora", hip, True, F32)
    ptrs = [t.data_ptr() for t in state8(tr_b.opt).values()]
    checkpoint.load_checkpoint(d8, tr_b.bank, tr_b.D, optim=optim(tr_b))
    assert ptrs == [t.data_ptr() for t in state8(tr_b.opt).values()], "the buffers captured graphs hold must stay"
    assert_same_bits(state8(tr_a.opt), state8(tr_b.opt), "after the load")
    b3 = fresh_inputs(batch, gen, F32)
    ts, crop = PLAN[2]
    tr_a.train_step(b3, training_steps=ts, crop=crop), tr_b.train_step(b3, training_steps=ts, crop=crop)
    assert_same_bits(params(tr_a), params(tr_b), "the step after the load: parameters")
    for oa, ob in ((tr_a.opt, tr_b.opt), (tr_a.opt_D, tr_b.opt_D)):
        assert_same_bits(state8(oa), state8(ob), "the step after the load: optimizer state")
        assert oa.counters.tolist() == ob.counters.tolist() == [3, 0]
    # 2. an fp32 file into the 8-bit optimizer: quantised, nearest or tied against the file's moments
    _, tr_c, _ = make("lora", hip, True, F32)
    checkpoint.load_checkpoint(d32, tr_c.bank, tr_c.D, optim=optim(tr_c))
    for name, opt in optim(tr_c).items():
        m, v = file32[name]["m"][0], file32[name]["v"][0]
        m8, v8, am, av = (t[0].cpu() for t in (opt.m8, opt.v8, opt.absmax_m, opt.absmax_v))
        assert torch.equal(am.view(I32), R.block_max(m).view(I32)) and torch.equal(av.view(I32), R.block_max(v).view(I32))
        R.assert_nearest_or_tied(m, m8, am, True, 2.0 ** -22, f"{name}: first moment quantised at the load")
        R.assert_nearest_or_tied(v, v8, av, False, 2.0 ** -22, f"{name}: second moment quantised at the load")
        assert opt.counters.tolist() == [2, 0]
    assert torch.equal(tr_c.opt_D.m[1].cpu(), file32["D"]["m"][1])  # the small segment: copied
    # 3. the 8-bit file into a plain FlatAdamW: dequantised, bit for bit
    _, tr_d, _ = make("lora", hip, False, F32)
    checkpoint.load_checkpoint(d8, tr_d.bank, tr_d.D, optim=optim(tr_d))
    for name, opt in optim(tr_d).items():
        f = file8[name]
        assert torch.equal(opt.m[0].cpu().view(I32), R.dequantize(f["m8"][0], f["absmax_m"][0], True).view(I32)), name
        assert torch.equal(opt.v[0].cpu().view(I32), R.dequantize(f["v8"][0], f["absmax_v"][0], False).view(I32)), name
    assert torch.equal(tr_d.opt_D.m[1].cpu(), file8["D"]["m"][0]) and tr_d.opt.counters.tolist() == [2, 0]
    # everything else as the parent class: another number of micro-steps is refused
    _, tr_n, _ = make("lora", hip, True, F32, gradient_accumulation_steps=2)
    with pytest.raises(ValueError, match="accum_steps"):
        checkpoint.load_checkpoint(d8, tr_n.bank, tr_n.D, optim=optim(tr_n))
