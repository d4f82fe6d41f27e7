"""The plumbing the step's drivers share (CPU, through the ABI simulator): the fixed-address staging of a batch
(streams.StaticBatch), what follows a failed graph capture (CoMatTrainer.abandon_capture, SegmentedStep._capture) and the
replay-or-capture helper of segments.SegmentedStep."""
import numpy as np
import pytest
import torch

from comat_amd import streams
from comat_amd.segments import SegmentedStep
from comat_amd.streams import StaticBatch
from test_step import make_world


def _batch(bs=2, L=7):
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g)
    ids = torch.randint(1, 50, (bs, 9), generator=g)
    return dict(prompt_embeds=r(bs, L, 16), negative_prompt_embeds=r(bs, L, 16), gan_null_embeds=r(bs, L, 16),
                gan_pooled_null_embeds=r(bs, 12), latents=r(bs, 4, 8, 8), real_latents=r(bs, 4, 8, 8),
                noises=[r(bs, 4, 8, 8) for _ in range(3)], blip_input_ids=ids, blip_attention_mask=(ids != 3).long(),
                add_time_ids=(64, 64, 0, 0, 64, 64), attributes=[[[2, 3], [5]]], masks=[np.zeros((2, 8, 8), dtype=bool)])


def _addresses(staged):
    return {k: v.data_ptr() for k, v in staged.items() if torch.is_tensor(v)}, [n.data_ptr() for n in staged["noises"]]


def test_static_batch_fixed_addresses_and_values(sim):
    sb = StaticBatch(sim)
    b1, b2 = _batch(), _batch()
    b2["latents"] = b2["latents"] + 1
    s1, fresh1 = sb.stage(b1, strict=True)
    a1 = _addresses(s1)
    s2, fresh2 = sb.stage(b2, strict=True)
    assert fresh1 and not fresh2
    assert _addresses(s2) == a1
    assert set(a1[0]) == set(StaticBatch.KEYS) - {"pooled_prompt_embeds", "negative_pooled_prompt_embeds"} and len(a1[1]) == 3
    for k in a1[0]:
        assert s2[k].data_ptr() != b2[k].data_ptr() and torch.equal(s2[k], b2[k]) and s2[k].dtype == b2[k].dtype
    assert all(torch.equal(d, s) and d.data_ptr() != s.data_ptr() for d, s in zip(s2["noises"], b2["noises"]))
    assert s2["blip_input_ids"].dtype == torch.int64 and s2["blip_attention_mask"].dtype == torch.int64
    # host metadata passes through by reference
    for k in ("add_time_ids", "attributes", "masks"):
        assert s2[k] is b2[k]


def test_static_batch_reallocates_per_key(sim):
    sb = StaticBatch(sim)
    s0, _ = sb.stage(_batch(), strict=True)
    a0 = _addresses(s0)
    keep = s0  # the old buffers stay alive: a new one cannot land on a freed address
    b = dict(_batch(), prompt_embeds=torch.randn(2, 5, 16))  # one key changes its shape
    s1, fresh = sb.stage(b, strict=True)
    a1 = _addresses(s1)
    assert fresh and torch.equal(s1["prompt_embeds"], b["prompt_embeds"])
    assert [k for k in a0[0] if a0[0][k] != a1[0][k]] == ["prompt_embeds"] and a0[1] == a1[1]
    assert not sb.stage(b, strict=True)[1]
    # another number of noises
    b = dict(b, noises=b["noises"] + [torch.randn(2, 4, 8, 8)])
    s2, fresh = sb.stage(b, strict=True)
    assert fresh and len(s2["noises"]) == 4 and _addresses(s2)[0] == a1[0]
    assert all(torch.equal(d, s) for d, s in zip(s2["noises"], b["noises"]))
    assert not sb.stage(b, strict=True)[1]
    # a dtype change of one key
    b3 = dict(b, latents=b["latents"].double())
    s3, fresh = sb.stage(b3, strict=True)
    assert fresh and s3["latents"].dtype == torch.float64
    # a key disappears, then appears again
    b4 = {k: v for k, v in b3.items() if k != "gan_pooled_null_embeds"}
    s4, fresh = sb.stage(b4, strict=True)
    assert fresh and "gan_pooled_null_embeds" not in s4
    assert not sb.stage(b4, strict=True)[1]
    assert sb.stage(b3, strict=True)[1]
    del keep


def test_static_batch_unlisted_tensor(sim):
    sb = StaticBatch(sim)
    b = dict(_batch(), renoise=torch.randn(2, 4, 8, 8))
    with pytest.raises(KeyError, match="StaticBatch.KEYS"):
        sb.stage(b, strict=True)
    staged, _ = sb.stage(b, strict=False)
    assert staged["renoise"] is b["renoise"]


def test_static_batch_keeps_nothing_of_an_earlier_batch(sim):
    sb = StaticBatch(sim)
    first, _ = sb.stage(dict(_batch(), caption="a red cube"), strict=True)
    later = _batch()
    del later["attributes"]
    staged, _ = sb.stage(later, strict=True)
    assert first["caption"] == "a red cube" and "caption" not in staged and "attributes" not in staged
    assert set(staged) == set(later) and staged is not first


def test_abandon_capture_drops_streams_and_queued_work(sim):
    _, batch, _, tr = make_world(torch.float32, sim, False)
    tr._d_pending, tr._d_keep = True, torch.zeros(3)
    streams._ttq[(sim, 0)] = streams._TTQueue(sim, None, None)
    streams._side_keep.append(torch.zeros(1))
    streams._join_queued = True
    tr.abandon_capture()
    assert tr._d_stream is None and tr._g_stream is None and tr._d_pending is False and tr._d_keep is None
    assert not streams._ttq and not streams._side_dirty and not streams._side_keep and streams._join_queued is False


class _FailingSegment:
    name = "stub"

    def capture(self, inputs, **kw):
        raise RuntimeError("x")


def test_failed_capture_becomes_a_state_and_the_step_goes_on_eagerly(sim, capsys):
    dtype = torch.float32
    _, batch, _, tr_e = make_world(dtype, sim, False)
    _, _, _, tr_g = make_world(dtype, sim, False)
    st = SegmentedStep(tr_g)
    tr_g._d_pending = True
    assert st._capture(_FailingSegment(), ()) is False
    assert st.failed == "stub: RuntimeError: x" and tr_g._d_pending is False
    assert "capture of segment 'stub' failed" in capsys.readouterr().err
    # through the helper: the eager result is this call's result, and nothing is registered
    st.failed = None
    where, ran = {}, []
    outs = st._replay_or_capture(where, "k", lambda x: ran.append(x) or (x + 1,), (torch.ones(2),), _FailingSegment)
    assert torch.equal(outs[0], torch.full((2,), 2.0)) and len(ran) == 1
    assert where == {} and st.head_seg is None and st.d_seg is None and not st.unet_segs
    assert st.failed == "stub: RuntimeError: x"
    # from now on a call of the stepper is the plain eager step, bit for bit
    kw = dict(training_steps=[1, 2], crop=(1, 0, 63, 63))
    le, lg = tr_e.train_step(batch, **kw), st(batch, **kw)
    same = lambda a, b: torch.allclose(a.float(), b.float(), rtol=0, atol=0)
    for k in ("step_loss", "Blip", "G_loss", "D_loss"):
        assert same(le[k], lg[k]), k
    assert same(tr_e.bank.flat, tr_g.bank.flat) and same(tr_e.D.bank.flat, tr_g.D.bank.flat) and same(tr_e.D.head, tr_g.D.head)
    assert same(tr_e.opt.m[0], tr_g.opt.m[0]) and same(tr_e.opt.v[0], tr_g.opt.v[0])
    assert same(tr_e.opt_D.m[0], tr_g.opt_D.m[0]) and same(tr_e.opt_D.v[0], tr_g.opt_D.v[0])
