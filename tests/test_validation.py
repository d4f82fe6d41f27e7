"""Validation sampling inside the trainer (comat_amd/validate.py, CoMatTrainer.validate; training_script.py:428-494) on the tiny
step world of tests/test_text_encoder_step.py: 64 x 64 images, 3 denoise steps, 2 prompts x 2 images.

No tolerance anywhere.  The bytes of a run are the definition of comat_image_u8 (tests/test_image_u8.py::expected) applied to the
VAE decode of the sampler's latents, computed by hand from the same draws; the invariance tests run the same steps twice from one
seed - `step, step, step` and `step, validate, step, validate, step` - and compare everything a later step reads, bit for bit."""
import dataclasses
import struct
import types
import zlib

import numpy as np
import pytest
import torch

from comat_amd import config, ops
from comat_amd.validate import (ValidationConfig, ValidationResult, Validator, contact_sheet, draw_noise, sample_seed, save_images,
                                write_png)
from helpers import fp8_state
from test_image_u8 import expected
from test_text_encoder_step import BS, CLIP, L, _ids, make_world
from validate_sim import val_dev  # noqa: F401 - fixture

F32 = torch.float32
VCFG = ValidationConfig(num_inference_steps=3, num_validation_images=2, seed=11, height=64, width=64, batch_size=2)
STEPS = [dict(training_steps=[1, 2], crop=(1, 0, 63, 63)), dict(training_steps=[1, 2], crop=(0, 1, 63, 63)),
         dict(training_steps=[1, 2], crop=(1, 1, 63, 63))]


@pytest.fixture
def vdev(val_dev):
    with fp8_state():
        yield val_dev


def val_batch(w, P=2, seed=40, captions=True):
    """validation prompts for the world w, under the training batch's keys"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    ucfg = w.tr.pipe.unet.cfg
    b = {}
    if w.tr.cfg.text_flag is not None:
        ids, null = _ids(P, seed=seed)
        b.update(prompt_input_ids=ids, null_input_ids=null)
        if w.tr.pipe.is_sdxl:
            C2 = ucfg.cross_attention_dim - CLIP.hidden
            b.update(prompt_embeds_2=r(P, L, C2), negative_prompt_embeds_2=r(P, L, C2))
    else:
        Lb = w.batch["prompt_embeds"].shape[1]
        b.update(prompt_embeds=r(P, Lb, ucfg.cross_attention_dim), negative_prompt_embeds=r(P, Lb, ucfg.cross_attention_dim))
    if w.tr.pipe.is_sdxl:
        b.update(pooled_prompt_embeds=r(P, ucfg.pooled_dim), negative_pooled_prompt_embeds=r(P, ucfg.pooled_dim),
                 add_time_ids=(64, 64, 0, 0, 64, 64))
    if captions:
        ids = torch.randint(1, config.TINY_BLIP.vocab_size, (P, 9), generator=g)
        b.update(blip_input_ids=ids, blip_attention_mask=torch.ones_like(ids))
    return b


# ---- 1. the draws ------------------------------------------------------------------------------------------------------------
def test_draw_noise_depends_on_its_three_integers_only():
    state = torch.random.get_rng_state()
    lat, noises = draw_noise(11, 1, 0, 8, 8, 3)
    assert lat.shape == (4, 8, 8) and noises.shape == (3, 4, 8, 8) and lat.dtype == noises.dtype == F32
    torch.manual_seed(123)
    torch.randn(5)
    lat2, noises2 = draw_noise(11, 1, 0, 8, 8, 3)
    assert torch.equal(lat, lat2) and torch.equal(noises, noises2)
    torch.random.set_rng_state(state)
    draw_noise(11, 1, 0, 8, 8, 3)
    assert torch.equal(torch.random.get_rng_state(), state), "the global generator was advanced"
    seeds = {sample_seed(s, p, i) for s in (0, 11, 12) for p in range(4) for i in range(4)}
    assert len(seeds) == 48 and all(0 <= s < 2 ** 63 for s in seeds)
    assert sample_seed(11, 1, 0) != sample_seed(11, 0, 1)
    assert not torch.equal(draw_noise(11, 0, 1, 8, 8, 3)[0], lat)


class RecordingPipe:
    """a stand-in pipeline that records what the validator hands the sampler and decodes zeros"""
    is_sdxl, graphed, attn_dict, device = False, None, {}, "cpu"

    def __init__(self):
        self.calls = []
        self.scheduler = types.SimpleNamespace(num_inference_steps=None, timesteps=[], set_timesteps=lambda n: list(range(n)))
        self.unet = types.SimpleNamespace(cfg=types.SimpleNamespace(in_channels=4))

    def forward(self, prompt_embeds, negative_prompt_embeds, latents=None, noises=None, **kw):
        assert kw["training_timesteps"] == () and kw["output_type"] == "latent_tokens" and not torch.is_grad_enabled()
        self.calls.append((prompt_embeds.clone(), latents.clone(), [n.clone() for n in noises]))
        return torch.zeros(latents.shape[0] * 64, 4)

    def decode_tokens(self, lat, bs, h, w, raw=False):
        assert raw
        return torch.zeros(bs * 64 * 64, 3), 64, 64


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1)])
@pytest.mark.parametrize("batch_size", [1, 3, 4])
def test_a_sample_gets_the_same_draws_whatever_the_grouping(sim, batch_size, order):
    from validate_sim import ValidateSimKernels
    ops.set_kernel_backend(ValidateSimKernels())
    pipe = RecordingPipe()
    P, N = 3, 2
    marks = torch.tensor(order, dtype=F32).reshape(P, 1, 1).expand(P, 5, 6).contiguous()  # prompt content: which prompt this is
    cfg = dataclasses.replace(VCFG, batch_size=batch_size, num_validation_images=N)
    torch.manual_seed(batch_size)
    state = torch.random.get_rng_state()
    res = Validator(pipe).run(cfg, marks, marks)
    assert torch.equal(torch.random.get_rng_state(), state)
    assert res.images.shape == (P, N, 64, 64, 3) and res.images.dtype == torch.uint8 and res.seed == 11
    assert bool((res.images == 128).all()) and not res.bad.any() and res.caption_loss is None  # rint(0.5 * 255) = 128: half to even
    seen, k = [], 0
    for pe, lat, noises in pipe.calls:
        assert lat.shape[0] <= batch_size
        for j in range(lat.shape[0]):
            p, i = divmod(k, N)  # prompts outer, images inner
            assert int(pe[j, 0, 0]) == order[p], "the sample's prompt is not the one of its place"
            want_lat, want_noises = draw_noise(11, p, i, 8, 8, 3)
            assert torch.equal(lat[j], want_lat) and all(torch.equal(noises[s][j], want_noises[s]) for s in range(3))
            seen.append((p, i))
            k += 1
    assert seen == [(p, i) for p in range(P) for i in range(N)]
    assert len(pipe.calls) == -(-P * N // batch_size)


def test_a_run_without_a_seed_reports_the_one_it_drew(sim):
    from validate_sim import ValidateSimKernels
    ops.set_kernel_backend(ValidateSimKernels())
    pipe = RecordingPipe()
    e = torch.zeros(1, 5, 6)
    res = Validator(pipe).run(dataclasses.replace(VCFG, seed=None, num_validation_images=1), e, e)
    assert isinstance(res.seed, int) and 0 <= res.seed < 2 ** 63
    assert torch.equal(pipe.calls[0][1][0], draw_noise(res.seed, 0, 0, 8, 8, 3)[0])


# ---- 2. the bytes ------------------------------------------------------------------------------------------------------------
def by_hand(w, vb, cfg, P):
    """the definition applied to vae(forward(...)) with the same draws and the same grouping -> (bytes [P, N, H, W, 3], images in
    [0, 1] as tokens per sample)"""
    pipe, N = w.tr.pipe, cfg.num_validation_images
    samples = [(p, i) for p in range(P) for i in range(N)]
    out, floats = [], []
    guided = cfg.guidance_scale > 1
    graphed, pipe.graphed = pipe.graphed, None  # eager launches, as a validation call without prepared graphs
    with torch.no_grad():
        for k in range(0, len(samples), cfg.batch_size):
            chunk = samples[k:k + cfg.batch_size]
            idx = torch.tensor([p for p, _ in chunk])
            draws = [draw_noise(cfg.seed, p, i, 8, 8, cfg.num_inference_steps) for p, i in chunk]
            lat = pipe.forward(vb["prompt_embeds"][idx], vb["negative_prompt_embeds"][idx] if guided else None, height=64, width=64,
                               training_timesteps=(), num_inference_steps=cfg.num_inference_steps, guidance_scale=cfg.guidance_scale,
                               latents=torch.stack([d[0] for d in draws]),
                               noises=[torch.stack([d[1][s] for d in draws]) for s in range(cfg.num_inference_steps)],
                               output_type="latent_tokens", guidance_rescale=cfg.guidance_rescale)
            z0 = ops.cast_grad(ops.affine(lat, 1.0 / pipe.vae.cfg.scaling_factor, 0.0), getattr(pipe.vae, "dtype", pipe.dtype))
            raw, H, W = pipe.vae(z0, len(chunk), 8, 8)
            assert (H, W) == (64, 64)
            out.append(expected(raw.float().cpu().numpy()).reshape(len(chunk), 64, 64, 3))
            img01 = ops.affine(raw, 0.5, 0.5)
            floats += [img01[j * 64 * 64:(j + 1) * 64 * 64] for j in range(len(chunk))]
    pipe.graphed = graphed
    return np.concatenate(out).reshape(P, N, 64, 64, 3), floats


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_run_gives_the_definition_of_the_decoded_sampler_output(vdev, dtype):
    w = make_world(dtype, vdev, flag=False)
    vb = val_batch(w)
    cfg = dataclasses.replace(VCFG, batch_size=3)  # 4 samples: a call of three and a call of one
    state = torch.random.get_rng_state()
    res = w.tr.validate(cfg, vb)
    assert torch.equal(torch.random.get_rng_state(), state), "run advanced the global generator"
    want, floats = by_hand(w, vb, cfg, 2)
    got = res.images.numpy()
    assert got.shape == (2, 2, 64, 64, 3) and res.seed == 11 and not res.bad.any()
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
    assert len(np.unique(got)) > 20 and not np.array_equal(got[0, 0], got[0, 1]) and not np.array_equal(got[0, 0], got[1, 0])
    again = w.tr.validate(cfg, vb)
    assert torch.equal(again.images, res.images) and torch.equal(again.caption_loss, res.caption_loss)
    # the caption loss: minus the captioner's score of the same float images, sample by sample
    assert res.caption_loss.shape == (2, 2) and res.caption_loss.dtype == F32
    with torch.no_grad():
        for k, img in enumerate(floats):
            p = k // 2
            score = w.tr.blip.score(img, 1, 64, 64, vb["blip_input_ids"][p:p + 1].to(vdev), vb["blip_attention_mask"][p:p + 1].to(vdev))[0]
            assert float(res.caption_loss[p, k % 2]) == -float(score.float()), (p, k % 2)
    assert Validator(w.tr.pipe).run(cfg, vb["prompt_embeds"], vb["negative_prompt_embeds"]).caption_loss is None


# ---- 3. a validation call leaves training where it was ---------------------------------------------------------------------------
EPOCH0 = [0]  # fp8._epoch (a process-wide count of closed steps) when the run began


def snapshot(tr, logs):
    """everything a later step reads, as host copies"""
    c = lambda t: None if t is None else t.detach().cpu().clone()
    s = {}
    for i, b in enumerate(tr.trained):
        s[f"bank{i}.flat"], s[f"bank{i}.grad"] = c(b.flat), c(b.flat_grad)
    s["D.flat"], s["D.grad"], s["D.head"], s["D.head_grad"] = c(tr.D.bank.flat), c(tr.D.bank.flat_grad), c(tr.D.head), c(tr.D.head_grad)
    for name, o in (("opt", tr.opt), ("opt_D", tr.opt_D)):
        for j, t in enumerate(list(o.m) + list(o.v)):
            s[f"{name}.moment{j}"] = c(t)
        for f in ("counters", "window", "train_loss", "lr_now", "gnorm_sq"):
            s[f"{name}.{f}"] = c(getattr(o, f))
        s[f"{name}.index"] = o._index
    for k, v in logs.items():
        s[f"logs.{k}"] = c(v) if isinstance(v, torch.Tensor) else v
    st = ops.fp8._states.get(ops.fp8._key(tr.device))
    if st is not None:
        for f in ("scale", "amax", "hist", "count", "clip_steps", "worst", "clip_now"):
            s[f"fp8.{f}"] = c(getattr(st, f)[:st.n])
        s["fp8.host"] = (st.n, list(st.ready), sorted(st.used), st.unready, ops.fp8._epoch - EPOCH0[0])
    s["switches"] = (ops.fused_masked_attention(), ops.fp8_scaling(), ops.fp8_recipe(), ops.side_streams_enabled(),
                     tr.pipe.share_text_kv, tr.pipe.gradient_checkpointing, tr.rng.getstate())
    s["pipe"] = (sorted(tr.pipe.attn_dict), tr.pipe.graphed is None, tr.pipe.trained_runner is None)
    return s


def assert_same(a, b, what):
    assert a.keys() == b.keys(), (what, a.keys() ^ b.keys())
    for k in a:
        if isinstance(a[k], torch.Tensor):
            bits = lambda t: t.reshape(-1).contiguous().view(torch.uint8)  # (NaN equals NaN, -0 is not +0)
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(bits(a[k]), bits(b[k])), f"{what}: {k} differs"
        else:
            assert a[k] == b[k], f"{what}: {k} differs: {a[k]} / {b[k]}"


def run_steps(build, validate, stepper=None, vcfg=VCFG, extra=None):
    """three steps of a fresh world, a validation call after the first and after the second where `validate` -> snapshots"""
    ops.fp8_reset()
    w = build()
    tr = w.tr
    EPOCH0[0] = ops.fp8._epoch
    if extra is not None:
        extra(w)
    step = tr.train_step if stepper is None else stepper(tr)
    vb = val_batch(w)
    trace, results = [], []
    for it, fixed in enumerate(STEPS):
        if w.tr.cfg.attrcon:
            fixed = dict(fixed, attrcon_steps=[2])
        logs = step(w.batch, **fixed)
        trace.append(snapshot(tr, dict(logs)))
        if validate and it < 2:
            sentinel = tr.pipe.attn_dict = {"kept": torch.ones(1)}
            graphs = None if tr.pipe.graphed is None else len(tr.pipe.graphed.graphs)
            results.append(tr.validate(vcfg, vb))
            assert tr.pipe.attn_dict is sentinel, "pipe.attn_dict was not put back"
            tr.pipe.attn_dict = {}
            assert graphs is None or len(tr.pipe.graphed.graphs) == graphs, "a validation call captured a graph"
            assert_same(snapshot(tr, {}), {k: v for k, v in trace[-1].items() if not k.startswith("logs.")}, f"right after validation {it}")
    return trace, results


def check_invariance(build, **kw):
    plain, _ = run_steps(build, False, **kw)
    mixed, results = run_steps(build, True, **kw)
    for it, (a, b) in enumerate(zip(plain, mixed)):
        assert_same(a, b, f"step {it}")
    assert not torch.equal(plain[0]["bank0.flat"], plain[2]["bank0.flat"]), "the steps did not move the weights"
    assert len(results) == 2 and results[0].images.shape == (2, 2, 64, 64, 3)
    assert not torch.equal(results[0].images, results[1].images), "validation does not see the step between its two calls"
    return results


def fp8_world(dev):
    from test_fp8 import _fp8_step_world
    ops.set_fp8_scaling("delayed")
    ops.set_fp8_recipe(history=2, margin=1.0)
    tr, _, batch, cfg, _ = _fp8_step_world(dev, F32)
    assert tr.fp8_calibrate(batch)
    return types.SimpleNamespace(tr=tr, batch=batch, cfg=cfg)


CASES = {
    "lora": lambda d: make_world(F32, d, flag=False),
    "accum2": lambda d: make_world(F32, d, flag=False, gradient_accumulation_steps=2),  # validation 1 falls inside the window
    "text_lora_ids": lambda d: make_world(F32, d, flag=True),
    "cfg_scale_1": lambda d: make_world(F32, d, flag=False, cfg_scale=1.0),
    "cfg_rescale": lambda d: make_world(F32, d, flag=False, cfg_rescale=0.7),
    "sdxl": lambda d: make_world(F32, d, flag=False, sdxl=True),
    "fp8_delayed": fp8_world,
}


@pytest.mark.parametrize("case", list(CASES))
def test_validation_between_steps_changes_no_later_result(vdev, case):
    build = lambda: CASES[case](vdev)
    # validation samples as the run trains: --cfg_scale and --cfg_rescale serve both (training_script.py:472)
    vcfg = dataclasses.replace(VCFG, guidance_scale=1.0 if case == "cfg_scale_1" else 7.5, guidance_rescale=0.7 if case == "cfg_rescale" else 0.0)
    results = check_invariance(build, vcfg=vcfg)
    assert all(r.caption_loss is not None and bool(torch.isfinite(r.caption_loss).all()) and not r.bad.any() for r in results)


@pytest.mark.gpu
@pytest.mark.parametrize("stepper", ["segments", "graph", "prepared"])
def test_validation_between_replayed_steps(hip, stepper):
    """the captured graphs of SegmentedStep / GraphedStep replay after a validation call with the bits they gave before; `prepared`:
    the no-grad UNet's graphs exist for the validation call's key too, so validation itself replays them"""
    from comat_amd.segments import SegmentedStep
    from comat_amd.step import GraphedStep
    with fp8_state():
        build = lambda: make_world(torch.bfloat16, hip, flag=False)
        extra = None
        if stepper == "prepared":
            extra = lambda w: w.tr.pipe.prepare_graphs(BS, 64, 64, w.batch["prompt_embeds"].shape[1], 3)
        make = {"segments": SegmentedStep, "graph": GraphedStep, "prepared": None}[stepper]
        check_invariance(build, stepper=make, extra=extra)
    ops.set_fused_masked_attention(False)


# ---- 4. files ----------------------------------------------------------------------------------------------------------------
def read_png(path):
    """-> (width, height, colour type, pixel rows as numpy) with zlib and struct alone; every chunk's CRC is checked"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, tag = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        chunks.append((tag, body))
        at += 12 + n
    assert [t for t, _ in chunks][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    Wd, Hd, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0)
    ch = {2: 3, 0: 1}[colour]
    raw = np.frombuffer(zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT")), dtype=np.uint8).reshape(Hd, 1 + Wd * ch)
    assert not raw[:, 0].any()  # filter type 0 on every row
    return Wd, Hd, colour, raw[:, 1:].reshape(Hd, Wd, ch)


def test_write_png(tmp_path):
    g = torch.Generator().manual_seed(3)
    rgb = torch.randint(0, 256, (5, 7, 3), generator=g, dtype=torch.uint8)
    grey = torch.randint(0, 256, (4, 9), generator=g, dtype=torch.uint8)
    for name, img, colour in (("rgb.png", rgb, 2), ("grey.png", grey, 0), ("grey1.png", grey[..., None], 0), ("np.png", rgb.numpy(), 2)):
        p = write_png(str(tmp_path / name), img)
        Wd, Hd, c, px = read_png(p)
        arr = np.asarray(img).reshape(Hd, Wd, -1)
        assert (Hd, Wd) == tuple(np.asarray(img).shape[:2]) and c == colour and np.array_equal(px, arr)
    for bad in (rgb.float(), rgb[..., :2], torch.zeros(0, 4, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="write_png"):
            write_png(str(tmp_path / "bad.png"), bad)


def test_write_png_is_read_by_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    g = torch.Generator().manual_seed(4)
    rgb = torch.randint(0, 256, (6, 5, 3), generator=g, dtype=torch.uint8)
    grey = torch.randint(0, 256, (3, 8), generator=g, dtype=torch.uint8)
    assert np.array_equal(np.asarray(Image.open(write_png(str(tmp_path / "a.png"), rgb))), rgb.numpy())
    assert np.array_equal(np.asarray(Image.open(write_png(str(tmp_path / "b.png"), grey))), grey.numpy())


def fake_result(P=2, N=3, H=4, W=5, pad=1):
    g = torch.Generator().manual_seed(9)
    return ValidationResult(images=torch.randint(0, 256, (P, N, H, W, 3), generator=g, dtype=torch.uint8), bad=torch.zeros(P, N, dtype=torch.bool),
                            seed=1, caption_loss=None, sheet_pad=pad, device="cpu")


def test_contact_sheet_and_save_images(val_dev, tmp_path):
    res = fake_result()
    res.device = str(val_dev)
    sheets = contact_sheet(res)  # 3 images: 2 a row, a last row with one
    assert len(sheets) == 2 and all(s.shape == (1 + 2 * 5, 1 + 2 * 6, 3) and s.dtype == torch.uint8 for s in sheets)
    for p, s in enumerate(sheets):
        want = torch.full((11, 13, 3), 255, dtype=torch.uint8)
        for j in range(3):
            y0, x0 = 1 + (j // 2) * 5, 1 + (j % 2) * 6
            want[y0:y0 + 4, x0:x0 + 5] = res.images[p, j]
        assert torch.equal(s, want)
    assert contact_sheet(res, cols=3, background=0)[0].shape == (6, 19, 3)
    paths = save_images(str(tmp_path), res, step=120)
    names = sorted(p[len(str(tmp_path)) + 1:] for p in paths)
    assert names == sorted([f"validation/step_120/prompt_{i}_{j}.png" for i in range(2) for j in range(3)]
                           + [f"validation/step_120/sheet_{i}.png" for i in range(2)])
    assert np.array_equal(read_png(paths[1])[3], res.images[0, 1].numpy())
    assert np.array_equal(read_png(paths[-1])[3], sheets[1].numpy())


# ---- 5. misuse ---------------------------------------------------------------------------------------------------------------
def test_config_and_from_args():
    assert ValidationConfig() == ValidationConfig(40, 7.5, 0.0, 4, None, 512, 512, 1, 2)
    args = types.SimpleNamespace(total_step=25, cfg_scale=5.0, cfg_rescale=0.7, num_validation_images=3, seed=7, resolution=256)
    assert ValidationConfig.from_args(args, batch_size=2) == ValidationConfig(25, 5.0, 0.7, 3, 7, 256, 256, 2, 2)
    for field, bad in (("num_validation_images", 0), ("num_validation_images", -1), ("batch_size", 0), ("num_inference_steps", 0),
                       ("height", 60), ("width", 0), ("sheet_pad", -1), ("seed", 1.5)):
        with pytest.raises(ValueError, match=field):
            ValidationConfig(**{field: bad})


def test_misuse_names_the_field(val_dev):
    w = make_world(F32, val_dev, flag=False)
    vb = val_batch(w, captions=False)
    ids, null = _ids(2, seed=1)
    with pytest.raises(ValueError, match="prompt_input_ids"):  # ids, but no text tower to encode them
        w.tr.validate(VCFG, dict(vb, prompt_input_ids=ids, null_input_ids=null))
    with pytest.raises(ValueError, match="prompt_embeds"):
        w.tr.validate(VCFG, {})
    with pytest.raises(ValueError, match="negative_prompt_embeds"):
        w.tr.validate(VCFG, dict(prompt_embeds=vb["prompt_embeds"]))
    w.tr.validate(dataclasses.replace(VCFG, guidance_scale=1.0, num_validation_images=1), dict(prompt_embeds=vb["prompt_embeds"][:1]))
    with pytest.raises(ValueError, match="input_ids"):
        Validator(w.tr.pipe).run(VCFG, vb["prompt_embeds"], vb["negative_prompt_embeds"], input_ids=torch.ones(2, 9, dtype=torch.long),
                                 attention_mask=torch.ones(2, 9, dtype=torch.long))
    x = make_world(F32, val_dev, flag=False, sdxl=True)
    xb = val_batch(x, captions=False)
    with pytest.raises(ValueError, match="pooled_prompt_embeds"):
        x.tr.validate(VCFG, {k: v for k, v in xb.items() if "pooled" not in k})
    t = make_world(F32, val_dev, flag=True)
    with pytest.raises(ValueError, match="prompt_embeds"):  # a trained tower encodes ids: embeddings are refused (encode_prompts)
        t.tr.validate(VCFG, dict(val_batch(t, captions=False), prompt_embeds=vb["prompt_embeds"]))
