"""bank.MasterBank under its three subclasses - unet.VAEBank, unet.UNetBank, clip.ClipTextBank - on the tiny configurations:
layout, the refresh launch, state-dict round trip, one holder per layer, the step's protocol.  Simulator and real kernels.

The refresh identities are exact (no tolerance): the launch rounds the fp32 master ONCE to the compute dtype, round to nearest
even like torch's `.to()`, and writes the same bits in both orientations."""
import numpy as np
import pytest
import torch

from comat_amd import config, refresh, weights
from comat_amd.clip import TEXT_PREFIX, ClipTextBank, ClipTextEncoder
from comat_amd.unet import UNet, UNetBank, VAEBank, VAEDecoder

KINDS = ("vae", "unet", "clip")
DTYPES = (torch.bfloat16, torch.float32)
# per bank: a weight whose file lacks it / holds it in another shape, a layer and a request of ANOTHER kind than its model makes
PROBE = dict(vae=("decoder.conv_out.weight", "post_quant_conv", lambda b, n: b.conv(n)),
             unet=("conv_in.weight", "conv_in", lambda b, n: b.linear(n)),
             clip=("encoder.layers.1.mlp.fc1.weight", "encoder.layers.1.mlp.fc1", lambda b, n: b.norm(n)))


def source(kind):
    """the state dict a bank is built from (fresh tensors per call)"""
    if kind == "vae":
        sd = weights.make_vae_weights(config.TINY_VAE, perturb_norms=True)
        g = torch.Generator().manual_seed(3)  # entries the bank does not train: carried along as they came
        return {"encoder.conv_in.weight": torch.randn(8, 3, 3, 3, generator=g), "quant_conv.bias": torch.randn(8, generator=g), **sd}
    if kind == "unet":
        return weights.make_unet_weights(config.TINY_UNET, perturb_norms=True)
    return {TEXT_PREFIX + n: t for n, t in weights.make_clip_text_weights(config.TINY_CLIP_TEXT, perturb_norms=True).items()}


def make(kind, dtype, dev):
    """(bank, source state dict, a function that builds one more model over the bank)"""
    sd = source(kind)
    if kind == "vae":
        bank = VAEBank(config.TINY_VAE, sd, dtype, dev)
        model = lambda: VAEDecoder(config.TINY_VAE, sd, dtype, dev, bank=bank)
    elif kind == "unet":
        bank = UNetBank(config.TINY_UNET, sd, dtype, dev)
        model = lambda: UNet(config.TINY_UNET, sd, dtype, dev, bank=bank)
    else:
        bank = ClipTextBank(config.TINY_CLIP_TEXT, sd, dtype, dev)
        model = lambda: ClipTextEncoder(config.TINY_CLIP_TEXT, None, dtype, dev, bank)
    model()
    return bank, sd, model


def numel(shape):
    return int(np.prod(shape))


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("kind", KINDS)
def test_layout(dev, kind, dtype):
    bank, sd, _ = make(kind, dtype, dev)
    assert list(bank.layout) == bank.names == list(bank.params)
    assert all(o % 8 == 0 for o, _, _ in bank.layout.values())
    used = torch.zeros(bank.flat.numel(), dtype=torch.bool)
    for n, (o, stored, shp) in bank.layout.items():
        assert numel(stored) == numel(shp) and not used[o:o + numel(stored)].any()  # no two entries overlap
        used[o:o + numel(stored)] = True
        assert bank.params[n].data_ptr() == bank._view(bank.flat, n).data_ptr() and tuple(bank.params[n].shape) == stored
        assert bank.params[n].grad.data_ptr() == bank._view(bank.flat_grad, n).data_ptr()
    if kind != "clip":  # (every entry of the tiny tower is a multiple of 8 elements long)
        assert not used.all()
    flat = bank.flat.cpu()
    assert float(flat[~used].abs().sum()) == 0.0 and float(flat[used].abs().max()) > 0
    assert (bank.flat_c is None) == (dtype == torch.float32) and bank.flat_t.dtype == dtype
    assert (bank.gate is None) == (kind == "vae")


@pytest.mark.parametrize("dtype", DTYPES, ids=("bf16", "fp32"))
@pytest.mark.parametrize("kind", KINDS)
def test_refresh(dev, kind, dtype):
    """what the per-holder refresh() of ops.TrainableLinear / TrainableConv computes, from one launch, on random finite masters"""
    bank, _, _ = make(kind, dtype, dev)
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        bank.flat.copy_((torch.randn(bank.flat.numel(), generator=g) * 3.0).to(dev))
    bank.mark_updated()
    bank.ensure_compute_copy()
    seen = set()
    for name, (kd, h) in bank._made.items():
        if not hasattr(h, "w"):  # a norm's pair of tensors, the embedding tables: read from the master
            continue
        seen.add(name)
        master = bank._view(bank.flat, name + ".weight")
        assert torch.equal(h.w.reshape(master.shape), master.to(dtype)), name
        if kd[0] == "linear":
            assert torch.equal(h.wt, h.w.t()), name
        else:
            assert torch.equal(h.wd, h.w.flip(1, 2).permute(3, 1, 2, 0)), name
    assert len(seen) == len([h for h in bank.holders if hasattr(h, "w")]) > 10
    if kind == "vae":
        assert {"decoder.conv_out", "post_quant_conv"} <= seen
        assert bank._made["decoder.conv_out"][1].wd.shape[-1] == 3 and tuple(bank._made["post_quant_conv"][1].w.shape) == (4, 4)
        want_w, want_t = np.zeros(bank.flat.numel(), np.int32), np.zeros(bank.flat_t.numel(), np.int32)
        for n, ot in bank._toff.items():
            o, stored, _ = bank.layout[n]
            want_w[o:o + numel(stored)] = 1
            want_t[ot:ot + numel(stored)] = 1
        cw, ct = refresh.covered(bank._plan.problems, bank._plan.tiles, bank.flat.numel(), bank.flat_t.numel())
        assert np.array_equal(ct, want_t) and np.array_equal(cw, want_w)  # every matrix element once, nothing else


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_round_trip(dev, kind):
    bank, sd, _ = make(kind, torch.float32, dev)
    out = bank.state_dict()
    assert {k: tuple(v.shape) for k, v in out.items()} == {k: tuple(v.shape) for k, v in sd.items()}
    assert kind == "clip" or list(out) == list(sd)  # (the tower's bank keeps the model's order of parameters, not the file's)
    assert all(torch.equal(out[k], sd[k].float()) for k in sd)
    with torch.no_grad():
        bank.flat.mul_(1.5)
    before = bank.flat.clone()
    out = {k: v.clone() for k, v in bank.state_dict().items()}  # (on the CPU an entry that needs no permutation is a view of `flat`)
    bank.flat.zero_()
    bank.load_state_dict(out)
    assert torch.equal(bank.flat, before) and not bank._fresh
    key = (TEXT_PREFIX if kind == "clip" else "") + PROBE[kind][0]
    assert key in out
    with pytest.raises(KeyError, match=PROBE[kind][0].replace(".", r"\.")):
        bank.load_state_dict({k: v for k, v in out.items() if k != key})
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        bank.load_state_dict({**out, key: torch.zeros(3)})
    assert torch.equal(bank.flat, before)  # a refused file changes nothing


@pytest.mark.parametrize("kind", KINDS)
def test_one_holder_per_layer(dev, kind):
    bank, _, model = make(kind, torch.bfloat16, dev)
    bank.ensure_compute_copy()
    counts = (len(bank.holders), len(bank._problems), len(bank._affine), len(bank._made))
    made = {n: h for n, (_, h) in bank._made.items()}
    model()  # a second VAEDecoder / UNet / ClipTextEncoder over the same bank
    assert (len(bank.holders), len(bank._problems), len(bank._affine), len(bank._made)) == counts
    assert all(bank._made[n][1] is h for n, h in made.items()) and bank._fresh
    _, layer, other = PROBE[kind]
    with pytest.raises(ValueError, match="was built as"):
        other(bank, layer)


@pytest.mark.parametrize("kind", KINDS)
def test_protocol(dev, kind):
    bank, _, _ = make(kind, torch.bfloat16, dev)
    e0 = bank.epoch
    bank.ensure_compute_copy()
    assert bank.epoch == e0 + 1 and bank._fresh
    bank.ensure_compute_copy()
    assert bank.epoch == e0 + 1  # fresh: nothing is launched, nothing counted
    bank.mark_updated()
    bank.ensure_compute_copy()
    assert bank.epoch == e0 + 2
    norms = [t for k, pair in bank._made.values() if k == "norm" for t in pair]
    assert len(norms) == len(bank._affine) > 0 and len(bank.holders) > 0
    assert bank.training and all(h.requires_grad for h in bank.holders) and all(t.comat_train for t in norms)
    bank.set_requires_grad(False)
    assert not bank.training and not any(h.requires_grad for h in bank.holders) and not any(t.comat_train for t in norms)
    assert bank.gate is None or not bank.gate.requires_grad
    bank.set_requires_grad(True)
    assert all(h.requires_grad for h in bank.holders) and all(t.comat_train for t in norms)
    assert bank.gate is None or bank.gate.requires_grad
    bank.flat_grad.fill_(2.0)
    bank.zero_grad()
    assert float(bank.flat_grad.abs().sum()) == 0.0 and bank._fresh  # clearing gradients stales no copy
