"""unet.VAEEncoder (AutoencoderKL.encode up to the moments) against two references: the encoder of transformers' Janus VQ-VAE - the
latent-diffusion / taming encoder AutoencoderKL ports, an implementation neither this project nor diffusers wrote (the decoder's
counterpart: tests/test_models.py::test_vae_decoder_against_third_party_ldm_decoder) - and a plain-torch restatement under diffusers'
names, written here.  Tolerances are helpers.check's, as the decoder's tests use them."""
import pytest
import torch
import torch.nn.functional as F

from comat_amd import config, weights
from comat_amd.unet import VAEEncoder
from helpers import check, tok

DTYPES = [torch.float32, torch.bfloat16]


def encode_ref(sd, cfg, x, pad_mode="bottom_right"):
    """AutoencoderKL.encode's moments in plain torch, NCHW.  pad_mode: 'bottom_right' is diffusers' Downsample2D with padding 0
    (F.pad(0, 1, 0, 1)); 'symmetric' (conv padding 1) and 'dropped' (no pad, the last row and column lost) are the two mistakes"""
    G = cfg.norm_groups
    conv = lambda h, n, **kw: F.conv2d(h, sd[n + ".weight"], sd[n + ".bias"], **kw)
    gn = lambda h, n: F.group_norm(h, G, sd[n + ".weight"], sd[n + ".bias"], 1e-6)

    def res(h, n):
        y = conv(F.silu(gn(h, n + ".norm1")), n + ".conv1", padding=1)
        y = conv(F.silu(gn(y, n + ".norm2")), n + ".conv2", padding=1)
        return (conv(h, n + ".conv_shortcut") if n + ".conv_shortcut.weight" in sd else h) + y

    h = conv(x, "encoder.conv_in", padding=1)
    nb = len(cfg.block_out_channels)
    for i in range(nb):
        for j in range(cfg.layers_per_block):
            h = res(h, f"encoder.down_blocks.{i}.resnets.{j}")
        if i < nb - 1:
            n = f"encoder.down_blocks.{i}.downsamplers.0.conv"
            if pad_mode == "bottom_right":
                h = conv(F.pad(h, (0, 1, 0, 1)), n, stride=2)
            elif pad_mode == "symmetric":
                h = conv(h, n, stride=2, padding=1)
            else:
                h = F.pad(conv(h, n, stride=2), (0, 1, 0, 1))
    h = res(h, "encoder.mid_block.resnets.0")
    a = "encoder.mid_block.attentions.0"
    B, Cc, hh, ww = h.shape
    t = gn(h, a + ".group_norm").reshape(B, Cc, hh * ww).transpose(1, 2)
    lin = lambda v, n: F.linear(v, sd[f"{a}.{n}.weight"], sd[f"{a}.{n}.bias"])
    p = torch.softmax(lin(t, "to_q") @ lin(t, "to_k").transpose(1, 2) * Cc ** -0.5, dim=-1)
    h = h + lin(p @ lin(t, "to_v"), "to_out.0").transpose(1, 2).reshape(B, Cc, hh, ww)
    h = res(h, "encoder.mid_block.resnets.1")
    h = conv(F.silu(gn(h, "encoder.conv_norm_out")), "encoder.conv_out", padding=1)
    return conv(h, "quant_conv")


def ldm_encoder_to_diffusers_names(enc_sd, n_levels, n_blocks):
    """state dict of an LDM / taming encoder (`conv_in, down.{i}.block.{j}, down.{i}.downsample.conv, mid.block_1, mid.attn_1,
    mid.block_2, norm_out, conv_out`; 1x1-conv attention projections, `nin_shortcut`) -> diffusers' AutoencoderKL names"""
    out = {}

    def res(src, dst):
        for part in ("norm1", "conv1", "norm2", "conv2"):
            for wb in ("weight", "bias"):
                out[f"{dst}.{part}.{wb}"] = enc_sd[f"{src}.{part}.{wb}"]
        if f"{src}.nin_shortcut.weight" in enc_sd:
            out[f"{dst}.conv_shortcut.weight"] = enc_sd[f"{src}.nin_shortcut.weight"]
            out[f"{dst}.conv_shortcut.bias"] = enc_sd[f"{src}.nin_shortcut.bias"]

    for wb in ("weight", "bias"):
        out[f"encoder.conv_in.{wb}"] = enc_sd[f"conv_in.{wb}"]
        out[f"encoder.conv_norm_out.{wb}"] = enc_sd[f"norm_out.{wb}"]
        out[f"encoder.conv_out.{wb}"] = enc_sd[f"conv_out.{wb}"]
        out[f"encoder.mid_block.attentions.0.group_norm.{wb}"] = enc_sd[f"mid.attn_1.norm.{wb}"]
    res("mid.block_1", "encoder.mid_block.resnets.0")
    res("mid.block_2", "encoder.mid_block.resnets.1")
    for src, dst in (("q", "to_q"), ("k", "to_k"), ("v", "to_v"), ("proj_out", "to_out.0")):
        w = enc_sd[f"mid.attn_1.{src}.weight"]
        out[f"encoder.mid_block.attentions.0.{dst}.weight"] = w.reshape(w.shape[0], w.shape[1])
        out[f"encoder.mid_block.attentions.0.{dst}.bias"] = enc_sd[f"mid.attn_1.{src}.bias"]
    for i in range(n_levels):
        for j in range(n_blocks):
            res(f"down.{i}.block.{j}", f"encoder.down_blocks.{i}.resnets.{j}")
        if i < n_levels - 1:
            for wb in ("weight", "bias"):
                out[f"encoder.down_blocks.{i}.downsamplers.0.conv.{wb}"] = enc_sd[f"down.{i}.downsample.conv.{wb}"]
    return out


MULT, N_BLOCKS = (1, 2, 2), 1
LDM_CFG = config.VAEConfig(block_out_channels=tuple(32 * m for m in MULT), layers_per_block=N_BLOCKS, norm_groups=32)


@pytest.fixture(scope="module")
def ldm():
    """(the third-party encoder, its weights under diffusers' names without quant_conv) - built once, never changed"""
    from transformers.models.janus.configuration_janus import JanusVQVAEConfig
    from transformers.models.janus.modeling_janus import JanusVQVAEEncoder

    torch.manual_seed(21)
    enc = JanusVQVAEEncoder(JanusVQVAEConfig(base_channels=32, channel_multiplier=list(MULT), num_res_blocks=N_BLOCKS, latent_channels=4,
                                             in_channels=3, double_latent=True, dropout=0.0)).eval().float()
    with torch.no_grad():
        for name, p in enc.named_parameters():  # generic values everywhere (norm scales and every bias included)
            p.copy_(torch.randn_like(p) * (0.3 if p.dim() > 1 else 0.5) + (1.0 if "norm" in name and name.endswith("weight") else 0.0))
        for blk in enc.down[-1].attn:            # the level attentions SD's VAE does not have: identity
            blk.proj_out.weight.zero_()
            blk.proj_out.bias.zero_()
    sd = {k: v.detach().clone() for k, v in ldm_encoder_to_diffusers_names(enc.state_dict(), len(MULT), N_BLOCKS).items()}
    return enc, sd


@pytest.mark.parametrize("hw", [(16, 24), (8, 8)], ids=lambda s: "x".join(map(str, s)))
def test_vae_encoder_against_third_party_ldm_encoder(dev, ldm, hw):
    """identity quant_conv: the moments are the third-party encoder's output (16 x 24: not square, three levels -> 4 x 6 latents)"""
    enc, sd = ldm
    sd = dict(sd)
    sd["quant_conv.weight"], sd["quant_conv.bias"] = torch.eye(8).reshape(8, 8, 1, 1), torch.zeros(8)
    B, (H, W) = 2, hw
    x = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(H))
    with torch.no_grad():
        want = enc(x.clone())
    assert want.shape == (B, 8, H // 4, W // 4)
    got, h, w = VAEEncoder(LDM_CFG, sd, torch.float32, dev)(tok(x).to(dev), B, H, W)
    assert (h, w) == (H // 4, W // 4) and not got.requires_grad
    check(got, tok(want), torch.float32, "product VAE encoder vs transformers' LDM encoder")
    check(tok(encode_ref(sd, LDM_CFG, x)), tok(want), torch.float32, "the restatement below the other cases")


@pytest.mark.parametrize("hw", [(16, 24), (8, 8)], ids=lambda s: "x".join(map(str, s)))
def test_vae_encoder_with_a_quant_conv(dev, ldm, hw):
    _, sd = ldm
    sd = dict(sd)
    g = torch.Generator().manual_seed(3)
    sd["quant_conv.weight"], sd["quant_conv.bias"] = torch.randn(8, 8, 1, 1, generator=g) * 0.4, torch.randn(8, generator=g) * 0.3
    B, (H, W) = 2, hw
    x = torch.randn(B, 3, H, W, generator=g)
    got, _, _ = VAEEncoder(LDM_CFG, sd, torch.float32, dev)(tok(x).to(dev), B, H, W)
    check(got, tok(encode_ref(sd, LDM_CFG, x)), torch.float32, "moments behind a random quant_conv")


def tiny_encoder_weights(dtype):
    sd = weights.make_vae_encoder_weights(config.TINY_VAE, perturb_norms=True)
    return {k: v.to(dtype).float() for k, v in sd.items()}


@pytest.mark.parametrize("dtype", DTYPES)
def test_vae_encode_tiny(dev, dtype):
    """TINY_VAE (four levels, three downsamplers) in both compute dtypes against the restatement on the same rounded weights"""
    sd = tiny_encoder_weights(dtype)
    B, H, W = 2, 16, 24
    x = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(9)).to(dtype).float()
    got, h, w = VAEEncoder(config.TINY_VAE, sd, dtype, dev)(tok(x).to(dev, dtype), B, H, W)
    assert (h, w) == (2, 3) and got.dtype == dtype and got.shape == (B * 6, 8)
    check(got, tok(encode_ref(sd, config.TINY_VAE, x)), dtype, "tiny VAE moments")


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_pad_is_one_row_below_and_one_column_right(dev, dtype):
    """large values in the image's last row and last column: a symmetric pad (which never reads them with the stride-2 grid it
    lands on) and a dropped edge both miss the reference by far more than the tolerance"""
    sd = tiny_encoder_weights(dtype)
    B, H, W = 1, 16, 16
    x = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(4)) * 0.3
    x[:, :, -1, :] += 6.0
    x[:, :, :, -1] -= 6.0
    x = x.to(dtype).float()
    ref = tok(encode_ref(sd, config.TINY_VAE, x))
    got, _, _ = VAEEncoder(config.TINY_VAE, sd, dtype, dev)(tok(x).to(dev, dtype), B, H, W)
    check(got, ref, dtype, "moments of an image with a loud last row and column")
    for wrong in ("symmetric", "dropped"):
        with pytest.raises(AssertionError):
            check(tok(encode_ref(sd, config.TINY_VAE, x, pad_mode=wrong)), ref, dtype, wrong)


def test_bad_sizes_and_weights_layout(sim):
    sd = weights.make_vae_encoder_weights(config.TINY_VAE)
    assert all(k.startswith(("encoder.", "quant_conv.")) for k in sd) and sd["quant_conv.weight"].shape == (8, 8, 1, 1)
    assert sd["encoder.conv_out.weight"].shape[0] == 8 and "encoder.down_blocks.2.downsamplers.0.conv.weight" in sd
    assert "encoder.down_blocks.3.downsamplers.0.conv.weight" not in sd
    assert not set(sd) & set(weights.make_vae_weights(config.TINY_VAE))
    with pytest.raises(ValueError, match="multiples of 8"):
        VAEEncoder(config.TINY_VAE, sd, torch.float32, sim)(torch.zeros(12 * 16, 3), 1, 12, 16)
