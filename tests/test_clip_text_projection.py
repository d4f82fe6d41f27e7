"""SDXL's second text tower (comat_amd.clip with ClipTextConfig.projection_dim) against transformers' CLIPTextModelWithProjection -
imported with the tiny config and random weights, never restated - on the simulator and on the real kernels: hidden_states[-2]
and text_embeds from ONE pass, both pooling rules (the config's eos_token_id decides), both key spellings, and
clip.encode_prompt_sdxl against the two transformers models put together by hand.

Bounds, relative L2 per tensor.  fp32 storage: 1e-3, the project's parity bar.  bf16 storage: twice the error measured against
that same fp32 CPU model on bf16-representable weights - the largest figure over the cases of this file, on an MI355X and on the
simulator (DESIGN.md section 6 has the table):
    hidden_states[-2]   measured 5.162e-3 (MI355X; simulator 5.162e-3)   -> bound 1.04e-2
    text_embeds         measured 6.480e-3 (MI355X; simulator 6.561e-3)   -> bound 1.32e-2
    prompt_embeds       measured 4.884e-3 (MI355X; simulator 4.889e-3)   -> bound 9.78e-3   (encode_prompt_sdxl, both towers)

Mutants (test_mutants_lie_outside_the_bounds, on the CPU against the checker alone), relative L2 of the mistake:
    the last hidden state where the penultimate is due   7.3e-1
    pooling at position 0                                1.0
    the two channel blocks swapped                       1.4
    quick-GELU for GELU                                  7.9e-3 (hidden_states[-2]), 8.8e-3 (text_embeds)
The first three lie outside every bound in use.  The bf16 bounds are TOO LOOSE TO REJECT quick-GELU for GELU: at the checker's weight
scale the two activations differ by less than twice the rounding error of bf16 storage.  The fp32 bound (1e-3) rejects it on both
tensors, and every case of this file runs in fp32 as well; the test asserts exactly that."""
import dataclasses

import pytest
import torch
import transformers

import test_clip_text as T1
from clip2_sim import clip2_dev  # noqa: F401 - fixture
from comat_amd.clip import PROJ_NAME, ClipLoRABank, ClipTextEncoder, encode_prompt_sdxl
from comat_amd.config import TINY_CLIP_TEXT_2 as CFG2
from test_clip_text import FP32_BOUND, bf16_values, rel

BF16_HIDDEN_BOUND, BF16_EMBEDS_BOUND, BF16_PROMPT_BOUND = 1.04e-2, 1.32e-2, 9.78e-3
END = CFG2.vocab_size - 1  # the legacy rule: the end token has the largest id
EOS_NEW = 5  # the other rule: an end token that is NOT the largest id present
_MODELS = {}


def cfg_of(eos):
    return dataclasses.replace(CFG2, eos_token_id=eos)


def hf_model2(eos=2, act=CFG2.act):
    """the checker, built once per (eos_token_id, activation) and never changed: CLIPTextModelWithProjection of the tiny twin, its
    weights redrawn as test_clip_text.hf_model draws them - the same values for every key - text_projection at hidden ** -0.5"""
    if (eos, act) not in _MODELS:
        hc = transformers.CLIPTextConfig(vocab_size=CFG2.vocab_size, hidden_size=CFG2.hidden, intermediate_size=CFG2.mlp,
                                         num_hidden_layers=CFG2.layers, num_attention_heads=CFG2.heads,
                                         max_position_embeddings=CFG2.max_pos, hidden_act=act, layer_norm_eps=CFG2.eps,
                                         projection_dim=CFG2.projection_dim, eos_token_id=eos, pad_token_id=0, bos_token_id=1,
                                         attn_implementation="eager")
        m = transformers.CLIPTextModelWithProjection(hc).eval()
        g = torch.Generator().manual_seed(12)
        sd = {}
        for name, t in m.state_dict().items():
            if not t.is_floating_point():
                sd[name] = t
            elif "layer_norm" in name:
                sd[name] = bf16_values((1.0 if name.endswith("weight") else 0.0) + 0.2 * torch.randn(t.shape, generator=g))
            elif name.endswith("bias"):
                sd[name] = bf16_values(0.1 * torch.randn(t.shape, generator=g))
            elif "embedding" in name:
                sd[name] = bf16_values(0.5 * torch.randn(t.shape, generator=g))
            else:  # (text_projection among them: hidden ** -0.5)
                sd[name] = bf16_values(torch.randn(t.shape, generator=g) * t.shape[1] ** -0.5)
        m.load_state_dict(sd)
        for p in m.parameters():
            p.requires_grad_(False)
        assert PROJ_NAME in sd and tuple(sd[PROJ_NAME].shape) == (CFG2.projection_dim, CFG2.hidden)
        _MODELS[(eos, act)] = m
    return _MODELS[(eos, act)]


def make_ids2(B, L, eos, seed=0):
    """random ids, the end token, then pads of id 0 - as SDXL's second tokenizer pads.  eos = 2 stands for the legacy rule: its
    end token is END, the largest id; under the other rule larger ids than the end token occur before it"""
    g = torch.Generator().manual_seed(seed)
    end_id = END if eos == 2 else eos
    ids = torch.randint(3 if eos == 2 else eos + 1, CFG2.vocab_size - (2 if eos == 2 else 0), (B, L), generator=g)
    for b in range(B):
        end = max(1, (L * (b + 2)) // (B + 2))
        ids[b, end] = end_id
        ids[b, end + 1:] = 0
    return ids


def model2_outputs(ids, eos=2, act=CFG2.act):
    """(hidden_states[-2] [B*L, hidden], text_embeds [B, projection_dim], the model's output) of the checker"""
    with torch.no_grad():
        out = hf_model2(eos, act)(input_ids=ids, attention_mask=None, output_hidden_states=True)
    return out.hidden_states[-2].reshape(-1, CFG2.hidden), out.text_embeds, out


def bound(dtype, bf16):
    return FP32_BOUND if dtype == torch.float32 else bf16


@pytest.mark.parametrize("eos", [2, EOS_NEW])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,L", [(2, 77), (3, 8)])
def test_hidden_state_and_text_embeds_match_the_model(clip2_dev, dtype, B, L, eos):
    ids = make_ids2(B, L, eos, seed=B * L + eos)
    if eos != 2:
        assert not torch.equal(ids.argmax(-1), (ids == eos).int().argmax(-1)), "the two rules agree: the case shows nothing"
    enc = ClipTextEncoder(cfg_of(eos), hf_model2(eos).state_dict(), dtype, clip2_dev)
    pen, emb, _ = model2_outputs(ids, eos)
    with torch.no_grad():
        got_pen, got_emb = enc(ids, output="pooled")
        alone = enc(ids, output="penultimate")
    assert got_pen.shape == (B * L, CFG2.hidden) and got_emb.shape == (B, CFG2.projection_dim)
    assert got_pen.dtype == dtype and got_emb.dtype == dtype
    assert torch.equal(got_pen, alone)  # the state kept on the way is the one the early return gives
    e_pen, e_emb = rel(got_pen, pen), rel(got_emb, emb)
    print(f"clip2 B={B} L={L} eos={eos} {dtype}: hidden_states[-2] rel {e_pen:.3e} text_embeds rel {e_emb:.3e}")
    assert e_pen < bound(dtype, BF16_HIDDEN_BOUND), e_pen
    assert e_emb < bound(dtype, BF16_EMBEDS_BOUND), e_emb


def test_both_key_spellings_load_and_a_missing_projection_raises(clip2_dev):
    ids = make_ids2(2, 8, 2)
    sd = dict(hf_model2().state_dict())
    strip = lambda k: k[len("text_model."):] if k.startswith("text_model.") else k
    bare = {strip(k): v for k, v in sd.items()}
    prefixed = {(k if k == PROJ_NAME else "text_model." + k): v for k, v in bare.items()}
    assert PROJ_NAME in bare and PROJ_NAME in prefixed and set(bare) != set(prefixed)
    outs = []
    for d in (bare, prefixed):
        with torch.no_grad():
            outs.append(ClipTextEncoder(CFG2, d, torch.float32, clip2_dev)(ids, output="pooled"))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    with pytest.raises(KeyError, match="text_projection"):
        ClipTextEncoder(CFG2, {k: v for k, v in bare.items() if k != PROJ_NAME}, torch.float32, clip2_dev)
    with pytest.raises(ValueError, match="text_projection.*shape"):
        ClipTextEncoder(CFG2, dict(bare, **{PROJ_NAME: torch.zeros(CFG2.projection_dim + 1, CFG2.hidden)}), torch.float32, clip2_dev)


def test_towers_without_a_projection_and_with_a_bank_raise(clip2_dev):
    ids = make_ids2(2, 8, 2)
    plain = ClipTextEncoder(dataclasses.replace(CFG2, projection_dim=None), hf_model2().state_dict(), torch.float32, clip2_dev)
    with pytest.raises(ValueError, match="projection_dim"):
        plain(ids, output="pooled")
    with pytest.raises(ValueError, match="output must be"):
        plain(ids, output="embeds")
    # "last" and "penultimate" of a tower with a projection are the plain tower's, bit for bit
    proj = ClipTextEncoder(CFG2, hf_model2().state_dict(), torch.float32, clip2_dev)
    with torch.no_grad():
        for output in ("last", "penultimate"):
            assert torch.equal(plain(ids, output=output), proj(ids, output=output)), output
    bank = ClipLoRABank(CFG2, ClipLoRABank.init(CFG2, 4), torch.float32, clip2_dev)
    with pytest.raises(NotImplementedError, match="not built"):
        ClipTextEncoder(CFG2, hf_model2().state_dict(), torch.float32, clip2_dev, bank)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,L", [(2, 77), (3, 8)])
def test_encode_prompt_sdxl_matches_the_two_models_put_together(clip2_dev, dtype, B, L):
    ids_1, ids_2 = T1.make_ids(B, L, seed=B + L), make_ids2(B, L, 2, seed=B * L)
    enc1 = ClipTextEncoder(T1.CFG, T1.hf_model().state_dict(), dtype, clip2_dev)
    enc2 = ClipTextEncoder(CFG2, hf_model2().state_dict(), dtype, clip2_dev)
    pen2, emb2, _ = model2_outputs(ids_2)
    with torch.no_grad():
        pen1 = T1.model_outputs(ids_1)[1]
        got, pooled = encode_prompt_sdxl(enc1, enc2, ids_1, ids_2)
    want = torch.cat([pen1, pen2], dim=1).reshape(B, L, T1.CFG.hidden + CFG2.hidden)
    assert got.shape == want.shape and pooled.shape == emb2.shape and got.dtype == dtype
    e, e_p = rel(got, want), rel(pooled, emb2)
    print(f"encode_prompt_sdxl B={B} L={L} {dtype}: prompt_embeds rel {e:.3e} pooled rel {e_p:.3e}")
    assert e < bound(dtype, BF16_PROMPT_BOUND), e
    assert e_p < bound(dtype, BF16_EMBEDS_BOUND), e_p
    # each block against its own model: a block that is right only in the sum of the two would show here
    assert rel(got[..., :T1.CFG.hidden], want[..., :T1.CFG.hidden]) < bound(dtype, T1.BF16_OUT_BOUND)
    assert rel(got[..., T1.CFG.hidden:], want[..., T1.CFG.hidden:]) < bound(dtype, BF16_HIDDEN_BOUND)


def test_encode_prompt_sdxl_passes_the_first_towers_gradient_and_refuses_misfits(clip2_dev):
    B, L = 2, 8
    ids_1, ids_2 = T1.make_ids(B, L), make_ids2(B, L, 2)
    factors = T1.lora_factors(4, seed=3)
    bank = ClipLoRABank(T1.CFG, factors, torch.float32, clip2_dev)
    enc1 = ClipTextEncoder(T1.CFG, T1.hf_model().state_dict(), torch.float32, clip2_dev, bank)
    enc2 = ClipTextEncoder(CFG2, hf_model2().state_dict(), torch.float32, clip2_dev)
    got, pooled = encode_prompt_sdxl(enc1, enc2, ids_1, ids_2)
    assert got.requires_grad and not pooled.requires_grad
    w = torch.randn(got.shape, generator=torch.Generator().manual_seed(1)).to(clip2_dev)
    (got * w).sum().backward()
    leaves = {k: v.clone().requires_grad_(True) for k, v in factors.items()}
    ref = torch.cat([T1.model_with_lora(ids_1, leaves)[1], model2_outputs(ids_2)[0]], dim=1).reshape(got.shape)
    (ref * w.cpu()).sum().backward()
    last = f"layers.{T1.CFG.layers - 1}."
    for n in bank.names:
        if last not in n:
            assert float(leaves[n].grad.norm()) > 0 and rel(bank.params[n].grad, leaves[n].grad) < FP32_BOUND, n
    with pytest.raises(ValueError, match="text_projection"):
        encode_prompt_sdxl(enc1, enc1, ids_1, ids_2)
    with pytest.raises(ValueError, match="differ in shape"):
        encode_prompt_sdxl(enc1, enc2, ids_1, ids_2[:, :-1])


def test_mutants_lie_outside_the_bounds():
    """on the CPU, the checker against itself: what each mistake would cost, against the loosest bound its tensor is held to"""
    B, L = 2, 77
    ids_1, ids_2 = T1.make_ids(B, L, seed=1), make_ids2(B, L, 2, seed=2)
    pen2, emb2, out = model2_outputs(ids_2)
    with torch.no_grad():
        pen1 = T1.model_outputs(ids_1)[1]
        m = hf_model2()
        proj = dict(m.named_parameters())[PROJ_NAME]
        at_zero = out.last_hidden_state[:, 0] @ proj.t()
    q_pen, q_emb, _ = model2_outputs(ids_2, act="quick_gelu")
    right = torch.cat([pen1, pen2], dim=1)
    swapped = torch.cat([pen2, pen1], dim=1)
    mutants = {
        "the last hidden state where the penultimate is due": (rel(out.hidden_states[-1].reshape(-1, CFG2.hidden), pen2), BF16_HIDDEN_BOUND),
        "pooling at position 0": (rel(at_zero, emb2), BF16_EMBEDS_BOUND),
        "quick-GELU for GELU, hidden_states[-2]": (rel(q_pen, pen2), BF16_HIDDEN_BOUND),
        "quick-GELU for GELU, text_embeds": (rel(q_emb, emb2), BF16_EMBEDS_BOUND),
        "the two channel blocks swapped": (rel(swapped, right), BF16_PROMPT_BOUND),
    }
    for name, (e, b) in mutants.items():
        print(f"mutant {name}: rel {e:.3e} (bound {b:.3e})")
    for name, (e, b) in mutants.items():
        assert e > FP32_BOUND, (name, e)
        if not name.startswith("quick-GELU"):  # (the module docstring: the bf16 bounds do not reject that one)
            assert e > b > FP32_BOUND, (name, e, b)
