"""The CLIP text tower (comat_amd.clip) against transformers' CLIPTextModel - the reference's own library, imported with the tiny
config and random weights, never restated - on the simulator and on the real kernels: outputs, both key spellings, causality bit
for bit, and the LoRA factors' gradients against the same model with W + U D in its four projections under torch autograd on the
CPU.

Bounds.  fp32 storage: 1e-3 relative per tensor, the project's parity bar.  bf16 storage: twice the error measured against that
same fp32 CPU model on bf16-representable weights and factors - the largest figure over the cases of this file, on an MI355X and
on the simulator (which agree to two digits; DESIGN.md section 6 has the table):
    outputs, frozen tower    measured 5.38e-3 (MI355X and simulator)          -> bound 1.08e-2
    outputs, with LoRA       measured 7.93e-3 (MI355X; simulator 7.93e-3)     -> bound 1.59e-2   (W + U D is rounded to bf16 once more)
    factor gradients         measured 2.74e-2 (MI355X; simulator 2.65e-2)     -> bound 5.48e-2   (per tensor, relative L2)
"""
import copy

import pytest
import torch
import transformers

from clip_sim import clip_dev  # noqa: F401 - fixture
from comat_amd import ops
from comat_amd.clip import PROJS, ClipLoRABank, ClipTextEncoder, lora_key
from comat_amd.config import TINY_CLIP_TEXT as CFG

FP32_BOUND = 1e-3
BF16_OUT_BOUND, BF16_LORA_OUT_BOUND, BF16_GRAD_BOUND = 1.08e-2, 1.59e-2, 5.48e-2
END = CFG.vocab_size - 1  # CLIP's end token has the largest id; SD pads with it


def bf16_values(t):
    return t.to(torch.bfloat16).float()


_MODEL = {}


def hf_model():
    """the checker, built once and never changed: CLIPTextModel of the tiny config, its random weights redrawn at a scale at which
    every part of the tower matters (transformers' own initialisation leaves the attention and MLP branches near zero)"""
    if "m" not in _MODEL:
        hc = transformers.CLIPTextConfig(vocab_size=CFG.vocab_size, hidden_size=CFG.hidden, intermediate_size=CFG.mlp,
                                         num_hidden_layers=CFG.layers, num_attention_heads=CFG.heads,
                                         max_position_embeddings=CFG.max_pos, hidden_act=CFG.act, layer_norm_eps=CFG.eps,
                                         projection_dim=32, attn_implementation="eager")
        m = transformers.CLIPTextModel(hc).eval()
        g = torch.Generator().manual_seed(11)
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
            else:
                sd[name] = bf16_values(torch.randn(t.shape, generator=g) * t.shape[1] ** -0.5)
        m.load_state_dict(sd)
        for p in m.parameters():
            p.requires_grad_(False)
        _MODEL["m"] = m
    return _MODEL["m"]


def bare_sd():
    """the model's state dict under the names without the text_model. prefix (transformers 5.x)"""
    return {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in hf_model().state_dict().items()}


def make_ids(B, L, seed=0):
    """random ids, an end token, then a run of repeated pad ids (the end token's id, as SD's tokenizer pads)"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, CFG.vocab_size - 2, (B, L), generator=g)
    for b in range(B):
        end = max(1, (L * (b + 2)) // (B + 2))
        ids[b, end:] = END
    return ids


def model_outputs(ids, weights=None):
    """(last_hidden_state, hidden_states[-2]) of the checker as [B*L, hidden]; weights: replacements for named parameters"""
    m = hf_model()
    kw = dict(input_ids=ids, attention_mask=None, output_hidden_states=True)
    out = m(**kw) if weights is None else torch.func.functional_call(m, weights, args=(), kwargs=kw)
    d = CFG.hidden
    return out.last_hidden_state.reshape(-1, d), out.hidden_states[-2].reshape(-1, d)


def rel(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((got - ref).norm() / ref.norm())


def lora_factors(rank, seed):
    """random factors with NON-zero up factors (at up = 0 the down gradients vanish and show nothing), bf16-representable"""
    g = torch.Generator().manual_seed(seed)
    sd = ClipLoRABank.init(CFG, rank, g)
    for k in sd:
        # down ~ N(0, 1 / rank) in variance and up ~ N(0, 1 / hidden): the entries of U D have the frozen weights' variance, 1 / hidden,
        # at every rank - the factors matter as much as the weights they sit on and leave the attention logits at their scale
        if k.endswith("up.weight"):
            sd[k] = bf16_values(torch.randn(sd[k].shape, generator=g) * CFG.hidden ** -0.5)
        else:
            sd[k] = bf16_values(sd[k] * rank ** 0.5)
    return sd


def model_with_lora(ids, factors):
    """the checker with W + U D in q_proj / k_proj / v_proj / out_proj of every layer; factors: leaves that require grad"""
    m = hf_model()
    names = dict(m.named_parameters())
    pre = "text_model." if any(n.startswith("text_model.") for n in names) else ""
    weights = {}
    for i in range(CFG.layers):
        for p in PROJS:
            n = f"{pre}encoder.layers.{i}.self_attn.{p}.weight"
            weights[n] = names[n] + factors[lora_key(i, p, "up")] @ factors[lora_key(i, p, "down")]
    return model_outputs(ids, weights)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,L", [(2, 77), (4, 77), (2, 8), (4, 8)])
def test_outputs_match_the_model(clip_dev, dtype, B, L):
    ids = make_ids(B, L, seed=B * L)
    enc = ClipTextEncoder(CFG, hf_model().state_dict(), dtype, clip_dev)
    last, pen = model_outputs(ids)
    bound = FP32_BOUND if dtype == torch.float32 else BF16_OUT_BOUND
    for output, ref in (("last", last), ("penultimate", pen)):
        with torch.no_grad():
            got = enc(ids, output=output)
        assert got.shape == (B * L, CFG.hidden) and got.dtype == dtype
        e = rel(got, ref)
        print(f"clip outputs {output} B={B} L={L} {dtype}: rel {e:.3e}")
        assert e < bound, (output, e)


def test_both_key_spellings_load_and_a_missing_key_raises(clip_dev):
    ids = make_ids(2, 8)
    bare = bare_sd()
    prefixed = {"text_model." + k: v for k, v in bare.items()}
    prefixed["text_model.embeddings.position_ids"] = torch.arange(CFG.max_pos)[None]  # transformers 4.31 stores it; ignored
    with torch.no_grad():
        a = ClipTextEncoder(CFG, bare, torch.float32, clip_dev)(ids)
        b = ClipTextEncoder(CFG, prefixed, torch.float32, clip_dev)(ids)
    assert torch.equal(a, b)
    for sd in (bare, prefixed):
        key = next(k for k in sd if k.endswith("layers.1.self_attn.v_proj.bias"))
        with pytest.raises(KeyError, match=r"layers\.1\.self_attn\.v_proj\.bias"):
            ClipTextEncoder(CFG, {k: v for k, v in sd.items() if k != key}, torch.float32, clip_dev)
    wrong = dict(bare)
    wrong["encoder.layers.0.mlp.fc1.weight"] = torch.zeros(CFG.mlp, CFG.hidden + 1)
    with pytest.raises(ValueError, match=r"layers\.0\.mlp\.fc1\.weight"):
        ClipTextEncoder(CFG, wrong, torch.float32, clip_dev)
    with pytest.raises(ValueError, match="output"):
        ClipTextEncoder(CFG, bare, torch.float32, clip_dev)(ids, output="pooled")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("p", [1, 40, 76])
def test_causal_bit_for_bit(clip_dev, dtype, p):
    """changing the id at position p leaves rows < p of the output unchanged, bit for bit, with LoRA in the tower"""
    B, L = 2, 77
    ids = make_ids(B, L, seed=3)
    other = ids.clone()
    other[:, p] = (ids[:, p] + 5) % (CFG.vocab_size - 2)
    bank = ClipLoRABank(CFG, lora_factors(4, seed=1), dtype, clip_dev)
    enc = ClipTextEncoder(CFG, hf_model().state_dict(), dtype, clip_dev, bank)
    with torch.no_grad():
        a = enc(ids).reshape(B, L, -1)
        b = enc(other).reshape(B, L, -1)
    assert torch.equal(a[:, :p], b[:, :p])
    assert not torch.equal(a[:, p], b[:, p])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rank,B,L,output", [(4, 2, 77, "last"), (16, 2, 77, "last"), (16, 4, 8, "last"), (4, 4, 8, "penultimate")])
def test_lora_outputs_and_factor_gradients(clip_dev, dtype, rank, B, L, output):
    ids = make_ids(B, L, seed=rank + L)
    fsd = lora_factors(rank, seed=rank)
    g = torch.Generator().manual_seed(5)
    gout = bf16_values(torch.randn(B * L, CFG.hidden, generator=g))
    leaves = {k: v.clone().requires_grad_(True) for k, v in fsd.items()}
    ref = model_with_lora(ids, leaves)[0 if output == "last" else 1]
    (ref * gout).sum().backward()

    bank = ClipLoRABank(CFG, fsd, dtype, clip_dev)
    enc = ClipTextEncoder(CFG, hf_model().state_dict(), dtype, clip_dev, bank)
    bank.zero_grad()
    got = enc(ids, output=output)
    got.backward(gout.to(device=clip_dev, dtype=dtype))
    if clip_dev.type == "cuda":
        torch.cuda.synchronize()
    out_bound, grad_bound = (FP32_BOUND, FP32_BOUND) if dtype == torch.float32 else (BF16_LORA_OUT_BOUND, BF16_GRAD_BOUND)
    e = rel(got, ref)
    print(f"clip lora output r={rank} B={B} L={L} {output} {dtype}: rel {e:.3e}")
    assert e < out_bound
    assert set(bank.names) == set(fsd)
    worst = 0.0
    for name in bank.names:
        want, have = leaves[name].grad, bank.params[name].grad
        if want is None or float(want.norm()) == 0.0:  # the last layer's factors under "penultimate"
            assert output == "penultimate" and f"layers.{CFG.layers - 1}." in name
            assert float(have.abs().max()) == 0.0, name
            continue
        assert float(want.norm()) > 0
        worst = max(worst, rel(have, want))
        assert rel(have, want) < grad_bound, (name, rel(have, want))
    print(f"clip lora grads r={rank} B={B} L={L} {output} {dtype}: worst rel {worst:.3e}")


def test_bank_initial_state_and_interface(clip_dev):
    g = torch.Generator().manual_seed(0)
    sd = ClipLoRABank.init(CFG, 16, g)
    assert len(sd) == CFG.layers * 4 * 2
    downs = torch.cat([v.reshape(-1) for k, v in sd.items() if k.endswith("down.weight")])
    assert abs(float(downs.std()) - 1 / 16) < 0.05 / 16 and all(not v.any() for k, v in sd.items() if k.endswith("up.weight"))
    bank = ClipLoRABank(CFG, sd, torch.bfloat16, clip_dev)
    assert isinstance(bank, ops.LoRAStore) and all(grp.scale == 1.0 for grp in bank.groups)
    assert [grp.size for grp in bank.groups] == [3, 1] * CFG.layers
    assert bank.flat.numel() == bank.flat_grad.numel() == sum(v.numel() for v in sd.values())
    assert bank.names[0] == "text_model.encoder.layers.0.self_attn.q_proj.lora_linear_layer.down.weight"
    bank.flat_grad.fill_(1.0)
    bank.zero_grad()
    assert not bank.flat_grad.any()
    bank.set_requires_grad(False)
    bank.set_requires_grad(True)
    bank.ensure_compute_copy()
    short = copy.copy(sd)
    del short[lora_key(1, "out_proj", "up")]
    with pytest.raises(KeyError, match=r"layers\.1\.self_attn\.out_proj\.lora_linear_layer\.up\.weight"):
        ClipLoRABank(CFG, short, torch.float32, clip_dev)
