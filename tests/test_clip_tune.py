"""The text tower trained in full (comat_amd.clip.ClipTextBank, `--tune_text_encoder`) against transformers' CLIPTextModel under
torch autograd on the CPU - the checker of tests/test_clip_text.py, built again here - on the simulator and on the real kernels:
outputs and the gradient of EVERY parameter, both embedding tables included, with padded ids so that table rows repeat.

Bounds, per tensor, relative L2.  fp32 storage: 1e-3, the project's parity bar.  bf16 storage: twice the error measured against
that same fp32 CPU model on bf16-representable weights - the largest figure over the cases of this file, on an MI355X and on the
simulator (DESIGN.md section 6 has the table):
    outputs               measured 5.38e-3 (MI355X; simulator 5.36e-3)   -> bound 1.08e-2
    parameter gradients   measured 1.60e-2 (MI355X; simulator 1.48e-2)   -> bound 3.20e-2   (worst tensor: a layer-1 q_proj.bias at
                          B, L = 4, 8; the two tables: 7.8e-3 on both)
"""
import pytest
import torch
import transformers

from clip_tune_sim import tune_dev  # noqa: F401 - fixture
from comat_amd import ops
from comat_amd.clip import POS_NAME, TOK_NAME, ClipTextBank, ClipTextEncoder
from comat_amd.config import TINY_CLIP_TEXT as CFG

FP32_BOUND = 1e-3
BF16_OUT_MEASURED, BF16_GRAD_MEASURED = 5.38e-3, 1.60e-2  # (the larger of MI355X and simulator, over the cases below)
BF16_OUT_BOUND, BF16_GRAD_BOUND = 2 * BF16_OUT_MEASURED, 2 * BF16_GRAD_MEASURED
END = CFG.vocab_size - 1  # CLIP's end token has the largest id; SD pads with it
CASES = [(2, 77, "last"), (2, 77, "penultimate"), (4, 8, "last"), (4, 8, "penultimate")]


def bf16_values(t):
    return t.to(torch.bfloat16).float()


def hf_config():
    return transformers.CLIPTextConfig(vocab_size=CFG.vocab_size, hidden_size=CFG.hidden, intermediate_size=CFG.mlp,
                                       num_hidden_layers=CFG.layers, num_attention_heads=CFG.heads,
                                       max_position_embeddings=CFG.max_pos, hidden_act=CFG.act, layer_norm_eps=CFG.eps,
                                       projection_dim=32, attn_implementation="eager")


_MODEL = {}


def hf_model():
    """the checker, built once and never changed: CLIPTextModel of the tiny config, its random weights redrawn at a scale at which
    every part of the tower matters (transformers' own initialisation leaves the attention and MLP branches near zero)"""
    if "m" not in _MODEL:
        m = transformers.CLIPTextModel(hf_config()).eval()
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


def bare(name):
    return name[len("text_model."):] if name.startswith("text_model.") else name


def make_ids(B, L, seed=0):
    """random ids, an end token, then a run of repeated pad ids (the end token's id, as SD's tokenizer pads)"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, CFG.vocab_size - 2, (B, L), generator=g)
    for b in range(B):
        end = max(1, (L * (b + 2)) // (B + 2))
        ids[b, end:] = END
    return ids


def rel(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return float((got - ref).norm() / ref.norm())


_REF = {}


def reference(B, L, output):
    """(ids, upstream gradient, output, {bare name: gradient}) of the checker with every parameter a leaf; computed once per case"""
    key = (B, L, output)
    if key not in _REF:
        m = hf_model()
        ids = make_ids(B, L, seed=B * L)
        g = torch.Generator().manual_seed(5)
        gout = bf16_values(torch.randn(B * L, CFG.hidden, generator=g))
        leaves = {n: p.detach().clone().requires_grad_(True) for n, p in m.named_parameters()}
        out = torch.func.functional_call(m, leaves, args=(), kwargs=dict(input_ids=ids, attention_mask=None,
                                                                         output_hidden_states=True))
        ref = (out.last_hidden_state if output == "last" else out.hidden_states[-2]).reshape(-1, CFG.hidden)
        (ref * gout).sum().backward()
        _REF[key] = (ids, gout, ref.detach(), {bare(n): p.grad for n, p in leaves.items()})
    return _REF[key]


def tower(dtype, dev, sd=None):
    bank = ClipTextBank(CFG, hf_model().state_dict() if sd is None else sd, dtype, dev)
    return bank, ClipTextEncoder(CFG, None, dtype, dev, bank)


def run_backward(enc, bank, ids, gout, output, dev, dtype):
    bank.zero_grad()
    got = enc(ids, output=output)
    got.backward(gout.to(device=dev, dtype=dtype))
    ops.join_side_streams()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,L,output", CASES)
def test_outputs_and_every_parameter_gradient(tune_dev, dtype, B, L, output):
    ids, gout, ref, grads = reference(B, L, output)
    bank, enc = tower(dtype, tune_dev)
    got = run_backward(enc, bank, ids, gout, output, tune_dev, dtype)
    out_bound, grad_bound = (FP32_BOUND, FP32_BOUND) if dtype == torch.float32 else (BF16_OUT_BOUND, BF16_GRAD_BOUND)
    assert got.shape == (B * L, CFG.hidden) and got.dtype == dtype
    e = rel(got, ref)
    print(f"clip tune output B={B} L={L} {output} {dtype}: rel {e:.3e}")
    assert set(bank.names) == set(grads) and len(bank.names) == 2 + 16 * CFG.layers + 2
    worst, worst_name, failed = 0.0, None, []
    for name in bank.names:
        want, have = grads[name], bank.params[name].grad
        assert want is None or have.shape == want.shape
        if name.endswith("k_proj.bias") and want is not None:
            # softmax does not see a constant added to every key: this gradient is zero in exact arithmetic, both sides hold
            # rounding noise - held to the bound relative to the query bias' gradient, its neighbour of the same shape
            scale = float(grads[name.replace("k_proj", "q_proj")].norm())
            assert float(want.norm()) < 1e-4 * scale and float(have.float().norm()) < grad_bound * scale, name
            continue
        if want is None or float(want.norm()) == 0.0:  # "penultimate": the last layer and the final norm are not on the path
            assert output == "penultimate" and (f"layers.{CFG.layers - 1}." in name or name.startswith("final_layer_norm")), name
            assert float(have.abs().max()) == 0.0, name
            continue
        r = rel(have, want)
        if r > worst:
            worst, worst_name = r, name
        if not r < grad_bound:
            failed.append((name, r))
    print(f"clip tune grads B={B} L={L} {output} {dtype}: worst rel {worst:.3e} ({worst_name}); "
          f"tables {rel(bank.params[TOK_NAME].grad, grads[TOK_NAME]):.3e} {rel(bank.params[POS_NAME].grad, grads[POS_NAME]):.3e}")
    assert e < out_bound
    assert not failed, failed
    if output == "penultimate":
        zero = [n for n in bank.names if f"layers.{CFG.layers - 1}." in n or n.startswith("final_layer_norm")]
        assert len(zero) == 18 and all(not bank.params[n].grad.any() for n in zero)
    # rows of the token table that no id names received nothing
    unnamed = torch.ones(CFG.vocab_size, dtype=torch.bool)
    unnamed[ids.reshape(-1)] = False
    assert not bank.params[TOK_NAME].grad.cpu()[unnamed].any()
    assert L == CFG.max_pos or not bank.params[POS_NAME].grad.cpu()[L:].any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_two_backward_passes_accumulate_and_repeat_bit_for_bit(tune_dev, dtype):
    ids, gout, _, _ = reference(2, 77, "last")
    bank, enc = tower(dtype, tune_dev)
    run_backward(enc, bank, ids, gout, "last", tune_dev, dtype)
    once = bank.flat_grad.clone()
    run_backward(enc, bank, ids, gout, "last", tune_dev, dtype)
    assert torch.equal(bank.flat_grad, once)
    got = enc(ids)  # no zero_grad: the tables' gradients accumulate as the other parameters' do
    got.backward(gout.to(device=tune_dev, dtype=dtype))
    ops.join_side_streams()
    for name in (TOK_NAME, POS_NAME):
        g1 = bank._view(once, name)
        assert torch.equal(bank.params[name].grad, g1 + g1), name


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("output", ["last", "penultimate"])
def test_forward_after_an_update_equals_a_rebuilt_tower(tune_dev, dtype, output):
    ids = make_ids(4, 8, seed=2)
    bank, enc = tower(dtype, tune_dev)
    with torch.no_grad():
        before = enc(ids, output=output)
        g = torch.Generator().manual_seed(3)
        bank.flat.add_((0.05 * torch.randn(bank.flat.numel(), generator=g)).to(tune_dev) * (bank.flat != 0))
        bank.mark_updated()
        after = enc(ids, output=output)
        _, rebuilt = tower(dtype, tune_dev, bank.state_dict())
        assert not torch.equal(after, before)
        assert torch.equal(after, rebuilt(ids, output=output))


def test_frozen_bank_takes_no_gradient_and_saves_nothing(tune_dev):
    ids, gout, _, _ = reference(4, 8, "last")
    bank, enc = tower(torch.float32, tune_dev)
    bank.set_requires_grad(False)
    out = enc(ids)
    assert not out.requires_grad
    bank.set_requires_grad(True)
    with torch.no_grad():
        assert not enc(ids).requires_grad
    assert not bank.flat_grad.any()


def test_state_dict_loads_into_the_model_and_keeps_the_key_spelling(tune_dev):
    m = hf_model()
    src = m.state_dict()
    bank, _ = tower(torch.bfloat16, tune_dev)
    sd = bank.state_dict()
    floats = {k for k, v in src.items() if v.is_floating_point() and not k.endswith("position_ids")}
    assert set(sd) == floats and all(v.dtype == torch.float32 and v.device.type == "cpu" for v in sd.values())
    assert all(torch.equal(sd[k], src[k]) for k in floats)
    fresh = transformers.CLIPTextModel(hf_config())
    full = dict(sd, **{k: v for k, v in fresh.state_dict().items() if k not in sd})  # the position_ids buffer where there is one
    assert all(k.endswith("position_ids") for k in full if k not in sd)
    fresh.load_state_dict(full, strict=True)
    # the other spelling: loaded and given back as it came
    other = {("text_model." + bare(k)) if bare(k) == k else bare(k): v for k, v in sd.items()}
    other["embeddings.position_ids" if "embeddings.position_ids" not in other else "x.position_ids"] = torch.arange(CFG.max_pos)[None]
    bank2 = ClipTextBank(CFG, other, torch.float32, tune_dev)
    assert set(bank2.state_dict()) == {k for k in other if not k.endswith("position_ids")}
    assert torch.equal(bank2.flat, bank.flat)
    bank2.load_state_dict(sd)  # either spelling is taken
    assert torch.equal(bank2.flat, bank.flat)


def test_load_refuses_a_missing_key_and_a_wrong_shape_by_name(tune_dev):
    bank, _ = tower(torch.float32, tune_dev)
    sd = bank.state_dict()
    key = next(k for k in sd if k.endswith("layers.1.self_attn.v_proj.bias"))
    short = {k: v for k, v in sd.items() if k != key}
    for call in (lambda: bank.load_state_dict(short), lambda: ClipTextBank(CFG, short, torch.float32, tune_dev)):
        with pytest.raises(KeyError, match=r"layers\.1\.self_attn\.v_proj\.bias"):
            call()
    wrong = dict(sd)
    wk = next(k for k in sd if k.endswith(TOK_NAME))
    wrong[wk] = torch.zeros(CFG.vocab_size + 1, CFG.hidden)
    for call in (lambda: bank.load_state_dict(wrong), lambda: ClipTextBank(CFG, wrong, torch.float32, tune_dev)):
        with pytest.raises(ValueError, match="token_embedding"):
            call()
    with pytest.raises(ValueError, match="another config, dtype or device"):
        ClipTextEncoder(CFG, None, torch.bfloat16, tune_dev, bank)


def test_bank_interface(tune_dev):
    bank, enc = tower(torch.bfloat16, tune_dev)
    n_lin = 6 * CFG.layers
    assert bank.flat.dtype == bank.flat_grad.dtype == torch.float32 and bank.flat.numel() == bank.flat_grad.numel()
    assert bank.flat.numel() >= sum(p.numel() for p in hf_model().parameters())
    # only the Linear weights have a compute copy: the tables are read from the master
    lin = sum(v.numel() for k, v in bank.params.items() if v.dim() == 2 and k not in (TOK_NAME, POS_NAME))
    assert bank.flat_c.numel() == bank.flat_t.numel() == lin and bank.flat_c.dtype == torch.bfloat16
    assert len(bank.holders) == n_lin + 1 and bank.gate.requires_grad
    bank.ensure_compute_copy()
    e0 = bank.epoch
    bank.ensure_compute_copy()
    assert bank.epoch == e0  # nothing changed: no second refresh
    bank.mark_updated()
    bank.ensure_compute_copy()
    assert bank.epoch == e0 + 1
    bank.flat_grad.fill_(1.0)
    bank.zero_grad()
    assert not bank.flat_grad.any()
    bank.set_requires_grad(False)
    assert not bank.gate.requires_grad and not any(h.requires_grad for h in bank.holders)
    bank.set_requires_grad(True)
    assert ClipTextBank(CFG, hf_model().state_dict(), torch.float32, tune_dev).flat_c is None
