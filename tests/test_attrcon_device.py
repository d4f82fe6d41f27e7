"""The attribute-concentration loss as device work (losses.mask_loss_device, StepConfig.attrcon_on_device) on the CPU mirror
of its entry points (tests/attrcon_sim.py): the window tables of the OR resize, the batched tables and the autograd node against
the oracle (oracle/losses.py), the empty and the non-finite cases, and a whole tiny step.  The edge cases (40 tokens, a column
named twice, the golden totals, a NaN in a gathered column) run on both legs of `attrcon_dev`, the library included; its
other comparisons are in tests/test_attrcon_device_gpu.py and, entry point by entry point, tests/test_attrcon_kernels.py."""
import os

import numpy as np
import pytest
import torch

from attrcon_cases import RESIZE_SHAPES, Oracle, check_against, device_maps, maps_of, ragged_batch, resize_masks_case, run_device
from attrcon_sim import AttrconSimKernels, attrcon_dev, attrcon_sim, sim_matches_binding  # noqa: F401 - attrcon_dev, attrcon_sim are fixtures
from comat_amd import losses, ops
from helpers import check, rel_l2


def test_binding_declares_the_entry_points_and_the_simulator_mirrors_them():
    from comat_amd import _hip, ops
    for n in ("comat_mask_resize_any", "comat_attrcon_workspace_floats", "comat_attrcon_gather_fwd", "comat_attrcon_loss",
              "comat_attrcon_gather_bwd"):
        assert n in _hip.SIGNATURES
    names, differ = sim_matches_binding()
    assert not differ, differ
    assert not any(hasattr(_hip.HipKernels, n) for n in names)  # module functions: HipKernels and SimKernels stay in step
    assert ops.attrcon_kernels() is _hip  # no backend that has them: the binding, which refuses CPU tensors
    with pytest.raises(RuntimeError, match="HBM"):
        z = torch.zeros(4, dtype=torch.int32)
        _hip.mask_resize_any(torch.zeros(1, 4, 4, dtype=torch.uint8), z, z, z, z, torch.zeros(1, 16), 1, 4, 4, 4)


@pytest.mark.parametrize("H, W, res", RESIZE_SHAPES)
def test_or_resize_equals_resize_masks(attrcon_sim, H, W, res):
    """window tables + logical OR == Resize(antialias=True) > 0, bit for bit: the host form and the entry point's mirror"""
    m = resize_masks_case(H, W)
    ref = losses.resize_masks(m, res)
    assert ref[1].sum() == 0 and ref[2].all() and all(ref[i].sum() >= 1 for i in (3, 4, 5, 6))
    assert np.array_equal(losses.resize_masks_any(m, res), ref)
    win = torch.from_numpy(np.concatenate([losses.any_windows(H, res), losses.any_windows(W, res)]))
    out = torch.full((7, res * res), -1.0)
    attrcon_sim.mask_resize_any(torch.from_numpy(m.astype(np.uint8)), win[0], win[1], win[2], win[3], out, 7, H, W, res)
    assert np.array_equal(out.numpy(), ref)
    attrcon_sim.mask_resize_any(None, None, None, None, None, None, 0, H, W, res)  # n = 0: no launch, nothing touched
    assert attrcon_sim.launches["comat_mask_resize_any"] == 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ragged_batch_against_the_oracle(attrcon_sim, dtype):
    case = ragged_batch(dtype)
    ref = Oracle(case)
    attn_d = device_maps(case, torch.device("cpu"), dtype)
    tl, pl = run_device(case, attn_d, torch.device("cpu"))
    check_against(ref, tl, pl, attn_d, dtype)
    a = attn_d["1"]["up_8"][0].grad.reshape(case["bs"], 2, 8, 8, 11)
    assert float(a[1].abs().max()) == 0.0 and float(a[0].abs().max()) > 0.0  # the skipped sample: exactly nothing
    # one resize per resolution, one loss launch per (timestep, layer), one gather / gradient launch per map
    n = attrcon_sim.launches
    assert (n["comat_mask_resize_any"], n["comat_attrcon_loss"], n["comat_attrcon_gather_fwd"], n["comat_attrcon_gather_bwd"]) == (3, 6, 15, 15)


def test_empty_cases_launch_nothing(attrcon_sim):
    bs, heads, L = 2, 2, 9
    attn = {"1": maps_of(bs, heads, (("up_8", 8),), L, 1, 3, torch.float32)}
    attn["1"]["up_8"][0].requires_grad_(True)
    m = np.ones((1, 16, 16), dtype=bool)
    for masks, attrs in (([None, None], [[[1]], [[2]]]), ([m, m], [[], []])):
        tl, pl = losses.mask_loss_device(attn, masks, attrs, ("up_8",), bs, torch.device("cpu"))
        assert float(tl) == 0.0 and float(pl) == 0.0
        assert not tl.requires_grad and not pl.requires_grad  # no gradient flows: the maps' gradients are zero
    assert attn["1"]["up_8"][0].grad is None and sum(attrcon_sim.launches.values()) == 0


def _one_layer_case(attrs, L, seed, masks=None):
    bs, H = len(attrs), 32
    if masks is None:
        rng = np.random.default_rng(seed)
        masks = [rng.random((len(a), H, H)) < 0.3 for a in attrs]
    return dict(attn={"7": maps_of(bs, 2, (("up_8", 8),), L, 2, seed, torch.float32)}, masks=masks, attrs=attrs, layers=("up_8",), bs=bs)


def test_more_than_32_tokens_in_one_sample(attrcon_dev):
    """40 tokens in 5 objects next to a sample with 2: TOK is the batch's maximum, the short rows are padded"""
    attrs = [[list(range(8 * i, 8 * i + 8)) for i in range(5)], [[3], [9]]]
    case = _one_layer_case(attrs, 41, 5)
    attn_d = device_maps(case, attrcon_dev, torch.float32)
    tl, pl = run_device(case, attn_d, attrcon_dev)
    check_against(Oracle(case), tl, pl, attn_d, torch.float32)


def test_one_token_column_named_by_two_objects(attrcon_dev):
    """column 4 belongs to both objects: its gradient is the sum of both mentions"""
    case = _one_layer_case([[[2, 4], [4, 6]]], 9, 6)
    attn_d = device_maps(case, attrcon_dev, torch.float32)
    tl, pl = run_device(case, attn_d, attrcon_dev)
    check_against(Oracle(case), tl, pl, attn_d, torch.float32)


def test_golden_totals_of_the_reference_assembly(attrcon_dev):
    """tests/golden/mask_loss.npz = the totals of the reference's own get_mask_loss, read as
    tests/test_losses.py::test_mask_loss_against_the_reference_assembly reads them"""
    from comat_amd import attr_index
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "mask_loss.npz"))
    bs, layers = int(d["bs"]), [str(s) for s in d["layers"]]
    subtrees = [[[2, 3], [6, 7]], [[2, 3]], [[1, 2], [4, 5], [8], [10, [11, 12]]]]
    pieces = [{1: "a", 2: "red", 3: "car", 4: "and", 5: "a", 6: "blue", 7: "dog"},
              {1: "a", 2: "tall", 3: "tree"},
              {1: "a", 2: "cat", 3: "a", 4: "big", 5: "cat", 6: "and", 7: "the", 8: "sky", 9: "a", 10: "green", 11: "skate", 12: "board"}]
    got = [attr_index.nouns_and_attributes(st, pc) for st, pc in zip(subtrees, pieces)]
    attn_dict = {}
    for key in d.files:
        if key.startswith("map:"):
            _, ts, place = key.split(":")
            attn_dict.setdefault(ts, {})[place] = [torch.from_numpy(m).to(attrcon_dev) for m in d[key]]
    masks = [np.concatenate([d[f"mask:{n}"][0] for n in nouns]) if "tree" not in nouns else None for nouns, _ in got]
    tl, pl = losses.mask_loss_device(attn_dict, masks, [a for _, a in got], layers, bs, attrcon_dev)
    if attrcon_dev.type == "cpu":  # the leg that counts its launches
        assert ops.attrcon_kernels().launches["comat_attrcon_loss"] > 0
    assert abs(float(tl) - float(d["token_loss"])) < 2e-5 * max(1.0, abs(float(d["token_loss"])))
    assert abs(float(pl) - float(d["pixel_loss"])) < 2e-5 * max(1.0, abs(float(d["pixel_loss"])))


def test_nan_in_a_gathered_column_is_carried_and_elsewhere_is_not_read(attrcon_dev):
    case = ragged_batch(torch.float32)
    dev = attrcon_dev

    def run(col):
        attn_d = device_maps(case, dev, torch.float32)
        if col is not None:
            with torch.no_grad():
                attn_d["1"]["up_8"][1][0, 3, 5, col] = float("nan")  # sample 0, head 0
        tl, pl = run_device(case, attn_d, dev)
        return tl, pl, attn_d

    tl0, pl0, clean = run(None)
    tl, pl, d = run(3)  # token 3: an attribute token of sample 0's first object
    assert torch.isnan(tl) and torch.isnan(d["1"]["up_8"][1].grad).any()
    assert not torch.isnan(d["41"]["up_8"][0].grad).any()  # another (timestep, layer) node
    tl, pl, d = run(9)  # no token of any sample names column 9
    assert torch.equal(tl, tl0) and torch.equal(pl, pl0)
    for ts in clean:
        for k in clean[ts]:
            for a, b in zip(d[ts][k], clean[ts][k]):
                assert torch.equal(a.grad, b.grad)


def test_masks_of_two_sizes_fall_back_to_the_host_assembly(attrcon_sim):
    case = ragged_batch(torch.float32)
    case["masks"][2] = np.repeat(case["masks"][2], 2, axis=2)  # [1, 48, 96]
    cpu = torch.device("cpu")
    got, ref = device_maps(case, cpu, torch.float32), device_maps(case, cpu, torch.float32)
    tl, pl = run_device(case, got, cpu)
    tl_h, pl_h = run_device(case, ref, cpu, fn=losses.mask_loss)
    assert torch.equal(tl, tl_h) and torch.equal(pl, pl_h) and attrcon_sim.launches["comat_attrcon_loss"] == 0


def test_token_position_beyond_the_maps_is_refused(attrcon_sim):
    case = ragged_batch(torch.float32)
    case["attrs"][0] = [[2, 11], [7]]
    with pytest.raises(ValueError, match="outside"):
        losses.mask_loss_device(case["attn"], case["masks"], case["attrs"], case["layers"], case["bs"], torch.device("cpu"))


def test_flag_without_attrcon_raises():
    from comat_amd.step import StepConfig
    with pytest.raises(ValueError, match="attrcon_on_device"):
        StepConfig(attrcon_on_device=True, attrcon=False)
    assert StepConfig(attrcon_on_device=True, attrcon=True).attrcon_on_device and not StepConfig().attrcon_on_device


def test_tiny_step_with_the_flag_matches_the_oracle_step(attrcon_sim, monkeypatch):
    """the configuration of tests/test_step.py::test_train_step_matches_oracle[attrcon], switched by the environment as a
    benchmark run would, held to that test's fp32 bounds"""
    from oracle import step as OS
    from test_step import make_world
    dtype, cpu = torch.float32, torch.device("cpu")
    monkeypatch.setenv("COMAT_ATTRCON_DEVICE", "1")
    cfg, batch, W, trainer = make_world(dtype, cpu, True)
    assert trainer.attrcon_on_device
    assert not make_world(dtype, cpu, False)[3].attrcon_on_device  # a configuration without the loss is left alone
    ts, crop, acs = [1, 2], (1, 0, 63, 63), [2]
    opt = torch.optim.AdamW(list(W["lora"].values()), lr=cfg.lr, betas=(cfg.adam_beta1, cfg.adam_beta2), eps=cfg.adam_epsilon,
                            weight_decay=cfg.adam_weight_decay)
    d_params = list(W["d_lora"].values()) + [W["head_w"], W["head_b"]]
    opt_D = torch.optim.AdamW(d_params, lr=cfg.lr_D, betas=(cfg.adam_beta1_D, cfg.adam_beta2_D), eps=cfg.adam_epsilon,
                              weight_decay=cfg.adam_weight_decay)
    ref = OS.train_step(W, batch, cfg, ts, crop, acs, opt, opt_D)
    logs = trainer.train_step(batch, training_steps=ts, crop=crop, attrcon_steps=acs)
    assert attrcon_sim.launches["comat_attrcon_loss"] == 3  # one captured timestep, three layers
    for k, r in (("Blip", "Blip"), ("G_loss", "G_loss"), ("D_loss", "D_loss"), ("step_loss", "loss"), ("token_loss", "token_loss"),
                 ("pixel_loss", "pixel_loss")):
        check(logs[k], ref[r], dtype, k)
    bank, dbank = trainer.bank, trainer.D.bank
    g_ref = torch.cat([ref["g_grads"][n].reshape(-1) for n in bank.names])
    d_ref = torch.cat([ref["d_grads"][n].reshape(-1) for n in dbank.names])
    assert rel_l2(bank.flat_grad, g_ref) < 1e-3, f"G LoRA grads rel-L2 {rel_l2(bank.flat_grad, g_ref):.3e}"
    assert rel_l2(dbank.flat_grad, d_ref) < 1e-3
    p_ref = torch.cat([W["lora"][n].detach().reshape(-1) for n in bank.names])
    assert rel_l2(bank.flat, p_ref) < 3e-4
