"""The attribute-concentration loss as device work on the library (comat_mask_resize_any, comat_attrcon_*): the resize bit for
bit, the batched kernels against the oracle for every kernel variant (staged and plain row chunks, fp32 and bf16 maps), run-to-run
bits, no host synchronisation, and a whole tiny step through SegmentedStep."""
import numpy as np
import pytest
import torch

from attrcon_cases import RESIZE_SHAPES, Oracle, check_against, device_maps, maps_of, ragged_batch, resize_masks_case, run_device
from comat_amd import _hip, losses

pytestmark = pytest.mark.gpu

_ORACLES = {}


def oracle_of(key, make):
    """(case, its oracle values), computed once per module and left unchanged"""
    if key not in _ORACLES:
        case = make()
        _ORACLES[key] = (case, Oracle(case))
    return _ORACLES[key]


@pytest.mark.parametrize("H, W, res", RESIZE_SHAPES)
def test_resize_kernel_equals_resize_masks(hip, H, W, res):
    m = resize_masks_case(H, W)
    win = torch.from_numpy(np.concatenate([losses.any_windows(H, res), losses.any_windows(W, res)])).to(hip)
    out = torch.full((7, res * res), -1.0, device=hip)
    _hip.mask_resize_any(torch.from_numpy(m.astype(np.uint8)).to(hip), win[0], win[1], win[2], win[3], out, 7, H, W, res)
    assert np.array_equal(out.cpu().numpy(), losses.resize_masks(m, res))
    # a source that starts off a 16-byte boundary: the element-wise row reads
    buf = torch.zeros(7 * H * W + 3, dtype=torch.uint8, device=hip)
    buf[3:].copy_(torch.from_numpy(m.astype(np.uint8)).reshape(-1))
    out.fill_(-1.0)
    _hip.mask_resize_any(buf[3:], win[0], win[1], win[2], win[3], out, 7, H, W, res)
    assert np.array_equal(out.cpu().numpy(), losses.resize_masks(m, res))


# L = 11: rows that are not a multiple of 16 bytes (every block's chunk of rows still is: the staged kernels); "up_3": 9 rows of
# 11 elements are no whole number of 16-byte vectors (the plain kernels); L = 77: the production row
CASES = {"L11": dict(L=11), "L77": dict(L=77), "plain": dict(L=11, reses=(("mid_4", 4), ("up_3", 3)), n_per=(1, 2))}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", list(CASES))
def test_ragged_batch_against_the_oracle(hip, dtype, name):
    case, ref = oracle_of((name, dtype), lambda: ragged_batch(dtype, **CASES[name]))
    attn_d = device_maps(case, hip, dtype)
    tl, pl = run_device(case, attn_d, hip)
    check_against(ref, tl, pl, attn_d, dtype)
    k = case["layers"][-1]
    a = attn_d["1"][k][0].grad.reshape(case["bs"], 2, -1)
    assert float(a[1].abs().max()) == 0.0 and float(a[0].abs().max()) > 0.0  # the skipped sample: exact zeros


def _res64_case(dtype):
    m = np.zeros((3, 48, 48), dtype=bool)
    m[0, 3:20, 5:30] = m[1, 25:47, 10:40] = m[2, 0:9, 40:48] = True
    return dict(attn={"9": maps_of(1, 2, (("up_64", 64),), 77, 1, 4, dtype)}, masks=[m], attrs=[[[2, 3], [7, 8], [70, 76]]],
                layers=("up_64",), bs=1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_one_map_at_res_64(hip, dtype):
    """npix 4096: 16 (bf16) / 32 (fp32) blocks per head in the gather, 32 in the gradient writer"""
    case, ref = oracle_of(("res64", dtype), lambda: _res64_case(dtype))
    attn_d = device_maps(case, hip, dtype)
    tl, pl = run_device(case, attn_d, hip)
    check_against(ref, tl, pl, attn_d, dtype)


def test_two_calls_give_the_same_bits(hip):
    case, _ = oracle_of(("L77", torch.bfloat16), lambda: ragged_batch(torch.bfloat16, **CASES["L77"]))
    runs = []
    for _ in range(2):
        attn_d = device_maps(case, hip, torch.bfloat16)
        tl, pl = run_device(case, attn_d, hip)
        runs.append((tl, pl, attn_d))
    (tl0, pl0, d0), (tl1, pl1, d1) = runs
    assert torch.equal(tl0, tl1) and torch.equal(pl0, pl1)
    for ts in d0:
        for k in d0[ts]:
            for a, b in zip(d0[ts][k], d1[ts][k]):
                assert torch.equal(a.grad, b.grad)


def test_no_host_synchronisation_and_batches_back_to_back(hip):
    """forward and backward complete under torch's sync debug mode "error"; two different batches issued back to back, the
    second staged while the first may still be queued, each match their own oracle"""
    dtype = torch.float32
    c1, r1 = oracle_of(("L11", dtype), lambda: ragged_batch(dtype, **CASES["L11"]))
    c2 = dict(c1, masks=[c1["masks"][2], c1["masks"][0], None], attrs=[[[1, 8]], [[5], [9, 10]], [[3]]])
    r2 = Oracle(c2)
    d1, d2 = device_maps(c1, hip, dtype), device_maps(c2, hip, dtype)
    run_device(c1, device_maps(c1, hip, dtype), hip)  # the window tables of these shapes are cached from here on
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        tl1, pl1 = run_device(c1, d1, hip)
        tl2, pl2 = run_device(c2, d2, hip)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    check_against(r1, tl1, pl1, d1, dtype)
    check_against(r2, tl2, pl2, d2, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_segmented_step_with_the_flag_matches_eager(hip, dtype, monkeypatch):
    """tests/test_segments.py::test_segmented_step_matches_eager[attrcon] with the flag on: six optimisation steps, eager vs
    segments, every logged loss, the parameters of G and D and the optimizer moments bit-identical"""
    from comat_amd.segments import SegmentedStep
    from test_segments import PLAN, run_plan
    from test_step import make_world
    monkeypatch.setenv("COMAT_ATTRCON_DEVICE", "1")
    cfg, batch, W, tr_e = make_world(dtype, hip, True)
    cfg, _, _, tr_g = make_world(dtype, hip, True)
    assert tr_e.attrcon_on_device and tr_g.attrcon_on_device
    tr_e.pipe.share_text_kv = False
    st = SegmentedStep(tr_g)
    run_plan(tr_e, st, batch, dtype, True, torch.equal)
    assert st.stats()["replays"] >= 10 and st.head_seg.replays == len(PLAN) - 1
