"""Shared inputs and comparisons of tests/test_attrcon_device.py (simulator) and tests/test_attrcon_device_gpu.py (library)."""
import numpy as np
import torch

from comat_amd import losses
from helpers import check
from oracle import losses as OL

# (H, W, res) of the resize cases: down by 12 / 8 / 4, non-square with W not a multiple of 16, identity, up by 2, production
RESIZE_SHAPES = [(48, 48, 4), (97, 61, 8), (97, 61, 16), (64, 64, 64), (16, 16, 32), (512, 512, 64)]


def resize_masks_case(H, W):
    """[7, H, W] bool: random at density 0.01, empty, full, one set pixel in each corner"""
    m = np.zeros((7, H, W), dtype=bool)
    m[0] = np.random.default_rng(H * 1000 + W).random((H, W)) < 0.01
    m[2] = True
    m[3, 0, 0] = m[4, 0, W - 1] = m[5, H - 1, 0] = m[6, H - 1, W - 1] = True
    return m


def maps_of(bs, heads, reses, L, n_per, seed, dtype):
    """tests/test_losses._maps: {layer: n_per softmax maps [bs * heads, res, res, L]} rounded to dtype, as fp32"""
    g = torch.Generator().manual_seed(seed)
    return {name: [torch.softmax(torch.randn(bs * heads, res, res, L, generator=g) * 2, -1).to(dtype).float() for _ in range(n_per)]
            for name, res in reses}


def ragged_batch(dtype, L=11, heads=2, reses=(("mid_4", 4), ("up_8", 8), ("up_16", 16)), n_per=(2, 3)):
    """the inputs of tests/test_losses.py::test_mask_loss_ragged_batch: bs 3, a sample with two objects (one single-token
    attribute), a sample without masks, a sample with one object; two captured timesteps"""
    bs, H = 3, 48
    attn = {"41": maps_of(bs, heads, reses, L, n_per[0], 1, dtype), "1": maps_of(bs, heads, reses, L, n_per[1], 2, dtype)}
    m0 = np.zeros((2, H, H), dtype=bool)
    m0[0, 3:20, 5:30] = True
    m0[1, 25:47, 10:40] = True
    m2 = np.zeros((1, H, H), dtype=bool)
    m2[0, 0:9, 40:48] = True
    return dict(attn=attn, masks=[m0, None, m2], attrs=[[[2, 3, 4], [7]], [[1]], [[5, 6]]], layers=tuple(n for n, _ in reses), bs=bs)


class Oracle:
    """oracle.losses.mask_loss on a case, computed once: the two losses and, after backward of tl + 0.3 pl, every map's gradient"""

    def __init__(self, case):
        self.attn = {ts: {k: [m.clone().requires_grad_(True) for m in v] for k, v in d.items()} for ts, d in case["attn"].items()}
        om = [None if m is None else [torch.from_numpy(x)[None, None] for x in m] for m in case["masks"]]
        self.tl, self.pl = OL.mask_loss(self.attn, om, case["attrs"], case["layers"], case["bs"])
        if self.tl.requires_grad:
            (self.tl + 0.3 * self.pl).backward()


def device_maps(case, dev, dtype):
    return {ts: {k: [m.detach().clone().to(dev, dtype).requires_grad_(True) for m in v] for k, v in d.items()} for ts, d in case["attn"].items()}


def run_device(case, attn_d, dev, fn=None):
    tl, pl = (fn or losses.mask_loss_device)(attn_d, case["masks"], case["attrs"], case["layers"], case["bs"], dev)
    (tl + 0.3 * pl).backward()
    return tl, pl


def check_against(ref: Oracle, tl, pl, attn_d, dtype):
    """the bounds and factors of test_mask_loss_ragged_batch"""
    f = 10 if dtype == torch.bfloat16 else 1
    check(tl, ref.tl, torch.float32, "token loss", factor=f)
    check(pl, ref.pl, torch.float32, "pixel loss", factor=f)
    for ts in ref.attn:
        for k in ref.attn[ts]:
            for a, b in zip(attn_d[ts][k], ref.attn[ts][k]):
                check(a.grad, b.grad, dtype, f"d loss / d map {ts} {k}", factor=2)
