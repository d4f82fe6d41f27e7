"""Attribute-concentration losses on the captured cross-attention maps (HIP gather kernel + tiny reductions).

Mirrors `get_grounding_loss_by_layer` (attn_utils/tc_loss_utils.py:66-173) and the per-sample / per-timestep /
per-layer assembly of `GsamSegModel.get_mask_loss` (attr_concen_utils/gsam_interface.py:140-228).  The object masks
(FastSAM + GroundingDINO, out of scope) and the attribute token lists (spaCy, out of scope) are INPUTS.
One pass of the strided gather kernel over each captured map produces, for all attribute tokens at once, the masked
and unmasked spatial sums per head (token loss) and the head-mean map per token (pixel loss); the remaining
reductions run on [heads, n_tok] and [n_tok, res*res] tensors.
`mask_loss_device` (StepConfig.attrcon_on_device) is the same loss as device work for the whole batch: the mask resize, the
gather, the remaining reductions and their gradients in HIP kernels driven by tables in device memory, no host synchronisation.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .resize import aa_taps


def _apply_taps(x: np.ndarray, start: np.ndarray, wts: np.ndarray) -> np.ndarray:
    """x [n, S, W] -> [n, res, W]: out[:, o] = sum_t wts[o, t] * x[:, start[o] + t]  (taps beyond the source carry
    weight 0).  <= 17 taps per output row: a gather + small contraction, no dense [res, S] GEMM on the host."""
    kt = wts.shape[1]
    idx = np.minimum(start[:, None].astype(np.int64) + np.arange(kt)[None], x.shape[1] - 1)  # [res, kt]
    return np.einsum("ok,nokw->now", wts.astype(np.float64), x[:, idx, :])


def resize_masks(masks: np.ndarray, res: int) -> np.ndarray:
    """masks [n_obj, H, W] bool -> [n_obj, res*res] float {0,1}: torchvision Resize(antialias=True) on a bool mask
    followed by `> 0` (tc_loss_utils.py:88-98)."""
    n, H, W = masks.shape
    ys, yw, _ = aa_taps(H, res, "bilinear")
    xs, xw, _ = aa_taps(W, res, "bilinear")
    rows = _apply_taps(masks.astype(np.float64), ys, yw)                              # [n, res, W]
    out = _apply_taps(np.ascontiguousarray(rows.transpose(0, 2, 1)), xs, xw)          # [n, res(x), res(y)]
    return (out.transpose(0, 2, 1) > 0.0).astype(np.float32).reshape(n, res * res)


def _bce(p, t):
    """The formula of F.binary_cross_entropy(p, t, reduction="none"), the logarithms clamped at -100 as torch clamps them.  The
    fused torch operator checks 0 <= p <= 1 - on a GPU with a device-side assertion - and a NaN probability fails that check: a
    step with a NaN in it would abort the process instead of reaching the optimizer's skip.  These operators carry the NaN.
    Same precision, NOT the same bits: a few per cent of the values differ from the fused operator's in the last place, and the
    gradient, which autograd takes through log and clamp where torch's backward uses the closed form (p - t) / (p (1 - p)),
    differs by about 1e-7 relative in about a third of the elements."""
    return (t - 1.0) * torch.log(1.0 - p).clamp(min=-100.0) - t * torch.log(p).clamp(min=-100.0)


def grounding_loss_by_layer(masks_res: torch.Tensor, word_token_idx_ls, res, attn_maps):
    """masks_res: [n_obj, res*res] fp32 {0,1} on the device; attn_maps: list of [heads, res, res, L] maps of ONE
    sample (views of the stored probabilities).  Returns (token_loss, pixel_loss) scalars."""
    n_obj = len(word_token_idx_ls)
    dev = masks_res.device
    if n_obj == 0:
        z = torch.zeros((), device=dev)
        return z, z
    tok_idx = torch.tensor([t for w in word_token_idx_ls for t in w], dtype=torch.int32, device=dev)
    tok_obj = torch.tensor([i for i, w in enumerate(word_token_idx_ls) for _ in w], dtype=torch.int32, device=dev)
    inv_len = torch.tensor([1.0 / len(w) for w in word_token_idx_ls for _ in w], dtype=torch.float32, device=dev)
    onehot = F.one_hot(tok_obj.long(), n_obj).float()  # [n_tok, n_obj]
    token_loss = torch.zeros((), device=dev)
    avg_sum = None
    for a in attn_maps:
        h = a.shape[0]
        num, den, avg = ops.attnmap_gather(a.reshape(h, res * res, a.shape[-1]), masks_res, tok_idx, tok_obj)
        act = (num / den).mean(0)  # [n_tok]
        token_loss = token_loss + (((1.0 - act) ** 2) * inv_len).sum()
        avg_sum = avg if avg_sum is None else avg_sum + avg
    token_loss = token_loss / n_obj
    # [n_obj, npix]: the tokens of one object are summed - a masked reduction over <= a handful of tokens, in a fixed
    # order (no vendor GEMM on the path, no atomics)
    word = (onehot.t()[:, :, None] * (avg_sum / len(attn_maps))[None]).sum(1)
    pixel_loss = _bce(word, masks_res).mean(1).sum() / n_obj
    return token_loss, pixel_loss


def mask_loss(attn_dict, masks_per_sample, attributes_per_sample, train_layer_ls, bs, device):
    """`get_mask_loss` with detector outputs as inputs.  attn_dict: {timestep: {place_res: [(bs*heads,res,res,L)]}};
    masks_per_sample[i]: [n_obj, H, W] bool numpy array or None; attributes_per_sample[i]: list[n_obj] of token
    index lists.  Returns (token_loss, pixel_loss) averaged over the batch (gsam_interface.py:225-226)."""
    token_loss = torch.zeros((), device=device)
    pixel_loss = torch.zeros((), device=device)
    for idx in range(bs):
        masks, attrs = masks_per_sample[idx], attributes_per_sample[idx]
        if masks is None or len(attrs) == 0:
            continue
        cache = {}
        for ts in attn_dict:
            for layer in train_layer_ls:
                res = int(layer.split("_")[1])
                if res not in cache:
                    cache[res] = torch.from_numpy(resize_masks(masks, res)).to(device)
                maps = [m.reshape(bs, m.shape[0] // bs, *m.shape[1:])[idx] for m in attn_dict[ts][layer]]
                tl, pl = grounding_loss_by_layer(cache[res], attrs, res, maps)
                token_loss = token_loss + tl
                pixel_loss = pixel_loss + pl
    return token_loss / bs, pixel_loss / bs


# ---- the same loss as device work (StepConfig.attrcon_on_device) -----------------------------------------------------------
def any_windows(n_in: int, res: int) -> np.ndarray:
    """int32 [2, res]: per output index the half-open source range [lo, hi) of the bilinear antialias taps with weight > 0.  The
    taps are non-negative, so `resize > 0` is the logical OR of the source pixels in the window (comat_mask_resize_any)."""
    start, wts, _ = aa_taps(n_in, res, "bilinear")
    win = np.zeros((2, res), dtype=np.int32)
    for o in range(res):
        pos = np.nonzero(wts[o] > 0)[0]
        assert len(pos) and (wts[o] >= 0).all() and len(pos) == pos[-1] - pos[0] + 1, "positive taps form one run"
        win[0, o], win[1, o] = start[o] + pos[0], min(start[o] + pos[-1] + 1, n_in)
    return win


def resize_masks_any(masks: np.ndarray, res: int) -> np.ndarray:
    """`resize_masks` by the window tables on the host: what comat_mask_resize_any computes, bit for bit"""
    n, H, W = masks.shape
    (ylo, yhi), (xlo, xhi) = any_windows(H, res), any_windows(W, res)
    rows = np.stack([masks[:, ylo[o]:yhi[o]].any(1) for o in range(res)], 1)             # [n, res, W]
    out = np.stack([rows[:, :, xlo[o]:xhi[o]].any(2) for o in range(res)], 2)            # [n, res, res]
    return out.astype(np.float32).reshape(n, res * res)


_WINDOWS = {}  # (H, W, res, device) -> int32 [4, res] on the device: ylo, yhi, xlo, xhi


def _staged(host: torch.Tensor, device) -> torch.Tensor:
    """host tensor -> device without a synchronisation.  On a GPU the source is a FRESH pinned tensor of torch's caching host
    allocator: the allocator hands its block out again only after the copy has executed, so the host may run steps ahead of
    the device without overwriting tables whose copy is still queued."""
    if torch.device(device).type != "cuda":
        return host.to(device)
    return host.pin_memory().to(device, non_blocking=True)


def _windows(H, W, res, device):
    key = (H, W, res, str(device))
    t = _WINDOWS.get(key)
    if t is None:
        t = _WINDOWS[key] = _staged(torch.from_numpy(np.concatenate([any_windows(H, res), any_windows(W, res)])), device)
    return t


def pack_attrcon_tables(attributes_per_sample, active, L=None):
    """host side of the device tables: (int32 [2 * bs + 3 * bs * TOK] = n_obj | n_tok | tok_idx | tok_obj | inv_len bits, OBJ, TOK).
    A sample that is not `active` (no masks, or no attributes) gets n_obj = 0."""
    bs = len(attributes_per_sample)
    flat = [[(t, i, 1.0 / len(w)) for i, w in enumerate(a) for t in w] if on else [] for a, on in zip(attributes_per_sample, active)]
    OBJ = max([len(a) for a, on in zip(attributes_per_sample, active) if on] + [1])
    TOK = max([len(f) for f in flat] + [1])
    tab = np.zeros(2 * bs + 3 * bs * TOK, dtype=np.int32)
    idx, obj = tab[2 * bs:2 * bs + bs * TOK].reshape(bs, TOK), tab[2 * bs + bs * TOK:2 * bs + 2 * bs * TOK].reshape(bs, TOK)
    inv = tab[2 * bs + 2 * bs * TOK:].view(np.float32).reshape(bs, TOK)
    for b, f in enumerate(flat):
        if not f:
            continue
        tab[b], tab[bs + b] = len(attributes_per_sample[b]), len(f)
        idx[b, :len(f)], obj[b, :len(f)], inv[b, :len(f)] = zip(*f)
        if min(idx[b, :len(f)]) < 0 or (L is not None and max(idx[b, :len(f)]) >= L):
            raise ValueError(f"sample {b}: attribute token positions {sorted(set(idx[b, :len(f)].tolist()))} outside the maps' {L} columns")
    return tab, OBJ, TOK


def mask_loss_device(attn_dict, masks_per_sample, attributes_per_sample, train_layer_ls, bs, device):
    """`mask_loss` - same arguments, same two scalars - as device work: the masks and the ragged token tables of the whole batch
    go to the device in two non-blocking copies from pinned memory, one comat_mask_resize_any launch per resolution resizes every
    object mask of the batch, and each (timestep, layer) is one autograd node over its captured maps (ops.attrcon_layer_loss: a
    gather launch pair per map, one loss launch pair, one gradient launch per map in the backward).  No device-to-host read, no
    pageable copy, no per-sample loop.
    Differences from `mask_loss`: the values agree to fp32 rounding, not bit for bit (another summation order); where a clamp of
    `_bce` is active (a probability of exactly 0 or 1) the gradient is 0, where autograd through log and clamp gives 0 / 0.
    Samples whose masks differ in (H, W) within one batch are not packed: such a call is answered by `mask_loss`."""
    active = [m is not None and len(a) > 0 for m, a in zip(masks_per_sample, attributes_per_sample)]
    if not any(active):  # nothing to launch
        z = torch.zeros((), device=device)
        return z, z.clone()
    shapes = {tuple(m.shape[1:]) for m, on in zip(masks_per_sample, active) if on}
    if len(shapes) > 1:
        return mask_loss(attn_dict, masks_per_sample, attributes_per_sample, train_layer_ls, bs, device)
    (H, W), = shapes
    first = next(iter(attn_dict.values()))[train_layer_ls[0]][0]
    tab_h, OBJ, TOK = pack_attrcon_tables(attributes_per_sample, active, L=first.shape[-1])
    masks_h = np.zeros((bs, OBJ, H, W), dtype=np.uint8)
    for b, (m, a) in enumerate(zip(masks_per_sample, attributes_per_sample)):
        if active[b]:
            if m.shape[0] < len(a):
                raise ValueError(f"sample {b}: {len(a)} attribute lists, {m.shape[0]} masks")
            masks_h[b, :len(a)] = m[:len(a)]
    tab_d, masks_d = _staged(torch.from_numpy(tab_h), device), _staged(torch.from_numpy(masks_h), device)
    n = bs * TOK
    tab = ops.AttrconTables(tab_d[:bs], tab_d[bs:2 * bs], tab_d[2 * bs:2 * bs + n].view(bs, TOK),
                            tab_d[2 * bs + n:2 * bs + 2 * n].view(bs, TOK), tab_d[2 * bs + 2 * n:].view(torch.float32).view(bs, TOK),
                            bs, OBJ, TOK)
    k, resized = ops.attrcon_kernels(), {}
    for layer in train_layer_ls:
        res = int(layer.split("_")[1])
        if res not in resized:
            win = _windows(H, W, res, device)
            out = torch.empty((bs, OBJ, res * res), dtype=torch.float32, device=device)
            k.mask_resize_any(masks_d, win[0], win[1], win[2], win[3], out, bs * OBJ, H, W, res)
            resized[res] = out
    token_loss = pixel_loss = None
    for ts in attn_dict:
        for layer in train_layer_ls:
            res = int(layer.split("_")[1])
            maps = [m.reshape(m.shape[0], res * res, m.shape[-1]) for m in attn_dict[ts][layer]]
            tl, pl = ops.attrcon_layer_loss(tab, resized[res], maps)
            token_loss = tl if token_loss is None else token_loss + tl
            pixel_loss = pl if pixel_loss is None else pixel_loss + pl
    return token_loss, pixel_loss
