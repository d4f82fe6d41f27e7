"""The ABI simulator with the entry points of the attribute-concentration loss on the device (comat_mask_resize_any,
comat_attrcon_workspace_floats, comat_attrcon_gather_fwd, comat_attrcon_loss, comat_attrcon_gather_bwd; include/comat_hip.h) -
TEST INFRASTRUCTURE ONLY.  The binding keeps their wrappers as module functions (comat_amd._hip, handed out by
ops.attrcon_kernels()); this subclass of the simulator carries their mirrors under the same names and argument lists and counts
its launches, and the tests of `StepConfig.attrcon_on_device` install it over the `sim` leg of conftest's `dev` fixture
(`attrcon_dev` below)."""
from __future__ import annotations

import collections

import pytest
import torch

from sim_backend import SimKernels, _refuse

NAMES = ("mask_resize_any", "attrcon_workspace_floats", "attrcon_gather_fwd", "attrcon_loss", "attrcon_gather_bwd")


def _bce(p, t):
    """comat_attrcon_loss: value and derivative of one term.  The logarithms are clamped at -100 (a NaN is carried), the
    derivative of a clamped logarithm is 0 - except that a NaN probability is carried into it too."""
    lp, lq = torch.log(p), torch.log(1.0 - p)
    cp, cq = torch.where(lp < -100.0, torch.full_like(lp, -100.0), lp), torch.where(lq < -100.0, torch.full_like(lq, -100.0), lq)
    nanp = torch.where(torch.isnan(p), p, torch.zeros_like(p))
    dcp = torch.where(lp >= -100.0, 1.0 / p, nanp)
    dcq = torch.where(lq >= -100.0, -1.0 / (1.0 - p), nanp)
    return (t - 1.0) * cq - t * cp, (t - 1.0) * dcq - t * dcp


class AttrconSimKernels(SimKernels):
    def __init__(self):
        super().__init__()
        self.launches = collections.Counter()

    @staticmethod
    def _tokens(n_obj, n_tok, b, TOK):
        return min(max(int(n_tok[b]), 0), TOK) if int(n_obj[b]) > 0 else 0

    def mask_resize_any(self, masks, ylo, yhi, xlo, xhi, out, n, H, W, res):
        name = "comat_mask_resize_any"
        _refuse(name, 0 <= n <= 65535 and H > 0 and 0 < W <= 32768 and 0 < res <= 65535, "bad shape")
        if n == 0:
            return
        _refuse(name, all(t is not None for t in (masks, ylo, yhi, xlo, xhi, out)), "null pointer")
        assert masks.dtype == torch.uint8 and out.dtype == torch.float32
        self.launches[name] += 1
        m, o = masks.reshape(-1, H, W)[:n] != 0, out.reshape(-1, res, res)
        for oy in range(res):
            rows = m[:, max(int(ylo[oy]), 0):min(int(yhi[oy]), H)].any(1)  # [n, W]
            for ox in range(res):
                o[:n, oy, ox] = rows[:, max(int(xlo[ox]), 0):min(int(xhi[ox]), W)].any(1).float()

    def attrcon_workspace_floats(self, M, bs, heads, npix, TOK):
        return 0 if min(M, bs, heads, npix, TOK) <= 0 else max(bs * heads * TOK * (-(-npix // 128) * 2 + npix), bs * -(-npix // 256))

    @staticmethod
    def _shape(name, bs, heads, npix, L, OBJ, TOK):
        _refuse(name, 0 < bs <= 65535 and 0 < heads <= 65535 and min(npix, L, OBJ, TOK) > 0, "bad shape")

    def attrcon_gather_fwd(self, amap, masks, n_obj, n_tok, tok_idx, tok_obj, num, den, avg, ws, bs, heads, npix, L, OBJ, TOK):
        name = "comat_attrcon_gather_fwd"
        _refuse(name, all(t is not None for t in (amap, masks, n_obj, n_tok, tok_idx, tok_obj, num, den, avg, ws)), "null pointer")
        _refuse(name, amap.dtype in (torch.float32, torch.bfloat16), "bad dtype")
        self._shape(name, bs, heads, npix, L, OBJ, TOK)
        self.launches[name] += 1
        a = amap.reshape(bs, heads, npix, L).float()
        mk, num, den, avg = masks.reshape(bs, OBJ, npix), num.reshape(bs, heads, TOK), den.reshape(bs, heads, TOK), avg.reshape(bs, TOK, npix)
        for b in range(bs):
            nt = self._tokens(n_obj, n_tok, b, TOK)
            if nt == 0:
                continue
            idx = tok_idx.reshape(bs, TOK)[b, :nt].long()
            col = a[b][:, :, idx.clamp(0, L - 1)]                                       # [heads, npix, nt]
            col = torch.where((idx >= 0) & (idx < L), col, torch.zeros_like(col))       # a column outside [0, L): the value 0
            m = mk[b][tok_obj.reshape(bs, TOK)[b, :nt].long().clamp(0, OBJ - 1)]        # [nt, npix]: tok_obj clamped
            num[b, :, :nt] = (col * m.t()[None]).sum(1)  # the order of sums of den: under a full mask num carries den's bits
            den[b, :, :nt] = col.sum(1)
            avg[b, :nt] += col.mean(0).t()

    def attrcon_loss(self, num, den, avg, masks, n_obj, n_tok, tok_obj, inv_len, g_num, g_den, g_avg, out, ws, M, bs, heads, npix,
                     OBJ, TOK):
        name = "comat_attrcon_loss"
        _refuse(name, all(t is not None for t in (num, den, avg, masks, n_obj, n_tok, tok_obj, inv_len, g_num, g_den, g_avg, out, ws)),
                "null pointer")
        _refuse(name, 0 < M <= 1024, "bad M")
        self._shape(name, bs, heads, npix, 1, OBJ, TOK)
        self.launches[name] += 1
        sh = (M, bs, heads, TOK)
        num, den, g_num, g_den = num.reshape(sh), den.reshape(sh), g_num.reshape(sh), g_den.reshape(sh)
        avg, g_avg, mk = avg.reshape(bs, TOK, npix), g_avg.reshape(bs, TOK, npix), masks.reshape(bs, OBJ, npix)
        tl, pl = torch.zeros(()), torch.zeros(())
        for b in range(bs):
            nt = self._tokens(n_obj, n_tok, b, TOK)
            if nt == 0:
                continue
            no = min(int(n_obj[b]), OBJ)
            n, d = num[:, b, :, :nt], den[:, b, :, :nt]  # [M, heads, nt]
            act = (n / d).mean(1)                        # [M, nt]
            w = inv_len.reshape(bs, TOK)[b, :nt] / (no * bs)
            tl = tl + (w * (1.0 - act) ** 2).sum()
            ga = (-2.0 * w * (1.0 - act) / heads)[:, None, :]
            g_num[:, b, :, :nt] = ga / d
            g_den[:, b, :, :nt] = -ga * n / (d * d)
            obj = tok_obj.reshape(bs, TOK)[b, :nt].long()
            for i in range(no):
                ts = torch.nonzero(obj == i).reshape(-1)
                word = avg[b, ts].sum(0) / M if len(ts) else torch.zeros(npix)
                l, dp = _bce(word, mk[b, i])
                pl = pl + l.sum() / (no * npix * bs)
                if len(ts):
                    g_avg[b, ts] = (dp / (no * npix * bs * M))[None].expand(len(ts), npix)
        out[0], out[1] = tl, pl

    def attrcon_gather_bwd(self, g_num, g_den, g_avg, masks, n_obj, n_tok, tok_idx, tok_obj, go, damap, bs, heads, npix, L, OBJ, TOK):
        name = "comat_attrcon_gather_bwd"
        _refuse(name, all(t is not None for t in (g_num, g_den, g_avg, masks, n_obj, n_tok, tok_idx, tok_obj, go, damap)), "null pointer")
        _refuse(name, damap.dtype in (torch.float32, torch.bfloat16), "bad dtype")
        self._shape(name, bs, heads, npix, L, OBJ, TOK)
        self.launches[name] += 1
        d = torch.zeros((bs, heads, npix, L), dtype=torch.float32)  # the kernel writes every element
        g_num, g_den, g_avg, mk = g_num.reshape(bs, heads, TOK), g_den.reshape(bs, heads, TOK), g_avg.reshape(bs, TOK, npix), masks.reshape(bs, OBJ, npix)
        for b in range(bs):
            for t in range(self._tokens(n_obj, n_tok, b, TOK)):  # ascending: a column named twice accumulates
                c, o = int(tok_idx.reshape(bs, TOK)[b, t]), min(max(int(tok_obj.reshape(bs, TOK)[b, t]), 0), OBJ - 1)
                if not 0 <= c < L:  # a column outside [0, L): no gradient
                    continue
                d[b, :, :, c] += go[0] * (g_num[b, :, t, None] * mk[b, o][None] + g_den[b, :, t, None]) + go[1] * g_avg[b, t][None] / heads
        damap.copy_(d.reshape(damap.shape).to(damap.dtype))


def sim_matches_binding():
    """(names, mismatches): the mirrors above against the binding's module functions, by argument list"""
    import inspect

    from comat_amd import _hip
    args = lambda f, skip: list(inspect.signature(f).parameters)[skip:]
    return NAMES, [n for n in NAMES if args(getattr(_hip, n), 0) != args(getattr(AttrconSimKernels, n), 1)]


@pytest.fixture
def attrcon_dev(dev):
    """conftest's `dev` with the simulator that knows the entry points on the sim leg; the hip leg is the real library"""
    from comat_amd import ops
    if dev.type == "cpu":
        ops.set_kernel_backend(AttrconSimKernels())
    return dev


@pytest.fixture
def attrcon_sim(sim):
    from comat_amd import ops
    k = AttrconSimKernels()
    ops.set_kernel_backend(k)
    return k
