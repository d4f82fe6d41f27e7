"""LoRA: the store of the trainable factors, and the projections that carry them as autograd operators in the low-rank form
(_LoRAGroupLinear) and over merged weights (_LoRAMergedLinear).  `_lora_tail` and `_train_merged` are rebound by their
setters: read them through this module, never by value."""
from __future__ import annotations

import os

import torch
from torch.autograd import Function

from . import fp8, streams
from ._hip import UN_COPY
from .backend import _c, _uniform_stride, kernels


class LoRAGroup:
    """The LoRA factors of G projections that read the SAME input (q/k/v of a self-attention, k/v of a
    cross-attention, or a single projection):  y_i = x W_i^T + b_i + s * (x D_i^T) U_i^T.
    The G down factors are adjacent in the store's flat buffers, so `down_cat` [G*r, in] is ONE matrix: one GEMM
    produces all low-rank activations and one GEMM all down-gradients."""

    def __init__(self, store, index, down_cat, ups, rank, scale=1.0):
        self.store, self.index = store, index
        self.down_cat, self.ups = down_cat, ups      # fp32 leaves (views of store.flat) with .grad views
        self.rank, self.scale, self.size = rank, scale, len(ups)

    def compute_copies(self):
        """(down_cat [G*r, in], [up_i [out_i, r]], down_cat^T [in, G*r], [up_i^T [r, out_i]]) in the compute dtype."""
        self.store.ensure_compute_copy()
        return self.store.group_views[self.index]


class LoRAStore:
    """All trainable LoRA factors of one model in ONE flat fp32 buffer (+ one flat gradient buffer).  Every factor
    is a leaf view whose .grad is a view of the flat gradient: the GEMM epilogues accumulate weight gradients in
    place, RCCL all-reduces the flat buffer and the fused clip+AdamW kernel consumes it.  Two derived buffers are
    refreshed by one kernel each after an optimizer step: `flat_c` (compute-dtype copy) and `flat_t` (compute-dtype
    TRANSPOSED copies of the grouped down factors, so their data-gradient runs through the k-contiguous GEMM path).

    spec: list of groups; a group is a list of (down_name, up_name, down [r, in], up [out, r]) sharing `in`."""

    def __init__(self, spec, dtype, device, scale=1.0):
        self.names, shapes, layout = [], [], []
        off = toff = 0
        for members in spec:
            r, cin = members[0][2].shape
            assert all(tuple(m[2].shape) == (r, cin) and m[3].shape[1] == r for m in members)
            g = dict(down_off=off, rank=r, cin=cin, n=len(members), t_off=toff, ups=[], ut_offs=[])
            for dn, _, d, _ in members:
                self.names.append(dn)
                shapes.append((off, tuple(d.shape)))
                off += r * cin
            for _, un, _, u in members:
                self.names.append(un)
                shapes.append((off, tuple(u.shape)))
                g["ups"].append((off, tuple(u.shape)))
                off += u.shape[0] * r
            toff += len(members) * r * cin
            for _, _, _, u in members:  # transposed up factors U^T [r, out] follow the group's transposed down block
                g["ut_offs"].append(toff)
                toff += u.shape[0] * r
            layout.append(g)
        total = off
        src = {}
        for members in spec:
            for dn, un, d, u in members:
                src[dn], src[un] = d, u
        self.dtype, self.device = dtype, device
        self.flat = torch.empty(total, dtype=torch.float32, device=device)
        self.flat.copy_(torch.cat([src[n].detach().reshape(-1).float() for n in self.names]).to(device))
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=device)
        self.flat_c = None if dtype == torch.float32 else torch.empty(total, dtype=dtype, device=device)
        self.flat_t = torch.empty(toff, dtype=dtype, device=device)
        self._fresh, self.epoch = False, 0  # epoch counts refreshes: consumers that cache products of the copies compare it
        self._merged = {}

        def leaf(o, shp):
            n = shp[0] * shp[1]
            p = self.flat[o:o + n].view(shp).requires_grad_(True)
            p.grad = self.flat_grad[o:o + n].view(shp)
            return p

        self.params = {n: leaf(o, shp) for n, (o, shp) in zip(self.names, shapes)}
        comp = self.flat if self.flat_c is None else self.flat_c
        self.groups, self.group_views, self._leaves, tiles = [], [], list(self.params.values()), []
        for gi, g in enumerate(layout):
            r, cin, n = g["rank"], g["cin"], g["n"]
            dcat = leaf(g["down_off"], (n * r, cin))
            ups = [leaf(o, shp) for o, shp in g["ups"]]
            self._leaves += [dcat] + ups
            self.groups.append(LoRAGroup(self, gi, dcat, ups, r, scale))
            cv = lambda o, shp: comp[o:o + shp[0] * shp[1]].view(shp)
            uts = [self.flat_t[to:to + shp[0] * shp[1]].view(shp[1], shp[0]) for to, (_, shp) in zip(g["ut_offs"], g["ups"])]
            self.group_views.append((cv(g["down_off"], (n * r, cin)), [cv(o, shp) for o, shp in g["ups"]],
                                     self.flat_t[g["t_off"]:g["t_off"] + n * r * cin].view(cin, n * r), uts))
            mats = [(g["down_off"], g["t_off"], n * r, cin)] + [(o, to) + shp for to, (o, shp) in zip(g["ut_offs"], g["ups"])]
            for o, to, rows, cols in mats:  # 32 x 32 tiles of every matrix transpose_cast_tiles transposes
                tiles += [(o, to, rows, cols, r0, c0) for r0 in range(0, rows, 32) for c0 in range(0, cols, 32)]
        self._tiles = torch.tensor(tiles, dtype=torch.int64).to(device)

    def ensure_compute_copy(self):
        if not self._fresh:
            k = kernels()
            if self.flat_c is not None:
                k.unary(UN_COPY, self.flat, self.flat_c, self.flat.numel())
            k.transpose_cast_tiles(self.flat, self.flat_t, self._tiles)
            self._fresh = True
            self.epoch += 1
            if self._merged:  # merged weights that exist follow the parameters
                self._merge_entries()

    def mark_updated(self):
        """call after an in-place update of `flat` (optimizer kernel): the derived copies are refreshed lazily."""
        self._fresh = False

    # ---- merged weights W + s U D (see lora_group_linear / _LoRAMergedLinear) ---------------------------------------
    def merged_weights(self, grp, lins):
        """([W_i + s U_i D_i], [their transposes]) in the compute dtype for the projections `lins` of group `grp`: persistent
        buffers (one [G, N, K] + one [G, K, N] allocation when the frozen weights are co-allocated), created at the first
        use and refreshed in place whenever the compute copies are (once per optimizer step), so captured graphs can read
        them.  Memory: a second and third copy of every LoRA'd attention weight (SD1.5: 2 x 186 MB per UNet)."""
        self.ensure_compute_copy()
        key = (grp.index, tuple(id(l) for l in lins))
        ent = self._merged.get(key)
        if ent is None:
            if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("merged LoRA weights must exist before a capture begins (run the call eagerly once)")
            G = len(lins)
            shp = tuple(lins[0].w.shape)
            if G > 1 and all(tuple(l.w.shape) == shp for l in lins):
                wm = list(lins[0].w.new_empty((G,) + shp).unbind(0))
                wmt = list(lins[0].w.new_empty((G, shp[1], shp[0])).unbind(0))
            else:
                wm = [torch.empty_like(l.w) for l in lins]
                wmt = [torch.empty_like(l.wt) for l in lins]
            ent = self._merged[key] = dict(grp=grp, lins=tuple(lins), wm=wm, wmt=wmt)
            self._build_merge_table()
            self._merge_entries([ent])
        return ent["wm"], ent["wmt"]

    def _entry_problems(self, ent):
        """rows of comat_lora_merge's problem table for one entry, or None when the grouped kernel cannot take it"""
        grp, lins = ent["grp"], ent["lins"]
        _, ucs, dct, _ = self.group_views[grp.index]
        r, Gr = grp.rank, grp.size * grp.rank
        k = kernels()
        if not hasattr(k, "lora_merge"):
            return None
        rows = []
        for i, lin in enumerate(lins):
            dt_i = dct[:, i * r:(i + 1) * r]
            if not k.lora_merge_ok(lin.w, ucs[i], dt_i, r, r, Gr):
                return None
            N, Kd = lin.w.shape
            rows.append((lin.w.data_ptr(), ucs[i].data_ptr(), dt_i.data_ptr(), ent["wm"][i].data_ptr(), ent["wmt"][i].data_ptr(),
                         N, Kd, r, r, Gr))
        return rows

    def _build_merge_table(self):
        """device tables of ONE comat_lora_merge launch over every merged entry the grouped kernel takes (rebuilt whenever
        an entry is added - eagerly: the refresh inside a captured step only reads them)"""
        # one launch, one scale: the groups of a store share it (LoRAStore(scale=...) hands the same value to every group)
        assert all(g.scale == self.groups[0].scale for g in self.groups), "LoRA groups of one store must share their scale"
        probs, rest = [], []
        for ent in self._merged.values():
            rows = self._entry_problems(ent)
            if rows is None:
                rest.append(ent)
            else:
                probs += rows
        self._merge_rest = rest
        # a graph captured earlier replays comat_lora_merge with the addresses of the table it saw: superseded tables stay alive
        # (a few KB each; entries are only ever added while the model's first eager step runs)
        old = getattr(self, "_merge_table", None)
        if old is not None:
            self._merge_tables_kept = getattr(self, "_merge_tables_kept", []) + [old]
        self._merge_table = self._merge_tables(probs) if probs else None

    def _merge_tables(self, rows):
        """(problem table, tile table) of one comat_lora_merge launch over the problem rows `rows`: a tile is
        (problem, n0, k0), one per 64 x 64 block of the problem's [N, K] output"""
        import numpy as np
        tiles = []
        for pi, row in enumerate(rows):
            n0, k0 = np.meshgrid(np.arange(0, row[5], 64), np.arange(0, row[6], 64), indexing="ij")
            tiles.append(np.stack([np.full(n0.size, pi), n0.reshape(-1), k0.reshape(-1)], 1))
        return (torch.tensor(rows, dtype=torch.int64).to(self.device),
                torch.from_numpy(np.concatenate(tiles).astype(np.int32)).to(self.device))

    def _merge_entries(self, ents=None):
        """refresh the merged weights: every entry (ents None: one grouped launch + the entries it cannot take) or just
        `ents` (a new entry).  One scale per store (LoRAStore(scale=...) hands the same value to every group)."""
        k = kernels()
        if ents is None:
            if getattr(self, "_merge_table", None) is not None:
                k.lora_merge(self._merge_table[0], self._merge_table[1], self.groups[0].scale)
            for ent in getattr(self, "_merge_rest", ()):
                self._merge_into(ent)
            return
        for ent in ents:
            rows = self._entry_problems(ent)
            if rows is None:
                self._merge_into(ent)
            else:
                k.lora_merge(*self._merge_tables(rows), ent["grp"].scale)

    def _merge_into(self, ent):
        """one entry through comat_gemm (fp32 parity mode, shapes the grouped kernel does not take): Wm_i = W_i + s U_i D_i
        and WmT_i = W_i^T + s D_i^T U_i^T, a batched launch each for a co-allocated group"""
        grp, lins, wm, wmt = ent["grp"], ent["lins"], ent["wm"], ent["wmt"]
        _, ucs, dct, _ = self.group_views[grp.index]
        G, r = grp.size, grp.rank
        Gr = G * r
        k = kernels()
        N, Kd = lins[0].w.shape
        sw, su, sm = _uniform_stride([l.w for l in lins]), _uniform_stride(ucs), _uniform_stride(wm)
        swt, smt = _uniform_stride([l.wt for l in lins]), _uniform_stride(wmt)
        if G > 1 and None not in (sw, su, sm, swt, smt):
            # Wm_i[N, K] = W_i + s * U_i[N, r] (D^T[K, G*r] columns i*r..)^T  for all i in one batched launch
            k.gemm(ucs[0], dct, wm[0], N, Kd, r, r, Gr, Kd, batch=(G, 1), sA=(su, 0), sB=(r, 0), sC=(sm, 0),
                   R=lins[0].w, ldr=Kd, sR=(sw, 0), alpha=grp.scale, beta=1.0)
            k.gemm(dct, ucs[0], wmt[0], Kd, N, r, Gr, r, N, batch=(G, 1), sA=(r, 0), sB=(su, 0), sC=(smt, 0),
                   R=lins[0].wt, ldr=N, sR=(swt, 0), alpha=grp.scale, beta=1.0)
        else:
            for i, lin in enumerate(lins):
                N, Kd = lin.w.shape
                k.gemm(ucs[i], dct[:, i * r:(i + 1) * r], wm[i], N, Kd, r, r, Gr, Kd, R=lin.w, ldr=Kd, alpha=grp.scale, beta=1.0)
                k.gemm(dct[:, i * r:(i + 1) * r], ucs[i], wmt[i], Kd, N, r, Gr, r, N, R=lin.wt, ldr=N, alpha=grp.scale, beta=1.0)

    def zero_grad(self):
        self.flat_grad.zero_()
        for p in self._leaves:  # keep the views bound (the GEMM epilogues accumulate into them in place)
            if p.grad is None:
                raise RuntimeError("LoRA .grad view was dropped")

    def set_requires_grad(self, flag: bool):
        for p in self._leaves:
            p.requires_grad_(flag)

    def state_dict(self):
        return {n: p.detach().clone() for n, p in self.params.items()}


def _u_product(k, grp, lins, gs, uts, u, sg, su):
    """u[:, i*r:(i+1)*r] = s * g_i U_i for all i, through the transposed copies U_i^T [r, N] (refreshed with the other compute
    copies once per optimizer step): both operands k-contiguous, i.e. the pipelined kernel instead of a k-major gather.  sg / su:
    the spacing of the g_i (dQ / dK / dV of the fused attention backward) and of the U_i^T in one buffer each (ONE launch) or None"""
    M, r, Gr = u.shape[0], grp.rank, grp.size * grp.rank
    if sg is not None and su is not None:
        N0 = lins[0].out_features
        k.gemm(gs[0], uts[0], u, M, r, N0, N0, N0, Gr, alpha=grp.scale, batch=(grp.size, 1), sA=(sg, 0), sB=(su, 0), sC=(r, 0))
    else:
        for i, lin in enumerate(lins):
            N = lin.out_features
            k.gemm(gs[i], uts[i], u[:, i * r:(i + 1) * r], M, r, N, N, N, Gr, alpha=grp.scale)


def _factor_grads(grp, lins, gs, h, u, x, want_ups, want_down, pre=None, batched_ups=None):
    """The LoRA weight gradients, C += A^T B in fp32 in place, as k-major problems (A, B, C, M, N, K, lda, ldb, ldc): dU_i [N, r] +=
    g_i^T h_i in projection order, then d[D_1; ..; D_G] [G*r, K] += u^T x.  Queued on the grouped kernel, else (fp32 parity mode,
    odd shapes) one launch each - `batched_ups`: launches all G dU_i at once instead - still off the dependent chain.
    `pre`: produces operands only these problems read, in front of them on their stream."""
    M, Kd = x.shape
    r, Gr = grp.rank, grp.size * grp.rank
    probs = [(gs[i], h[:, i * r:(i + 1) * r], grp.ups[i].grad, lin.out_features, r, M, lin.out_features, Gr, r)
             for i, lin in enumerate(lins) if want_ups[i]]
    if want_down:
        probs.append((u, x, grp.down_cat.grad, Gr, Kd, M, Gr, Kd, Kd))
    if not probs:
        return
    k = kernels()
    if streams._tt_grouping and all(k.tt_group_ok(*pr) for pr in probs):
        streams._tt_enqueue(x.device, probs, (gs, h, u, x), pre=pre)
        return

    def weight_grads():
        if pre is not None:
            pre()
        if batched_ups is not None:
            batched_ups()
        for A, B, Cacc, Mp, Np, Kp, lda, ldb, ldc in probs[grp.size if batched_ups is not None else 0:]:
            k.gemm(A, B, Cacc, Mp, Np, Kp, lda, ldb, ldc, transA=True, transB=True, R=Cacc, ldr=ldc, beta=1.0)

    streams.run_off_chain(x.device, weight_grads, (gs, h, u, x))


class _LoRAGroupLinear(Function):
    """(y_1 .. y_G) with y_i = x W_i^T + b_i + (h_i) U_i^T (+ residual),  h = s * x [D_1; ..; D_G]^T.
    Forward: one GEMM for h, then ONE K-segmented GEMM per projection ([x | h_i] . [W_i | U_i]^T).
    Backward: u_i = s * g_i U_i (G small GEMMs into one [M, G*r] buffer), dx = sum_i g_i W_i + u [D_1; ..; D_G] as
    ONE K-segmented GEMM, and the LoRA weight gradients in fp32 straight out of the GEMM epilogue, accumulated in
    place into the flat gradient buffer (training_utils/pipeline.py:123-144 keeps LoRA params in fp32) on the side
    stream: dU_i += g_i^T h_i, d[D_1; ..; D_G] += u^T x (one GEMM)."""

    @staticmethod
    def forward(ctx, x, residual, grp, lins, down_cat, *ups):
        x = _c(x)
        M, Kd = x.shape
        G, r = grp.size, grp.rank
        Gr = G * r
        dc, ucs, dct, uts = grp.compute_copies()
        k = kernels()
        h = x.new_empty((M, Gr))
        if residual is not None:
            assert G == 1
            residual = _c(residual)
        sw, su = _uniform_stride([lin.w for lin in lins]), _uniform_stride(ucs)
        use8 = [fp8.use_fp8(lin, Kd) for lin in lins]
        k.gemm(x, dc, h, M, Gr, Kd, Kd, Kd, Gr, alpha=grp.scale)
        ktail_ok = r % 16 == 0 and Gr % 8 == 0  # the low-rank product can ride in an fp8 product's launch as a bf16 k-tail
        g8 = fp8.fp8_weight_group(lins) if (all(use8) and G > 1 and su is not None and ktail_ok
                                            and all(lin.bias is None for lin in lins)) else None
        if g8 is not None:
            # q / k / v (k / v) of one attention: ONE batched fp8 product (shared input bytes, a scale per frozen weight) and ONE
            # batched low-rank product on top of it - 3 launches for the group instead of 1 + 2 G
            x8, sx = fp8.fp8_act(x, lins[0])
            N = lins[0].out_features
            ys = x.new_empty((G, M, N))
            kt = dict(ktail=(h, ucs[0], r, Gr, r, r, su)) if fp8._ktail else {}
            k.gemm(x8, g8[0], ys, M, N, Kd, Kd, Kd, N, batch=(G, 1), sB=(N * Kd, 0), sC=(M * N, 0), scales=(sx, g8[1], 1), **kt)
            if not kt:
                k.gemm(h, ucs[0], ys, M, N, r, Gr, r, N, batch=(G, 1), sA=(r, 0), sB=(su, 0), sC=(M * N, 0), R=ys, ldr=N,
                       sR=(M * N, 0), beta=1.0)
            ys = list(ys.unbind(0))
        elif not any(use8) and sw is not None and su is not None and residual is None and all(lin.bias is None for lin in lins):
            # co-allocated frozen weights (frozen_linear_group) + adjacent up factors: ONE batched launch for the group
            N = lins[0].out_features
            ys = x.new_empty((G, M, N))
            k.gemm_segments([(x, lins[0].w, Kd, Kd, Kd, 0, sw), (h, ucs[0], r, Gr, r, r, su)], ys, M, N, N, batch=G, sC=M * N)
            ys = list(ys.unbind(0))
        else:
            # one launch per projection; under fp8_forward the frozen part of an eligible one runs on the fp8 MFMA (x quantised once
            # for the group), with the low-rank product as its bf16 k-tail (+ bias + residual: ONE launch) or in a launch behind it
            x8, sx = fp8.fp8_act(x, lins[use8.index(True)]) if any(use8) else (None, None)
            beta = 1.0 if residual is not None else 0.0
            ys = []
            for i, lin in enumerate(lins):
                N = lin.out_features
                y = x.new_empty((M, N))
                if not use8[i]:
                    k.gemm_segments([(x, lin.w, Kd, Kd, Kd), (h[:, i * r:(i + 1) * r], ucs[i], r, Gr, r)], y, M, N, N,
                                    bias=lin.bias, R=residual, ldr=N, beta=beta)
                else:
                    kt = dict(ktail=(h[:, i * r:(i + 1) * r], ucs[i], r, Gr, r, 0, 0)) if fp8._ktail and ktail_ok else {}
                    w8, sw8 = fp8.fp8_weight(lin)
                    k.gemm(x8, w8, y, M, N, Kd, Kd, Kd, N, bias=lin.bias, R=residual, ldr=N, beta=beta, scales=(sx, sw8), **kt)
                    if not kt:
                        k.gemm(h[:, i * r:(i + 1) * r], ucs[i], y, M, N, r, Gr, r, N, R=y, ldr=N, beta=1.0)
                ys.append(y)
        ctx.save_for_backward(x, h, dct, *uts)
        ctx.grp, ctx.lins = grp, lins
        ctx.has_res = residual is not None
        assert down_cat.grad is not None and all(u.grad is not None for u in ups), \
            "LoRA factors need preallocated .grad views"
        return tuple(ys)

    @staticmethod
    def backward(ctx, *gs):
        x, h, dct, *uts = ctx.saved_tensors
        grp, lins = ctx.grp, ctx.lins
        M, Kd = x.shape
        G, r = grp.size, grp.rank
        Gr = G * r
        k = kernels()
        gs = [_c(g) if g is not None else x.new_zeros((M, lin.out_features)) for g, lin in zip(gs, lins)]
        u = x.new_empty((M, Gr))
        # when the incoming gradients sit at a constant spacing in one buffer (dQ/dK/dV of the fused attention
        # backward) and so do the up factors, the G per-projection GEMMs below are ONE batched launch each
        sg, su = _uniform_stride(gs), _uniform_stride(uts)
        sgu = _uniform_stride([grp.ups[i].grad for i in range(G)])
        batched = sg is not None and su is not None and sgu is not None
        # the input gradient's segments: every projection's frozen part, then the low-rank part that reads u
        segs = [(gs[i], lin.wt, lin.out_features, lin.out_features, lin.out_features) for i, lin in enumerate(lins)]
        segs.append((u, dct, Gr, Gr, Gr))
        dx = x.new_empty((M, Kd)) if ctx.needs_input_grad[0] else None
        _u_product(k, grp, lins, gs, uts, u, sg if batched else None, su)
        want_down, want_ups = ctx.needs_input_grad[4], ctx.needs_input_grad[5:]

        def batched_ups():  # off the grouped kernel, the dU_i of gradients and factors at constant spacings are ONE launch
            N0, gu = lins[0].out_features, grp.ups[0].grad
            k.gemm(gs[0], h, gu, N0, r, M, N0, Gr, r, transA=True, transB=True, R=gu, ldr=r, beta=1.0,
                   batch=(G, 1), sA=(sg, 0), sB=(r, 0), sC=(sgu, 0), sR=(sgu, 0))

        _factor_grads(grp, lins, gs, h, u, x, want_ups, want_down, batched_ups=batched_ups if batched and all(want_ups) else None)
        if dx is not None:
            k.gemm_segments(segs, dx, M, Kd, Kd)
        return (dx, (gs[0] if ctx.has_res else None), None, None, None) + (None,) * G


# COMAT_LORA_TAIL (default 1, round 6): the rank-r products the factor gradients need ride in the launch that shares their A operand
# (comat_gemm_params::epi2 = 4, "tail columns"): h = s x D^T as r extra output columns of the forward projection, u = s g U as r
# extra columns of a single projection's data-gradient.  0 = both as launches of their own in front of the weight-gradient group
# (round 5).  Same operands, fp32 accumulation, same rounding: the results differ at most in summation order.
_lora_tail = os.environ.get("COMAT_LORA_TAIL", "1") != "0"


def set_lora_tail(flag: bool):
    global _lora_tail
    _lora_tail = bool(flag)


def _merged_forward(x, lins, grp, residual, h=None):
    """y_i = x (W_i + s U_i D_i)^T + b_i (+ residual): one plain GEMM per projection or one batched GEMM for a co-allocated
    group; no segments.  h [M, G r] (optional): receives s x [D_1; ..; D_G]^T from the SAME launches (tail columns of the
    products: the down factors' compute copies are the extra rows of B)."""
    x = _c(x)
    M, Kd = x.shape
    wm, _ = grp.store.merged_weights(grp, lins)
    k = kernels()
    G, r = len(lins), grp.rank
    Gr = G * r
    dc, rt = (None, 0) if h is None else (grp.compute_copies()[0], r)  # (the tail's operand, its r extra output columns)
    sm = _uniform_stride(wm)
    if G > 1 and sm is not None and residual is None and all(l.bias is None for l in lins):
        N = lins[0].out_features
        ys = x.new_empty((G, M, N))
        tail = {} if h is None else dict(tail=(dc, h, r, Gr, r * Kd, r, grp.scale))
        k.gemm(x, wm[0], ys, M, N + rt, Kd, Kd, Kd, N, batch=(G, 1), sA=(0, 0), sB=(sm, 0), sC=(M * N, 0), **tail)
        return tuple(ys.unbind(0))
    ys = []
    if residual is not None:
        residual = _c(residual)
    for i, (lin, w) in enumerate(zip(lins, wm)):
        N = lin.out_features
        y = x.new_empty((M, N))
        tail = {} if h is None else dict(tail=(dc[i * r:(i + 1) * r], h[:, i * r:(i + 1) * r], r, Gr, 0, 0, grp.scale))
        k.gemm(x, w, y, M, N + rt, Kd, Kd, Kd, N, bias=lin.bias, R=residual, ldr=N, beta=1.0 if residual is not None else 0.0, **tail)
        ys.append(y)
    return tuple(ys)


# COMAT_TRAIN_MERGED (default 1, round 5): the TRAINED calls use the merged weights too.  0 = the low-rank form of rounds 1-4
# (_LoRAGroupLinear: h = s x D^T on the dependent chain, then a K-segmented product).
_train_merged = os.environ.get("COMAT_TRAIN_MERGED", "1") != "0"


def set_train_merged(flag: bool):
    global _train_merged
    _train_merged = bool(flag)


class _LoRAMergedLinear(Function):
    """(y_1 .. y_G) with y_i = x W_eff,i^T + b_i (+ residual),  W_eff,i = W_i + s U_i D_i  (LoRAStore.merged_weights: both
    orientations refreshed once per optimizer step) - the same function as _LoRAGroupLinear
    (training_utils/pipeline.py:94-115), arranged so that nothing of the low-rank branch sits on the dependent chain:
      forward   ONE plain (batched) GEMM;
      backward  dx = sum_i g_i W_eff,i on the issuing stream (one K-segmented GEMM over the g_i, no u segment);
                the factor gradients dU_i += g_i^T (s x D_i^T), d[D_1; ..] += (s g_i U_i)^T x need the two M x G r products
                h and u - nobody else reads them, so they are launched with their weight-gradient group on the side stream."""

    @staticmethod
    def forward(ctx, x, residual, grp, lins, down_cat, *ups):
        x = _c(x)
        # the up factors' gradients dU_i += g_i^T h_i need h = s x D^T: r extra columns of this launch (round 6) instead of a
        # launch of its own in the backward pass
        h = x.new_empty((x.shape[0], grp.size * grp.rank)) if _lora_tail and any(u.requires_grad for u in ups) else None
        ys = _merged_forward(x, lins, grp, residual, h)
        if h is None:
            ctx.save_for_backward(x)
        else:
            ctx.save_for_backward(x, h)
        ctx.grp, ctx.lins = grp, lins
        ctx.epoch = getattr(grp.store, "epoch", 0)  # the merged weights this forward multiplied by
        ctx.has_res = residual is not None
        assert down_cat.grad is not None and all(u.grad is not None for u in ups), \
            "LoRA factors need preallocated .grad views"
        return ys

    @staticmethod
    def backward(ctx, *gs):
        x, *rest = ctx.saved_tensors
        h = rest[0] if rest else None
        grp, lins = ctx.grp, ctx.lins
        M, Kd = x.shape
        G, r = grp.size, grp.rank
        Gr = G * r
        k = kernels()
        gs = [_c(g) if g is not None else x.new_zeros((M, lin.out_features)) for g, lin in zip(gs, lins)]
        want_down, want_ups = ctx.needs_input_grad[4], ctx.needs_input_grad[5:]
        dx = u = None
        u_done = False
        if ctx.needs_input_grad[0]:
            _, wmt = grp.store.merged_weights(grp, lins)
            # (merged_weights refreshes lazily: an optimizer step of this store between a forward and its backward would hand
            # the backward other weights than the forward used)
            assert getattr(grp.store, "epoch", 0) == ctx.epoch, \
                "LoRA factors were updated between a trained call's forward and its backward"
            dx = x.new_empty((M, Kd))
            if G == 1:
                N = lins[0].out_features
                if want_down and _lora_tail:  # u = s g U rides along: U^T [r, N] is the tail of W_eff^T [K, N]
                    u, u_done = x.new_empty((M, r)), True
                    k.gemm(gs[0], wmt[0], dx, M, Kd + r, N, N, N, Kd, tail=(grp.compute_copies()[3][0], u, r, r, 0, 0, grp.scale))
                else:
                    k.gemm(gs[0], wmt[0], dx, M, Kd, N, N, N, Kd)
            else:
                k.gemm_segments([(gs[i], wmt[i], lin.out_features, lin.out_features, lin.out_features)
                                 for i, lin in enumerate(lins)], dx, M, Kd, Kd)
        if want_down or any(want_ups):
            dc, _, _, uts = grp.compute_copies()
            h_done = h is not None
            if h is None and any(want_ups):
                h = x.new_empty((M, Gr))
            if u is None and want_down:
                u = x.new_empty((M, Gr))
            sg, su = _uniform_stride(gs), _uniform_stride(uts)

            def low_rank():  # whatever did not ride in a neighbour's launch: h = s x [D_1; ..]^T, u_i = s g_i U_i
                if h is not None and not h_done:
                    k.gemm(x, dc, h, M, Gr, Kd, Kd, Kd, Gr, alpha=grp.scale)
                if u is not None and not u_done:
                    _u_product(k, grp, lins, gs, uts, u, sg, su)

            pre = low_rank if (not h_done and any(want_ups)) or (want_down and not u_done) else None
            _factor_grads(grp, lins, gs, h, u, x, want_ups, want_down, pre=pre)
        return (dx, (gs[0] if ctx.has_res else None), None, None, None) + (None,) * G


def lora_group_linear(x, lins, grp: LoRAGroup | None, residual=None):
    """(x W_i^T + b_i + lora_i(x)) for the projections `lins` that share the input x; a tuple of len(lins).
    Merged weights W + s U D (refreshed once per optimizer step) serve the no-grad calls (COMAT_NOGRAD_MERGED, default 1 since
    round 4) and the trained calls (COMAT_TRAIN_MERGED, default 1 since round 5: _LoRAMergedLinear); 0 selects the low-rank
    products of rounds 1-3 (_LoRAGroupLinear)."""
    if grp is None:
        from .ops import linear  # (ops imports this module)
        assert residual is None or len(lins) == 1
        return tuple(linear(x, lin, residual) for lin in lins)
    # Measured at full SD1.5 size (profiles/r04_f_nograd_merged.txt): against the fp32 forward the merged call is as accurate as
    # the unmerged one at every LoRA magnitude (1.32e-2 vs 1.34e-2 of the output; the share of the LoRA's own effect that is
    # lost: 3.6e-2 vs 3.7e-2 at |U| = 0.02, 0.297 vs 0.296 at a tenth of that - bf16 rounding of the ACTIVATIONS dominates both),
    # and a no-grad UNet forward takes 6.74 instead of 7.32 ms.
    # (not under fp8_forward: there the frozen part runs on e4m3 weights quantised once - a merged weight would have to be
    # re-quantised after every optimizer step.  comat_weights_refresh_q8 does exactly that for fully trained weights -
    # unet.UNetBank(fp8=True) - and could serve merged weights the same way; that is not built)
    lins, train = tuple(lins), torch.is_grad_enabled()
    if not fp8._on and not train and os.environ.get("COMAT_NOGRAD_MERGED", "1") != "0":
        return _merged_forward(x, lins, grp, residual)
    merged = not fp8._on and train and _train_merged
    return (_LoRAMergedLinear if merged else _LoRAGroupLinear).apply(x, residual, grp, lins, grp.down_cat, *grp.ups)


def lora_linear(x, lin, grp: LoRAGroup | None, residual=None):
    return lora_group_linear(x, (lin,), grp, residual)[0]
