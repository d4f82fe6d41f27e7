"""MasterBank: the parameters of a model that is trained in full, in ONE flat fp32 master and ONE flat gradient.

What `--tune_vae` (unet.VAEBank), `--full_finetuning` (unet.UNetBank) and `--tune_text_encoder` (clip.ClipTextBank) have in common;
each of them states only what it adds.
  * every entry starts on a 32-byte boundary of `flat` / `flat_grad` (pad elements are zero and stay zero under AdamW) and is KEPT in
    the layout the kernels read (conv weights [Cout, KH, KW, Cin]), so that gradients accumulate in place and AdamW stays
    elementwise; `_stored` / `_source` translate to and from the layout of the state-dict file.  `params[name]` is a leaf view
    whose .grad is a view of the flat gradient;
  * a MATRIX (Linear / conv weight) has a compute-dtype forward copy in `flat_c` (in fp32 the master is the copy) and a second
    orientation in `flat_t` (wt of a Linear, wd of a conv), both rewritten from the master by ONE comat_weights_refresh launch
    (refresh.RefreshPlan) in ensure_compute_copy() after an update.  `flat_t` holds the matrices only; `flat_c` is either full-size
    at the master's offsets or, `compact`, shares flat_t's.  Biases, norm parameters and whatever else is no matrix are read from
    the master;
  * a layer is built ONCE per name: a second request (a second model over the same bank) gets the same holder, a request of
    another kind is refused;
  * `gate`: a one-element tensor that requires grad while the bank is trained - the extra autograd input of every trained node
    (ops.gate_of), so that layers whose data input carries no gradient still run in the backward pass.  None for a bank whose
    every layer has a differentiable input;
  * `epoch` counts refreshes: consumers that memoise products of the weights compare it;
  * zero_grad / set_requires_grad / mark_updated / ensure_compute_copy: what the training step asks of a bank (LoRAStore's protocol).
"""
from __future__ import annotations

import torch

from . import ops, refresh


def _numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


class MasterBank:
    MODEL = "model"      # names the model in refusals
    ENTRIES = "entries"
    weight_file = None   # the checkpoint file that holds state_dict() (checkpoint.py)

    def __init__(self, shapes, matrices, dtype, device, compact=False, gate=True):
        """shapes: name -> (stored shape, source shape), in the master's order; matrices: the names that have a forward copy and a
        second orientation, in flat_t's order"""
        self.dtype, self.device, self.compact = dtype, device, compact
        self.names = list(shapes)
        self.layout, self._toff, off, toff = {}, {}, 0, 0
        for n, (stored, source) in shapes.items():
            self.layout[n] = (off, tuple(stored), tuple(source))
            off += -(-_numel(stored) // 8) * 8
        for n in matrices:
            self._toff[n] = toff
            toff += -(-_numel(self.layout[n][1]) // 8) * 8
        self.flat = torch.zeros(off, dtype=torch.float32, device=device)
        self.flat_grad = torch.zeros(off, dtype=torch.float32, device=device)
        self.flat_c = None if dtype == torch.float32 else torch.zeros(toff if compact else off, dtype=dtype, device=device)
        self.flat_t = torch.zeros(toff, dtype=dtype, device=device)
        self.gate = torch.zeros(1, dtype=torch.float32, device=device, requires_grad=True) if gate else None
        self.params, self.holders, self._affine, self._made = {}, [], [], {}
        for n in self.names:
            p = self._view(self.flat, n).requires_grad_(True)
            p.grad = self._view(self.flat_grad, n)
            self.params[n] = p
        self._problems, self._owner, self._plan = [], [], None  # _owner: per problem row, the layer it belongs to
        self._fresh, self.epoch, self.training = False, 0, True

    def _view(self, buf, name):
        o, stored, _ = self.layout[name]
        return buf[o:o + _numel(stored)].view(stored)

    # ---- state dicts: two hooks - which key of a file holds a name, and the file's layout of a tensor ---------------------------
    def _keys_of(self, sd):
        """name -> the key of `sd` that holds it, for every name that `sd` has"""
        return {n: n for n in self.names if n in sd}

    def _stored(self, name, t):
        """a tensor of the file in the bank's layout (OIHW -> kernel layout)"""
        return t.permute(0, 2, 3, 1) if t.dim() == 4 else t

    def _source(self, name, t):
        """the inverse of _stored"""
        return t.permute(0, 3, 1, 2) if t.dim() == 4 else t

    def _lacks(self, missing):
        return f"{self.MODEL} state dict lacks {len(missing)} {self.ENTRIES}: {missing[:3]}..."

    def load_state_dict(self, sd):
        """copies every entry of the bank from a state dict in the file's names and layout into the existing buffers; a missing
        key (KeyError) or another shape (ValueError) is refused by name, before anything is copied"""
        found = self._keys_of(sd)
        missing = [n for n in self.names if n not in found]
        if missing:
            raise KeyError(self._lacks(missing))
        for n in self.names:
            got = tuple(sd[found[n]].shape)
            if got != self.layout[n][2]:
                raise ValueError(f"{self.MODEL} state dict: {found[n]} has shape {got}, the bank holds {self.layout[n][2]}")
        with torch.no_grad():
            for n in self.names:
                self._view(self.flat, n).copy_(self._stored(n, sd[found[n]].detach().float()).to(self.device))
        self.mark_updated()

    def state_dict(self):
        """every entry of the bank in the file's layout (fp32, CPU), under its name"""
        return {n: self._source(n, self._view(self.flat, n).detach().to("cpu", torch.float32)).contiguous() for n in self.names}

    # ---- what a model's layers are built from ---------------------------------------------------------------------------------
    def _once(self, name, kind, make):
        """the holder of layer `name`, made at its first request (with its refresh problems) and handed out again afterwards"""
        ent = self._made.get(name)
        if ent is not None:
            if ent[0] != kind:
                raise ValueError(f"{type(self).__name__}: {name} was built as {ent[0]}, now asked for as {kind}")
            return ent[1]
        h, problems = make()
        if problems is not None:  # a weight holder (a norm's pair of tensors has no fields of its own)
            if self.gate is not None:
                h.gate = self.gate
            h.requires_grad = self.training
            self.holders.append(h)
            self._problems += problems
            self._owner += [name] * len(problems)
            self._plan = None
            self._fresh = False  # the new holder's copies have not been written yet
        self._made[name] = (kind, h)
        return h

    def _parts(self, name):
        """(w, w_grad, bias, bias_grad, (master offset, w offset, wt offset)) of layer `name`"""
        wn, bn = name + ".weight", name + ".bias"
        (o, stored, _), ot = self.layout[wn], self._toff[wn]
        ow = o if self.flat_c is None or not self.compact else ot  # fp32: the master is the forward copy, the launch leaves it alone
        w = (self.flat if self.flat_c is None else self.flat_c)[ow:ow + _numel(stored)].view(stored)
        b = bn in self.layout
        return (w, self._view(self.flat_grad, wn), self._view(self.flat, bn) if b else None,
                self._view(self.flat_grad, bn) if b else None, (o, ow, ot))

    def linear(self, name, cls=ops.TrainableLinear):
        """a Linear or 1x1 conv (the same [N, K] matrix in the kernel layout)"""
        def make():
            w, wg, b, bg, (o, ow, ot) = self._parts(name)
            N, K = w.shape[0], w.numel() // w.shape[0]
            return (cls(w.reshape(N, K), wg.reshape(N, K), b, bg, wt=self.flat_t[ot:ot + N * K].view(K, N)),
                    refresh.linear_problem(o, ow, ot, N, K))
        return self._once(name, ("linear", cls.__name__), make)

    def conv(self, name, stride=1, pad=1):
        def make():
            w, wg, b, bg, (o, ow, ot) = self._parts(name)
            Cout, KH, KW, Cin = w.shape
            return (ops.TrainableConv(w, wg, b, bg, stride=stride, pad=pad, wd=self.flat_t[ot:ot + w.numel()].view(Cin, KH, KW, Cout)),
                    refresh.conv_problems(o, ow, ot, Cout, KH, KW, Cin))
        return self._once(name, ("conv", stride, pad), make)

    def norm(self, name):
        """(weight, bias) of a norm: views of the master that carry their gradient views (`comat_grad`, `comat_train`)"""
        def make():
            out = []
            for leaf in (".weight", ".bias"):
                t = self._view(self.flat, name + leaf)
                t.comat_grad, t.comat_train = self._view(self.flat_grad, name + leaf), self.training
                self._affine.append(t)
                out.append(t)
            return tuple(out), None
        return self._once(name, "norm", make)

    # ---- the protocol of the training step ----------------------------------------------------------------------------------------
    def _plan_slots(self):
        """per refresh problem the slot of a quantised weight (the _q8 launch), or None: the plain launch"""
        return None

    def _plan_extra(self):
        """the buffers the _q8 launch takes beyond the three flat ones"""
        return ()

    def ensure_compute_copy(self):
        if not self._fresh:
            if self._problems:
                if self._plan is None:  # built once the holders exist; the launch only reads it
                    self._plan = refresh.RefreshPlan(self._problems, self.device, slots=self._plan_slots())
                self._plan.run(self.flat, self.flat_c, self.flat_t, *self._plan_extra())
            self._fresh = True
            self.epoch += 1

    def mark_updated(self):
        """call after an in-place update of `flat` (optimizer kernel, load): the derived copies are refreshed lazily"""
        self._fresh = False

    def zero_grad(self):
        self.flat_grad.zero_()

    def set_requires_grad(self, flag: bool):
        self.training = bool(flag)
        if self.gate is not None:
            self.gate.requires_grad_(self.training)
        for h in self.holders:
            h.requires_grad = self.training
        for t in self._affine:
            t.comat_train = self.training
