"""Gradient checkpointing of the TRAINED UNet calls (`--gradient_checkpointing`, scripts/sd15.sh:7, scripts/sdxl.sh:7;
applied in training_utils/pipeline.py:73-74) - per call, not per block as diffusers does.

Without it the K trained calls of a step keep their activations until the backward pass: K x one call's activations, which
grow with the batch.  With it, what lives between a call and its backward is
  * the call's inputs: model input, timestep (or its sinusoid), text context, SDXL added embedding, and
  * the call's outputs: eps and, on capturing steps, the cross-attention maps the loss reads;
the backward of the call first runs the forward again with autograd recording and then differentiates THAT recording with
the incoming gradients (of eps, and of the maps on capturing steps).  The LoRA weight gradients land in `bank.flat_grad` as
a side effect of that nested backward, exactly as they do in the plain one.  The K calls then need the activations of one.

The value pass (whose eps feeds the sampler) is the recorded forward itself, run on detached inputs, with the outputs
detached and the recording dropped at once: it launches the kernels the recomputation will launch, so both passes give the
same bits (a `torch.no_grad()` pass may select other kernels: merged LoRA forms, fp8 producers, attention variants).
fp8 forward: the scale words change only in fp8_end_of_step (delayed) or are a function of the input bits (just in time),
so both passes quantise identically; a site's running abs-max is a maximum (idempotent) and the clip accounting is derived
from it at the end of the step; producer-emitted bytes are stamped and consumed inside one pass.

Text keys / values: every checkpointed call projects its own (`kv_cache=None`), as the replayed segments do - a cache that
held an autograd graph across calls would keep what this module exists to free.  The untrained calls keep their sharing.

Not checkpointed: the discriminator.  The reference's flag reaches the discriminator's UNet through the deep-copied
arguments, but here each discriminator forward (generator side and D side) is followed at once by its backward, so
call-level recomputation cannot lower its peak.  The same holds for the VAE + BLIP head.
"""
from __future__ import annotations

import torch
from torch.autograd import Function

from . import streams

_anchors = {}


def anchor(device):
    """The dummy leaf that makes a checkpointed call's outputs require grad when no INPUT does (the first trained denoise
    step; every SDXL step): the LoRA factors are not inputs of the node - their gradients are a side effect of its backward
    (see segments.GraphedSegment).  One per device, never written."""
    device = torch.device(device)
    a = _anchors.get(device)
    if a is None:
        a = _anchors[device] = torch.zeros((), device=device, requires_grad=True)
    return a


def _leaves(inputs, needs):
    return [x.detach().requires_grad_(bool(n)) for x, n in zip(inputs, needs)]


class _Recompute(Function):
    """fn(*tensors) -> tuple of tensors, with nothing of fn's recording kept between forward and backward"""

    @staticmethod
    def forward(ctx, fn, anchor_, *inputs):
        needs = [x.requires_grad for x in inputs]
        with torch.enable_grad():  # the recorded forward: the kernels the recomputation launches, hence the same bits
            outs = fn(*_leaves(inputs, needs))
        outs = tuple(outs) if isinstance(outs, (tuple, list)) else (outs,)
        ctx.fn, ctx.needs = fn, needs
        ctx.save_for_backward(*inputs)
        res = tuple(o.detach() for o in outs)
        ctx.mark_non_differentiable(*[r for r, o in zip(res, outs) if not o.requires_grad])
        ctx.set_materialize_grads(False)
        return res  # `outs` dies here, and the recording with it

    @staticmethod
    def backward(ctx, *gos):
        leaves = _leaves(ctx.saved_tensors, ctx.needs)
        # The nested backward below queues LoRA weight-gradient groups and would queue its OWN end-of-backward join: the
        # groups would then be cut at every call, where the plain backward cuts them by size and by output overlap only
        # (the split-K of a group is bit-reproducible for a given grouping).  Queued here, on the outer backward, the
        # join runs once, when the outer `.backward()` ends, and the latch is dropped there as after any backward.
        streams._queue_join()
        with torch.enable_grad():
            outs = ctx.fn(*leaves)
        outs = tuple(outs) if isinstance(outs, (tuple, list)) else (outs,)
        pairs = [(o, g) for o, g in zip(outs, gos) if g is not None and o.requires_grad]
        del outs
        torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
        del pairs
        # this call's recording is gone; what the side streams still read of it is released too (the groups already
        # launched: the main stream waits for them; a group still filling keeps its few operands until it is launched)
        streams.release_side_operands()
        return (None, None) + tuple(x.grad for x in leaves)


def checkpoint(fn, *inputs):
    """fn(*inputs) -> tuple of tensors, checkpointed: same values, same gradients, fn's activations live only while it runs
    (here, and once more inside the backward pass)"""
    return _Recompute.apply(fn, anchor(inputs[0].device), *inputs)


def unet_call(unet, x, B, H, W, t, ctx, L, capture_places=(), added=None):
    """`unet(x, B, H, W, t, ctx, L, capture_places=..., added=...)` -> (eps, maps) as one checkpointed call.  `t`: a host
    timestep (its embedding is memoised by the UNet) or its sinusoid as a device tensor."""
    cap = tuple(capture_places)
    counts = []
    tensor_t = torch.is_tensor(t)

    def fn(x_, ctx_, *rest):
        rest = list(rest)
        t_ = rest.pop(0) if tensor_t else t
        eps, maps = unet(x_, B, H, W, t_, ctx_, L, capture_places=cap, added=rest[0] if rest else None, kv_cache=None)
        counts[:] = [len(maps[p]) for p in cap]
        return (eps,) + tuple(m for p in cap for m in maps[p])

    outs = checkpoint(fn, x, ctx, *((t,) if tensor_t else ()), *((added,) if added is not None else ()))
    maps, i = {}, 1
    for p, n in zip(cap, counts):
        maps[p] = list(outs[i:i + n])
        i += n
    return outs[0], maps
