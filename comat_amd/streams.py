"""Streams of the host code: the side streams that take work off the critical path of a backward pass, the one stream
hipGraphs are captured on, the fixed-address copy of a batch that captured graphs read (StaticBatch), and the deferred,
grouped LoRA weight gradients that run on the side streams.  The flags a setter rebinds
(`_side_enabled`, `_side_suspended`, `_tt_grouping`) are read through this module, never imported by value."""
import gc
import os

import torch

from .backend import kernels

# ---- side stream for work that is off the critical path of backward (LoRA weight gradients) -----------------------
_side = {}
_side_keep = []
_side_enabled = True
_side_suspended = 0  # >0: weight gradients stay on the issuing stream (see no_side_streams)
_side_dirty = []  # side streams that received work since the last join
_join_queued = False  # the end-of-backward join (join_side_streams) is queued


def set_side_stream_enabled(flag: bool):
    global _side_enabled
    _side_enabled = bool(flag)


def side_streams_enabled():
    return _side_enabled


def _side_stream(dev):
    """A second HIP stream (None on CPU / when disabled), one per stream that issues backward work: the K = B*H*W
    split-K GEMMs of the LoRA weight gradients have few tiles each and no consumer until the optimizer, so they
    overlap the main backward chain."""
    if dev.type != "cuda" or not _side_enabled or _side_suspended:
        return None
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    st = _side.get(key)
    if st is None:
        st = _side[key] = torch.cuda.Stream(device=dev)
    return st


def run_off_chain(dev, fn, keep, queue=None):
    """Run `fn` (launches whose results nothing on the dependent chain reads) on the side stream of the current stream if
    there is one, else here; `keep` (the tensors that own its operands) stays alive until join_side_streams(), which is queued.
    `queue` (a _TTQueue flushing a group) brings its own streams - the side stream decided when the group's first problem was
    queued, and the issuing stream, which takes the launches when there is no side stream - and has queued the join already."""
    side, issuing = (_side_stream(dev), None) if queue is None else (queue.side, queue.issuing)
    if side is None:
        if issuing is None:
            fn()
        else:
            with torch.cuda.stream(issuing):
                fn()
        return
    # every operand has been produced on the issuing stream
    side.wait_stream(issuing if issuing is not None else torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fn()
    if not any(st is side for _, st in _side_dirty):
        _side_dirty.append((dev, side))
    _side_keep.append(keep)  # operands stay alive until join_side_streams()
    if queue is None:
        _queue_join()


# ---- the stream hipGraphs of this package are captured on ---------------------------------------------------------------
_capture = {}


def capture_stream(dev):
    """ONE capture stream per device for every hipGraph the package records for replay on the main stream (step graph,
    step segments, no-grad UNet forwards).  Kernels pick their workspaces by stream, so these graphs share one set of
    workspaces - legal because they are only ever replayed on one stream, one after the other - and that set is created
    and zeroed HERE, eagerly, together with the set of the stream's side stream: a workspace first touched inside a
    capture would be zeroed by a node of that one graph only (see _hip.HipKernels._no_capture)."""
    dev = torch.device(dev)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    st = _capture.get(dev)
    if st is None:
        st = _capture[dev] = torch.cuda.Stream(device=dev)
    prepare_capture_stream(dev, st)  # idempotent per kernel backend instance (tests install a fresh one per test)
    return st


class graph_capture:
    """`torch.cuda.graph(g, pool=..., stream=...)` with Python's cyclic garbage collector switched off for the duration of
    the capture.  torch collects garbage BEFORE the capture begins; a collection that the allocation counters trigger in the
    MIDDLE of it runs finalizers of whatever became unreachable - an old CUDAGraph, a stream, pool memory of a finished
    test or stepper - and those release HIP objects while a stream is capturing: the capture is invalidated at best (the
    replay then faults), the process aborts at worst (both seen on MI355X, round 3).  Captures are short; the collector
    is switched back on (to its previous state) at the end."""

    def __init__(self, graph, pool=None, stream=None, **kw):
        self._ctx = torch.cuda.graph(graph, pool=pool, stream=stream, **kw)

    def __enter__(self):
        self._gc_was_on = gc.isenabled()
        r = self._ctx.__enter__()  # synchronises, collects garbage, empties the cache, begins the capture
        gc.disable()
        return r

    def __exit__(self, *exc):
        try:
            return self._ctx.__exit__(*exc)
        finally:
            if self._gc_was_on:
                gc.enable()


def capture_kwargs(thread_local=None):
    """keyword arguments of graph_capture.  More than one rank: RCCL's watchdog thread polls events while we capture - only
    THIS thread's calls may invalidate the capture ("thread_local"; the default "global" mode would abort it).
    thread_local=None decides from torch.distributed being initialised."""
    if thread_local is None:
        import torch.distributed as dist
        thread_local = dist.is_available() and dist.is_initialized()
    return {"capture_error_mode": "thread_local"} if thread_local else {}


class StaticBatch:
    """The tensors of a batch at fixed device addresses, for the graphs that read them.  ONE list of keys for every stepper
    (step.GraphedStep, segments.SegmentedStep): a tensor missing here would be read at the address it had at capture time."""

    KEYS = ("prompt_embeds", "negative_prompt_embeds", "gan_null_embeds", "latents", "real_latents",
            "pooled_prompt_embeds", "negative_pooled_prompt_embeds", "gan_pooled_null_embeds",
            "blip_input_ids", "blip_attention_mask")

    def __init__(self, device):
        self.device = device
        self.buffers = {}  # key -> list of buffers (one per entry of `noises`, one for a tensor)
        self.staged_keys = None

    def stage(self, batch, strict):
        """-> (staged, reallocated).  `staged` is a fresh dict(batch) in which every tensor under KEYS and every entry of
        `noises` is a fixed-address buffer holding a copy (same shape and dtype, on the device); everything else - host-side
        metadata: masks, token lists, time ids - passes through by reference.  Buffers are re-created per key when shape,
        dtype or (noises) their number change; `reallocated`: this call created a buffer or staged another set of keys than
        the previous one (graphs that baked the old addresses in are stale).  strict: a tensor under any other key raises."""
        if strict:
            for k, v in batch.items():
                if torch.is_tensor(v) and k not in self.KEYS:
                    raise KeyError(f"batch tensor '{k}' has no fixed-address staging buffer (StaticBatch.KEYS): a captured "
                                   "graph would keep reading the address it saw at capture time")
        staged = dict(batch)
        keys = tuple(k for k in self.KEYS + ("noises",) if batch.get(k) is not None)
        reallocated, self.staged_keys = keys != self.staged_keys, keys
        for k in keys:
            srcs = batch[k] if k == "noises" else [batch[k]]
            dsts = self.buffers.get(k)
            if dsts is None or [(d.shape, d.dtype) for d in dsts] != [(s.shape, s.dtype) for s in srcs]:
                dsts = self.buffers[k] = [torch.empty_like(s, device=self.device) for s in srcs]
                reallocated = True
            for d, s in zip(dsts, srcs):
                d.copy_(s, non_blocking=True)
            staged[k] = dsts if k == "noises" else dsts[0]
        return staged, reallocated


def reset_capture_stream(dev):
    """after a FAILED capture: the capture stream (and streams forked from it) may be left in capture mode by the runtime -
    forget it, the next capture_stream() call makes a fresh one"""
    dev = torch.device(dev)
    if dev.type != "cuda":
        return  # (the CPU simulator has no streams)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    st = _capture.pop(dev, None)
    if st is not None:
        _side.pop((dev, st.cuda_stream), None)


def prepare_capture_stream(dev, st):
    """create the per-stream workspaces of `st` and of the side stream forked from it, outside any capture (idempotent)"""
    k = kernels()
    if not hasattr(k, "prepare_stream"):
        return
    global _side_suspended
    made = False
    with torch.cuda.stream(st):
        made |= bool(k.prepare_stream(dev))
        saved, _side_suspended = _side_suspended, 0
        try:
            side = _side_stream(torch.device(dev))
        finally:
            _side_suspended = saved
        if side is not None:
            with torch.cuda.stream(side):
                made |= bool(k.prepare_stream(dev))
    if made:
        torch.cuda.synchronize(dev)


class no_side_streams:
    """Context: LoRA weight gradients of backward passes started inside it run on their issuing stream.  Used for the
    D step when it is itself forked onto its own stream inside a hipGraph capture: a fork from a forked stream (nested)
    crashes hipStreamEndCapture on ROCm 7.2, a single level of forks captures fine."""

    def __enter__(self):
        global _side_suspended
        _side_suspended += 1

    def __exit__(self, *exc):
        global _side_suspended
        _side_suspended -= 1


def join_side_streams():
    """Make the current stream wait for everything queued on the side streams since the last join.  Queued
    automatically as an autograd end-of-backward callback, so LoRA gradients are complete (in stream order) when
    `.backward()` returns.  Only streams that were actually forked are waited for: inside a hipGraph capture a wait on
    a stream that is not part of the capture would be an illegal cross-capture dependency."""
    global _join_queued
    _join_queued = False
    flush_weight_grads()
    for dev, st in _side_dirty:
        torch.cuda.current_stream(dev).wait_stream(st)
    _side_dirty.clear()
    _side_keep.clear()


def release_side_operands():
    """In the middle of a backward pass (recompute._Recompute: a checkpointed call's backward has ended): the current stream
    waits for the weight-gradient groups launched so far and their operands are released - they belong to a recording that
    is gone, and kept until the end of the backward they would add up over the K calls.  Nothing is flushed: a group that
    is still filling stays queued with its operands, so the grouping is that of a backward without this call."""
    for dev, st in _side_dirty:
        torch.cuda.current_stream(dev).wait_stream(st)
    _side_dirty.clear()
    _side_keep.clear()


def _queue_join():
    global _join_queued
    if not _join_queued:
        _join_queued = True
        torch.autograd.Variable._execution_engine.queue_callback(join_side_streams)


def reset_side_stream_state():
    """Start of a top-level forward/backward: join what a previous backward may have left behind (an exception in the
    middle of a backward skips its end-of-backward callback; the latch would stay set and no later backward would ever
    join the side streams again) and drop the latch."""
    global _join_queued
    if _side_dirty or any(q.items for q in _ttq.values()):
        join_side_streams()
    _join_queued = False
    _side_keep.clear()


def drop_side_stream_state():
    """After a FAILED graph capture: forget the weight gradients the aborted pass queued and the side streams it marked
    (their operands belong to the dead capture - they must not be launched), without joining anything."""
    global _join_queued
    _ttq.clear()
    _side_dirty.clear()
    _side_keep.clear()
    _join_queued = False


# ---- deferred, grouped LoRA weight gradients -----------------------------------------------------------------------
# dU = g^T h and dD = u^T x of every LoRA projection are k-major products over the token axis with a handful of output
# tiles each (~720 per SD1.5 step).  Nothing reads them before the optimizer, so a backward pass QUEUES them here and
# hands them to comat_gemm_tt_grouped in groups of <= TT_GROUP problems: one launch fills the chip where 48 small ones
# each paid their own split-K combine.  A group is flushed when it is full, when a new problem
# accumulates into an output the group already holds (the same factor at another denoise step: the two must stay in
# stream order), and at the end of the backward pass (join_side_streams).  Grouping is a pure function of the call
# sequence, so results stay bit-reproducible run to run, eager or replayed from a graph.
TT_GROUP = 48
_ttq = {}  # (device, issuing stream) -> _TTQueue
_tt_grouping = os.environ.get("COMAT_TT_GROUPED", "1") != "0"


def set_tt_grouping(flag: bool):
    """tests / A-B runs: False issues every weight gradient as its own comat_gemm launch (the round-2 path)"""
    global _tt_grouping
    flush_weight_grads()
    _tt_grouping = bool(flag)


class _TTQueue:
    def __init__(self, dev, issuing, side):
        self.dev, self.issuing, self.side = dev, issuing, side
        self.items, self.outs, self.keep, self.pre = [], set(), [], []

    def add(self, prob, keep, pre=None):
        # the byte range the problem accumulates into: [C, C + ((M - 1) ldc + N) * 4).  A problem whose output OVERLAPS one
        # the group already holds (the same factor at another denoise step, or any partially overlapping view) must not
        # share its launch: the two read-modify-write passes would race
        lo = prob[2].data_ptr()
        hi = lo + ((prob[3] - 1) * prob[8] + prob[4]) * 4
        if len(self.items) >= TT_GROUP or any(lo < h and l < hi for l, h in self.outs):
            self.flush()
        self.items.append(prob)
        self.outs.add((lo, hi))
        self.keep.append(keep)
        if pre is not None:
            self.pre.append(pre)

    def flush(self):
        if not self.items:
            return
        items, keep, pre = self.items, self.keep, self.pre
        self.items, self.outs, self.keep, self.pre = [], set(), [], []

        def launch():
            for fn in pre:  # operands the problems read that nothing on the issuing stream needs (merged LoRA: h, u)
                fn()
            kernels().gemm_tt_grouped(items)

        run_off_chain(self.dev, launch, keep, queue=self)


def _tt_enqueue(dev, problems, keep, pre=None):
    """queue weight-gradient problems [(A, B, C, M, N, K, lda, ldb, ldc)] of the backward pass running on the current
    stream; `keep` = tensors that own the operands; `pre` = a callable that produces operands only these problems read
    (launched right in front of their group, on the stream the group runs on)"""
    cur = torch.cuda.current_stream(dev) if dev.type == "cuda" else None  # (CPU tensors, tests with the ABI simulator: no streams)
    key = (dev, 0 if cur is None else cur.cuda_stream)
    q = _ttq.get(key)
    if q is None:
        q = _ttq[key] = _TTQueue(dev, cur, None)
    if not q.items:
        q.side = _side_stream(dev)  # decided per group: side streams may be suspended for a forked D step
    for j, pr in enumerate(problems):
        q.add(pr, keep, pre if j == 0 else None)
    _queue_join()


def flush_weight_grads():
    """launch every queued weight-gradient group (idempotent)"""
    for q in list(_ttq.values()):
        q.flush()
