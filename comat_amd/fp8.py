"""Host state of the fp8 forward (BASELINE.json configs[4]: "fp8 MFMA UNet forward with bf16 backward").

Inside `with fp8_forward(True)` the FORWARD product of every frozen Linear / conv that was tagged `allow_fp8` (the
generator UNet's block layers, comat_amd/unet.py) and whose contraction length per tap is a multiple of 64 runs on
the fp8 (OCP e4m3) MFMA: the activation is quantised per tensor on the fly (abs-max scale), the frozen weight once.
The LoRA branch, the attention products, norms and every BACKWARD product stay in the storage dtype and use the
unquantised saved activations and weights: gradients are those of the bf16 network evaluated at the fp8 forward's
activations (the usual straight-through treatment of the quantiser).

The attribute protocol.  This module keeps per-layer and per-tensor facts as Python attributes on objects it does not own:
  on a holder (FrozenLinear / FrozenGegluLinear / FrozenConv)
    allow_fp8    set by the model builder (unet.py), read by fp8_eligible: the layer may run on the fp8 MFMA
    _fp8_name    set by the model builder, read by fp8_report: the name a clip report gives the layer's site
    _fp8_site, _fp8_index   (scale [1], amax [1]) views into the device's site table and (table, row): set by fp8_site() at the
                 holder's first use, read by fp8_act, fp8_producer_site and the tests; STALE after fp8_reset() - the holder keeps
                 pointing at the table that was dropped (tests build new holders)
    _w8          (e4m3 bytes, scale [1]) of the weight in its forward orientation: set by fp8_weight / fp8_weight_group, read
                 by the wrappers in ops and lora; never refreshed (the weight is frozen): stale if somebody rewrites holder.w.
                 On a TRAINED holder (ops.Trainable*, `--full_finetuning`) it is set by the holder's bank (unet.UNetBank.fp8_own) to
                 views of the bank's fixed byte buffer and scale vector, which the refresh launch after every optimizer update
                 rewrites from the master (comat_weights_refresh_q8): owned and refreshed by the bank, never set by fp8_weight
    _w8_group    (bytes [G, N, K], scales [G]) on the FIRST holder of a co-allocated group: set and read by fp8_weight_group
  on a tensor (the output of a norm, of the fused attention)
    _fp8         (bytes, scale view of the site, epoch, tensor version): set by fp8_stamp when the producing kernel emitted the
                 bytes its consumer will multiply, read by fp8_act, which uses them only if the site is the consumer's, no
                 fp8_end_of_step() came in between (the scale would be another) and the tensor was not written since.  The
                 attribute lives on the Python object: a view or a copy of the tensor does not carry it.
Flags that a setter or a context rebinds (`_on`, `_scaling`, `_calibrating`, `_trusting`, `_recipe`, `_epoch`) are read through
this module (`fp8._on`), never imported by value."""
import contextlib
import os
import warnings
import weakref

import torch

from .backend import _uniform_stride, kernels

_on = False


@contextlib.contextmanager
def fp8_forward(flag=True):
    global _on
    prev, _on = _on, bool(flag)
    try:
        yield
    finally:
        _on = prev


def fp8_eligible(holder, k_inner):
    return bool(getattr(holder, "allow_fp8", False)) and k_inner % 64 == 0


def use_fp8(holder, k_inner):
    return _on and fp8_eligible(holder, k_inner)


def fp8_weight(holder):
    """(e4m3 bytes, scale) of a weight in its forward orientation.  Frozen: quantised here, once (never refreshed).  Trained: the
    bytes are its bank's, rewritten by every refresh (unet.UNetBank.fp8_own) - quantising here would cache bytes that the next
    optimizer update leaves stale, so a trained holder without them is refused."""
    w8 = getattr(holder, "_w8", None)
    if w8 is None:
        if getattr(holder, "trainable", False):
            raise RuntimeError(f"fp8 forward: the trained layer {getattr(holder, '_fp8_name', '?')} has no quantised weight - its "
                               f"bank owns and refreshes the bytes (build the UNetBank with fp8=True and the UNet with fp8_forward)")
        w8 = holder._w8 = kernels().fp8_quantize(holder.w.contiguous())
    return w8


def fp8_weight_group(lins):
    """(bytes [G, N, K], scales [G]) of projections whose frozen weights are co-allocated at a constant spacing (frozen_linear_group):
    each weight under ITS OWN scale, as fp8_weight would quantise it, but in one buffer - the group's fp8 products are then one
    batched launch (comat_gemm_params::s_scale_b).  None when the weights are not co-allocated."""
    g8 = getattr(lins[0], "_w8_group", None)
    if g8 is None:
        if len(lins) < 2 or _uniform_stride([lin.w for lin in lins]) is None:
            return None
        G, (N, Kd) = len(lins), lins[0].w.shape
        w8 = torch.empty((G, N, Kd), dtype=torch.uint8, device=lins[0].w.device)
        sc = torch.empty(G, dtype=torch.float32, device=w8.device)
        for i, lin in enumerate(lins):
            lin._w8 = kernels().fp8_quantize(lin.w.contiguous(), out=w8[i], scale=sc[i:i + 1])
        g8 = lins[0]._w8_group = (w8, sc)
    return g8


# ---- activation scales ------------------------------------------------------------------------------------------------
# "jit" (rounds 2-5): every activation that enters an fp8 product is quantised under its OWN abs-max - two launches per tensor
# (a reduction with a ticket, then the bytes), ~1 300 of them per SDXL forward.
# "delayed" (round 6; COMAT_FP8_SCALING=delayed, bench.py --config c5): a quantisation SITE (the input of one frozen layer) keeps
# a scale and a running abs-max in two device words (include/comat_hip.h, ABI 8).  Every tensor that passes the site during an
# optimizer step is quantised under the scale that is already there - the abs-max over ALL of the previous step's calls of that
# site (every denoise step, trained or not) - and folds its own abs-max into the running maximum; fp8_end_of_step() (after the
# optimizer) turns the maxima into the next step's scales.  One launch per tensor, and none where the producer emits the bytes
# itself: LayerNorm / GroupNorm(+SiLU) store the e4m3 bytes next to their output when told whom they feed (`fp8_for=`) - the
# same bits as quantising the stored output.  Values beyond the previous step's abs-max saturate at +-448 * scale, as in every
# delayed-scaling recipe.  Before the first step the scales come from fp8_calibration(): one no-grad pass in which every site
# quantises just in time AND records its abs-max.  A site that has no scale yet when a step reaches it (no calibration, or a layer
# the calibration pass never ran) does the same on its own: just in time until the next fp8_end_of_step(), delayed from then on.
# COMAT_FP8_KTAIL (default 1): the LoRA up projection of a frozen projection rides in the fp8 product's launch as a bf16 k-tail
# (comat_gemm_params::A2k); 0 = its own launch behind it (rounds 2-5), for A/B runs
_ktail = os.environ.get("COMAT_FP8_KTAIL", "1") != "0"
# COMAT_FP8_GEGLU_Q8 (default 1): `ff.net.0.proj` + GEGLU emits the e4m3 bytes for `ff.net.2` from its epilogue (comat_gemm_params::q8)
_geglu_q8 = os.environ.get("COMAT_FP8_GEGLU_Q8", "1") != "0"
# COMAT_FP8_FLASH_Q8 (default 1): the fused attention forward emits the e4m3 bytes for its output projection (comat_flash_attn_fwd_q)
_flash_q8 = os.environ.get("COMAT_FP8_FLASH_Q8", "1") != "0"
_MAX_SITES = 4096
_MAX_HISTORY = 16
_scaling = os.environ.get("COMAT_FP8_SCALING", "jit")
_calibrating = False
_states = {}
_epoch = 0  # bumped by fp8_end_of_step(): bytes a producer emitted under the scales of an earlier step are stale
_warned_capture = False
_trusting = None  # inside fp8_capture_on_trust(): the set of scale-less sites captured in the delayed form


def set_fp8_scaling(mode: str):
    global _scaling
    assert mode in ("jit", "delayed"), mode
    _scaling = mode


def fp8_scaling():
    return _scaling


# ---- the delayed-scaling recipe ------------------------------------------------------------------------------------------
# None (no call of set_fp8_recipe, none of the environment variables): fp8_end_of_step() launches comat_fp8_scales_update - the
# scale of a step is the previous step's abs-max / 448.  Set: it launches comat_fp8_scales_update_hist instead (still one launch
# per device): the scale is `margin` x the maximum over the last `history` steps' abs-maxima / 448, `account` records which sites
# exceeded the scale they were quantised under (fp8_report, logs["fp8_clipped_sites"]), and `reduce_amax` takes the abs-maxima
# over all data-parallel ranks first, so that every rank quantises the same weights' inputs on the same grid.
# COMAT_FP8_HISTORY / COMAT_FP8_MARGIN / COMAT_FP8_REDUCE_AMAX set the same values at import (bench.py --config c5 under a recipe).
_recipe = None


def set_fp8_recipe(history=1, margin=1.0, account=True, reduce_amax=False):
    global _recipe
    history, margin = int(history), float(margin)
    if not 1 <= history <= _MAX_HISTORY:
        raise ValueError(f"fp8 recipe: history must be in [1, {_MAX_HISTORY}], got {history}")
    if not (margin >= 1.0 and margin != float("inf")):
        raise ValueError(f"fp8 recipe: margin must be finite and >= 1, got {margin}")
    if _recipe is not None and _recipe["history"] != history:
        for st in _states.values():  # the table is laid out [n, history]: another length starts a fresh window
            st.start_window()
    _recipe = dict(history=history, margin=margin, account=bool(account), reduce_amax=bool(reduce_amax))


def clear_fp8_recipe():
    """back to the plain update (comat_fp8_scales_update); the history tables keep their contents"""
    global _recipe
    _recipe = None


def fp8_recipe():
    """the recipe in force (a copy), or None"""
    return None if _recipe is None else dict(_recipe)


if any(v in os.environ for v in ("COMAT_FP8_HISTORY", "COMAT_FP8_MARGIN", "COMAT_FP8_REDUCE_AMAX")):
    set_fp8_recipe(history=os.environ.get("COMAT_FP8_HISTORY", "1"), margin=os.environ.get("COMAT_FP8_MARGIN", "1.0"),
                   reduce_amax=os.environ.get("COMAT_FP8_REDUCE_AMAX", "0") != "0")


class _Fp8State:
    """the scale / running-maximum words of every quantisation site on one device and the recipe's tables (fixed addresses:
    captured graphs read them); host side: which sites have a scale (`ready`), which were used since the last update, who they feed.
    Invariants, kept by the methods (nobody else writes these fields): unready == ready.count(False); `count` (how much of a
    site's history window is filled) is zeroed whenever the window starts afresh - another length, a recalibration."""

    def __init__(self, device):
        self.scale = torch.zeros(_MAX_SITES, dtype=torch.float32, device=device)
        self.amax = torch.zeros(_MAX_SITES, dtype=torch.int32, device=device)  # float bits of a non-negative value
        self.hist = torch.zeros((_MAX_SITES, _MAX_HISTORY), dtype=torch.float32, device=device)  # used as [n, history]
        self.count = torch.zeros(_MAX_SITES, dtype=torch.int32, device=device)
        self.clip_steps = torch.zeros(_MAX_SITES, dtype=torch.int32, device=device)
        self.worst = torch.zeros(_MAX_SITES, dtype=torch.float32, device=device)
        self.clip_now = torch.zeros(_MAX_SITES, dtype=torch.int32, device=device)
        self.n = 0
        self.ready = []        # per site: a scale is in force (the site was used before some fp8_end_of_step())
        self.unready = 0       # how many are not
        self.used = set()      # sites used since the last fp8_end_of_step()
        self.holders = []      # per site: weak reference to the layer it feeds (fp8_report names it)
        self.after_calibration = False

    def add_site(self, holder):
        """-> the row of a new site in front of `holder` (no scale yet; no device allocation)"""
        assert self.n < _MAX_SITES, "fp8: site table full"
        i = self.n
        self.n += 1
        self.ready.append(False)
        self.unready += 1
        self.holders.append(weakref.ref(holder))
        return i

    def start_window(self):
        self.count.zero_()

    def start_calibration(self):
        """fresh running maxima and a fresh window; the update that follows accounts no clips"""
        self.amax.zero_()
        self.start_window()
        self.after_calibration = True

    def close_step(self):
        """every site used since the last call has a scale from here on -> (did one of them lack it: the scale word holds its
        last call's own scale, not one in force; was this step a calibration pass)"""
        fresh = False
        for i in self.used:
            if not self.ready[i]:
                fresh, self.ready[i] = True, True
                self.unready -= 1
        self.used.clear()
        after_cal, self.after_calibration = self.after_calibration, False
        return fresh, after_cal

    def load(self, sd):
        """copies into the EXISTING fixed-address tables (captured graphs read those addresses)"""
        n = int(sd["n"])
        if n != self.n:
            raise ValueError(f"fp8 state: {n} sites saved, {self.n} in this process (a different network or fp8 layer selection)")
        with torch.no_grad():
            for key in ("scale", "hist", "count", "clip_steps", "worst"):
                getattr(self, key)[:n].copy_(sd[key])
            self.amax[:n].zero_()
            self.clip_now[:n].zero_()
        self.ready[:] = [bool(r) for r in sd["ready"]]
        self.unready = self.ready.count(False)
        self.used.clear()
        self.after_calibration = False


def _key(device):
    return str(torch.device(device))


def fp8_state(device):
    """allocate the site table of `device` (call once OUTSIDE any graph capture: UNet.__init__ does)"""
    key = _key(device)
    st = _states.get(key)
    if st is None:
        st = _states[key] = _Fp8State(device)
    return st


def fp8_site(holder, device):
    """(scale [1], amax [1]) views of the site in front of `holder` (index assigned at first use; no device allocation)"""
    site = getattr(holder, "_fp8_site", None)
    if site is None:
        st = fp8_state(device)
        i = st.add_site(holder)
        holder._fp8_index = (st, i)
        site = holder._fp8_site = (st.scale[i:i + 1], st.amax[i:i + 1])
    return site


def _ready(holder):
    """is a scale in force for the site of `holder` (or promised to be when the launch runs: fp8_capture_on_trust)?"""
    st, i = holder._fp8_index
    if st.ready[i]:
        return True
    if _trusting is not None:
        _trusting.add((st, i))
        return True
    return False


def _use(holder):
    """note that the site of `holder` sees a tensor this step -> _ready"""
    st, i = holder._fp8_index
    st.used.add(i)
    return _ready(holder)


class fp8_capture_on_trust:
    """`with fp8_capture_on_trust() as c:` around a CAPTURE whose owner replays the graph only once fp8_pending(c.sites) is False
    (GraphedUNetForward): sites without a scale are captured in the delayed form all the same - the scale words are read at replay
    time - instead of the two-launch just-in-time form; c.sites collects them."""

    def __enter__(self):
        global _trusting
        self.sites = set()
        self.prev, _trusting = _trusting, self.sites
        return self

    def __exit__(self, *exc):
        global _trusting
        _trusting = self.prev
        return False


class fp8_sites_preserved:
    """`with fp8_sites_preserved(device):` around launches that are not part of the step - the warm-up run a graph owner makes before
    it captures (GraphedUNetForward: on inputs that need not be this step's) and the capture itself: the running maxima and the
    host-side `used` marks are put back afterwards, so such a run never reaches a scale.  Enter and leave outside any capture."""

    def __init__(self, device):
        self.st = _states.get(_key(device)) if _scaling == "delayed" else None

    def __enter__(self):
        st = self.st
        if st is not None and st.n:
            self.amax, self.used = st.amax[:st.n].clone(), set(st.used)
        else:
            self.st = None
        return self

    def __exit__(self, *exc):
        st = self.st
        if st is not None:
            st.amax[:self.amax.numel()].copy_(self.amax)
            st.used = self.used
        return False


def fp8_pending(sites):
    """sites: what fp8_capture_on_trust collected; drops those that have a scale by now -> does one still lack it?"""
    if sites:
        for st, i in [s_ for s_ in sites if s_[0].ready[s_[1]]]:
            sites.discard((st, i))
    return bool(sites)


def fp8_unready(device):
    """does a site of `device` still lack a scale?  (host-side flag: no launch, no sync)"""
    st = _states.get(_key(device))
    return st is not None and st.unready > 0


def fp8_reset():
    """forget every site table, as a new process would (tests; holders built before keep pointing at the old tables, and so do
    captured graphs: never inside a run)"""
    global _warned_capture
    _states.clear()
    _warned_capture = False


@contextlib.contextmanager
def fp8_calibration():
    """`with fp8_calibration():` every site quantises just in time (its own abs-max) and records the abs-max: run the sampler once
    under it, then fp8_end_of_step() (TrainableSDPipeline.fp8_calibrate does both).  A recalibration starts a fresh history window,
    and the update that follows it accounts no clips (every call ran under its own scale)."""
    global _calibrating
    prev, _calibrating = _calibrating, True
    try:
        for st in _states.values():
            st.start_calibration()
        yield
    finally:
        _calibrating = prev


def _reduce_amax(st):
    """the abs-maxima over all ranks: the words are int32 bits of non-negative floats, so the integer MAX is the float max"""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return
    assert not (st.amax.is_cuda and torch.cuda.is_current_stream_capturing()), "fp8: the abs-max all-reduce must not be captured"
    dist.all_reduce(st.amax[:st.n], op=dist.ReduceOp.MAX)


def fp8_end_of_step(gnorm_sq=None):
    """delayed scaling: the running maxima of this step become the next step's scales (one launch per device; a no-op otherwise).
    Every site used since the last call has a scale from here on.
    gnorm_sq: the device word the optimizer's skip reads (FlatAdamW.gnorm_sq) - where it is not finite the update of the weights was
    skipped, and the scales skip theirs: every running maximum of that device is cleared first (decided on the device, no host
    sync), so that the update treats every site as unseen and a skipped step leaves scale, history and count as they were.
    One exception: a site whose SCALE is not finite keeps its maximum.  Such a scale comes from a site without a scale that met a
    NaN in its first, just-in-time step (an uncalibrated first step that was poisoned: the word it quantised under is its own NaN
    abs-max / 448, and close_step() marks it ready).  Every later step of that site quantises to NaN bytes and is skipped; were its
    maximum cleared with the others, the scale would never recover.  Kept, the first finite abs-max of the site replaces it - the
    sites heal in network order, one skipped step each - and fp8_calibrate() heals all of them at once."""
    global _epoch
    if _scaling != "delayed":
        return
    _epoch += 1
    r = _recipe
    for st in _states.values():
        if not st.n:
            continue
        fresh, after_cal = st.close_step()
        if gnorm_sq is not None and gnorm_sq.device == st.amax.device:
            keep = torch.isfinite(gnorm_sq) | ~torch.isfinite(st.scale[:st.n])
            st.amax[:st.n].mul_(keep.to(torch.int32))  # (bits of a non-negative float: times 0 or 1)
        if r is None:
            kernels().fp8_scales_update(st.amax, st.scale, st.n)
            continue
        if r["reduce_amax"]:
            _reduce_amax(st)
        acc = (st.clip_steps, st.worst, st.clip_now) if r["account"] else (None, None, None)
        kernels().fp8_scales_update_hist(st.amax, st.scale, st.hist, st.count, *acc, st.n, r["history"], r["margin"],
                                         r["account"] and not after_cal and not fresh)


def fp8_act(x, holder):
    """(e4m3 bytes, scale [1]) of the activation x entering the fp8 product of `holder`"""
    global _warned_capture
    k = kernels()
    if _scaling != "delayed":
        return k.fp8_quantize(x)
    sc, am = fp8_site(holder, x.device)
    ready = _use(holder)
    if _calibrating or not ready:
        # no scale in force yet (calibration pass, or a site first reached now): this call's own abs-max, recorded for the next step
        if not _calibrating and not _warned_capture and x.is_cuda and torch.cuda.is_current_stream_capturing():
            _warned_capture = True
            warnings.warn("fp8 delayed scaling: a site without a scale is being captured - the graph keeps the two-launch "
                          "just-in-time form for it; calibrate (fp8_calibrate) before prepare_graphs()", stacklevel=2)
        return k.fp8_quantize(x, scale=sc, amax=am)[0], sc
    pre = getattr(x, "_fp8", None)
    # the producer of x stored the bytes for this very site, this step, and x has not been written since
    if pre is not None and pre[1] is sc and pre[2] == _epoch and pre[3] == x._version:
        return pre[0], sc
    return k.fp8_quantize_scaled(x, sc, am), sc


def fp8_producer_site(holder, k_inner, device):
    """a norm that feeds `holder`: the site it should quantise for, or None (no fp8, not eligible, jit scales, calibration pass,
    no scale in force yet)"""
    if holder is None or _scaling != "delayed" or _calibrating or not use_fp8(holder, k_inner):
        return None
    site = fp8_site(holder, device)
    if not _ready(holder):
        return None  # fp8_act quantises just in time (and marks the site used)
    _use(holder)
    return site


def fp8_stamp(y, q8, site):
    """attach the bytes a producer emitted for `site` to its output (fp8_act checks scale, step and version before it uses them)"""
    y._fp8 = (q8, site[0], _epoch, y._version)


def fp8_clipped_sites(device, out):
    """out [] int32 (fixed address) = the number of sites the latest update flagged; one launch, no host sync"""
    st = _states[_key(device)]
    return torch.sum(st.clip_now[:st.n], dim=(0,), dtype=torch.int32, out=out)


def _name(st, i):
    h = st.holders[i]()
    return getattr(h, "_fp8_name", None) or f"site{i}"


def fp8_report(device, top=8):
    """host-side view of the clip accounting (synchronises: for logs and tests): the number of sites, those the latest update
    flagged, the cumulative count of flagged (site, step) pairs, and the `top` sites by worst overshoot (abs-max / 448 over the
    scale it was quantised under), each with the name of the layer it feeds"""
    st = _states.get(_key(device))
    if st is None or not st.n:
        return dict(sites=0, clipped_now=[], clip_steps=0, top=[])
    n = st.n
    now, steps, worst = st.clip_now[:n].cpu(), st.clip_steps[:n].cpu(), st.worst[:n].cpu()
    entry = lambda i: dict(site=i, name=_name(st, i), worst=float(worst[i]), clip_steps=int(steps[i]), clipped_now=bool(now[i]))
    order = sorted((i for i in range(n) if steps[i] > 0), key=lambda i: (-float(worst[i]), i))
    return dict(sites=n, clipped_now=[entry(i) for i in torch.nonzero(now).reshape(-1).tolist()], clip_steps=int(steps.sum()),
                top=[entry(i) for i in order[:top]])


def fp8_state_dict(device):
    """what a resumed run needs to continue under the same scales: host tensors of the site tables, the ready flags, the recipe"""
    st = fp8_state(device)
    n = st.n
    cp = lambda t: t[:n].detach().cpu().clone()
    return dict(n=n, scale=cp(st.scale), hist=cp(st.hist), count=cp(st.count), clip_steps=cp(st.clip_steps), worst=cp(st.worst),
                ready=list(st.ready), recipe=fp8_recipe())


def fp8_load_state_dict(device, sd):
    """the site table must be the one the UNet constructor built (_Fp8State.load)"""
    fp8_state(device).load(sd)
    if sd.get("recipe") is not None:
        set_fp8_recipe(**sd["recipe"])
