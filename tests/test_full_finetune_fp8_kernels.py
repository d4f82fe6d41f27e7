"""comat_weights_refresh_q8 (include/comat_hip.h): the refresh launch of a fully trained UNet that also re-quantises the
fp8-eligible weights - their e4m3 bytes at the forward copy's element offsets and one scale per weight.

Every case runs on the ABI simulator (tests/sim_backend.py) and, marked gpu, on the library.  The copies are held bit for
bit to comat_weights_refresh on the same tables; scales and bytes bit for bit to the CPU oracle's quantiser (oracle/fp8.py) on the
forward copy of each layer (a conv: the whole [Cout, KH, KW, Cin] tensor under ONE scale).  The byte buffer is pre-filled with a
poison byte, the scales with NaN and the copies with NaN halos: nothing outside the quantised layers may change.  The table is
that of tests/test_full_finetune_kernels.py (a few thousand elements), with two layers left unquantised (slot -1).
"""
import functools

import pytest
import torch

from comat_amd import refresh
from oracle import fp8 as OF
from test_full_finetune_kernels import HALO, LAYERS, refresh_layout

F32, BF16 = torch.float32, torch.bfloat16
SLOT = {("lin", 24, 32): 0, ("lin", 128, 64): 1, ("conv", 32, 3, 4): -1, ("conv", 4, 3, 32): 2, ("conv", 32, 3, 96): 3,
        ("conv", 24, 1, 40): -1, ("lin", 5, 7): 4, ("lin", 65, 63): 5}
N_SLOTS = 6
POISON = 0xA5
TINY_SCALE = torch.tensor(2.0 ** -100, dtype=F32) / 448.0


def kernels():
    from comat_amd import ops
    return ops.kernels()


def count(L):
    return L[1] * L[2] if L[0] == "lin" else L[1] * L[2] * L[2] * L[3]


@functools.lru_cache(maxsize=None)
def table():
    """(place, buffer length, problems, slot per problem row) of LAYERS under SLOT; shared, never written"""
    assert HALO % 2 == 1
    place, n, problems = refresh_layout()
    slots = []
    for L in LAYERS:
        slots += [SLOT[L]] * (1 if L[0] == "lin" else L[2] * L[2])
    assert len(slots) == len(problems)
    return place, n, problems, slots


@functools.lru_cache(maxsize=None)
def base_master():
    _, n, _, _ = table()
    return torch.randn(n, generator=torch.Generator().manual_seed(23))


def offset_of(L):
    return next(off for M, off, _ in table()[0] if M == L)


def run(dev, dtype, master, state=None):
    """one call on fresh (poisoned) buffers, or on those of an earlier call -> dict of device buffers"""
    _, n, problems, slots = table()
    if state is None:
        nan = float("nan")
        state = dict(w=None if dtype == F32 else torch.full((n,), nan, dtype=dtype, device=dev),
                     wt=torch.full((n,), nan, dtype=dtype, device=dev),
                     q8=torch.full((n,), POISON, dtype=torch.uint8, device=dev),
                     scales=torch.full((N_SLOTS,), nan, dtype=F32, device=dev),
                     amax=torch.zeros(N_SLOTS, dtype=torch.int32, device=dev),
                     plan=refresh.RefreshPlan(problems, dev, slots=slots))
    md = master.to(dev)
    state["plan"].run(md, state["w"], state["wt"], state["q8"], state["scales"], state["amax"])
    assert torch.equal(md.cpu(), master), "the master was written"
    return state


def check_against_oracle(state, dtype, master, what=""):
    """K2 + K3: every slot's scale and every quantised layer's bytes are the oracle's on the layer's forward copy; every other
    byte keeps the poison"""
    place, n, _, _ = table()
    q8, scales = state["q8"].cpu(), state["scales"].cpu()
    poison = torch.ones(n, dtype=torch.bool)
    for L, off, doff in place:
        if SLOT[L] < 0:
            continue
        fwd = master[off:off + count(L)].to(dtype)  # what fp8_weight() would read from holder.w
        want_q, want_s = OF.quantize(fwd)
        got_s = scales[SLOT[L]]
        assert got_s.view(torch.int32) == OF.scale_of(fwd).view(torch.int32), f"{what}{L}: scale {float(got_s)} != oracle {float(want_s)}"
        bad = int((q8[doff:doff + count(L)] != want_q).sum())
        assert bad == 0, f"{what}{L}: {bad} of {count(L)} bytes differ from the oracle"
        assert not bool(((q8[doff:doff + count(L)] & 0x7F) == 0x7F).any()), f"{what}{L}: a NaN byte"
        poison[doff:doff + count(L)] = False
    assert bool((q8[poison] == POISON).all()), f"{what}a byte outside the quantised layers was written"


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_refresh_q8_copies_scales_and_bytes(dev, dtype):
    """K1, K2, K3"""
    place, n, problems, _ = table()
    master = base_master()
    st = run(dev, dtype, master)
    # K1: the copies are those of the plain launch on the same tables, halos included
    nan = float("nan")
    w0 = None if dtype == F32 else torch.full((n,), nan, dtype=dtype, device=dev)
    wt0 = torch.full((n,), nan, dtype=dtype, device=dev)
    refresh.RefreshPlan(problems, dev).run(master.to(dev), w0, wt0)
    bits = lambda t: t.cpu().view(torch.int16 if t.dtype == BF16 else torch.int32)
    if w0 is not None:
        assert torch.equal(bits(st["w"]), bits(w0)), "w differs from comat_weights_refresh's"
    assert torch.equal(bits(st["wt"]), bits(wt0)), "wt differs from comat_weights_refresh's"
    inside = torch.zeros(n, dtype=torch.bool)
    for L, off, doff in place:
        inside[doff:doff + count(L)] = True
    if w0 is not None:  # K3: the halos of the copies survive
        assert torch.isnan(st["w"].cpu()[~inside].float()).all() and not torch.isnan(st["w"].cpu()[inside].float()).any()
    assert torch.isnan(st["wt"].cpu()[~inside].float()).all() and not torch.isnan(st["wt"].cpu()[inside].float()).any()
    check_against_oracle(st, dtype, master)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("where", ["conv_last", "partial_tile", "negative"])
def test_refresh_q8_placement_of_the_maximum(dev, dtype, where):
    """K4: the single largest magnitude of a slot sits in the last element of the last tap's second column tile, in the last
    partial tile of a two-row-tile matrix, or is negative: the scale follows"""
    master = base_master().clone()
    if where == "conv_last":
        L = ("conv", 32, 3, 96)
        master[offset_of(L) + count(L) - 1] = 37.5
    elif where == "partial_tile":
        L = ("lin", 65, 63)
        master[offset_of(L) + 64 * 63 + 62] = 37.5
    else:
        L = ("lin", 128, 64)
        master[offset_of(L) + 70 * 64 + 5] = -37.5
    st = run(dev, dtype, master)
    assert st["scales"].cpu()[SLOT[L]].view(torch.int32) == (torch.tensor(37.5) / 448.0).view(torch.int32)
    check_against_oracle(st, dtype, master, what=f"{where}: ")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_refresh_q8_all_zero_slot(dev, dtype):
    """K5"""
    master = base_master().clone()
    L = ("conv", 4, 3, 32)
    off = offset_of(L)
    master[off:off + count(L)] = 0.0
    st = run(dev, dtype, master)
    assert st["scales"].cpu()[SLOT[L]].view(torch.int32) == TINY_SCALE.view(torch.int32)
    assert int(st["q8"].cpu()[off:off + count(L)].max()) == 0
    check_against_oracle(st, dtype, master)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
def test_refresh_q8_no_stale_maximum(dev, dtype):
    """K6: a second call after one slot shrank by 64 and another grew by 64; a third, unchanged call gives the second's bits"""
    master = base_master().clone()
    st = run(dev, dtype, master)
    check_against_oracle(st, dtype, master, what="first call: ")
    for L, f in ((("lin", 128, 64), 1.0 / 64), (("conv", 32, 3, 96), 64.0)):
        off = offset_of(L)
        master[off:off + count(L)] *= f
    st = run(dev, dtype, master, st)
    check_against_oracle(st, dtype, master, what="second call: ")
    q2, s2 = st["q8"].cpu().clone(), st["scales"].cpu().clone()
    st = run(dev, dtype, master, st)
    assert torch.equal(st["q8"].cpu(), q2) and torch.equal(st["scales"].cpu().view(torch.int32), s2.view(torch.int32))


def test_refresh_q8_refusals(dev):
    """K7"""
    _, n, problems, slots = table()
    plan = refresh.RefreshPlan(problems, dev, slots=slots)
    k = kernels()
    m = torch.zeros(n, device=dev)
    w, wt = torch.zeros(n, dtype=BF16, device=dev), torch.zeros(n, dtype=BF16, device=dev)
    q8 = torch.full((n,), POISON, dtype=torch.uint8, device=dev)
    sc, am = torch.zeros(N_SLOTS, device=dev), torch.zeros(N_SLOTS, dtype=torch.int32, device=dev)
    ok = [m, w, wt, q8, sc, am, plan.d_problems, plan.d_slots, plan.d_tiles]
    cases = []
    for nul in range(9):  # each null pointer; index 1 is bf16 mode without w
        a = list(ok)
        a[nul] = None
        cases.append(a)
    cases.append(ok[:8] + [plan.d_tiles[:0]])                          # n_tiles 0
    cases.append(ok[:8] + [plan.d_tiles[:1].expand(2 ** 31, 3)])       # n_tiles 2^31 (a view: no memory behind it is touched)
    cases.append(ok[:4] + [sc[:0], am[:0]] + ok[6:])                   # n_slots 0
    for a in cases:
        with pytest.raises(RuntimeError, match="comat_weights_refresh_q8"):
            k.weights_refresh_q8(*a)
    assert float(w.float().abs().max()) == 0.0 and float(wt.float().abs().max()) == 0.0  # nothing was launched
    assert bool((q8 == POISON).all()) and float(sc.abs().max()) == 0.0 and int(am.abs().max()) == 0


def test_bank_slot_table(sim):
    """K8 (CPU only, no kernel): the slot table UNetBank builds for the fp8 test network"""
    from comat_amd import ops, weights
    from comat_amd.unet import UNet, UNetBank, _Mods
    from test_fp8 import FP8_UNET
    sd = weights.make_unet_weights(FP8_UNET, perturb_norms=True)
    bank = UNetBank(FP8_UNET, sd, F32, "cpu", fp8=True)
    UNet(FP8_UNET, sd, F32, "cpu", bank=bank, fp8_forward=True)
    table_, owner = bank.slot_table(), bank._owner
    assert len(table_) == len(bank._problems) == len(owner)
    by_name = {}
    for name, s in zip(owner, table_):
        by_name.setdefault(name, set()).add(s)
    assert all(len(v) == 1 for v in by_name.values()), "the problems (taps) of one weight carry different slots"
    n_el = 0
    for name, (s,) in ((k_, tuple(v)) for k_, v in by_name.items()):
        h = bank._made[name][1]
        k_inner = h.cin if isinstance(h, ops.TrainableConv) else h.in_features
        eligible = k_inner % 64 == 0 and not any(f in name for f in _Mods.NO_FP8)
        assert (s >= 0) == eligible, (name, s, k_inner)
        assert (getattr(h, "_w8", None) is not None) == eligible
        n_el += eligible
        if isinstance(h, ops.TrainableConv):
            assert sum(o == name for o in owner) == h.kh * h.kw
    used = sorted(s for (s,) in map(tuple, by_name.values()) if s >= 0)
    assert used == list(range(n_el)) and n_el == len(bank._slot) and n_el > 100  # dense in [0, n_slots)
    assert any(s == -1 for s in table_)
