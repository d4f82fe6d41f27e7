"""Tables of comat_weights_refresh (include/comat_hip.h): every fully trained weight of a model as a list of row-major matrices
whose compute-dtype copy and transpose are rewritten from the fp32 master in ONE launch after an optimizer step.

Plain host functions on integers (no device, no kernels): tests/test_full_finetune_kernels.py enumerates what a table covers.
Offsets are in ELEMENTS of the three flat buffers the launch is given (master, forward copies, second orientations)."""
from __future__ import annotations

import numpy as np
import torch

TILE = 64  # edge of the tile one workgroup moves (comat_amd/csrc/refresh.hip: WR_T)


def linear_problem(src, w, wt, N, K):
    """a Linear weight [N, K] at `src` of the master: w [N, K] at `w`, wt [K, N] at `wt`"""
    return [(src, w, wt, N, K, K, K, N)]


def conv_problems(src, w, wd, Cout, KH, KW, Cin):
    """a conv weight in the kernel layout [Cout, KH, KW, Cin]: one matrix per tap t = kh * KW + kw (Cout rows at pitch KH KW Cin
    from offset t Cin, Cin columns), whose transpose is tap KH KW - 1 - t (both taps flipped) of wd [Cin, KH, KW, Cout]"""
    taps = KH * KW
    return [(src + t * Cin, w + t * Cin, wd + (taps - 1 - t) * Cout, Cout, Cin, taps * Cin, taps * Cin, taps * Cout)
            for t in range(taps)]


def tile_table(problems):
    """int32 [n_tiles, 3] = (problem, r0, c0): one row per TILE x TILE block of every problem's [R, C]"""
    tiles = []
    for pi, (_, _, _, R, C, _, _, _) in enumerate(problems):
        assert R >= 1 and C >= 1
        r0, c0 = np.meshgrid(np.arange(0, R, TILE), np.arange(0, C, TILE), indexing="ij")
        tiles.append(np.stack([np.full(r0.size, pi), r0.reshape(-1), c0.reshape(-1)], 1))
    out = np.concatenate(tiles).astype(np.int32)
    assert out.shape[0] < 2 ** 31
    return out


def covered(problems, tiles, n_w, n_wt):
    """how often one launch over (problems, tiles) writes each element of the forward buffer (n_w elements) and of the second
    orientation (n_wt elements): (int32 [n_w], int32 [n_wt]).  What the kernel does, restated on indices."""
    cw, ct = np.zeros(n_w, np.int32), np.zeros(n_wt, np.int32)
    for pi, r0, c0 in np.asarray(tiles).tolist():
        _, w, wt, R, C, _, ldw, ldt = problems[pi]
        r = np.arange(r0, min(r0 + TILE, R)).reshape(-1, 1)
        c = np.arange(c0, min(c0 + TILE, C)).reshape(1, -1)
        np.add.at(cw, (w + r * ldw + c).reshape(-1), 1)
        np.add.at(ct, (wt + c * ldt + r).reshape(-1), 1)
    return cw, ct


class RefreshPlan:
    """the device tables of one launch, built once; `run` issues it"""

    def __init__(self, problems, device, slots=None):
        """slots: one entry per problem - the quantised weight it belongs to, or -1 (comat_weights_refresh_q8): `run` then also
        writes the e4m3 bytes and the per-weight scales"""
        self.problems = list(problems)
        self.tiles = tile_table(self.problems)
        self.d_problems = torch.tensor(self.problems, dtype=torch.int64).reshape(-1, 8).to(device)
        self.d_tiles = torch.from_numpy(self.tiles).to(device)
        self.slots = self.d_slots = None
        if slots is not None:
            self.slots = [int(s) for s in slots]
            assert len(self.slots) == len(self.problems)
            self.d_slots = torch.tensor(self.slots, dtype=torch.int32).to(device)

    def run(self, master, w, wt, q8=None, scales=None, amax=None):
        """w: the compute-dtype forward buffer, or None in fp32 mode (the master is the forward copy).  A plan with slots takes the
        byte buffer, the scale vector and the abs-max scratch as well."""
        from .backend import kernels
        if self.d_slots is None:
            assert q8 is None and scales is None and amax is None, "RefreshPlan: built without slots"
            kernels().weights_refresh(master, w, wt, self.d_problems, self.d_tiles)
        else:
            kernels().weights_refresh_q8(master, w, wt, q8, scales, amax, self.d_problems, self.d_slots, self.d_tiles)
