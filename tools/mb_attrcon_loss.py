"""The attribute-concentration loss of one SD1.5 step - forward and backward - by the host assembly (losses.mask_loss) against the
device path (losses.mask_loss_device): 10 captured maps in mid_8 / up_16 / up_32 / up_64 (1 + 3 + 3 + 3), 8 heads, L = 77, two
captured timesteps, 512^2 masks of 3 objects with 2-token attributes, per-GPU batch 1 and 4, bf16 maps.  Alternating windows from
one process.  Per arm and batch: the HOST time of a call (the wall clock until forward + backward have been issued, no
synchronisation inside the window - what a launch-bound step pays) and the DEVICE time (events around the same work).

    python tools/mb_attrcon_loss.py [--calls 10] [--rounds 7] [--out FILE]

Prints per arm the median, minimum and maximum over the rounds of the time per call."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from comat_amd import _hip, losses, ops  # noqa: E402

LAYERS = (("mid_8", 8, 1), ("up_16", 16, 3), ("up_32", 32, 3), ("up_64", 64, 3))
HEADS, L, TIMESTEPS = 8, 77, ("41", "1")


def world(bs, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    attn = {ts: {name: [torch.softmax(torch.randn(bs * HEADS, res, res, L, device=dev, generator=g) * 2, -1).to(torch.bfloat16)
                        .requires_grad_(True) for _ in range(n)] for name, res, n in LAYERS} for ts in TIMESTEPS}
    rng = np.random.default_rng(seed)
    masks = []
    for _ in range(bs):
        m = np.zeros((3, 512, 512), dtype=bool)
        for i in range(3):
            y, x = rng.integers(0, 300, 2)
            m[i, y:y + 200, x:x + 200] = True
        masks.append(m)
    attrs = [[[2, 3], [6, 7], [10, 11]] for _ in range(bs)]
    return attn, masks, attrs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ops.set_kernel_backend(_hip.HipKernels())
    dev = torch.device("cuda:0")
    layers = tuple(n for n, _, _ in LAYERS)
    lines = [f"{sum(n for _, _, n in LAYERS)} maps x {len(TIMESTEPS)} timesteps, {HEADS} heads, L = {L}, bf16, 3 objects x 2 tokens, 512^2 masks; "
             f"forward + backward, {args.calls} calls per window, {args.rounds} alternating rounds"]
    for bs in (1, 4):
        attn, masks, attrs = world(bs, dev)
        maps = [m for d in attn.values() for v in d.values() for m in v]

        def call(fn):
            tl, pl = fn(attn, masks, attrs, layers, bs, dev)
            (1e-3 * tl + 5e-5 * pl).backward()
            for m in maps:
                m.grad = None

        arms = {"host assembly": lambda: call(losses.mask_loss), "device path": lambda: call(losses.mask_loss_device)}
        for f in arms.values():  # warm-up: code objects, window tables, allocator pools
            f()
            f()
        torch.cuda.synchronize()
        host, devt = {k: [] for k in arms}, {k: [] for k in arms}
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.rounds):
            for name, f in arms.items():
                torch.cuda.synchronize()
                s.record()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    f()
                t1 = time.perf_counter()
                e.record()
                torch.cuda.synchronize()
                host[name].append((t1 - t0) * 1e3 / args.calls)
                devt[name].append(s.elapsed_time(e) / args.calls)
        for name in arms:
            for what, t in (("host  ", host[name]), ("events", devt[name])):
                lines.append(f"bs {bs}  {name:13s} {what} median {statistics.median(t):8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
