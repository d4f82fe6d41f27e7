"""The gated launches of a gradient-accumulation micro-step at the size of the C2 step's generator LoRA buffer, n = 25.6 M: comat_accum_zero
and comat_adamw_window with the gate closed (the launch leaves after one uniform load per block) against the gate open (the
buffer is cleared / the update is applied): alternating windows from one process, device events around each window.

    python tools/mb_accum_gate.py [--n 25600000] [--launches 50] [--rounds 9] [--out FILE]

Prints per arm the median, minimum and maximum over the rounds of the time per launch."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from comat_amd import _hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=25_600_000)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    K = _hip.HipKernels()
    dev = torch.device("cuda:0")
    n, hp, N = args.n, (0.9, 0.999, 1e-8, 1e-2), 4
    gen = torch.Generator(device=dev).manual_seed(0)
    g = torch.randn(n, device=dev, generator=gen)
    p, m, v = torch.randn(n, device=dev, generator=gen), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    scratch = torch.ones(n, device=dev)
    counters = torch.tensor([3, 0], dtype=torch.int32, device=dev)
    nsq = (g.double() ** 2).sum().float().reshape(1)
    word = torch.full((1,), 5e-5, dtype=torch.float32, device=dev)
    first, inside, last = (torch.tensor([i], dtype=torch.int32, device=dev) for i in (0, 1, N - 1))
    run = {"accum_zero, closed": lambda: K.accum_zero(scratch, n, inside),
           "accum_zero, open": lambda: K.accum_zero(scratch, n, first),
           "adamw_window, closed": lambda: K.adamw_window(p, g, m, v, n, word, *hp, counters, nsq, 0.1, inside, N),
           "adamw_window, open": lambda: K.adamw_window(p, g, m, v, n, word, *hp, counters, nsq, 0.1, last, N)}
    for f in run.values():
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in run}
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.rounds):
        for name, f in run.items():
            s.record()
            for _ in range(args.launches):
                f()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) * 1e3 / args.launches)
    lines = [f"n = {n}, {args.launches} launches per window, {args.rounds} alternating rounds, back-to-back launches on one stream"]
    for name, t in times.items():
        lines.append(f"{name:21s} median {statistics.median(t):7.1f} us  min {min(t):7.1f}  max {max(t):7.1f}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
