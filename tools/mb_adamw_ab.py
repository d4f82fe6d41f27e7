"""comat_adamw (learning rate by value) against comat_adamw_lr (learning rate read from a device word, 16-byte accesses) at the
size of the C2 step's generator LoRA buffer, n = 25.6 M: alternating windows from one process, device events around each window.

    python tools/mb_adamw_ab.py [--n 25600000] [--launches 50] [--rounds 9] [--out FILE]

Prints per kernel the median, minimum and maximum over the rounds of the time per launch, the bytes moved per launch (p, g, m, v
read; p, m, v written) over that time, and whether the two passes left the same bits in p, m, v."""
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
    n, hp = args.n, (0.9, 0.999, 1e-8, 1e-2)
    gen = torch.Generator(device=dev).manual_seed(0)
    g = torch.randn(n, device=dev, generator=gen)
    init = [torch.randn(n, device=dev, generator=gen), torch.zeros(n, device=dev), torch.zeros(n, device=dev)]
    counters = torch.tensor([3, 0], dtype=torch.int32, device=dev)
    nsq = (g.double() ** 2).sum().float().reshape(1)
    lr = 5e-5
    word = torch.full((1,), lr, dtype=torch.float32, device=dev)
    lr = float(word[0])
    A, B = [t.clone() for t in init], [t.clone() for t in init]
    run = {"adamw": lambda: K.adamw(A[0], g, A[1], A[2], n, lr, *hp, 0, nsq, 0.1, step_dev=counters),
           "adamw_lr": lambda: K.adamw_lr(B[0], g, B[1], B[2], n, word, *hp, counters, nsq, 0.1)}
    for f in run.values():  # one launch each on identical operands: the same bits; also the warm-up
        f()
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(A, B))
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
    nbytes = 7 * 4 * n
    lines = [f"n = {n}, {args.launches} launches per window, {args.rounds} alternating rounds, {nbytes / 1e6:.0f} MB per launch; "
             f"p, m, v bit-identical after one launch each: {same}"]
    for name, t in times.items():
        med = statistics.median(t)
        lines.append(f"{name:9s} median {med:7.1f} us  min {min(t):7.1f}  max {max(t):7.1f}  spread {max(t) - min(t):6.1f} us   "
                     f"{nbytes / med / 1e6:5.2f} TB/s at the median")
    a, b = times["adamw"], times["adamw_lr"]
    lines.append(f"adamw_lr median - adamw median = {statistics.median(b) - statistics.median(a):+.1f} us "
                 f"(spread of adamw's own repeats: {max(a) - min(a):.1f} us)")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    assert same, "comat_adamw_lr and comat_adamw left different bits"


if __name__ == "__main__":
    main()
