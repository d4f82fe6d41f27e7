"""comat_adamw_lr (fp32 moments, 28 bytes per element) against comat_adamw8_window with window == NULL (8-bit blockwise moments,
16 + 1/16 bytes per element) at SD1.5's parameter count, on synthetic flat buffers from a seed: alternating windows in one process,
device events around each window, a synchronise at its end.

    python tools/bench_optim8.py [--n 859520964] [--launches 20] [--rounds 5] [--out profiles/optim8.txt]

Prints per kernel the median, minimum and maximum over the rounds of the time per launch and the bytes per second at the median.
The fp32 kernel is the yardstick: the 8-bit launch must not be slower."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from comat_amd import _hip, optim8  # noqa: E402

SD15_PARAMETERS = 859_520_964


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=SD15_PARAMETERS)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    K = _hip.HipKernels()
    dev = torch.device("cuda:0")
    n, hp = args.n, (0.9, 0.999, 1e-8, 1e-2)
    gen = torch.Generator(device=dev).manual_seed(0)
    g = torch.randn(n, device=dev, generator=gen) * 1e-3
    p32 = torch.randn(n, device=dev, generator=gen) * 0.05
    p8 = p32.clone()
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    m8 = torch.full((n,), optim8.zero_code(True), dtype=torch.uint8, device=dev)
    v8 = torch.full((n,), optim8.zero_code(False), dtype=torch.uint8, device=dev)
    am, av = torch.zeros(optim8.n_blocks(n), device=dev), torch.zeros(optim8.n_blocks(n), device=dev)
    counters = torch.tensor([3, 0], dtype=torch.int32, device=dev)
    nsq = torch.zeros(1, device=dev)
    K.sumsq(g, n, nsq)
    word = torch.full((1,), 5e-5, dtype=torch.float32, device=dev)
    run = {"adamw_lr": lambda: K.adamw_lr(p32, g, m, v, n, word, *hp, counters, nsq, 0.1),
           "adamw8_window": lambda: optim8.adamw8_window(p8, g, m8, v8, am, av, n, word, *hp, counters, nsq, 0.1)}
    for f in run.values():  # warm-up; the moments leave zero
        f(), f()
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
            times[name].append(s.elapsed_time(e) / args.launches)
    nbytes = {"adamw_lr": 28 * n, "adamw8_window": (16 + 1 / 16) * n}
    lines = [f"build {_hip.build_id()}  {torch.cuda.get_device_name(0)}",
             f"n = {n}, {args.launches} launches per window, {args.rounds} alternating rounds ({args.launches * args.rounds} timed "
             f"launches per kernel)"]
    for name, t in times.items():
        med = statistics.median(t)
        lines.append(f"{name:14s} {nbytes[name] / 1e9:6.2f} GB per launch   median {med:7.3f} ms  min {min(t):7.3f}  max {max(t):7.3f}   "
                     f"{nbytes[name] / med / 1e9:5.2f} TB/s at the median")
    a, b = statistics.median(times["adamw_lr"]), statistics.median(times["adamw8_window"])
    lines.append(f"adamw8_window / adamw_lr = {b / a:.3f} in time for {nbytes['adamw8_window'] / nbytes['adamw_lr']:.3f} of the bytes; "
                 f"share of 6.3 TB/s: {nbytes['adamw8_window'] / b / 1e9 / 6.3:.2f} (8-bit), {nbytes['adamw_lr'] / a / 1e9 / 6.3:.2f} (fp32)")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    assert b <= a, "the 8-bit launch is slower than the fp32 launch: the code search is the bottleneck"


if __name__ == "__main__":
    main()
