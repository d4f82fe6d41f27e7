"""comat_conv2d_wgrad on the SD1.5 VAE decoder's real layers (batch 1, bf16), each timed against the forward comat_conv2d of the
same layer - the same FLOPs, on the same box, from one process in alternating windows, device events around each window.

    python tools/mb_conv_wgrad.py [--launches 20] [--rounds 7] [--out FILE]

Prints per layer the median time of both, the TFLOP/s of the weight gradient and the ratio wgrad / forward."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from comat_amd import _hip  # noqa: E402

# (name, Cin, Cout, Hin = Win, ups): 3x3, stride 1, pad 1
LAYERS = [("512->512 @ 64^2", 512, 512, 64, 1), ("512->512 @ 128^2", 512, 512, 128, 1), ("256->256 @ 256^2", 256, 256, 256, 1),
          ("128->128 @ 512^2", 128, 128, 512, 1), ("512->512 @ 64^2 ups 2", 512, 512, 64, 2), ("512->512 @ 128^2 ups 2", 512, 512, 128, 2),
          ("256->256 @ 256^2 ups 2", 256, 256, 256, 2), ("128->3 @ 512^2", 128, 3, 512, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    K = _hip.HipKernels()
    dev, bf = torch.device("cuda:0"), torch.bfloat16
    gen = torch.Generator(device=dev).manual_seed(0)
    lines = [f"bf16, batch 1, 3x3 stride 1 pad 1; {args.launches} launches per window, {args.rounds} alternating rounds; "
             f"library {_hip.build_id()}",
             f"{'layer':24s} {'wgrad us':>9s} {'TFLOP/s':>8s} {'fwd us':>9s} {'TFLOP/s':>8s} {'ratio':>6s}  kernel"]
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, cin, cout, hin, ups in LAYERS:
        ho = hin * ups
        x = (torch.randn(hin * hin, cin, device=dev, generator=gen) * 0.5).to(bf)
        dy = (torch.randn(ho * ho, cout, device=dev, generator=gen) * 0.5).to(bf)
        w = (torch.randn(cout, 3, 3, cin, device=dev, generator=gen) * 0.05).to(bf)
        y = torch.empty(ho * ho, cout, device=dev, dtype=bf)
        dw = torch.zeros(cout, 3, 3, cin, device=dev)
        run = {"wgrad": lambda: K.conv2d_wgrad(x, dy, dw, 1, hin, hin, cin, ho, ho, cout, 3, 3, 1, 1, ups),
               "fwd": lambda: K.conv2d(x, w, y, 1, hin, hin, cin, ho, ho, cout, 3, 3, 1, 1, mode=0, ups=ups)}
        run["wgrad"]()
        kid = _hip.last_gemm_kernel()
        run["fwd"]()
        torch.cuda.synchronize()
        times = {k: [] for k in run}
        for _ in range(args.rounds):
            for k, f in run.items():
                s.record()
                for _ in range(args.launches):
                    f()
                e.record()
                torch.cuda.synchronize()
                times[k].append(s.elapsed_time(e) * 1e3 / args.launches)
        flop = 2.0 * ho * ho * cout * 9 * cin
        tw, tf = statistics.median(times["wgrad"]), statistics.median(times["fwd"])
        lines.append(f"{name:24s} {tw:9.1f} {flop / tw * 1e-6:8.1f} {tf:9.1f} {flop / tf * 1e-6:8.1f} {tw / tf:6.2f}  {kid}"
                     f"  (wgrad min {min(times['wgrad']):.1f} max {max(times['wgrad']):.1f})")
        print(lines[-1], flush=True)
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
