"""Masked-attention microbenchmark on the text paths' shapes: ops.attention(need_probs=False) under a causal limit (and BLIP's
right-padded key mask) on the fused masked kernels (ops.set_fused_masked_attention(True): 1 launch forward, 2 backward) against
the materialised path (GEMM, softmax, GEMM forward; five to six launches backward), bf16, forward and forward + backward, each call
replayed from a hipGraph - what it costs inside a replayed step.  python tools/mb_masked_attention.py  (GPU box)

The rounds of the two paths alternate inside one process; the table gives the median and the minimum over the rounds."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from comat_amd import _hip, ops  # noqa: E402

# name, B, H, L or T, d, padded (BLIP: right-padded key mask on top of the causal limit), directions
SHAPES = [
    ("CLIP-L", 2, 12, 77, 64, False, ("fwd", "fwd+bwd")),
    ("CLIP-bigG", 2, 20, 77, 64, False, ("fwd",)),
    ("BLIP decoder", 1, 12, 32, 64, True, ("fwd", "fwd+bwd")),
    ("BLIP decoder", 4, 12, 32, 64, True, ("fwd", "fwd+bwd")),
]
ROUNDS, CALLS = 7, 20


def graph_of(fn, n=CALLS):
    """n calls back to back in one hipGraph (no host gaps)"""
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):  # this stream's workspaces exist before the capture
        fn()
        fn()
    st.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        for _ in range(n):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def replay_us(g, n=CALLS):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


def main():
    dev = torch.device("cuda:0")
    ops.set_kernel_backend(_hip.HipKernels())
    T = torch.bfloat16
    print(f"# library {_hip.build_id()}; us per call, {CALLS} calls per hipGraph replay, median (min) of {ROUNDS} alternating rounds")
    for name, B, H, L, d, padded, dirs in SHAPES:
        HD = H * d
        gen = torch.Generator(device=dev).manual_seed(B * L)
        q, k, v = (torch.randn(B * L, HD, device=dev, generator=gen).to(T) for _ in range(3))
        go = torch.randn(B * L, HD, device=dev, generator=gen).to(T)
        km = None
        if padded:  # captions of 32, 20, 26, 9 tokens
            km = torch.ones(B, L, dtype=torch.int8, device=dev)
            for b, n in enumerate((32, 20, 26, 9)[:B]):
                km[b, n:] = 0
        for direction in dirs:
            def call(fused):
                ops.set_fused_masked_attention(fused)
                if direction == "fwd":
                    with torch.no_grad():
                        ops.attention(q, k, v, B, L, L, H, d, causal=True, key_mask=km, need_probs=False)
                    return
                qg, kg, vg = (t.detach().requires_grad_(True) for t in (q, k, v))
                o, _ = ops.attention(qg, kg, vg, B, L, L, H, d, causal=True, key_mask=km, need_probs=False)
                o.backward(go)
            graphs = {fused: graph_of(lambda: call(fused)) for fused in (False, True)}
            t = {False: [], True: []}
            for _ in range(ROUNDS):
                for fused in (False, True):
                    t[fused].append(replay_us(graphs[fused]))
            med = {f: statistics.median(x) for f, x in t.items()}
            print(f"{name:13s} B={B} H={H:2d} L={L:2d} d={d} causal{' + key mask' if padded else '           '} {direction:8s}  "
                  f"materialised {med[False]:7.1f} ({min(t[False]):7.1f}) us   fused {med[True]:7.1f} ({min(t[True]):7.1f}) us   "
                  f"fused / materialised {med[True] / med[False]:5.2f}", flush=True)
    ops.set_fused_masked_attention(False)


if __name__ == "__main__":
    main()
