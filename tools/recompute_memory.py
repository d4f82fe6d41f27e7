"""Peak memory and step time of the step with and without gradient checkpointing (StepConfig.gradient_checkpointing,
comat_amd/recompute.py), under SegmentedStep, on the worlds bench.py builds:

    python tools/recompute_memory.py                      # every case below, one child process each -> a table
    python tools/recompute_memory.py --one c2 4 1         # one case in this process: config, batch, checkpointed -> one JSON line

Cases, plain and checkpointed: C2 (SD1.5 512^2, N = K = 5) at a per-GPU batch of 1, 4 and 8; C4 (SDXL 512^2, N = 50, K = 5,
attribute concentration) at 1 and at the reference's 6 (scripts/sdxl.sh).  The out-of-memory point is not searched for: the plain
step at a larger batch runs only if its need, estimated from its peak at the smaller batch (activations scale linearly with the
batch; what does not - weights, graphs' fixed buffers, workspaces - is taken from the checkpointed run's base), is under 80 % of
the free memory; else the table says "not run: estimated N GB".
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("c2", (1, 4, 8)), ("c4", (1, 6)))


def one(config, bs, ckpt, steps):
    import dataclasses

    import torch

    import bench
    from comat_amd import _hip, ops
    from comat_amd.segments import SegmentedStep
    from comat_amd.step import CoMatTrainer
    ops.set_kernel_backend(_hip.HipKernels())
    dev = torch.device("cuda:0")
    torch.cuda.set_per_process_memory_fraction(0.92)  # an over-sized case fails as a Python OOM
    free_gb = torch.cuda.mem_get_info()[0] / 2 ** 30  # before this process holds anything
    tr, batch, fixed, scfg, _, _ = bench.build_world(dev, torch.bfloat16, 0, config, bs=bs)
    tr = CoMatTrainer(tr.pipe, tr.bank, tr.blip, tr.D, dataclasses.replace(scfg, gradient_checkpointing=bool(ckpt)), seed=0)
    base = torch.cuda.memory_allocated()
    st = SegmentedStep(tr)
    for kw in list(bench.precapture_plan(scfg, fixed)) + [fixed, fixed]:  # every variant captured, then replays only
        st(batch, **kw)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    for _ in range(steps):
        st(batch, **fixed)
    torch.cuda.synchronize()
    ms = (time.time() - t0) / steps * 1e3
    print(json.dumps(dict(config=config, bs=bs, checkpointed=bool(ckpt), ms_per_step=round(ms, 1), failed=st.failed,
                          world_gb=round(base / 2 ** 30, 2), peak_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
                          reserved_gb=round(torch.cuda.max_memory_reserved() / 2 ** 30, 2), free_gb=round(free_gb, 1),
                          u_segments=len(st.unet_segs), u_pools=len(st.slot_pools))), flush=True)


def child(config, bs, ckpt, steps, timeout):
    cmd = [sys.executable, os.path.abspath(__file__), "--one", config, str(bs), str(int(ckpt)), "--steps", str(steps)]
    print(f"[recompute_memory] {config} bs {bs} {'checkpointed' if ckpt else 'plain'} ...", file=sys.stderr, flush=True)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        return dict(config=config, bs=bs, checkpointed=ckpt, error=(p.stderr.strip().splitlines() or ["?"])[-1][:200],
                    returncode=p.returncode)
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=3, metavar=("CONFIG", "BS", "CKPT"))
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--configs", default="c2,c4")
    ap.add_argument("--timeout", type=int, default=360, help="seconds per child process")
    args = ap.parse_args()
    if args.one:
        return one(args.one[0], int(args.one[1]), int(args.one[2]), args.steps)
    for config, sizes in CASES:
        if config not in args.configs.split(","):
            continue
        prev = None  # (bs, peak, world) of the plain step at the previous batch
        for bs in sizes:
            r = child(config, bs, True, args.steps, args.timeout)
            print(json.dumps(r), flush=True)
            if "error" in r:
                return 1  # a child that failed, whatever the reason: nothing more is started
            if prev is not None and "peak_gb" in r:
                fixed_gb = r["world_gb"]
                est = fixed_gb + (prev[1] - prev[2]) * bs / prev[0]
                if est > 0.8 * r["free_gb"]:
                    print(json.dumps(dict(config=config, bs=bs, checkpointed=False,
                                          note=f"not run: estimated {est:.0f} GB, {r['free_gb']:.0f} GB free")), flush=True)
                    continue
            p = child(config, bs, False, args.steps, args.timeout)
            print(json.dumps(p), flush=True)
            if "error" in p:
                return 1
            if "peak_gb" in p:
                prev = (bs, p["peak_gb"], p["world_gb"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
