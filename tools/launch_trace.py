"""Which kernels does the host code launch, with which operands, in which order, on which streams?

    python tools/launch_trace.py [--gpu] [--only SUBSTRING]

A refactor of the host code (comat_amd/ops.py and the modules behind it) must leave this unchanged; a performance change is
meant to change it, visibly.  The installed kernel backend - the simulator of the C ABI (tests/sim_backend.py) on the CPU, `HipKernels` with --gpu - is wrapped in a proxy that records every method call: the method's name, every scalar
argument, of every tensor argument (also inside tuples and lists) shape, strides, dtype and storage offset, and on the GPU
the current stream as an index by order of first appearance.  Addresses and values are not recorded: two runs of one tree
print the same lines.  Per scenario (miniature worlds of tests/test_step.py and tests/test_fp8_recipe.py, fp32 and bf16
storage; the plain eager step, and the step through segments.SegmentedStep and step.GraphedStep over several calls) it prints the number of calls and a SHA-256 over the records.  Run it on two trees and compare the lines; two
scenarios that differ in one switch must differ in their digest on both (the setter reaches the code that reads the flag)."""
import argparse
import functools
import hashlib
import itertools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def describe(v):
    if torch.is_tensor(v):
        return f"T{tuple(v.shape)}{v.stride()}{v.dtype}@{v.storage_offset()}"
    if isinstance(v, (tuple, list)):
        return "[" + ",".join(describe(x) for x in v) + "]"
    if v is None or isinstance(v, (bool, int, float, str, torch.dtype, torch.device)):
        return repr(v)
    return type(v).__name__


class Recorder:
    """proxy of a kernel backend: same attributes (a missing method stays missing: the host code asks with hasattr)"""

    def __init__(self, backend, gpu):
        self.__dict__.update(_b=backend, _gpu=gpu, _streams={}, records=[])

    def __setattr__(self, name, value):
        setattr(self._b, name, value)

    def __getattr__(self, name):
        fn = getattr(self._b, name)
        if not callable(fn):
            return fn

        def call(*a, **kw):
            rec = [name] + [describe(x) for x in a] + [f"{k}={describe(kw[k])}" for k in sorted(kw)]
            if self._gpu:
                st = torch.cuda.current_stream().cuda_stream
                rec.append(f"stream{self._streams.setdefault(st, len(self._streams))}")
            self.records.append(" ".join(rec))
            return fn(*a, **kw)
        return call


STEP = dict(training_steps=[1, 2], crop=(0, 0, 63, 63))


def scenarios(dev, gpu):
    from comat_amd import ops
    from test_fp8_recipe import _fp8_sd15_world
    from test_step import make_world
    for dtype, attrcon in itertools.product((torch.float32, torch.bfloat16), (False, True)):
        tag = f"{str(dtype)[6:]} {'attrcon' if attrcon else 'gan'}"
        for merged, tail, grouped in itertools.product((0, 1), repeat=3):
            def step(dtype=dtype, attrcon=attrcon, merged=merged, tail=tail, grouped=grouped):
                ops.set_train_merged(merged), ops.set_lora_tail(tail), ops.set_tt_grouping(grouped)
                _, b, _, tr = make_world(dtype, dev, attrcon, rank=8)
                tr.train_step(b, **STEP)
            yield f"step {tag} merged={merged} tail={tail} grouped={grouped}", step
    for dtype in (torch.float32, torch.bfloat16):
        tag = str(dtype)[6:]

        def sampler(dtype=dtype):
            _, b, _, tr = make_world(dtype, dev, False)
            with torch.no_grad():
                tr.pipe.forward(b["prompt_embeds"], b["negative_prompt_embeds"], height=64, width=64, num_inference_steps=3,
                                latents=b["latents"], noises=b["noises"], output_type="latent")
        yield f"sampler {tag}", sampler

        def rank4(dtype=dtype):  # the tiny configuration's own rank: weight gradients the grouped kernel does not take
            _, b, _, tr = make_world(dtype, dev, False)
            tr.train_step(b, **STEP)
        yield f"step {tag} gan rank=4", rank4
    # (the fp8 miniature of tests/test_fp8_recipe.py is an fp32-storage world)
    def fp8_jit():
        tr, b = _fp8_sd15_world(dev)
        tr.train_step(b, **STEP)
    yield "fp8 jit step", fp8_jit

    def fp8_delayed():
        ops.set_fp8_scaling("delayed")
        ops.set_fp8_recipe(history=4, margin=1.25)
        tr, b = _fp8_sd15_world(dev)
        assert tr.fp8_calibrate(b)
        for _ in range(2):
            tr.train_step(b, **STEP)
        ops.fp8_load_state_dict(dev, ops.fp8_state_dict(dev))
        tr.train_step(b, **STEP)
    yield "fp8 delayed: calibration, 2 steps, save/load, 1 step", fp8_delayed
    # the sampler's other modes (StepConfig.early_exit / .fast_training / .double_laststep, cfg_scale <= 1): one step each
    import dataclasses

    from comat_amd.step import CoMatTrainer
    modes = {"early_exit": dict(early_exit=True), "fast_training": dict(fast_training=True),
             "double_laststep": dict(double_laststep=True), "guidance off": dict(cfg_scale=1.0)}
    for dtype, (mode, kw) in itertools.product((torch.float32, torch.bfloat16), modes.items()):
        def mode_step(dtype=dtype, mode=mode, kw=kw):
            cfg, b, _, tr = make_world(dtype, dev, False)
            tr = CoMatTrainer(tr.pipe, tr.bank, tr.blip, tr.D, dataclasses.replace(cfg, **kw), seed=0)
            b = dict(b)
            if mode == "double_laststep":  # one more step noise for the extra step, and the re-noising draw
                b["noises"] = list(b["noises"]) + [b["noises"][0].flip(0)]
                b["renoise"] = b["latents"].flip(0)
            if mode == "guidance off":
                del b["negative_prompt_embeds"]
            tr.train_step(b, **STEP)
        yield f"step {str(dtype)[6:]} gan rank=4 {mode}", mode_step
    # the steppers (comat_amd/segments.py, step.GraphedStep): the step through their hooks, staging and replays included
    from comat_amd.segments import SegmentedStep

    def segmented(dtype, attrcon, calls, **kw):
        def run():
            _, b, _, tr = make_world(dtype, dev, attrcon, rank=8)
            st = SegmentedStep(tr, **kw)
            for _ in range(calls):
                st(b, **STEP)
            assert st.failed is None, st.failed
        return run
    if not gpu:
        for attrcon in (False, True):  # dry: every segment's function eagerly through the same hooks
            yield f"segments dry float32 {'attrcon' if attrcon else 'gan'}, 2 calls", segmented(torch.float32, attrcon, 2, dry=True)
        return
    # first call: eager pieces and their captures; then two calls of replays
    yield "segments bfloat16 gan, 3 calls", segmented(torch.bfloat16, False, 3)
    yield "segments bfloat16 attrcon, 3 calls", segmented(torch.bfloat16, True, 3)
    yield "segments bfloat16 gan use_d=own, 3 calls", segmented(torch.bfloat16, False, 3, use_d="own")
    for dtype in (torch.float32, torch.bfloat16):
        tag = str(dtype)[6:]

        def disabled(dtype=dtype):
            ops.set_side_stream_enabled(False)
            _, b, _, tr = make_world(dtype, dev, False, rank=8)
            tr.train_step(b, **STEP)
        yield f"step {tag} gan, side streams disabled", disabled

        def suspended(dtype=dtype):
            _, b, _, tr = make_world(dtype, dev, False, rank=8)
            with ops.no_side_streams():
                tr.train_step(b, **STEP)
        yield f"step {tag} gan, inside no_side_streams", suspended

        def graphed(dtype=dtype, split=None):  # an eager step and the capture, then two replays
            from comat_amd.step import GraphedStep
            before = os.environ.get("COMAT_GRAPH_SPLIT")
            if split is not None:
                os.environ["COMAT_GRAPH_SPLIT"] = split
            try:
                _, b, _, tr = make_world(dtype, dev, False, rank=8)
                gs = GraphedStep(tr)
                assert gs.supported(b)
                for _ in range(3):
                    gs(b, **STEP)
                assert gs.failed is None, gs.failed
            finally:
                if split is not None:
                    del os.environ["COMAT_GRAPH_SPLIT"]
                    if before is not None:
                        os.environ["COMAT_GRAPH_SPLIT"] = before
        yield f"step {tag} gan, captured whole-step graph, 3 calls", graphed
        if dtype == torch.bfloat16:
            yield f"step {tag} gan, captured whole-step graph, COMAT_GRAPH_SPLIT=1, 3 calls", functools.partial(graphed, split="1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true", help="HipKernels on cuda:0 (default: the CPU simulator of the C ABI)")
    ap.add_argument("--only", default="", help="run the scenarios whose name contains this")
    ap.add_argument("--dump", default=None, help="directory: one file of records per scenario")
    args = ap.parse_args()
    from comat_amd import _hip, ops
    from sim_backend import SimKernels
    dev =torch.device("cuda:0" if args.gpu else "cpu")
    env = {k: os.environ.get(k, "1") != "0" for k in ("COMAT_TRAIN_MERGED", "COMAT_LORA_TAIL", "COMAT_TT_GROUPED")}
    for name, run in scenarios(dev, args.gpu):
        if args.only not in name:
            continue
        rec = Recorder(_hip.HipKernels() if args.gpu else SimKernels(), args.gpu)
        ops.set_kernel_backend(rec)  # a fresh backend, and nothing left of the previous scenario's streams, sites and switches
        ops.fp8_reset(), ops.clear_fp8_recipe(), ops.set_fp8_scaling("jit"), ops.set_side_stream_enabled(True)
        ops.set_train_merged(env["COMAT_TRAIN_MERGED"]), ops.set_lora_tail(env["COMAT_LORA_TAIL"])
        ops.set_tt_grouping(env["COMAT_TT_GROUPED"])
        run()
        if args.gpu:
            torch.cuda.synchronize()
            ops.reset_capture_stream(dev)
        ops.drop_side_stream_state()
        text = "\n".join(rec.records)
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            with open(os.path.join(args.dump, "".join(c if c.isalnum() else "_" for c in name) + ".txt"), "w") as f:
                f.write(text + "\n")
        print(f"{name:60s} {len(rec.records):6d} calls  sha256 {hashlib.sha256(text.encode()).hexdigest()[:32]}", flush=True)


if __name__ == "__main__":
    main()
