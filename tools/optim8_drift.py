"""How far the tiny trainer's parameters move apart under `use_8bit_adam`: two trainers of the tiny configuration (tests/test_step.py's
world, LoRA, GAN leg on) step on the same batches, one with fp32 moments and one with 8-bit blockwise moments; after each step the
difference of the flat parameters in units of the learning rate - and, for the optimizer alone, an 8-bit optimizer on a copy of the
generator's parameters that is fed the fp32 trainer's own gradients.  A recorded figure, not a pass condition: it
depends on the gradient distribution, not on the kernel.

    python tools/optim8_drift.py [--steps 40] [--out FILE]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from comat_amd import _hip, ops, optim8  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from test_lr_schedule import STEP, fresh_inputs, world
    ops.set_kernel_backend(_hip.HipKernels())
    dev, dtype = torch.device("cuda:0"), torch.float32
    cfg, batch, plain = world(dtype, dev, use_8bit_adam=False)
    _, _, tr = world(dtype, dev, use_8bit_adam=True)
    # the optimizer alone: an 8-bit optimizer on a copy of the generator's parameters, fed the fp32 trainer's own gradients
    shadow_p, shadow_g = plain.bank.flat.clone(), torch.zeros_like(plain.bank.flat)
    shadow = optim8.FlatAdamW8bit([(shadow_p, shadow_g)], cfg.lr, (cfg.adam_beta1, cfg.adam_beta2), cfg.adam_epsilon,
                                  cfg.adam_weight_decay, cfg.max_grad_norm)
    gen = torch.Generator().manual_seed(40)
    lines = [f"build {_hip.build_id()}; tiny configuration, fp32, lr {cfg.lr} (G) / {cfg.lr_D} (D), {tr.bank.flat.numel()} generator and "
             f"{tr.D.bank.flat.numel()} discriminator LoRA parameters; |p8 - p32| / lr, max and mean over the parameters",
             "same gradients: an 8-bit optimizer fed the fp32 trainer's generator gradients; G, D: a second trainer under the flag on "
             "the same batches (its gradients follow its own parameters)"]
    for it in range(1, args.steps + 1):
        b = fresh_inputs(batch, gen, dtype)
        plain.train_step(b, **STEP), tr.train_step(b, **STEP)
        shadow_g.copy_(plain.bank.flat_grad)  # still the gradient the update read: it is cleared at the start of the next step
        shadow.step(plain.grad_scale)
        if it in (1, 2, 5, 10, 20, args.steps):
            ds = (shadow_p - plain.bank.flat).abs() / cfg.lr
            dg = (tr.bank.flat - plain.bank.flat).abs() / cfg.lr
            dd = (tr.D.bank.flat - plain.D.bank.flat).abs() / cfg.lr_D
            lines.append(f"step {it:3d}: same gradients max {float(ds.max()):.3f} mean {float(ds.mean()):.4f}   G max {float(dg.max()):.3f} "
                         f"mean {float(dg.mean()):.4f}   D max {float(dd.max()):.3f} mean {float(dd.mean()):.4f}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
