"""The fp8 recipe under data parallelism: with `reduce_amax` every rank ends a step with the SAME scale table (the abs-maxima are
all-reduced with MAX before the update), without it each rank keeps scales of its own.  Two ranks over gloo on the simulator, the
way tests/test_dist.py starts its ranks; an RCCL twin on two GPUs."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir, gpu=False):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.set_num_threads(2)
    from comat_amd import dist as cdist
    from comat_amd import ops
    from test_fp8 import _tagged, rnd
    if gpu:
        from comat_amd import _hip
        ops.set_kernel_backend(_hip.HipKernels())
        r, w, dev = cdist.init(backend="nccl")
        assert dev.type == "cuda"
    else:
        from sim_backend import SimKernels
        ops.set_kernel_backend(SimKernels())
        r, w, dev = cdist.init(backend="gloo")
    assert (r, w) == (rank, world)
    ops.set_fp8_scaling("delayed")
    out = {}
    for reduce in (False, True):
        ops.fp8_reset()
        ops.set_fp8_recipe(history=2, margin=1.25, reduce_amax=reduce)
        lins = [_tagged(ops.FrozenLinear(rnd(96, 128, seed=10 + i) * 0.1, None, torch.float32, dev)) for i in range(3)]
        xs = [rnd(40, 128, seed=20 + i) * (1.0 + 3.0 * ((rank + i) % 2)) for i in range(3)]  # which rank is larger differs by site
        with torch.no_grad(), ops.fp8_forward(True):
            for step in range(2):  # the first step just in time, the second under the (reduced) scales
                for lin, x in zip(lins, xs):
                    ops.linear((x * (1.0 + step)).to(dev), lin)
                ops.fp8_end_of_step()
        st = ops.fp8_state(dev)
        assert st.n == 3
        out[reduce] = st.scale[:3].cpu().clone()
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    cdist.barrier()
    dist.destroy_process_group()


def _check(tmp_path, world):
    r = [torch.load(os.path.join(tmp_path, f"rank{i}.pt")) for i in range(world)]
    assert not torch.equal(r[0][False], r[1][False])          # private scales: the ranks saw tensors of different magnitude
    assert torch.equal(r[0][True], r[1][True])                # reduced: one table
    assert torch.equal(r[0][True], torch.maximum(r[0][False], r[1][False]))  # ... each entry the larger rank's own value
    assert (r[0][False] > r[1][False]).any() and (r[0][False] < r[1][False]).any()


@pytest.mark.timeout(600)
def test_two_rank_gloo_amax_reduction(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), False), nprocs=world, join=True)
    _check(tmp_path, world)


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_two_rank_rccl_amax_reduction(tmp_path):
    """the same on two real GPUs over RCCL (one process per GPU); needs two devices"""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), True), nprocs=world, join=True)
    _check(tmp_path, world)
