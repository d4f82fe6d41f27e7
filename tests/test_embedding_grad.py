"""comat_embed_grad and comat_embed_fwd (include/comat_hip.h), the kernel pair behind the trained embedding tables of
`--tune_text_encoder`, on the simulator's mirrors (tests/clip_tune_sim.py) and on the real kernels.

The gradient kernel promises an ORDER, not a tolerance: the rows of one id are added to 0 in ascending index in fp32 and that sum
is added once to the table's row.  `restate` below is that sentence in numpy float32, one addition at a time; every comparison in
this file is on bits.  Rows that no id names start as a signalling-NaN pattern: any arithmetic on them, `+= 0` included, would
quiet it."""
import numpy as np
import pytest
import torch

from clip_tune_sim import EMBED_GRAD_MAX_N, sim_matches_binding, tune_dev  # noqa: F401 - fixture
from comat_amd import _hip, ops

MAX_N = EMBED_GRAD_MAX_N
SENTINEL = 0x7FA00001  # a signalling NaN
DIMS = (8, 40, 768)
NS = (1, 77, 616, MAX_N)
DTYPES = (torch.bfloat16, torch.float32)
L77 = 77


def make_ids(pattern, n, vocab, seed):
    """int64 [n] and the vocab of the launch"""
    g = torch.Generator().manual_seed(seed)
    if pattern == "null":  # the null prompt: every position names the end token
        return torch.full((n,), vocab - 1, dtype=torch.int64)
    if pattern == "collide":  # every row collides
        return torch.randint(0, vocab, (n,), generator=g)
    if pattern == "clamped":  # ids below 0 and at or above vocab: clamped as the forward clamps them
        ids = torch.randint(-4, vocab + 4, (n,), generator=g)
        ids[0], ids[-1] = -7, vocab + 1000
        return ids
    assert pattern == "padded"  # sequences of 77: random ids, an end token, then a pad run of the end token's id
    ids = torch.randint(3, vocab - 2, (n,), generator=g)
    for b, a in enumerate(range(0, n, L77)):
        end = a + 1 + (b * 13) % (L77 - 1)
        ids[end:a + L77] = vocab - 1
    return ids


def restate(ids, dy, start, vocab):
    """the kernel's contract, sequentially in float32: (result, named rows)"""
    out, v = start.copy(), np.clip(ids, 0, vocab - 1)
    rows = np.unique(v)
    for row in rows:
        acc = np.zeros(dy.shape[1], np.float32)
        for j in np.nonzero(v == row)[0]:  # ascending
            acc = acc + dy[j]
        out[row] = out[row] + acc
    return out, rows


def start_table(vocab, dim, named, seed, integer=False):
    """fp32 [vocab, dim]: a non-zero gradient of an earlier micro-step on the rows the ids name, the sentinel on every other row"""
    t = torch.full((vocab, dim), SENTINEL, dtype=torch.int32).view(torch.float32)
    g = torch.Generator().manual_seed(seed)
    fill = torch.randn(len(named), dim, generator=g)
    if len(named):
        t[torch.as_tensor(named)] = torch.round(fill * 4) if integer else fill
    return t


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def run(dev, ids, dy, table, vocab):
    n, dim = dy.shape
    t = table.clone().to(dev)  # (the caller's table stays what it was, on the CPU leg too)
    ops.table_kernels().embed_grad(ids.to(dev), dy.to(dev), t, n, dim, vocab)
    return t.cpu()


def check(dev, ids, vocab, dim, dtype, seed):
    n = ids.numel()
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(n, dim, generator=g).to(dtype)
    named = np.unique(np.clip(ids.numpy(), 0, vocab - 1))
    start = start_table(vocab, dim, named, seed + 1)
    want, _ = restate(ids.numpy(), dy.float().numpy(), start.numpy(), vocab)
    got = run(dev, ids, dy, start, vocab)
    assert torch.equal(bits(got), bits(torch.from_numpy(want))), "differs from the sequential fp32 restatement"
    unnamed = np.setdiff1d(np.arange(vocab), named)
    assert (bits(got)[torch.as_tensor(unnamed)] == SENTINEL).all(), "a row that no id names was written"
    assert torch.equal(bits(run(dev, ids, dy, start, vocab)), bits(got)), "a second run gives other bits"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("pattern,vocab", [("null", 100), ("padded", 1000), ("collide", 5), ("clamped", 50)])
def test_gradient_is_the_sequential_sum_bit_for_bit(tune_dev, pattern, vocab, n, dim, dtype):
    check(tune_dev, make_ids(pattern, n, vocab, seed=n + dim), vocab, dim, dtype, seed=7 * n + dim)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", [77, 616])
def test_clip_vocabulary_at_768(tune_dev, n, dtype):
    """vocab 49408, dim 768: the real token table's shape (8 prompts of 77 = 616 ids)"""
    check(tune_dev, make_ids("padded", n, 49408, seed=n), 49408, 768, dtype, seed=n)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("pattern,vocab,n,dim", [("null", 100, 77, 768), ("padded", 1000, 616, 40), ("collide", 5, MAX_N, 8),
                                                 ("clamped", 50, 616, 768), ("collide", 5, 1, 40)])
def test_integer_gradients_give_the_exact_sum(tune_dev, pattern, vocab, n, dim, dtype):
    ids = make_ids(pattern, n, vocab, seed=3)
    g = torch.Generator().manual_seed(n + dim)
    dy = torch.randint(-8, 9, (n, dim), generator=g)
    v = ids.clamp(0, vocab - 1)
    named = np.unique(v.numpy())
    start = start_table(vocab, dim, named, 5, integer=True)
    exact = torch.zeros(vocab, dim, dtype=torch.int64).index_add_(0, v, dy)
    got = run(tune_dev, ids, dy.to(dtype), start, vocab)
    rows = torch.as_tensor(named)
    assert torch.equal(got[rows].double(), start[rows].double() + exact[rows].double())


def test_more_ids_than_the_maximum_are_refused_before_any_launch(tune_dev):
    n, dim, vocab = MAX_N + 1, 8, 16
    assert _hip.EMBED_GRAD_MAX_N == MAX_N == ops.EMBED_GRAD_MAX_N
    ids = torch.zeros(n, dtype=torch.int64)
    table = start_table(vocab, dim, [], 0)
    t = table.to(tune_dev)
    with pytest.raises(RuntimeError, match=f"comat_embed_grad.*at most {MAX_N}"):
        ops.table_kernels().embed_grad(ids.to(tune_dev), torch.ones(n, dim).to(tune_dev), t, n, dim, vocab)
    assert (bits(t) == SENTINEL).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("B,L", [(1, 77), (4, 77), (4, 8)])
def test_position_form(tune_dev, B, L, dim, dtype):
    """ids i mod L: the position table's gradient is dy.reshape(B, L, dim).sum(0), taken sample by sample from 0"""
    n, npos = B * L, 77
    g = torch.Generator().manual_seed(B * L + dim)
    dy = torch.randn(n, dim, generator=g).to(dtype)
    start = start_table(npos, dim, list(range(L)), 9)
    acc = np.zeros((L, dim), np.float32)
    for b in range(B):
        acc = acc + dy.float().numpy().reshape(B, L, dim)[b]
    want = start.numpy().copy()
    want[:L] = want[:L] + acc
    got = run(tune_dev, torch.arange(n) % L, dy, start, npos)
    assert torch.equal(bits(got), bits(torch.from_numpy(want)))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n,L", [(1, 1), (77, 77), (616, 77), (MAX_N, 64), (32, 8)])
@pytest.mark.parametrize("pattern,vocab", [("null", 100), ("padded", 1000), ("collide", 5), ("clamped", 50)])
def test_fused_forward_is_the_cast_of_the_fp32_sum(tune_dev, pattern, vocab, n, L, dim, dtype):
    """the shapes of the gradient tests (sequences of L tokens, L <= the 77 rows of the position table)"""
    ids = make_ids(pattern, n, vocab, seed=n)
    g = torch.Generator().manual_seed(dim)
    tok, pos = torch.randn(vocab, dim, generator=g), torch.randn(77, dim, generator=g)
    want = (tok[ids.clamp(0, vocab - 1)] + pos[torch.arange(n) % L]).to(dtype)
    out = torch.full((n, dim), float("nan"), dtype=dtype, device=tune_dev)
    ops.table_kernels().embed_fwd(ids.to(tune_dev), tok.to(tune_dev), pos.to(tune_dev), out, n, L, dim, vocab)
    view = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert torch.equal(out.cpu().view(view), want.view(view))


def test_forward_refuses_more_tokens_than_positions(tune_dev):
    tok, pos = torch.zeros(4, 8).to(tune_dev), torch.zeros(3, 8).to(tune_dev)
    with pytest.raises(RuntimeError, match="comat_embed_fwd"):
        ops.table_kernels().embed_fwd(torch.zeros(4, dtype=torch.int64).to(tune_dev), tok, pos, torch.zeros(4, 8).to(tune_dev), 4, 4, 8, 4)


def test_binding_and_simulator_agree():
    names, differ = sim_matches_binding()
    assert not differ, differ
    assert {"comat_" + n for n in names} <= set(_hip.SIGNATURES)
