"""The full-vocabulary sampler (csrc/kernels/nucleus_sample.hip) on the MI355X against ``ref.nucleus_sample``, the
float64 definition: survivor counts and draws on rows with a built-in top-p gap (tests/nucleus_inputs.py), flat rows
whose masses are exact integers, pure temperature sampling, banned tokens, graph replay, the engine and two TP ranks."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import loop_inputs as li
import nucleus_inputs as ni
from jax_llama_amd import ops
from jax_llama_amd.models import LLaMAForCausalLM
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime.engine import DecodeEngine, GenerationConfig
from jax_llama_amd.utils.checkpoint import meta_state_dict_to_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
LEAD = 1e-4  # a row is left out of a draw comparison only when the reference's own Gumbel lead is below this


def _step(s):
    return torch.tensor([s], dtype=torch.int32, device=DEV)


def _reference(x, top_k, temperature, top_p, seed, step):
    """(tokens, survivor counts, rows left out) of the reference; at most 1 % left out, before any GPU result."""
    scored = ref.nucleus_scores(x, top_k, temperature, top_p, seed, step)
    tok = torch.tensor([int(i[np.argmax(s)]) for i, s in scored], dtype=torch.int32)
    kept = torch.tensor([i.size for i, _ in scored], dtype=torch.int32)
    out = torch.from_numpy(ni.leads(scored) < LEAD)
    assert int(out.sum()) <= 0.01 * x.shape[0], int(out.sum())
    return tok, kept, out


@pytest.mark.parametrize("temperature", [0.6, 1.3])
@pytest.mark.parametrize("top_k", [0, 65, 3000])
@pytest.mark.parametrize("v", [1000, 1025, 16384 + 3, 128256])
@pytest.mark.parametrize("n", [1, 63, 700, 5000])
def test_gap_rows_survivors_and_draws(n, v, top_k, temperature):
    """Head below and above a tile (2048) and the compaction capacity (4096); rows on the scalar path (V < 1024,
    V % 4 != 0) and the 16-byte path; top_k above the head (top-p alone decides) and below it (Z is the top k's)."""
    top_p, seed, step = 0.9, 77, 11
    x, c = ni.gap_rows(64 if v < 100000 else 16, v, n, top_k, temperature, top_p, seed=n + v)
    want, kept, out = _reference(x, top_k, temperature, top_p, seed, step)
    assert bool((kept == c).all())
    got, got_kept = ops.nucleus_sample(x.to(DEV), top_k, temperature, top_p, seed, _step(step), return_kept=True)
    assert torch.equal(got_kept.cpu(), kept)
    assert torch.equal(got.cpu()[~out], want[~out])


@pytest.mark.parametrize("v,top_k,top_p,count", [(8, 0, 0.5, 4), (40000, 0, 0.25, 10000), (8, 3, 1.0, 3),
                                                 (40000, 3, 1.0, 3), (8, 3, 0.5, 2), (40000, 3, 0.25, 1)])
def test_flat_rows_keep_exactly_the_lowest_indices(v, top_k, top_p, count):
    """All logits equal: every mass is 2^40, the cuts are integer arithmetic. top_p = 0.5 of 8 keeps ranks 0..3 (the mass
    before rank 4 is exactly 0.5: out, by the strict rule), 0.25 of 40000 keeps 10000 (ties across tiles, streamed);
    top_k = 3 keeps 3, and a top_p < 1 on top of it the ranks with less than top_p * 3 before them (Z is the top k's)."""
    x = torch.full((4096 if v == 8 else 256, v), 1.25)
    got, kept = ops.nucleus_sample(x.to(DEV), top_k, 1.0, top_p, 5, _step(2), return_kept=True)
    assert bool((kept.cpu() == count).all())
    drawn = set(got.cpu().tolist())
    assert drawn == set(range(count)) if count <= 4 else max(drawn) < count and len(drawn) > 200


def test_pure_temperature_identical_rows_follow_the_softmax():
    row = torch.randn(2000, generator=torch.Generator().manual_seed(21)) * 2
    draws = ops.nucleus_sample(row.expand(4096, 2000).contiguous().to(DEV), 0, 0.8, 1.0, 1234, _step(7)).cpu()
    li.check_draws(draws, row, 2000, 0.8, 1.0)


@pytest.mark.parametrize("top_k", [0, 200])
def test_4096_random_rows_pure_temperature_and_top_k_alone(top_k):  # (count cuts: no mass boundary to sit on)
    x = torch.randn(4096, 2000, generator=torch.Generator().manual_seed(31)) * 2
    want, kept, out = _reference(x, top_k, 0.8, 1.0, 99, 17)
    got, got_kept = ops.nucleus_sample(x.to(DEV), top_k, 0.8, 1.0, 99, _step(17), return_kept=True)
    assert torch.equal(got_kept.cpu(), kept)
    assert torch.equal(got.cpu()[~out], want[~out])


@pytest.mark.parametrize("top_k,top_p", [(0, 1.0), (0, 0.9), (3000, 1.0)])
def test_banned_tokens_are_never_drawn(top_k, top_p):
    """Most of every row at -inf (top_k = 3000 reaches into the bans); the last row all -inf: drawn as equal logits."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(512, 4100, generator=g)
    banned = torch.rand(512, 4100, generator=g) < 0.7
    x[banned] = float("-inf")
    x[-1] = float("-inf")
    got = ops.nucleus_sample(x.to(DEV), top_k, 1.0, top_p, 8, _step(4)).cpu().long()
    assert not bool(banned[torch.arange(511), got[:511]].any())
    assert int(got[-1]) == int(ref.nucleus_sample(x, top_k, 1.0, top_p, 8, 4)[-1])


def test_graph_replays_are_the_eager_result():
    x, _ = ni.gap_rows(64, 16384, 700, 0, 0.6, 0.9, seed=1)
    x, st = x.to(DEV), _step(9)
    eager = ops.nucleus_sample(x, 0, 0.6, 0.9, 3, st, return_kept=True)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.nucleus_sample(x, 0, 0.6, 0.9, 3, st, return_kept=True)
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("top_k", [0, 100])
def test_engine_draws_the_host_loop(top_k, use_graph):
    """generate(do_sample, top_k = 0 / 100, top_p = 0.9) on the scripted model is the host loop over
    ref.nucleus_sample token for token; the seed keeps the host loop's margins on every draw."""
    cfg = li.config()
    params = meta_state_dict_to_params(li.state_dict(li.SAMPLE_LEVELS), cfg.num_hidden_layers)
    model = LLaMAForCausalLM(cfg, device=DEV, _do_init=False).load_params(params)
    toks, mask = li.sample_batch(0)
    sample, m = (top_k, 1.0, 0.9, 2), {}
    want = ni.host_generate(toks, 26, 0, -1, sample, m)
    assert m["lead"] >= li.LEAD_MIN and m["top_p"] >= li.TOP_P_MIN, m
    gc = GenerationConfig(max_length=26, do_sample=True, top_k=top_k, temperature=1.0, top_p=0.9, seed=2,
                          pad_token_id=0, eos_token_id=-1)
    got = DecodeEngine(model, 3, 26, use_graph=use_graph).run(toks, mask, gc).cpu().to(torch.int32)
    assert torch.equal(got, want)


def test_two_ranks_draw_the_whole_rows_tokens():
    x, _ = ni.gap_rows(64, 2048, 63, 0, 0.6, 0.9, seed=2)
    want, _, out = _reference(x, 0, 0.6, 0.9, 21, 5)
    x = x.to(DEV)
    shards = [x[:, :1024].contiguous(), x[:, 1024:].contiguous()]  # a world of two on this one GPU
    comm = SimpleNamespace(size=2, all_gather=lambda t: torch.stack(shards))  # [tp, B, V / tp], as TPComm's
    whole = ops.nucleus_sample(x, 0, 0.6, 0.9, 21, _step(5))
    for shard in shards:
        assert torch.equal(ops.nucleus_sample(shard, 0, 0.6, 0.9, 21, _step(5), comm=comm), whole)
    assert torch.equal(whole.cpu()[~out], want[~out])
