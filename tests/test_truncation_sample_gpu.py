"""min_p and typical_p in the full-vocabulary sampler kernel (csrc/kernels/nucleus_sample.hip) on the MI355X against
``ref.nucleus_sample``, the float64 definition: drawn token and survivor count on the rows of
tests/truncation_inputs.py. No row has a token above and one below the entropy at exactly equal distance: on a rational
grid that needs sum_j n_j e^(-t_j) (t_j - h) = 0, which Lindemann-Weierstrass allows only when all t_j are equal (the
all -inf rows, where every d is 0). The head rows hold the nearest pair (d = 0.746 and 0.754) and exact ties."""
from __future__ import annotations

import pytest
import torch

import truncation_inputs as ti
from jax_llama_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
# head rows: ties in d across the typical threshold (typical_p = 0.2 keeps 3 of 4 equal logits) and in the logit across
# top_k, -inf bans, a row where min_p keeps the maximum alone; V <= 4100 compacts the typical descent's boundary bin,
# V = 1023 loads scalars, 4100 is no multiple of the tile. dead: all -inf. restream: a boundary bin above the list,
# typical_p = 0.75 cutting between two tied maxima (the streamed tie cut).
CASES = ([("head", v, *c) for v in (1023, 1024, 4100, 16384, 128256) for c in ti.COMBOS]
         + [("dead", 61, *c) for c in ti.COMBOS]
         + [("restream", v, 0, 1.0, 0.0, t) for v in (16384, 128256) for t in (0.75, 0.88)])


@pytest.mark.parametrize("kind,v,top_k,top_p,min_p,typical_p", CASES)
def test_tokens_and_survivor_counts_are_the_definitions(kind, v, top_k, top_p, min_p, typical_p):
    x, temperature, tok, kept = ti.case(kind, v, top_k, top_p, min_p, typical_p)
    step = torch.tensor([ti.STEP], dtype=torch.int32, device=DEV)
    got, got_kept = ops.nucleus_sample(x.to(DEV), top_k, temperature, top_p, ti.SEED, step, return_kept=True,
                                       **ti.options(min_p, typical_p))
    assert got_kept.cpu().tolist() == kept.tolist() and got.cpu().tolist() == tok.tolist()


def test_graph_replays_are_the_eager_result():
    x = ti.case("head", 16384, 43, 0.9, 0.1, 0.88)[0].to(DEV)
    st, opt = torch.tensor([9], dtype=torch.int32, device=DEV), dict(return_kept=True, min_p=0.1, typical_p=0.88)
    eager = [ops.nucleus_sample(x, 43, 1.0, 0.9, 3, st + i, **opt) for i in range(3)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.nucleus_sample(x, 43, 1.0, 0.9, 3, st, **opt)
    for i in range(3):  # step advanced between the replays, as the decode loop does
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[i][0]) and torch.equal(out[1], eager[i][1])
        st += 1
