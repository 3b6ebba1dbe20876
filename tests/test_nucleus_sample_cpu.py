"""The full-vocabulary sampler's definition (``ref.nucleus_sample``) against a loop-and-list twin on tiny rows, and the
routing of ``_sample`` on CPU tensors."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from jax_llama_amd import ops
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime.engine import GenerationConfig, _sample


def _twin(row, top_k, temperature, top_p, seed, step, r):
    """One row, with lists and loops: (token, number of survivors)."""
    inv_t = float(np.float32(1.0 / temperature))
    ranked = sorted(range(len(row)), key=lambda i: (-row[i], i))[:top_k or len(row)]
    l = {i: float(row[i]) * inv_t for i in ranked}
    if top_p < 1.0:
        e = [math.exp(l[i] - l[ranked[0]]) for i in ranked]
        ranked = [i for j, i in enumerate(ranked) if j == 0 or sum(e[:j]) < top_p * sum(e)]
    best = None
    for i in sorted(ranked):
        ctr = np.array([[i >> 2, r, step, 1]], dtype=np.uint32)
        w = int(ref.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[0, i & 3])
        score = l[i] - math.log(-math.log(((w >> 8) + 0.5) / 2.0 ** 24))
        if best is None or score > best[0]:
            best = (score, i)
    return best[1], len(ranked)


@pytest.mark.parametrize("top_k,temperature,top_p", [(0, 0.6, 0.9), (0, 1.0, 1.0), (5, 1.3, 0.5), (40, 0.7, 1.0)])
def test_reference_is_its_twin(top_k, temperature, top_p):
    g = torch.Generator().manual_seed(top_k)
    x = (torch.randn(12, 23, generator=g) * 2).round(decimals=1)  # coarse values: ties, broken by index
    x[3] = 0.5
    tok, kept = ref.nucleus_sample(x, top_k, temperature, top_p, (7 << 32) + 5, 9, return_kept=True)
    want = [_twin(x[r].tolist(), top_k, temperature, top_p, (7 << 32) + 5, 9, r) for r in range(12)]
    assert tok.tolist() == [t for t, _ in want] and kept.tolist() == [n for _, n in want]


def test_sample_routes_by_top_k_on_cpu():
    model = SimpleNamespace(comm=SimpleNamespace(size=1, rank=0))
    x = torch.randn(6, 300, generator=torch.Generator().manual_seed(1))
    step = torch.tensor([4], dtype=torch.int32)

    def gc(k):
        return GenerationConfig(max_length=8, do_sample=True, top_k=k, temperature=0.7, top_p=0.9, seed=11)
    for k in (0, None, 65, 1000):
        assert torch.equal(_sample(model, x, gc(k), None, step), ref.nucleus_sample(x, k, 0.7, 0.9, 11, 4))
    for k in (1, 50, 64):  # what topk_sample served before, it still serves
        assert torch.equal(_sample(model, x, gc(k), None, step), ref.topk_sample(x, k, 0.7, 0.9, 11, 4))
    assert not torch.equal(ref.nucleus_sample(x.repeat(20, 1), 65, 0.7, 0.9, 11, 4),
                           ref.topk_sample(x.repeat(20, 1), 64, 0.7, 0.9, 11, 4))  # other Philox streams
    with pytest.raises(ValueError):
        ops.nucleus_sample(torch.zeros(1, ops.NUCLEUS_MAX_V + 1), 0, 1.0, 0.9, 0, step)
