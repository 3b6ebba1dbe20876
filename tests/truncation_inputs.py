"""Rows for the min_p / typical_p tests of the full-vocabulary sampler, on an exact grid (logits multiples of 1/8, the
temperature a power of two: equal logits tie exactly in every arithmetic). Every keep / cut decision of the float64
definition is at least 1e-3 (relative) from its threshold: ``case`` asserts it through the definition's ``cuts``."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import nucleus_inputs as ni
from jax_llama_amd.ops import reference as ref

HEAD = np.array([0, 0.5, 0.5, 1, 1, 1, 1, 1.5, 2, 2, 3, 4.5, 5, 6])  # below the maximum, in l units
SEED, STEP = 5, 3
COMBOS = [(0, 1.0, 0.1, 1.0), (0, 1.0, 0.0, 0.2), (0, 1.0, 0.0, 0.88), (0, 0.9, 0.1, 1.0), (40, 1.0, 0.0, 0.88),
          (43, 0.9, 0.1, 0.88), (0, 0.9, 0.0, 1.0)]  # (top_k, top_p, min_p, typical_p); the last: no new option


def rows(v: int, temperature: float, seed: int) -> torch.Tensor:
    """Three rows: HEAD at random positions (equal logits: ties in d; at temperature 1 the tokens 1.5 and 0 below the
    maximum lie above and below the entropy, at d = 0.746 and 0.754) over a tail 24 and more below it; the same with
    30 % of the tail banned; a head of one token, which min_p keeps alone."""
    rng = np.random.default_rng(seed)
    x = np.tile(-(24.0 + (np.arange(v) % 8) / 8) * temperature, (3, 1))
    x[1, rng.random(v) < 0.3] = -np.inf
    for r, head in enumerate((HEAD, HEAD, HEAD[:1])):
        x[r, rng.permutation(v)[:head.size]] = -head * temperature
    return torch.from_numpy(x.astype(np.float32))


def restream_rows(v: int) -> torch.Tensor:
    """A cluster near the entropy (2/3 of the mass), 5000 light tokens, then two equal maxima, the last in d order,
    whose d shares the first radix bin (11 bits of fp32(d)) with the light tokens': more keys than the 4096 of the LDS
    list. typical_p = 0.75 keeps one of the two maxima (the streamed tie cut), 0.88 both."""
    n1 = v - 5008
    t1 = round(math.log(n1 / 4) * 8) / 8
    h = t1 * n1 * math.exp(-t1) / (2 + n1 * math.exp(-t1))
    t2 = math.floor((2 * h - 0.05) * 8) / 8  # d = t2 - h, just below the maxima's d = h
    x = np.full((3, v), -t1)
    x[:, 1::3][:, :5000] = -t2
    x[:, -7:] = -(2 * t1 + 8)
    x[np.arange(3), [3, v // 2, v - 9]] = x[:, 6] = 0.0
    d = np.float32([t2 - h, h]).view(np.uint32) >> 21
    assert d[0] == d[1] and t2 - h < h, "restream_rows: the light tokens left the maxima's radix bin"
    return torch.from_numpy(x.astype(np.float32))


def options(min_p: float, typical_p: float) -> dict:  # (the default cases make the calls that existed before)
    return dict(min_p=min_p, typical_p=typical_p) if min_p > 0.0 or typical_p < 1.0 else {}


@functools.lru_cache(maxsize=None)
def case(kind: str, v: int, top_k: int, top_p: float, min_p: float, typical_p: float):
    """(rows, temperature, the definition's tokens, its survivor counts); the margins hold, or the rows are wrong."""
    temperature, opt = 0.5 if v == 4100 else 1.0, options(min_p, typical_p)
    x = {"head": lambda: rows(v, temperature, v), "dead": lambda: torch.full((3, v), -math.inf),
         "restream": lambda: restream_rows(v)}[kind]()
    cuts = []
    scored = ref.nucleus_scores(x, top_k, temperature, top_p, SEED, STEP, **opt, **(dict(cuts=cuts) if opt else {}))
    assert all(np.abs(val / thr - 1).min(initial=1) >= 1e-3 for val, thr in cuts)  # (no option: top-p's, checked with min_p)
    assert ni.leads(scored).min() >= 1e-4  # the draw itself is not a close call either
    tok = torch.tensor([int(i[np.argmax(s)]) for i, s in scored], dtype=torch.int32)
    return x, temperature, tok, torch.tensor([i.size for i, _ in scored], dtype=torch.int32)
