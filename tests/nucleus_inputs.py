"""Input builders for the full-vocabulary sampler's tests (plain host code, numpy).

Gap rows put the top-p boundary where last-place arithmetic cannot move it: ``c`` upper tokens at random positions
with random logits (the survivors), and below them the rest, ``n - c`` lower head tokens and a flat tail, shifted in
fp64 until the mass before the first token of the rest is ``top_p + d`` of Z (the mass of the top k) and the mass before
the last upper token is below ``top_p - d``. ``c = n`` whenever top-k reaches far enough into the tail for the tail
to stay below the head; otherwise top-k binds first and ``c = 3k/4`` of the head survive. ``d`` is 1e-3 where the last
survivor carries that much: among c survivors of similar mass it carries about ``top_p / c`` of Z, so ``d = min(1e-3,
0.4 * top_p * e_last / U)`` (U = the survivors' mass), 5e-5 at the largest head (5000). Against it stand the kernel's
mass granularity V * 2^-40 < 2e-7 and the fp32 error of ``exp(l - m)``: the logits stay within |l - m| < 20, so a mass
is off by less than 20 * 2^-23 = 3e-6 of itself, and so are the cumulative fractions: over a decade of slack."""
from __future__ import annotations

import math

import numpy as np
import torch

import loop_inputs as li
from jax_llama_amd.ops import reference as ref

def gap_rows(b: int, v: int, n: int, top_k: int, temperature: float, top_p: float, seed: int):
    """fp32 ``[b, v]`` rows and the survivor count ``c`` of every one of them (asserted here in fp64)."""
    rng = np.random.default_rng(seed)
    n = min(n, v - v // 8)
    k = v if not top_k else min(top_k, v)
    c = n if k - n >= n // 4 + 1 else max(1, 3 * min(k, n) // 4)
    inv_t = float(np.float32(1.0 / temperature))
    rows = np.empty((b, v), dtype=np.float32)
    for r in range(b):
        pos = rng.permutation(v)[:n]
        lu = 2.0 + 0.5 * rng.random(c)            # the survivors, in l = x * inv_t units
        lo = 0.5 * rng.random(n - c)              # lower head, before the shift
        tail0 = (lo.min() if lo.size else 1.0) - 1.0
        m = lu.max()
        e_u = np.exp(lu - m)
        d = min(1e-3, 0.4 * top_p * e_u.min() / e_u.sum())
        in_k = np.concatenate([np.sort(lo)[::-1][:k - c], np.full(max(0, k - n), tail0)])  # the rest inside top-k
        shift = math.log(e_u.sum() * (1.0 / (top_p + d) - 1.0) / np.exp(in_k - m).sum())
        assert (lo.max() if lo.size else tail0) + shift < lu.min(), "gap_rows: the rest does not fit below the head"
        x = np.full(v, (tail0 + shift) / inv_t)
        x[pos[:c]] = lu / inv_t
        x[pos[c:]] = (lo + shift) / inv_t
        rows[r] = x.astype(np.float32)
        l = np.sort(rows[r].astype(np.float64))[::-1][:k] * inv_t
        e = np.exp(l - l[0])
        before = (np.cumsum(e) - e) / e.sum()
        assert d >= 4e-5 and before[c - 1] < top_p - d and (c == k or before[c] > top_p + 0.9 * d), (d, c)
    return torch.from_numpy(rows), c


def leads(scored) -> np.ndarray:
    """The reference's own Gumbel lead per row of ``ref.nucleus_scores``: best score - runner-up (inf when alone)."""
    return np.array([np.diff(np.sort(s)[-2:])[0] if s.size > 1 else np.inf for _, s in scored])


def top_p_distance(logits: torch.Tensor, top_k: int, temperature: float, top_p: float) -> float:
    """The smallest |mass fraction before a rank - top_p| over the ranks after the first, over all rows (fp64)."""
    x = logits.double().numpy() * float(np.float32(1.0 / temperature))
    k = x.shape[1] if not top_k else min(top_k, x.shape[1])
    l = -np.sort(-x, axis=1)[:, :k]
    e = np.exp(l - l[:, :1])
    before = (np.cumsum(e, 1) - e) / e.sum(1, keepdims=True)
    return float(np.abs(before[:, 1:] - top_p).min())


def host_generate(prompt: torch.Tensor, max_length: int, pad: int, eos: int, sample, margins: dict) -> torch.Tensor:
    """``loop_inputs.host_generate`` on the scripted sampling model with ``ref.nucleus_sample`` as the sampler;
    ``margins`` records the smallest score lead and top_p distance over all draws."""
    k, temperature, top_p, seed = sample
    b, s = prompt.shape
    seq = torch.full((b, max_length), pad, dtype=torch.int32)
    seq[:, :s] = prompt
    finished = torch.zeros(b, dtype=torch.bool)
    tok = prompt[:, -1].to(torch.int32)
    for cur in range(s, max_length):
        logits = li.analytic_logits(tok, li.SAMPLE_LEVELS)
        nxt = ref.nucleus_sample(logits, k, temperature, top_p, seed, cur)  # Philox step = cur_len before
        lead = leads(ref.nucleus_scores(logits, k, temperature, top_p, seed, cur))[~finished.numpy()]
        margins["lead"] = min(margins.get("lead", math.inf), float(lead.min(initial=math.inf)))
        margins["top_p"] = min(margins.get("top_p", math.inf), top_p_distance(logits, k, temperature, top_p))
        nxt = torch.where(finished, torch.full_like(nxt, pad), nxt)
        finished |= nxt == eos
        seq[:, cur] = nxt
        tok = nxt
    return seq
