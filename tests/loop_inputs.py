"""A scripted model whose generated tokens are known exactly, and a plain host transcription of the decode loop, so
that the sampler, the loop-state kernel and the graph-replaying engine are compared token for token (``torch.equal``)
instead of by agreement rates.

Plain host code (CPU tensors, numpy); ``tests/test_loop_cpu.py`` validates it against the CPU model path, the fp32
oracle and ``ops/reference.py``, and ``tests/test_loop_gpu.py`` runs the HIP kernels and the engine against it.

The model (``gpu_config(vocab_size=256, hidden_size=256)``, Meta layout):
  * ``tok_embeddings`` = the 256 rows of the Sylvester Hadamard matrix (+-1, mutually orthogonal; the RMS of a row is
    1, and ``1 / sqrt(1 + eps)`` rounds to 1 in bf16, so the normed row is the row);
  * every ``wo`` and ``w2`` is zero and every norm weight one: the residual stream stays the embedding of the current
    token while attention and the MLP still run on random ``wq / wk / wv / w1 / w3``;
  * ``output.weight[y] = sum_x a(y, x) * H[x]`` with ``a(y, x) = level / 256`` for the successors y of x: the logits
    row after token x is ``level`` at the successors (times one common factor within 1e-5 of 1) and exactly 0
    elsewhere. Successor j of x is ``(5 x + 3 + 64 j) % 256``: j = 0 is a permutation with one 256-cycle, every token
    has one predecessor per level, and the entries of ``output.weight`` are sums of four +-level / 256 (bf16-exact).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from jax_llama_amd.ops import reference as ref
from jax_llama_amd.utils.checkpoint import random_meta_state_dict
from helpers import gpu_config

V = 256
GREEDY_LEVELS = (8,)
SAMPLE_LEVELS = (8, 7, 6, 5)
LEAD_MIN = 1e-2   # every scripted draw: winning Gumbel score - runner-up (the common logits factor moves it by 5e-5)
TOP_P_MIN = 1e-3  # every scripted draw: |exclusive cumulative probability - top_p| of every candidate
_INV5 = 205       # 5 * 205 = 1025 = 1 mod 256
# (top_k, temperature, top_p, seed) of the scripted sampling runs. top_p lies between the cumulative sums of the four
# levels among the top k (the other candidates are zeros of e^-8 each): 0.638, 0.872, 0.958 at k = 50, T = 1; 0.643,
# 0.880, 0.967 at k = 10; 0.763, 0.945, 0.989 at T = 0.7. The seeds were searched on the CPU so that every draw of
# sample_batch() up to max_length 26 keeps both margins (guarded_host_generate asserts them on every use).
SAMPLE_BASE = (50, 1.0, 0.9, 82)
# one engine, two runs: (first run, second run). top_k alone moves the cumulative sums only through the zeros' mass,
# so its pair puts top_p between the third sum at k = 50 (0.872: three candidates kept) and at k = 10 (0.880: two).
SAMPLE_PAIRS = {"seed": (SAMPLE_BASE, (50, 1.0, 0.9, 84)), "temperature": (SAMPLE_BASE, (50, 0.7, 0.9, 82)),
                "top_p": (SAMPLE_BASE, (50, 1.0, 0.75, 82)), "top_k": ((50, 1.0, 0.876, 82), (10, 1.0, 0.876, 82))}
SAMPLE_S = 6


def config():
    return gpu_config(vocab_size=V, hidden_size=V)


def hadamard(n: int = V) -> torch.Tensor:
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < n:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    assert h.shape[0] == n
    return h


def succ(x, j: int = 0):
    """Successor j of token(s) x."""
    return (5 * x + 3 + 64 * j) % V


def pred(y: int, n: int = 1) -> int:
    """The token from which n greedy steps (successor 0) lead to y."""
    for _ in range(n):
        y = ((y - 3) * _INV5) % V
    return y


def analytic_logits(tok: torch.Tensor, levels) -> torch.Tensor:
    """fp32 [B, V]: the logits row after each token of ``tok`` [B] (levels at the successors, 0 elsewhere)."""
    tok = tok.reshape(-1).long()
    out = torch.zeros(tok.numel(), V, dtype=torch.float32)
    for j, lv in enumerate(levels):
        out[torch.arange(tok.numel()), succ(tok, j)] = float(lv)
    return out


def state_dict(levels, seed: int = 0) -> dict:
    cfg = config()
    sd = random_meta_state_dict(cfg, seed=seed)
    h = hadamard()
    a = torch.zeros(V, V, dtype=torch.float64)  # a[y, x]
    x = torch.arange(V)
    for j, lv in enumerate(levels):
        a[succ(x, j), x] = lv / 256.0
    out = a @ h
    assert torch.equal(out.to(torch.bfloat16).double(), out)  # sums of a few +-level / 256: exact in bf16
    sd["tok_embeddings.weight"] = h.to(torch.bfloat16)
    sd["output.weight"] = out.to(torch.bfloat16)
    sd["norm.weight"] = torch.ones(V, dtype=torch.bfloat16)
    for i in range(cfg.num_hidden_layers):
        p = f"layers.{i}."
        sd[p + "attention.wo.weight"] = torch.zeros_like(sd[p + "attention.wo.weight"])
        sd[p + "feed_forward.w2.weight"] = torch.zeros_like(sd[p + "feed_forward.w2.weight"])
        sd[p + "attention_norm.weight"] = torch.ones(V, dtype=torch.bfloat16)
        sd[p + "ffn_norm.weight"] = torch.ones(V, dtype=torch.bfloat16)
    return sd


def prompts(last_tokens, lengths, s: int, pad: int, seed: int = 0):
    """Left-padded prompts [B, s] (int32) and their mask: row i has ``lengths[i]`` random tokens ending in
    ``last_tokens[i]`` (only the last token decides what the scripted model generates)."""
    g = torch.Generator().manual_seed(seed)
    b = len(lengths)
    toks = torch.full((b, s), pad, dtype=torch.int32)
    mask = torch.zeros(b, s, dtype=torch.int32)
    for i, n in enumerate(lengths):
        toks[i, s - n:] = torch.randint(0, V, (n,), generator=g, dtype=torch.int32)
        toks[i, -1] = int(last_tokens[i])
        mask[i, s - n:] = 1
    return toks, mask


def sample_batch(pad: int = 0):
    """The prompts of the scripted sampling runs: 3 left-padded rows of SAMPLE_S tokens."""
    return prompts([5, 9, 130], [2, 6, 4], SAMPLE_S, pad, seed=4)


def sampled_eos(sample, nth: int, max_length: int = 26) -> int:
    """The token row 0 of sample_batch() draws as its (nth + 1)-th new one in a run without eos."""
    toks, mask = sample_batch()
    return int(host_generate(SAMPLE_LEVELS, toks, mask, max_length, 0, -1, sample)[0, SAMPLE_S + nth])


# ----------------------------------------------------------------------------------
# the sampler's numbers, as ref.topk_sample computes them
# ----------------------------------------------------------------------------------
def sample_detail(logits: torch.Tensor, k: int, temperature: float, top_p: float, seed: int, step: int):
    """``ref.topk_sample``'s own arithmetic (fp32 numpy, the same Philox counters) with its margins: (token int32 [B],
    lead fp32 [B] = winning Gumbel score - runner-up (inf with one kept candidate), top_p distance fp32 [B] = the
    smallest |exclusive cumulative probability - top_p| over the candidates after the first, which is always kept)."""
    vals, idx = ref.topk_sorted(logits, k)
    v = vals.numpy().astype(np.float32) / np.float32(temperature)
    p = np.exp(v - v[:, :1])
    p = p / p.sum(-1, keepdims=True)
    excl = np.cumsum(p, -1) - p
    keep = excl < np.float32(top_p)
    keep[:, 0] = True
    b = v.shape[0]
    ctr = np.zeros((b, k, 4), dtype=np.uint32)
    ctr[..., 0] = np.arange(k, dtype=np.uint32)[None]
    ctr[..., 1] = np.arange(b, dtype=np.uint32)[:, None]
    ctr[..., 2] = np.uint32(step)
    r = ref.philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))[..., 0]
    u = ((r >> 8).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    score = np.where(keep, v - np.log(-np.log(u)), -np.inf)
    order = np.sort(score, -1)
    lead = order[:, -1] - order[:, -2] if k > 1 else np.full(b, np.inf, dtype=np.float32)
    dist = np.abs(excl[:, 1:] - np.float32(top_p)).min(-1) if k > 1 else np.full(b, np.inf, dtype=np.float32)
    tok = idx[torch.arange(b), torch.from_numpy(score.argmax(-1))].to(torch.int32)
    return tok, torch.from_numpy(np.asarray(lead, dtype=np.float32)), torch.from_numpy(np.asarray(dist, np.float32))


# ----------------------------------------------------------------------------------
# the decode loop, on the host (runtime/engine.py's docstring)
# ----------------------------------------------------------------------------------
def host_generate(levels, prompt: torch.Tensor, mask, max_length: int, pad: int, eos: int, sample=None,
                  margins=None) -> torch.Tensor:
    """int32 [B, max_length]. ``sample`` = (top_k, temperature, top_p, seed) or None for greedy. ``mask`` is unused
    (a left-padded or holed prompt changes which keys attention reads, not what the scripted model emits). With a
    ``margins`` dict, the smallest score lead and top_p distance over all draws of unfinished rows are recorded."""
    b, s = prompt.shape
    seq = torch.full((b, max_length), pad, dtype=torch.int32)
    seq[:, :s] = prompt
    finished = torch.zeros(b, dtype=torch.bool)
    tok = prompt[:, -1].to(torch.int32)
    cur = s
    while cur < max_length and not bool(finished.all()):
        logits = analytic_logits(tok, levels)
        if sample is None:
            nxt = logits.argmax(-1).to(torch.int32)
        else:
            k, temperature, top_p, seed = sample
            nxt = ref.topk_sample(logits, min(k, V), temperature, top_p, seed, cur)  # Philox step = cur_len before
            if margins is not None:
                t2, lead, dist = sample_detail(logits, min(k, V), temperature, top_p, seed, cur)
                assert torch.equal(t2, nxt)
                live = ~finished
                margins["lead"] = min(margins.get("lead", math.inf), float(lead[live].min()))
                margins["top_p"] = min(margins.get("top_p", math.inf), float(dist[live].min()))
        nxt = torch.where(finished, torch.full_like(nxt, pad), nxt)
        finished |= nxt == eos
        seq[:, cur] = nxt
        tok = nxt
        cur += 1
    return seq


def guarded_host_generate(prompt, mask, max_length, pad, eos, sample) -> torch.Tensor:
    """The sampled host loop, asserting the margins that make its tokens immune to last-place arithmetic."""
    m = {}
    seq = host_generate(SAMPLE_LEVELS, prompt, mask, max_length, pad, eos, sample, margins=m)
    assert m["lead"] >= LEAD_MIN and m["top_p"] >= TOP_P_MIN, (sample, m)
    return seq


# ----------------------------------------------------------------------------------
# the sampler against the true distribution
# ----------------------------------------------------------------------------------
def true_distribution(row: torch.Tensor, k: int, temperature: float, top_p: float):
    """fp64: (token ids of the keep set, their renormalised probabilities) of one logits row."""
    x = row.double().numpy()
    order = np.lexsort((np.arange(x.size), -x))[:k]
    v = x[order] / temperature
    p = np.exp(v - v[0])
    p /= p.sum()
    excl = np.cumsum(p) - p
    keep = excl < top_p
    keep[0] = True
    q = p[keep]
    return order[keep], q / q.sum()


def top_p_boundary_row() -> torch.Tensor:
    """fp32 [8]: tokens 1, 3, 4, 6 at 2.5, the rest -inf. With k = 4 and T = 1 every probability is exactly 1/4 in any
    arithmetic (exp(0) = 1, exp(-inf) = 0), so the mass before the third candidate is exactly 0.5."""
    row = torch.full((8,), float("-inf"))
    row[[1, 3, 4, 6]] = 2.5
    return row


def chi2_bound(df: int) -> float:
    """The 1 - 1e-6 quantile of chi-square(df) (Wilson-Hilferty at z = 4.75 without scipy)."""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(1.0 - 1e-6, df))
    except ImportError:
        c = 2.0 / (9.0 * df)
        return df * (1.0 - c + 4.75 * math.sqrt(c)) ** 3


def check_draws(draws: torch.Tensor, row: torch.Tensor, k: int, temperature: float, top_p: float):
    """``draws``: independent samples of one logits row. No token outside the fp64 keep set (exact), and Pearson's
    chi-square over the kept tokens (cells expecting fewer than 5 pooled) below the 1 - 1e-6 quantile. Returns
    (chi-square, df)."""
    ids, q = true_distribution(row, k, temperature, top_p)
    d = draws.reshape(-1).long().numpy()
    n = d.size
    assert np.isin(d, ids).all(), sorted(set(d.tolist()) - set(ids.tolist()))
    counts = np.array([(d == t).sum() for t in ids], dtype=np.float64)
    exp = q * n
    small = exp < 5
    obs_c, exp_c = list(counts[~small]), list(exp[~small])
    if small.any():
        obs_c.append(counts[small].sum())
        exp_c.append(exp[small].sum())
    obs_c, exp_c = np.array(obs_c), np.array(exp_c)
    df = len(exp_c) - 1
    chi = float(((obs_c - exp_c) ** 2 / exp_c).sum())
    if df >= 1:
        assert chi < chi2_bound(df), (chi, df, chi2_bound(df))
    return chi, df
