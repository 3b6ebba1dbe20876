"""Beam search fixtures: a literal per-item transcription of the definition (the README's "Beam search" section; lists
and loops, independent of ``ops/reference.py``), and a scripted model on which a whole search is known exactly.

The scripted model is ``loop_inputs``' (Hadamard embeddings, zero ``wo`` / ``w2``), with EIGHT successors per token
and token-dependent levels: after token x the logit of successor j, ``(5 x + 3 + 32 j) % 256``, is ``level(x, j)``:
per token 8 different multiples of 1/4 drawn from [4, 7.75], a different SET for every token, so rows have different
log-sum-exps and beams do not tie. Token END = 200 is offered by every row at the one level END_LEVEL = 6.625 (and
is nobody's regular successor): as ``eos`` it makes hypotheses finish at every length. Every other logit is exactly 0.
``output.weight`` entries are sums of eight +-level / 256, integers / 1024 of at most 248, and row END is
``END_LEVEL * e_0`` (the Hadamard rows add up to 256 e_0): all exact in bf16 (asserted).

Margins. The model's logits are the levels times one common factor within LOGIT_FACTOR = 1e-5 of 1
(``loop_inputs``), and the log-sum-exp of a row is computed in fp32. A score accumulated over n steps is therefore
off by at most ``score_bound(n)`` = n * (LOGIT_FACTOR * MAX_LEVEL + LSE_ERR): per step the candidate's logit moves by
at most LOGIT_FACTOR * MAX_LEVEL and the fp32 log-sum-exp by LSE_ERR = the summation bound (V + 2) * 2^-24 relative on
the sum of V non-negative terms (which is its absolute effect on the logarithm), plus 2^-16 for the roundings of
``mx + log(se)`` (below 16: half an ulp is 2^-21), of the two score additions per step (below 128: 2 * 2^-18) and the
last places of the exponentials and the logarithm (2^-21 + 2^-17 = 8.1e-6 < 2^-16 = 1.5e-5). Length penalties only
shrink it (inv_pen <= 1 for
length_penalty >= 0). Every comparison the scripted searches make between two real scores must have a margin of
4 * score_bound(n) (``host_search`` asserts it on every use); returned scores are compared within score_bound(n).
Comparisons that no rounding can turn are exempt: between entries carrying the -1e7 penalty and the pool's initial
-1e7 entries, which win every tie by coming first.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import loop_inputs as li
from jax_llama_amd.utils.checkpoint import random_meta_state_dict

V = li.V
NEG = np.float32(-1.0e7)
NSUCC = 8
MAX_LEVEL = 7.75
END, END_LEVEL = 200, 6.625  # the token every row offers at one fixed level (the scripted searches' eos)
LOGIT_FACTOR = 1e-5
LSE_ERR = (V + 2) * 2.0 ** -24 + 2.0 ** -16
F32 = np.float32


def score_bound(steps: int) -> float:
    return steps * (LOGIT_FACTOR * MAX_LEVEL + LSE_ERR)


def succ(x: int, j: int) -> int:
    return (5 * x + 3 + 32 * j) % V


def _level_table():
    """Per token, 8 distinct quarter-multiples drawn from the 16 values 4, 4.25 .. 7.75 by a Fisher-Yates shuffle on a
    fixed linear congruential stream: rows get different level SETS, hence different log-sum-exps."""
    state, table = 12345, []
    for _ in range(V):
        q = list(range(16, 32))
        for i in range(15, 0, -1):
            state = (1103515245 * state + 12345) % (1 << 31)
            r = (state >> 8) % (i + 1)
            q[i], q[r] = q[r], q[i]
        table.append([v / 4.0 for v in q[:NSUCC]])
    return table


_LEVELS = _level_table()


def level(x: int, j: int) -> float:
    """A multiple of 1/4 in [4, 7.75], different for every j of one x."""
    return _LEVELS[x][j]


def analytic_logits(tok) -> torch.Tensor:
    """fp32 [n, V]: the logits row after each token of ``tok``."""
    toks = [int(t) for t in torch.as_tensor(tok).reshape(-1).tolist()]
    out = torch.zeros(len(toks), V, dtype=torch.float32)
    for r, x in enumerate(toks):
        for j in range(NSUCC):
            if succ(x, j) != END:
                out[r, succ(x, j)] = level(x, j)
        out[r, END] = END_LEVEL
    return out


def state_dict(seed: int = 0) -> dict:
    cfg = li.config()
    sd = random_meta_state_dict(cfg, seed=seed)
    h = li.hadamard()
    a = torch.zeros(V, V, dtype=torch.float64)  # a[y, x]
    for x in range(V):
        lv = [level(x, j) for j in range(NSUCC)]
        assert len(set(lv)) == NSUCC and all(4.0 <= v <= MAX_LEVEL and v * 4 == int(v * 4) for v in lv)
        for j in range(NSUCC):
            if succ(x, j) != END:
                a[succ(x, j), x] = lv[j] / 256.0
        a[END, x] = END_LEVEL / 256.0  # the Hadamard rows add up to 256 e_0: output.weight[END] = END_LEVEL e_0
    assert int((a != 0).sum(1).min()) == NSUCC and int((a != 0).sum(1).max()) == V
    out = a @ h
    assert torch.equal(out.to(torch.bfloat16).double(), out)  # sums of eight +-level / 256: exact in bf16
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


def inv_pen_table(max_length: int, length_penalty: float):
    """fp32 list: 1 / t ** length_penalty in fp64, rounded once; entry 0 unused."""
    return [F32(1.0)] + [F32(1.0 / float(t) ** float(length_penalty)) for t in range(1, max_length + 1)]


def row_topk(row, k: int):
    """[(value, index)] of the k largest entries of a list of floats: value descending, ties to the lower index."""
    order = sorted(range(len(row)), key=lambda i: (-float(row[i]), i))[:k]
    return [(F32(row[i]), i) for i in order]


def row_lse(row) -> np.float32:
    x = np.asarray(row, dtype=np.float32)
    mx = x.max()
    return F32(mx + np.log(np.exp(x - mx).sum(dtype=np.float32), dtype=np.float32))


# ----------------------------------------------------------------------------------
# the definition, one batch item at a time
# ----------------------------------------------------------------------------------
class Item:
    """One batch item's search state: lists of K entries."""

    def __init__(self, prompt, k: int, max_length: int, pad: int):
        row = [int(t) for t in prompt] + [pad] * (max_length - len(prompt))
        self.running_seq = [list(row) for _ in range(k)]
        self.seq = [list(row) for _ in range(k)]
        self.running_score = [F32(0.0)] + [NEG] * (k - 1)
        self.score = [NEG] * k
        self.is_finished = [False] * k


def items_from_tensors(running_seq, seq, running_score, score, is_finished):
    """The per-item states of state tensors [B, K, ...] (fresh lists)."""
    items = []
    for i in range(running_seq.shape[0]):
        st = Item([0], running_seq.shape[1], running_seq.shape[2], 0)
        st.running_seq, st.seq = running_seq[i].tolist(), seq[i].tolist()
        st.running_score = [F32(x) for x in running_score[i].tolist()]
        st.score = [F32(x) for x in score[i].tolist()]
        st.is_finished = [bool(x) for x in is_finished[i].tolist()]
        items.append(st)
    return items


def random_step_inputs(seed: int, b: int, k: int, length: int, ties: bool, all_finished: bool = False):
    """(cand_v [B*K, 2K] sorted, cand_i, lse, running_seq, seq, running_score, score, is_finished) for one step.
    ``ties``: small integers everywhere, so that log-probs coincide across beams and ranks and scores in the pool;
    tokens are drawn from 12 ids (5 is the tests' eos). ``all_finished``: every slot of every item is finished."""
    g = torch.Generator().manual_seed(seed)
    k2 = 2 * k
    if ties:
        cv = torch.randint(-3, 3, (b * k, k2), generator=g).float()
        lse = torch.randint(0, 3, (b * k,), generator=g).float()
        rs = torch.randint(-4, 0, (b, k), generator=g).float()
        sc = torch.randint(-6, 0, (b, k), generator=g).float()
    else:
        cv = torch.randn(b * k, k2, generator=g) * 3
        lse = torch.randn(b * k, generator=g) + 5
        rs = -torch.rand(b, k, generator=g) * 10
        sc = -torch.rand(b, k, generator=g) * 10
    cv = cv.sort(-1, descending=True).values.contiguous()
    ci = torch.randint(0, 12, (b * k, k2), generator=g, dtype=torch.int32)
    rseq = torch.randint(0, 50, (b, k, length), generator=g, dtype=torch.int32)
    seq = torch.randint(0, 50, (b, k, length), generator=g, dtype=torch.int32)
    fin = torch.rand(b, k, generator=g) < 0.5
    if all_finished:
        fin[:] = True
    sc = torch.where(fin, sc, torch.tensor(-1.0e7))
    return cv, ci, lse, rseq, seq, rs, sc, fin


def _check_margin(margin, values, keep: int, old: int = 0):
    """``values``: scores in their kept order (all entries, kept ones first). Records the smallest gap between adjacent
    kept entries and between the last kept and the first dropped, exempting the comparisons no rounding can turn."""
    if margin is None:
        return
    for i in range(min(keep, len(values) - 1)):
        (va, ia), (vb, ib) = values[i], values[i + 1]
        if vb <= -1e6:  # the lower one carries the penalty: the upper one is real (gap 1e7) or an initial pool entry
            assert va > -1e6 or ia < old, (values, keep)
            continue
        margin["min"] = min(margin.get("min", math.inf), float(va) - float(vb))


def item_step(st: Item, cands, lses, c: int, s: int, eos: int, early, inv_pen, margin=None):
    """One step at cur_len = c. ``cands[j]``: beam j's sorted top-2K [(logit, token)]; ``lses[j]``: its log-sum-exp.
    Returns beam_idx (list of K parents) and the K next input tokens."""
    k = len(st.running_score)
    k2 = 2 * k
    flat = []  # (lp, j, n, token)
    for j in range(k):
        assert len(cands[j]) == k2
        for n, (val, tok) in enumerate(cands[j]):
            lp = F32(st.running_score[j] + F32(F32(val) - F32(lses[j])))
            flat.append((lp, j, n, int(tok)))
    flat.sort(key=lambda e: (-float(e[0]), e[1], e[2]))
    _check_margin(margin, [(e[0], 0) for e in flat], k2)
    top = flat[:k2]
    run = []  # (run_lp, candidate rank)
    fin = []  # (fin_lp, just_finished, candidate rank)
    all_fin = all(st.is_finished)
    for r, (lp, j, n, tok) in enumerate(top):
        just = tok == eos
        run.append((F32(NEG + lp) if just else lp, r))
        f = F32(lp * inv_pen[c + 1 - s])
        if (not just) or (all_fin and early is True):
            f = F32(f + NEG)
        fin.append((f, just, r))
    run.sort(key=lambda e: (-float(e[0]), e[1]))
    if margin is not None:
        assert run[k - 1][0] > -1e6, "fewer than K candidates without eos"
    _check_margin(margin, [(e[0], 0) for e in run], k)

    def cand_seq(r):
        lp, j, n, tok = top[r]
        row = list(st.running_seq[j])
        row[c] = tok
        return row

    new_running_seq = [cand_seq(r) for _, r in run[:k]]
    new_running_score = [v for v, _ in run[:k]]
    beam_idx = [top[r][1] for _, r in run[:k]]
    tokens = [top[r][3] for _, r in run[:k]]
    merged = [(st.score[j], st.is_finished[j], list(st.seq[j]), j) for j in range(k)]
    merged += [(f, just, cand_seq(r), k + r) for f, just, r in fin]
    merged.sort(key=lambda e: (-float(e[0]), e[3]))
    _check_margin(margin, [(e[0], e[3]) for e in merged], k, old=k)
    st.running_seq, st.running_score = new_running_seq, new_running_score
    st.seq = [e[2] for e in merged[:k]]
    st.score = [e[0] for e in merged[:k]]
    st.is_finished = [bool(e[1]) for e in merged[:k]]
    return beam_idx, tokens


def search_continues(items, c: int, s: int, max_length: int, early, length_penalty: float, inv_pen) -> bool:
    if not c < max_length:
        return False
    if early is True and all(all(st.is_finished) for st in items):
        return False
    if c == s:
        return True
    d = max_length - s if (early == "never" and length_penalty > 0.0) else c - s
    for st in items:
        best_running = F32(st.running_score[0] * inv_pen[d])
        worst_finished = min(st.score) if any(st.is_finished) else NEG
        if best_running > worst_finished:
            return True
    return False


def search_result(items, nrs: int):
    seqs, scores = [], []
    for st in items:
        fin = any(st.is_finished)
        for r in range(nrs):
            seqs.append((st.seq if fin else st.running_seq)[r])
            scores.append((st.score if fin else st.running_score)[r])
    return torch.tensor(seqs, dtype=torch.int32), torch.tensor(np.asarray(scores, dtype=np.float32))


def host_search(prompt: torch.Tensor, k: int, max_length: int, pad: int, eos: int, length_penalty: float = 1.0,
                early=False, nrs: int = 1, margin=None, trace=None):
    """The whole search on the scripted model: (sequences int32 [B*nrs, L], scores fp32 [B*nrs], steps run). With a
    ``margin`` dict the smallest real-score gap of any comparison lands in ``margin["min"]``; ``trace`` (a list)
    receives per step ``(c, [per item (beam_idx, is_finished after, score after)])``."""
    b, s = prompt.shape
    items = [Item(prompt[i].tolist(), k, max_length, pad) for i in range(b)]
    inv_pen = inv_pen_table(max_length, length_penalty)
    last = [[int(prompt[i, -1])] * k for i in range(b)]
    c, steps = s, 0
    while search_continues(items, c, s, max_length, early, length_penalty, inv_pen):
        rec = []
        for i, st in enumerate(items):
            rows = analytic_logits(last[i]).tolist()
            wide = [row_topk(rows[j], 2 * k + 1) for j in range(k)]
            cands = [w[:2 * k] for w in wide]
            lses = [row_lse(rows[j]) for j in range(k)]
            if margin is not None:  # the per-row top-2K: the levels of one row are 1/8 apart or more
                assert all(float(w[n][0]) - float(w[n + 1][0]) >= 0.125 for w in wide for n in range(2 * k))
            beam_idx, last[i] = item_step(st, cands, lses, c, s, eos, early, inv_pen, margin)
            rec.append((beam_idx, list(st.is_finished), list(st.score)))
        if trace is not None:
            trace.append((c, rec))
        c += 1
        steps += 1
    seqs, scores = search_result(items, nrs)
    return seqs, scores, steps


def guarded_host_search(prompt, k, max_length, pad, eos, length_penalty=1.0, early=False, nrs=1, trace=None):
    """``host_search`` asserting the 4 x score_bound margin on every comparison; also returns score_bound(steps)."""
    m = {}
    seqs, scores, steps = host_search(prompt, k, max_length, pad, eos, length_penalty, early, nrs, margin=m,
                                      trace=trace)
    bound = score_bound(max_length - prompt.shape[1])
    assert m["min"] >= 4 * bound, (m, bound)
    return seqs, scores, bound


# ----------------------------------------------------------------------------------
# the scripted cases: prompts found by a CPU search over last tokens (host_search with its margins, eos = END or none)
# so that every comparison of every listed run keeps 4 x score_bound; test_beam_cpu.py checks what each case is said
# to hit
# ----------------------------------------------------------------------------------
S, MAX_LENGTH, PAD = 6, 16, 0
LENGTHS = [2, 6, 4]
LAST_TOKENS = {2: [255, 201, 17], 4: [70, 64, 70]}
# name -> (K, eos, length_penalty, early_stopping)
CASES = {
    "k2_lp1": (2, END, 1.0, False),      # beams finish mid-run while others go on; finished hypotheses are displaced
    "k2_lp0": (2, END, 0.0, False),      # length_penalty 0 / 1 / 2: three different winners; 0 ends after 6 steps
    "k2_lp2": (2, END, 2.0, False),
    "k2_early": (2, END, 1.0, True),     # ends after 5 of the 10 steps
    "k2_lp05": (2, END, 0.5, False),     # 7 steps ...
    "k2_never": (2, END, 0.5, "never"),  # ... and 8
    "k2_no_eos": (2, -1, 1.0, False),    # runs to max_length with nothing finished
    "k4_lp1": (4, END, 1.0, False),
    "k4_lp0": (4, END, 0.0, False),
    "k4_early": (4, END, 1.0, True),
    "k4_no_eos": (4, -1, 1.0, False),
}


def batch(last_tokens, pad: int = PAD):
    """3 left-padded prompts of S tokens ending in ``last_tokens``."""
    return li.prompts(last_tokens, LENGTHS, S, pad, seed=11)


_HOST = {}


def case(name: str, nrs: int = 1):
    """(prompts, mask, K, eos, length_penalty, early_stopping, host sequences, host scores, score bound, steps, trace)
    of a scripted case; the guarded host search runs once per (case, nrs)."""
    k, eos, lp, early = CASES[name]
    toks, mask = batch(LAST_TOKENS[k])
    if (name, nrs) not in _HOST:
        trace = []
        seqs, scores, bound = guarded_host_search(toks, k, MAX_LENGTH, PAD, eos, lp, early, nrs, trace=trace)
        _HOST[(name, nrs)] = (seqs, scores, bound, len(trace), trace)
    return (toks, mask, k, eos, lp, early) + _HOST[(name, nrs)]
