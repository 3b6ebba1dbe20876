"""The logits processors (the README's "Logits processors" section) written out on the host in lists and loops,
independent of ``ops/reference.py``; the decode loop of tests/loop_inputs.py with that definition before the pick and a
stop set; the rows the kernel is compared on; and the scripted scenarios of the engine tests.

Plain host code: tests/test_logits_proc_cpu.py checks ``ops/reference.py`` and the CPU engine against it, and
tests/test_logits_proc_gpu.py the HIP kernel (against the reference) and the graph-replaying engine (against the loop).

The scenarios run on ``loop_inputs.state_dict(SAMPLE_LEVELS)``: after token x the logits are 8 / 7 / 6 / 5 at the four
successors of x and 0 elsewhere, so only a prompt's last token decides the unprocessed greedy path P_0, P_1, ... The
rest of the prompt is free to plant tokens and bigrams of that path, which makes a processor change the pick at a
chosen step: a penalty of 1.25 turns the 8 into 6.4, below the 7; a banned token leaves the 7 on top. Every scenario
has a second variant for the one-engine-two-runs tests; ``two_runs`` asserts that each value an engine might keep from
the first run (``STALE``) would change the second run's tokens."""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

import loop_inputs as li
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime.engine import GenerationConfig

I32 = torch.int32
V = li.V
NEG_INF = np.float32(-np.inf)
GAP_MIN = 0.1  # greedy scenarios: the two largest processed logits of every unfinished row, at every step


# ----------------------------------------------------------------------------------
# the definition, in lists and loops
# ----------------------------------------------------------------------------------
@dataclass
class Proc:
    """One call's settings, as GenerationConfig names them. ``stop`` is the stop set (eos_token_id as a list)."""

    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    min_length: int = 0
    min_new_tokens: int = 0
    suppress_tokens: list = field(default_factory=list)
    stop: list = field(default_factory=list)

    def min_len(self, s: int) -> int:
        return max(self.min_length, s + self.min_new_tokens)


def process_row(row, hist, cur_len: int, col_offset: int, vocab: int, p: float, n: int, suppress, stop, min_len: int):
    """``row``: the np.float32 logits of columns [col_offset, col_offset + len(row)); ``hist``: the history's token
    ids, oldest first. Returns the processed row (a new list)."""
    row = list(row)
    v = len(row)

    def ban(t):
        if 0 <= t < vocab and 0 <= t - col_offset < v:
            row[t - col_offset] = NEG_INF

    if p != 1.0:
        pen, inv = np.float32(p), np.float32(1.0 / p)  # the quotient in fp64, rounded once
        seen = set()
        for t in hist:
            if t < 0 or t >= vocab or t in seen:
                continue
            seen.add(t)
            c = t - col_offset
            if 0 <= c < v:
                row[c] = row[c] * inv if row[c] > 0 else row[c] * pen
    if n >= 1 and len(hist) >= n:
        suffix = hist[len(hist) - n + 1:]
        for i in range(len(hist) - n + 1):
            if hist[i:i + n - 1] == suffix:
                ban(hist[i + n - 1])
    for t in suppress:
        ban(t)
    if cur_len < min_len:
        for t in stop:
            ban(t)
    return row


def process(logits: torch.Tensor, sequences: torch.Tensor, cur_len: int, hist_start, col_offset: int, vocab: int,
            p: float, n: int, suppress, stop, min_len: int) -> torch.Tensor:
    """fp32 [B, V_local]: ``process_row`` on every row over ``sequences[b, hist_start[b] : cur_len]``."""
    x = logits.numpy().astype(np.float32)
    out = np.empty_like(x)
    for b in range(x.shape[0]):
        hist = [int(t) for t in sequences[b, int(hist_start[b]):cur_len].tolist()]
        out[b] = np.array(process_row(list(x[b]), hist, cur_len, col_offset, vocab, p, n, list(suppress), list(stop),
                                      min_len), dtype=np.float32)
    return torch.from_numpy(out)


def first_attended(mask: torch.Tensor) -> list:
    """Per row: the first prompt column whose mask is 1; S for a fully masked row."""
    out = []
    for row in mask.tolist():
        out.append(row.index(1) if 1 in row else len(row))
    return out


# ----------------------------------------------------------------------------------
# the decode loop with processors and a stop set
# ----------------------------------------------------------------------------------
def host_generate(levels, prompt: torch.Tensor, mask: torch.Tensor, max_length: int, pad: int, proc: Proc,
                  sample=None, stats: Optional[dict] = None, hist_start=None, min_len=None) -> torch.Tensor:
    """``loop_inputs.host_generate`` with the definition applied before every pick (the prefill's included, where
    ``cur_len = S``) and ``finished |= token in proc.stop``. ``stats`` receives the smallest gap between the two
    largest processed logits of an unfinished row (greedy) or the sampler's margins (``sample``). ``hist_start`` /
    ``min_len``: these history starts / this minimum-length word instead of the call's own (``stale_sensitivity``)."""
    b, s = prompt.shape
    seq = torch.full((b, max_length), pad, dtype=I32)
    seq[:, :s] = prompt
    start = first_attended(mask) if hist_start is None else list(hist_start)
    word = proc.min_len(s) if min_len is None else min_len
    finished = torch.zeros(b, dtype=torch.bool)
    tok = prompt[:, -1].to(I32)
    cur = s
    while cur < max_length and not bool(finished.all()):
        logits = process(li.analytic_logits(tok, levels), seq, cur, start, 0, V, proc.repetition_penalty,
                         proc.no_repeat_ngram_size, proc.suppress_tokens, proc.stop, word)
        live = ~finished
        if sample is None:
            nxt = logits.argmax(-1).to(I32)
            if stats is not None:
                top2 = torch.topk(logits, 2, dim=-1).values
                stats["gap"] = min(stats.get("gap", math.inf), float((top2[:, 0] - top2[:, 1])[live].min()))
        else:
            k, temperature, top_p, seed = sample
            nxt, lead, dist = li.sample_detail(logits, min(k, V), temperature, top_p, seed, cur)
            assert torch.equal(nxt, ref.topk_sample(logits, min(k, V), temperature, top_p, seed, cur))
            if stats is not None:
                stats["lead"] = min(stats.get("lead", math.inf), float(lead[live].min()))
                stats["top_p"] = min(stats.get("top_p", math.inf), float(dist[live].min()))
        nxt = torch.where(finished, torch.full_like(nxt, pad), nxt)
        finished |= torch.tensor([int(t) in proc.stop for t in nxt.tolist()])
        seq[:, cur] = nxt
        tok = nxt
        cur += 1
    return seq


# ----------------------------------------------------------------------------------
# scripted scenarios
# ----------------------------------------------------------------------------------
def path(last: int, n: int) -> list:
    """The unprocessed greedy path P_0 .. P_{n-1} after a prompt ending in ``last``."""
    out = []
    for _ in range(n):
        last = int(li.succ(last))
        out.append(last)
    return out


def planted(rows, s: int, pad: int):
    """Left-padded prompts [B, s] and their mask from explicit token lists."""
    toks = torch.full((len(rows), s), pad, dtype=I32)
    mask = torch.zeros(len(rows), s, dtype=I32)
    for i, r in enumerate(rows):
        assert 1 <= len(r) <= s
        toks[i, s - len(r):] = torch.tensor(r, dtype=I32)
        mask[i, s - len(r):] = 1
    return toks, mask


@dataclass
class Scenario:
    toks: torch.Tensor
    mask: torch.Tensor
    pad: int
    proc: Proc
    max_length: int
    sample: Optional[tuple] = None


LASTS = (5, 9, 130)   # the rows' last prompt tokens (row 0's path runs into row 1's after four tokens)
FILL = (251, 252, 253, 254, 255, 250, 249)  # prompt filler: on no row's processed or unprocessed path
S, GEN = 8, 14
# the sampled scenario's top_k, temperature, top_p and seed; the seed was searched on the CPU so that every draw of
# both batch sizes and both variants keeps loop_inputs' margins (expected() asserts them on every use)
SAMPLE = (50, 1.0, 0.9, 4)


def _rows(b: int):
    return list(range(3)) if b == 3 else [1]


def scenario(name: str, b: int, variant: int = 0) -> Scenario:
    """``variant`` 1: the second run of the one-engine-two-runs tests: a shorter prompt with other history starts, and
    other settings chosen so that run 1's value of each would give other tokens (``stale_sensitivity``)."""
    rows = _rows(b)
    s = S - 2 * variant
    # variant 0: row 0 fills the prompt, rows 1 and 2 are left-padded (history starts 0, 2, 1); variant 1: row 1 fills
    # it (starts 1, 0, 2), so run 1's starts would drop the first two tokens of its history
    lens = {0: s - 1, 1: s, 2: s - 2} if variant else {0: s, 1: s - 2, 2: s - 1}
    when = {0: 4 - variant, 1: 0 + 3 * variant, 2: 5}  # the generated position where the processor first acts
    pad, proc, sample, prompts = 0, Proc(), None, []
    n_gram = 3 if variant else 2
    for r in rows:
        # (stop_set, and min_new's second run: row 2 ends like row 0, so that it meets a stop id too)
        twin = r == 2 and (name == "stop_set" or (name == "min_new" and variant))
        last, k = LASTS[0 if twin else r], when[r]
        pth = path(last, 20)
        body = list(FILL[:lens[r] - 1])
        if name in ("penalty", "sampled") or (name == "all" and not variant):
            body[0] = pth[k]  # P_k is history: its 8 becomes 6.4 (1.25) or 5.33 (1.5)
            if name == "penalty" and variant:
                # the 7 at step k is history too: 1.5 leaves the 6 on top (5.33, 4.67), run 1's 1.25 the 6.4
                body[1] = int(li.succ(pth[k - 1], 1))
        elif name == "ngram" or (name == "all" and variant and r < 2):
            # the n-gram (.., P_{k-1}, P_k) has occurred: P_k is banned at step k (variant 1: n = 3, k >= 2; run 1's
            # n = 2 would ban P_{k-1} a step earlier, and in "all" run 1's 1.25 would move the pick at step k - 2, while
            # 1.1 keeps every planted token on top: 7.27 against 7)
            gram = ([last] + pth)[k + 2 - n_gram:k + 2]
            body[:n_gram] = gram
        prompts.append(body + [last])
    toks, mask = planted(prompts, s, pad)
    if name == "penalty":
        proc = Proc(repetition_penalty=1.5 if variant else 1.25)
        if b == 3 and not variant:
            # row 1's padding is the third token it generates (its first pick moves to successor 1, then it follows
            # successor 0 again): padding is not history, or that token's 8 would be 6.4
            pad = int(li.succ(li.succ(li.succ(LASTS[1], 1))))
            toks, mask = planted(prompts, s, pad)
    elif name == "ngram":
        proc = Proc(no_repeat_ngram_size=n_gram)
    elif name == "min_new" and not variant:
        # eos = P_k of every row: unprocessed, row r stops at its generated position k
        proc = Proc(min_new_tokens=7, stop=sorted(path(LASTS[r], 20)[when[r]] for r in rows))
    elif name == "min_new":
        # the minimum-length word is 9 (run 1: 15). Every row's third token is a stop id, banned at cur_len 8; so is
        # the token X that the first row then generates at cur_len 12: it finishes there, where run 1's word bans X
        proc = Proc(min_new_tokens=3, stop=sorted({path(LASTS[0 if r == 2 else r], 20)[2] for r in rows}))
        proc.stop = sorted(proc.stop + [_token_at(toks, mask, pad, proc, s + 6)])
    elif name == "stop_set":
        ids = [path(LASTS[r], 20)[when[r] + 1] for r in rows[:2]]
        proc = Proc(stop=sorted(ids + ([FILL[6]] if len(ids) < 2 else [])))  # always two ids
    elif name == "suppress":
        proc = Proc(suppress_tokens=[path(LASTS[r], 20)[2 + variant] for r in rows])
    elif name == "all" and not variant:
        proc = Proc(repetition_penalty=1.25, no_repeat_ngram_size=2, min_new_tokens=9,
                    suppress_tokens=[int(li.succ(path(LASTS[rows[0]], 20)[0], 1))],
                    stop=[path(LASTS[r], 20)[7] for r in rows][:2])
    elif name == "all":
        # 1.1 and n = 3 on planted trigrams (above); the last row's first token is suppressed and its next one, Y, a
        # stop id banned at cur_len 7 < 9; X as in min_new: the first row finishes at cur_len 12 (run 1's word: 17)
        sup, y = (int(li.succ(LASTS[2])), int(li.succ(li.succ(LASTS[2], 1)))) if 2 in rows else FILL[5:7]
        proc = Proc(repetition_penalty=1.1, no_repeat_ngram_size=3, min_new_tokens=3, suppress_tokens=[sup], stop=[y])
        proc.stop = sorted(proc.stop + [_token_at(toks, mask, pad, proc, s + 6)])
    elif name == "sampled":
        proc = Proc(repetition_penalty=1.5 if variant else 1.25, no_repeat_ngram_size=2)
        sample = SAMPLE
    else:
        raise KeyError(name)
    return Scenario(toks, mask, pad, proc, S + GEN, sample)


def _token_at(toks, mask, pad, proc: Proc, col: int) -> int:
    """The token the first row holds at column ``col`` in the greedy host loop under ``proc``."""
    return int(host_generate(li.SAMPLE_LEVELS, toks, mask, S + GEN, pad, proc)[0, col])


def generation_config(sc: Scenario, single_eos=None) -> GenerationConfig:
    """The scenario as the engine takes it: ``eos_token_id`` is the stop list (``single_eos``: that value instead)."""
    p = sc.proc
    eos = list(p.stop) if p.stop else -1
    kw = dict(max_length=sc.max_length, pad_token_id=sc.pad, eos_token_id=eos if single_eos is None else single_eos,
              repetition_penalty=p.repetition_penalty, no_repeat_ngram_size=p.no_repeat_ngram_size,
              min_length=p.min_length, min_new_tokens=p.min_new_tokens, suppress_tokens=list(p.suppress_tokens) or None)
    if sc.sample is not None:
        k, t, tp, seed = sc.sample
        kw.update(do_sample=True, top_k=k, temperature=t, top_p=tp, seed=seed)
    return GenerationConfig(**kw)


GREEDY_SCENARIOS = ("penalty", "ngram", "min_new", "stop_set", "suppress", "all")


def expected(sc: Scenario) -> torch.Tensor:
    """The scenario's tokens by the host loop, after asserting that it tests what it claims: the processed run
    differs from the unprocessed one in at least 3 generated positions of every row, one of them the 4th generated
    token or later (a graph-replayed step), and no pick is a near tie."""
    s = sc.toks.shape[1]
    stats = {}
    want = host_generate(li.SAMPLE_LEVELS, sc.toks, sc.mask, sc.max_length, sc.pad, sc.proc, sc.sample, stats)
    plains = [li.host_generate(li.SAMPLE_LEVELS, sc.toks, sc.mask, sc.max_length, sc.pad, -1, sc.sample)]
    if sc.proc.stop and dataclasses.replace(sc.proc, stop=[]) != Proc():
        # processors and a stop set: also against the run that has the stop set alone
        plains.append(host_generate(li.SAMPLE_LEVELS, sc.toks, sc.mask, sc.max_length, sc.pad,
                                    Proc(stop=sc.proc.stop), sc.sample))
    for plain in plains:
        diff = want[:, s:] != plain[:, s:]
        assert bool((diff.sum(1) >= 3).all()), diff.sum(1).tolist()
        assert bool(diff[:, 3:].any(1).all())
    if sc.sample is None:
        assert stats["gap"] >= GAP_MIN, stats
    else:
        assert stats["lead"] >= li.LEAD_MIN and stats["top_p"] >= li.TOP_P_MIN, stats
    return want


# what of run 1 must change run 2's tokens, per two-run scenario (stale_sensitivity may find more)
STALE = {"penalty": {"repetition_penalty", "hist_start"}, "ngram": {"no_repeat_ngram_size", "hist_start"},
         "min_new": {"min_len", "stop"}, "stop_set": {"stop"}, "suppress": {"suppress_tokens"},
         "all": {"repetition_penalty", "no_repeat_ngram_size", "min_len", "hist_start", "stop", "suppress_tokens"},
         "sampled": {"repetition_penalty"}}


def stale_sensitivity(first: Scenario, second: Scenario) -> set:
    """What an engine that kept a value of run 1 would get wrong in run 2: the names among the by-value launch
    arguments (repetition_penalty, no_repeat_ngram_size) and the engine-owned device words (hist_start, min_len, stop,
    suppress_tokens) whose run-1 value, put in place of run 2's, changes run 2's host-loop tokens."""
    def run(proc=second.proc, **kw):
        return host_generate(li.SAMPLE_LEVELS, second.toks, second.mask, second.max_length, second.pad, proc,
                             second.sample, **kw)
    want, out = run(), set()
    for name in ("repetition_penalty", "no_repeat_ngram_size", "stop", "suppress_tokens"):
        if not torch.equal(run(dataclasses.replace(second.proc, **{name: getattr(first.proc, name)})), want):
            out.add(name)
    if not torch.equal(run(hist_start=first_attended(first.mask)), want):
        out.add("hist_start")
    if not torch.equal(run(min_len=first.proc.min_len(first.toks.shape[1])), want):
        out.add("min_len")
    return out


def two_runs(name: str):
    """(first, its tokens, second, its tokens) of a two-run scenario at B = 3, after asserting each run's conditions
    (``expected``) and that run 2 cannot pass with run 1's values: same (B, max_length), another prompt length, other
    history starts, a stop list of the same length, and STALE[name] within ``stale_sensitivity``."""
    first, second = scenario(name, 3, 0), scenario(name, 3, 1)
    want1, want2 = expected(first), expected(second)
    assert first.max_length == second.max_length and first.toks.shape[1] != second.toks.shape[1]
    assert all(a != b for a, b in zip(first_attended(first.mask), first_attended(second.mask)))
    assert len(first.proc.stop) == len(second.proc.stop)
    found = stale_sensitivity(first, second)
    assert STALE[name] <= found, (name, sorted(STALE[name] - found))
    return first, want1, second, want2


# ----------------------------------------------------------------------------------
# rows for the kernel against the reference
# ----------------------------------------------------------------------------------
def kernel_case(b: int, v: int, hist_len: int, start: int = 2, kind: str = "random", col_offset: int = 0,
                vocab: Optional[int] = None, seed: int = 0):
    """(logits fp32 [b, v], sequences int32 [b, L], cur_len, hist_start int32 [b]). The history of row r is
    ``sequences[r, start + r % 2 : cur_len]``; its tokens are drawn from [col_offset - 40, col_offset + v + 40) within
    the vocabulary (``kind`` "random"), all equal ("same") or two alternating ("two"), with two ids outside the
    vocabulary planted in longer histories. Logits at history tokens include 2.5, -2.5, +0.0, -0.0 and -inf."""
    vocab = col_offset + v if vocab is None else vocab
    g = torch.Generator().manual_seed(seed * 7919 + b * 31 + v + hist_len)
    cur_len = start + 1 + hist_len
    length = cur_len + 3
    lo, hi = max(0, col_offset - 40), min(vocab, col_offset + v + 40)
    seq = torch.randint(lo, hi, (b, length), generator=g, dtype=I32)
    hist_start = torch.tensor([start + r % 2 for r in range(b)], dtype=I32)
    if kind == "same":
        seq[:] = seq[:, :1]
    elif kind == "two":
        seq[:, 1::2] = seq[:, 1:2]
        seq[:, 0::2] = seq[:, 0:1]
    elif hist_len >= 8:
        seq[:, start + 3] = vocab + 5  # out of range: skipped
        seq[:, start + 5] = -3
        if hist_len >= 24:  # the last four tokens have occurred before: n = 2 .. 5 ban the token that followed them
            seq[:, start + 8:start + 12] = seq[:, cur_len - 4:cur_len]
        if hist_len >= 48:  # both edges of the shard (unsharded: the bitmap's first and last bits)
            edges = torch.cat([torch.arange(col_offset - 8, col_offset + 8),
                               torch.arange(col_offset + v - 8, col_offset + v + 8)]).clamp(0, vocab - 1)
            seq[:, start + 14:start + 46] = edges.to(I32)
    x = torch.randn(b, v, generator=g) * 3
    special = torch.tensor([2.5, -2.5, 0.0, -0.0, float("-inf")])
    for r in range(b):
        cols = [int(t) - col_offset for t in seq[r, int(hist_start[r]):cur_len].tolist()]
        cols = [c for c in dict.fromkeys(cols) if 0 <= c < v][:8]
        for i, c in enumerate(cols):
            x[r, c] = special[i % 5]
    return x, seq, cur_len, hist_start
