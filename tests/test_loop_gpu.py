"""What turns logits into output tokens, checked exactly on the MI355X: the loop-state kernel (``decode_update``)
against a plain transcription, the engine (eager and graph-replayed, one engine run twice with other settings) on the
scripted model of tests/loop_inputs.py against the host loop token for token, and the edges of the top-k / sampling /
argmax kernels against ``ops/reference.py``."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import loop_inputs as li
from jax_llama_amd import ops
from jax_llama_amd.models import LLaMAForCausalLM
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime import engine as eng_mod
from jax_llama_amd.runtime.engine import DecodeEngine, GenerationConfig
from jax_llama_amd.utils.checkpoint import meta_state_dict_to_params
from helpers import build, gpu_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32 = torch.int32
NO_INDEX = 0x7FFFFFFF  # the kernels' padding slot
_NEG_INF = float("-inf")


# ----------------------------------------------------------------------------------
# 3. decode_update
# ----------------------------------------------------------------------------------
def _update_reference(nxt, fin, seq, cur_len, tokens, positions, slot, pad, eos):
    """engine.py's docstring, transcribed: a finished row emits pad; finished |= token == eos; sequences[:, cur_len] =
    token where that column exists; the token is the next input; position, slot and cur_len advance by one."""
    t = torch.where(fin != 0, torch.full_like(nxt, pad), nxt)
    fin2 = ((fin != 0) | (t == eos)).to(I32)
    seq2 = seq.clone()
    cl = int(cur_len[0])
    if cl < seq.shape[1]:
        seq2[:, cl] = t
    return fin2, seq2, cur_len + 1, t.reshape(tokens.shape), positions + 1, slot + 1


def _update_state(b, length, cur, eos, flip, seed):
    g = torch.Generator().manual_seed(seed)
    nxt = torch.randint(0, 8, (b,), generator=g, dtype=I32)
    if eos >= 0:
        nxt[::3] = eos  # some rows draw eos, finished ones among them
    fin = (torch.rand(b, generator=g) < 0.4).to(I32)
    if flip:
        fin = 1 - fin
    seq = torch.randint(10, 99, (b, length), generator=g, dtype=I32)
    return [nxt, fin, seq, torch.tensor([cur], dtype=I32), torch.randint(0, 99, (b, 1), generator=g, dtype=I32),
            torch.randint(-5, 4000, (b, 1), generator=g, dtype=I32), torch.tensor([1234 + b], dtype=I32)]


@pytest.mark.parametrize("cur", [0, 7])
@pytest.mark.parametrize("pad,eos", [(2, 2), (0, 5), (0, -1)])
@pytest.mark.parametrize("b", [1, 63, 64, 65, 1024, 1025, 2500])
def test_decode_update_is_the_transcription(b, pad, eos, cur):
    """B around the launch's rounding to 64 threads, at its 1024-thread cap and in the stride loop past it; L = 8."""
    for flip in (False, True):  # every row once finished, once not (B = 1 included)
        host = _update_state(b, 8, cur, eos, flip, seed=b + cur)
        want = _update_reference(*host, pad, eos)
        dev = [t.to(DEV) for t in host]
        ops.ext().decode_update(*dev, pad, eos)
        torch.cuda.synchronize()
        got = [t.cpu() for t in dev[1:]]
        for name, g_, w_ in zip(("finished", "sequences", "cur_len", "tokens", "positions", "slot"), got, want):
            assert torch.equal(g_, w_), (name, flip)
        assert torch.equal(dev[0].cpu(), host[0])  # nxt is an input
        assert int(got[2][0]) == cur + 1 and int(got[5][0]) == int(host[6][0]) + 1
        if eos >= 0 and b >= 63:
            assert bool(((host[1] == 0) & (got[0] == 1)).any())  # a live row finished on its eos


@pytest.mark.parametrize("b", [3, 1025])
def test_decode_update_past_the_last_column_writes_no_token(b):
    """cur_len == L (the kernel's guarded path): no element of sequences changes, nor anything behind it, while the
    rest of the state advances. sequences is a [B, L] view at the front of a larger buffer of the test's own."""
    length, tail = 8, 256
    host = _update_state(b, length, length, 5, False, seed=b)
    want = _update_reference(*host, 0, 5)
    dev = [t.to(DEV) for t in host]
    buf = torch.full((b * length + tail,), -7, dtype=I32, device=DEV)
    buf[:b * length] = dev[2].reshape(-1)
    before = buf.clone()
    dev[2] = buf[:b * length].view(b, length)
    try:
        ops.ext().decode_update(*dev, 0, 5)
        torch.cuda.synchronize()
    finally:
        if ops.ext().DEBUG_BOUNDS:
            ops.bounds_error(reset=True)  # the bounds-checked build records this step: clear it for later tests
    assert torch.equal(buf, before)
    got = [t.cpu() for t in dev[1:]]
    for name, g_, w_ in zip(("finished", "sequences", "cur_len", "tokens", "positions", "slot"), got, want):
        assert torch.equal(g_, w_), name
    assert int(got[2][0]) == length + 1


# ----------------------------------------------------------------------------------
# 4. the engine on the scripted model
# ----------------------------------------------------------------------------------
_MODELS = {}


def _scripted(levels):
    if levels not in _MODELS:
        cfg = li.config()
        params = meta_state_dict_to_params(li.state_dict(levels), cfg.num_hidden_layers)
        _MODELS[levels] = LLaMAForCausalLM(cfg, device=DEV, _do_init=False).load_params(params)
    return _MODELS[levels]


def _gc(max_length, pad, eos, sample=None):
    if sample is None:
        return GenerationConfig(max_length=max_length, do_sample=False, pad_token_id=pad, eos_token_id=eos)
    k, t, p, seed = sample
    return GenerationConfig(max_length=max_length, do_sample=True, top_k=k, temperature=t, top_p=p, seed=seed,
                            pad_token_id=pad, eos_token_id=eos)


def _run(eng, toks, mask, gc):
    return eng.run(toks, mask, gc).cpu().to(I32)


GREEDY_S, GREEDY_EOS = 9, 200


def _greedy_batch(b, pad):
    """Row 0 emits eos as its first token, row 1 never within the run, the others after 2 .. 10 tokens; B = 1: 5."""
    steps = [5] if b == 1 else [1, 100] + [2 + i % 9 for i in range(b - 2)]
    lengths = [1 + (4 * i + 2) % GREEDY_S for i in range(b)]
    lengths[b // 2] = GREEDY_S
    return li.prompts([li.pred(GREEDY_EOS, n) for n in steps], lengths, GREEDY_S, pad, seed=b), steps


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("b", [1, 3, 20])
def test_engine_greedy_is_the_host_loop(monkeypatch, b, use_graph, fused):
    monkeypatch.setattr(eng_mod, "FUSED_GREEDY", fused)
    model = _scripted(li.GREEDY_LEVELS)
    max_length, pad = GREEDY_S + 14, 0
    (toks, mask), steps = _greedy_batch(b, pad)
    want = li.host_generate(li.GREEDY_LEVELS, toks, mask, max_length, pad, GREEDY_EOS)
    for row, n in enumerate(steps):  # the script does what the case says
        hit = (want[row, GREEDY_S:] == GREEDY_EOS).nonzero().reshape(-1).tolist()
        assert hit == ([n - 1] if n <= 14 else [])
    got = _run(DecodeEngine(model, b, max_length, use_graph=use_graph), toks, mask, _gc(max_length, pad, GREEDY_EOS))
    assert torch.equal(got, want)


def test_engine_greedy_fp8_kv_cache_is_the_host_loop():
    cfg = li.config()
    params = meta_state_dict_to_params(li.state_dict(li.GREEDY_LEVELS), cfg.num_hidden_layers)
    # its own model: the cache format is model state
    model = LLaMAForCausalLM(cfg, device=DEV, _do_init=False).load_params(params)
    model.set_kv_cache_format("fp8_e4m3")
    max_length, pad = GREEDY_S + 14, GREEDY_EOS
    (toks, mask), _ = _greedy_batch(3, pad)
    want = li.host_generate(li.GREEDY_LEVELS, toks, mask, max_length, pad, GREEDY_EOS)
    eng = DecodeEngine(model, 3, max_length, use_graph=True)
    assert eng.cache.kv_format == "fp8_e4m3"
    assert torch.equal(_run(eng, toks, mask, _gc(max_length, pad, GREEDY_EOS)), want)


@pytest.mark.parametrize("check_every", [1, 4, 1000])
def test_engine_early_exit(check_every):
    """Every row is finished after 3 steps: the sequences do not depend on when the host looks, with check_every 1
    and 4 the engine really stops, and the tail it never reached is pad."""
    model = _scripted(li.GREEDY_LEVELS)
    s, max_length, pad = GREEDY_S, GREEDY_S + 40, 7
    toks, mask = li.prompts([li.pred(GREEDY_EOS, n) for n in (1, 3, 2)], [4, 9, 1], s, pad, seed=5)
    want = li.host_generate(li.GREEDY_LEVELS, toks, mask, max_length, pad, GREEDY_EOS)
    eng = DecodeEngine(model, 3, max_length, use_graph=True, check_every=check_every)
    got = _run(eng, toks, mask, _gc(max_length, pad, GREEDY_EOS))
    assert torch.equal(got, want)
    assert torch.all(got[:, s + 3:] == pad)
    stopped = int(eng.cur_len.item())
    if check_every == 1000:
        assert stopped == max_length
    else:
        assert stopped == s + 1 + check_every * -(-2 // check_every)  # the first poll at or after the third token
        assert stopped < max_length


@pytest.mark.parametrize("extra,steps", [(1, 0), (2, 1)])
def test_engine_boundary_lengths(extra, steps):
    """max_length = S + 1: the prefill's token only, no decode step. S + 2: one step, eager (nothing is captured)."""
    model = _scripted(li.GREEDY_LEVELS)
    s, pad = GREEDY_S, 0
    (toks, mask), _ = _greedy_batch(3, pad)
    want = li.host_generate(li.GREEDY_LEVELS, toks, mask, s + extra, pad, -1)
    eng = DecodeEngine(model, 3, s + extra, use_graph=True)
    calls, step = [], eng._decode_step
    eng._decode_step = lambda: (calls.append(1), step())[1]
    got = _run(eng, toks, mask, _gc(s + extra, pad, -1))
    assert torch.equal(got, want)
    assert len(calls) == steps and eng._graph is None
    assert int(eng.cur_len.item()) == s + extra


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("eos_at,pad_is_eos", [(None, False), (2, False), (0, True)])
def test_engine_sampling_is_the_host_loop(use_graph, eos_at, pad_is_eos):
    """do_sample, top_k = 50, the guarded seed: the GPU engine draws the host loop's tokens (ref.topk_sample's)."""
    model = _scripted(li.SAMPLE_LEVELS)
    max_length = 26
    eos = -1 if eos_at is None else li.sampled_eos(li.SAMPLE_BASE, eos_at)
    pad = eos if pad_is_eos else 0
    toks, mask = li.sample_batch(pad)
    want = li.guarded_host_generate(toks, mask, max_length, pad, eos, li.SAMPLE_BASE)
    got = _run(DecodeEngine(model, 3, max_length, use_graph=use_graph), toks, mask,
               _gc(max_length, pad, eos, li.SAMPLE_BASE))
    assert torch.equal(got, want)


def _two_runs(model, levels, first, second, max_length):
    """One graph engine runs ``first`` then ``second`` (toks, mask, pad, eos, sample): each run is the host loop, and
    the second one also a fresh eager engine's."""
    b = first[0].shape[0]
    eng = DecodeEngine(model, b, max_length, use_graph=True)
    for i, (toks, mask, pad, eos, sample) in enumerate((first, second)):
        if sample is None:
            want = li.host_generate(levels, toks, mask, max_length, pad, eos)
        else:
            want = li.guarded_host_generate(toks, mask, max_length, pad, eos, sample)
        got = _run(eng, toks, mask, _gc(max_length, pad, eos, sample))
        assert torch.equal(got, want), ("first run", "second run")[i]
    assert eng._graph is not None
    fresh = _run(DecodeEngine(model, b, max_length, use_graph=False), toks, mask, _gc(max_length, pad, eos, sample))
    assert torch.equal(got, fresh)


def test_one_engine_two_runs_other_eos():
    """The second prompt meets the second eos mid-run, 8 tokens in, and never the first run's."""
    model = _scripted(li.GREEDY_LEVELS)
    t1, m1 = li.prompts([li.pred(200, 3), li.pred(200, 100)], [4, 6], 6, 0, seed=1)
    t2, m2 = li.prompts([li.pred(77, 8), li.pred(77, 100)], [6, 2], 6, 0, seed=2)
    assert int(li.host_generate(li.GREEDY_LEVELS, t2, m2, 26, 0, 77)[0, 6 + 7]) == 77
    _two_runs(model, li.GREEDY_LEVELS, (t1, m1, 0, 200, None), (t2, m2, 0, 77, None), 26)


def test_one_engine_two_runs_other_pad():
    model = _scripted(li.GREEDY_LEVELS)
    t1, m1 = li.prompts([li.pred(200, 3), li.pred(200, 100)], [4, 6], 6, 0, seed=1)
    t2, m2 = li.prompts([li.pred(200, 6), li.pred(200, 100)], [6, 2], 6, 9, seed=2)
    _two_runs(model, li.GREEDY_LEVELS, (t1, m1, 0, 200, None), (t2, m2, 9, 200, None), 26)


@pytest.mark.parametrize("what", sorted(li.SAMPLE_PAIRS))
def test_one_engine_two_runs_other_sampler_setting(what):
    """Another seed, temperature, top_p, or top_k 50 then 10: the replayed steps of the second run use the second
    run's values (tests/test_loop_cpu.py: each pair's two host runs differ after the first two tokens)."""
    model = _scripted(li.SAMPLE_LEVELS)
    toks, mask = li.sample_batch()
    first, second = li.SAMPLE_PAIRS[what]
    _two_runs(model, li.SAMPLE_LEVELS, (toks, mask, 0, -1, first), (toks, mask, 0, -1, second), 26)


def test_one_engine_two_key_masks_with_holes():
    """Random weights, so attention matters: one graph engine, the same prompt under two key masks with holes. The
    second run is a fresh eager engine's, and not the run under the first mask."""
    cfg = gpu_config()
    _, _, _, params = build(cfg, seed=21)
    model = LLaMAForCausalLM(cfg, device=DEV, _do_init=False).load_params(params)
    g = torch.Generator().manual_seed(22)
    toks = torch.randint(3, cfg.vocab_size, (2, 12), generator=g, dtype=I32)
    m1 = torch.ones(2, 12, dtype=I32)
    m1[0, [2, 5]] = 0
    m1[1, [1, 7, 8]] = 0
    m2 = torch.ones(2, 12, dtype=I32)
    m2[0, [0, 1, 3, 4, 6, 8, 9]] = 0
    m2[1, [2, 3, 4, 5, 6, 10]] = 0
    gc = _gc(40, 0, -1)
    eng = DecodeEngine(model, 2, 40, use_graph=True)
    a1 = _run(eng, toks, m1, gc)
    held = eng.key_mask  # alive, so that a second mask tensor cannot land on the address the graph recorded
    a2 = _run(eng, toks, m2, gc)
    assert held is not None
    assert eng._graph is not None and eng.key_mask is not None
    e1 = _run(DecodeEngine(model, 2, 40, use_graph=False), toks, m1, gc)
    e2 = _run(DecodeEngine(model, 2, 40, use_graph=False), toks, m2, gc)
    assert not torch.equal(e1[:, 14:], e2[:, 14:])  # the masks decide the tokens: a stale mask cannot pass
    assert torch.equal(a1, e1)
    assert torch.equal(a2, e2)


# ----------------------------------------------------------------------------------
# 5. sampler and argmax edges
# ----------------------------------------------------------------------------------
def _rows(b, v, seed):
    return torch.randn(b, v, generator=torch.Generator().manual_seed(seed)) * 2


def _check_candidates(x, k, idx_offset=0):
    want_v, want_i = ref.topk_sorted(x, k)
    got_v, got_i = ops.topk_candidates(x.to(DEV), k, idx_offset)
    got_v, got_i = got_v.cpu(), got_i.cpu()
    assert not bool((got_i == NO_INDEX).any())
    assert torch.equal(got_i, want_i + idx_offset)
    assert torch.equal(got_v, want_v)


@pytest.mark.parametrize("v,k", [(16383, 50), (16385, 50), (16388, 50), (32769 + 2, 50), (16384 + 10, 50), (64, 64),
                                 (1, 1), (65, 64)])
def test_topk_candidates_sizes(v, k):
    """Odd V: the scalar-load path through full 16384-logit chunks, the chunk boundary mid-row; a last chunk with
    fewer than k logits; k = V."""
    x = _rows(3, v, seed=v)
    x[1, max(0, v - 3):] = 30.0  # winners at the very end of the row ...
    x[2, :min(v, 2)] = 31.0      # ... and at its start
    if v > 16384:
        x[0, 16380:16384] = 29.0  # both sides of the chunk boundary
        x[0, 16384:min(v, 16388)] = 29.0
    _check_candidates(x, k)


@pytest.mark.parametrize("v", [1000, 16384 + 10])
def test_topk_candidates_minus_infinity(v):
    """All but 10 logits -inf: the 40 lowest-index -inf entries fill the top 50, never a padding slot. And a row that
    is all -inf: indices 0 .. 49."""
    x = torch.full((3, v), _NEG_INF)
    g = torch.Generator().manual_seed(v)
    for row in (0, 2):
        at = torch.randperm(v, generator=g)[:10]
        x[row, at] = torch.randn(10, generator=g)
    x[2, v - 1] = 1.0  # a finite logit in the short last chunk
    _check_candidates(x, 50)
    got_v, got_i = ops.topk_candidates(x.to(DEV), 50)
    assert torch.equal(got_i[1].cpu(), torch.arange(50, dtype=I32)) and bool(torch.isinf(got_v[1]).all())
    assert int(torch.isinf(got_v[0]).sum()) == 40


@pytest.mark.parametrize("v", [300, 16384 + 100])
def test_topk_candidates_signed_zeros_tie(v):
    """-0.0 and +0.0 are equal logits: across the top-k boundary the lower index wins, whatever the sign."""
    x = -1.0 - torch.rand(3, v, generator=torch.Generator().manual_seed(v))
    x[:, 100:145] = 5.0 + torch.arange(45, dtype=torch.float32)  # 45 above the zeros: 5 zeros make the top 50
    zeros = [3, 20, 70, 150, 200, 250, 260, 270] if v == 300 else [3, 20, 16383, 16384, 16390, 16400, 16410, 16420]
    x[0, zeros] = torch.tensor([-0.0, 0.0] * 4)
    x[1, zeros] = torch.tensor([-0.0] * 5 + [0.0] * 3)
    x[2, zeros] = torch.tensor([0.0] * 4 + [-0.0] * 4)
    want_i = ref.topk_sorted(x, 50)[1]
    for row in range(3):
        assert want_i[row, 45:].tolist() == zeros[:5]
    _check_candidates(x, 50)


def test_topk_candidates_index_offset():
    _check_candidates(_rows(3, 16385, seed=7), 50, idx_offset=1000)
    _check_candidates(_rows(3, 300, seed=8), 10, idx_offset=1000)


def _excluded(lead, dist):
    """The rows whose reference numbers are a near-tie: score lead below 1e-4, or an exclusive cumulative probability
    within 1e-5 of top_p."""
    return (lead < 1e-4) | (dist < 1e-5)


def _report(got, want, lead, dist, live):
    bad = ((got != want) & live).nonzero().reshape(-1).tolist()
    return [(r, int(got[r]), int(want[r]), float(lead[r]), float(dist[r])) for r in bad[:10]]


def _sharded_sample(x, tp, k, temperature, top_p, seed, step):
    """The extension calls ops.topk_sample makes under vocab-parallel TP, every rank's on this one GPU."""
    e = ops.ext()
    b, v = x.shape
    vl = v // tp
    kl = min(k, vl)
    lvs, lis = [], []
    for r in range(tp):
        xl = x[:, r * vl:(r + 1) * vl].contiguous()
        c = e.topk_chunks(vl) * kl
        cv = torch.empty(b, c, dtype=torch.float32, device=DEV)
        ci = torch.empty(b, c, dtype=I32, device=DEV)
        e.topk_chunk(xl, kl, r * vl, cv, ci)
        lv = torch.empty(b, kl, dtype=torch.float32, device=DEV)
        li_ = torch.empty(b, kl, dtype=I32, device=DEV)
        e.topk_merge(cv, ci, kl, 0, out_v=lv, out_i=li_)
        lvs.append(lv)
        lis.append(li_)
    cv, ci = torch.cat(lvs, 1).contiguous(), torch.cat(lis, 1).contiguous()  # gather_topk: rank order
    nxt = torch.empty(b, dtype=I32, device=DEV)
    e.topk_merge(cv, ci, k, 1, nxt=nxt, temperature=float(temperature), top_p=float(top_p), seed=int(seed), step=step)
    return nxt


@pytest.mark.parametrize("v,tp,k", [(1000, 2, 50), (1000, 4, 50), (128, 4, 50)])
def test_sharded_merge_is_the_unsharded_sampler(v, tp, k):
    """Two-stage merge of vocab-sharded candidates (idx_offset = r * v_local; (128, 4, 50): kl = 32 < k)."""
    b, temperature, top_p, seed = 64, 0.8, 0.9, 4321
    x = _rows(b, v, seed=v + tp)
    want, lead, dist = li.sample_detail(x, k, temperature, top_p, seed, 5)
    live = ~_excluded(lead, dist)
    assert int(live.sum()) >= b - 2
    step = torch.tensor([5], dtype=I32, device=DEV)
    whole = ops.topk_sample(x.to(DEV), k, temperature, top_p, seed, step).cpu()
    sharded = _sharded_sample(x.to(DEV), tp, k, temperature, top_p, seed, step).cpu()
    assert torch.equal(sharded, whole)
    assert torch.equal(whole[live], want[live]), _report(whole, want, lead, dist, live)


DRAW_CONFIGS = [(50, 0.8, 0.9), (50, 1.0, 1.0), (64, 1.3, 0.5)]


@pytest.mark.parametrize("k,temperature,top_p", DRAW_CONFIGS)
def test_4096_draws_are_the_reference(k, temperature, top_p):
    """4096 different rows in one launch against ref.topk_sample row by row. A row is left out only when the
    reference's own numbers call it a near-tie; at most 1 % may be, asserted before the GPU result is looked at."""
    x = _rows(4096, 2000, seed=31)
    seed, step = 99, 17
    want, lead, dist = li.sample_detail(x, k, temperature, top_p, seed, step)
    out = _excluded(lead, dist)
    print(f"left out: {int(out.sum())} of 4096 (lead < 1e-4: {int((lead < 1e-4).sum())}, "
          f"top_p within 1e-5: {int((dist < 1e-5).sum())})")
    assert int(out.sum()) <= 40
    got = ops.topk_sample(x.to(DEV), k, temperature, top_p, seed, torch.tensor([step], dtype=I32, device=DEV)).cpu()
    assert torch.equal(got[~out], want[~out]), _report(got, want, lead, dist, ~out)


@pytest.mark.parametrize("k,temperature,top_p", DRAW_CONFIGS)
def test_4096_identical_rows_draw_the_true_distribution(k, temperature, top_p):
    row = _rows(1, 2000, seed=21)[0]
    x = row.expand(4096, 2000).contiguous().to(DEV)
    draws = ops.topk_sample(x, k, temperature, top_p, 1234, torch.tensor([7], dtype=I32, device=DEV)).cpu()
    chi, df = li.check_draws(draws, row, k, temperature, top_p)
    print(f"chi-square {chi:.1f} at df {df}")


def test_top_p_at_a_cumulative_sum_excludes_the_candidate():
    """li.top_p_boundary_row(): four equal candidates, probabilities exactly 1/4 each, top_p = 0.5 exactly the mass
    before the third. The HF keep rule is strict (mass before < top_p): only the first two are ever drawn."""
    row = li.top_p_boundary_row()
    x = row.expand(4096, row.numel()).contiguous().to(DEV)
    draws = ops.topk_sample(x, 4, 1.0, 0.5, 77, torch.tensor([3], dtype=I32, device=DEV)).cpu()
    assert sorted(set(draws.tolist())) == [1, 3]
    li.check_draws(draws, row, 4, 1.0, 0.5)


@pytest.mark.parametrize("v", [1, 63, 1000, 1025, 128256 + 3])
def test_argmax_edges(v):
    """Random rows, then the maximum repeated across waves and stride positions of the 1024-thread row loop (the
    lowest index wins), an all -inf row (index 0), and -0.0 before +0.0 with nothing larger (the -0.0's index)."""
    x = _rows(6, v, seed=v)
    planted = []
    if v > 1:
        spots = {63: [62, 31, 40], 1000: [999, 700, 64, 63], 1025: [1024, 700], 128259: [6 + 2048, 6 + 1024, 128258]}[v]
        x[2, spots] = 50.0
        planted.append((2, min(spots)))
        x[3, [v - 1, v // 2]] = 50.0
        planted.append((3, v // 2))
        x[5] = -1.0 - x[5].abs()
        x[5, v // 3] = -0.0
        x[5, v - 1] = 0.0
        planted.append((5, v // 3))
    x[4] = _NEG_INF
    planted.append((4, 0))
    want = ref.argmax(x)
    for row, at in planted:
        assert int(want[row]) == at
    idx, val = ops.argmax(x.to(DEV))
    assert torch.equal(idx.cpu(), want)
    assert torch.equal(val.cpu(), x.max(-1).values)
    if v > 1:
        assert bool(np.signbit(val.cpu().numpy()[5]))  # the -0.0 itself
