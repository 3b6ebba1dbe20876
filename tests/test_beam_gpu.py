"""Beam search on the GPU: the cache reorder kernel against the gather (bit for bit), the step kernels against
``ops/reference.py`` (``torch.equal`` on every state tensor), the graph-replaying beam engine against the host search
of tests/beam_inputs.py, and the reorder's effect on a model that reads its cache."""
from __future__ import annotations

import types

import pytest
import torch

import beam_inputs as bi
import loop_inputs as li
from jax_llama_amd import ops
from jax_llama_amd.models import LLaMAForCausalLM
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime.engine import BeamEngine, GenerationConfig
from jax_llama_amd.utils.checkpoint import meta_state_dict_to_params
from helpers import build, gpu_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32 = torch.int32


# ----------------------------------------------------------------------------------
# 1. kv_beam_reorder
# ----------------------------------------------------------------------------------
NL, NB, NH, NT, DH = 2, 2, 2, 40, 128
GUARD = 4096  # bytes in front of, between and behind the cache tensors


def _patterns(k):
    ident = list(range(k))
    rot = [(j + 1) % k for j in range(k)]
    swap = [1, 0] + ident[2:]
    return {"identity": ident * NB, "all_from_one": [k - 1] * (k * NB), "rotation": rot * NB, "swap": swap * NB,
            "per_group": rot + [0] * k}


def _guarded_cache(k, fmt, seed):
    """A cache-like object whose tensors are views into ONE byte buffer with guard regions around each of them."""
    rows = NB * k
    shapes = [((NL, rows, NH, NT, DH), torch.uint8 if fmt == "fp8_e4m3" else torch.bfloat16)] * 2
    if fmt == "fp8_e4m3":
        shapes += [((NL, rows, NH, NT), torch.float32)] * 2
    sizes = [torch.Size(s).numel() * torch.empty(0, dtype=d).element_size() for s, d in shapes]
    total = GUARD + sum(n + GUARD for n in sizes)
    g = torch.Generator().manual_seed(seed)
    buf = torch.randint(0, 256, (total,), generator=g, dtype=torch.uint8).to(DEV)
    views, spans, off = [], [], GUARD
    for (shape, dt), n in zip(shapes, sizes):
        views.append(buf[off:off + n].view(dt).view(shape))
        spans.append((off, off + n))
        off += n + GUARD
    cache = types.SimpleNamespace(k=views[0], v=views[1], k_scale=views[2] if len(views) > 2 else None,
                                  v_scale=views[3] if len(views) > 2 else None,
                                  index_t=torch.zeros(1, dtype=I32, device=DEV))
    return cache, buf, spans


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


@pytest.mark.parametrize("fmt", ["bf16", "fp8_e4m3"])
@pytest.mark.parametrize("k", [2, 3, 8])
def test_kv_beam_reorder_is_the_gather(k, fmt):
    for count in (0, 1, 17, 40):
        for name, pat in _patterns(k).items():
            cache, buf, spans = _guarded_cache(k, fmt, seed=count + k)
            before = buf.clone()
            cache.index_t.fill_(count)
            idx = torch.tensor(pat, dtype=I32, device=DEV)
            ops.kv_beam_reorder(cache, idx, k)
            torch.cuda.synchronize()
            keep = torch.ones_like(buf, dtype=torch.bool)
            for (a, b), t in zip(spans, ops.kv_beam_tensors(cache)):
                keep[a:b] = False
                old = _bits(before[a:b].view(t.dtype).view(t.shape))
                new = _bits(t)
                want = _bits(ref.kv_beam_reorder(before[a:b].clone().view(t.dtype).view(t.shape), idx, k, count))
                assert torch.equal(new[:, :, :, :count], want[:, :, :, :count]), (name, count)
                if count == NT:
                    continue
                # past the count: the old content, or the same slot of another beam of the group
                tail_new = new[:, :, :, count:].reshape(NL, NB, k, NH, NT - count, -1)
                tail_old = old[:, :, :, count:].reshape(NL, NB, k, NH, NT - count, -1)
                ok = torch.zeros(tail_new.shape[:5], dtype=torch.bool, device=DEV)
                for j in range(k):
                    ok |= (tail_new == tail_old[:, :, j:j + 1]).all(-1)
                assert bool(ok.all()), (name, count)
            assert torch.equal(buf[keep], before[keep]), (name, count)  # the guards
    ops.check_bounds()


def test_kv_beam_reorder_rejects_wrong_shapes():
    cache, _, _ = _guarded_cache(2, "bf16", 0)
    with pytest.raises(RuntimeError):
        ops.ext().kv_beam_reorder(cache.k, torch.zeros(3, dtype=I32, device=DEV), cache.index_t, 2)
    with pytest.raises(RuntimeError):
        ops.ext().kv_beam_reorder(cache.k, torch.zeros(4, dtype=I32, device=DEV), cache.index_t, 9)


# ----------------------------------------------------------------------------------
# 2. beam_alive / beam_step
# ----------------------------------------------------------------------------------
def _step_both(seed, k, c, ties, early, lp, all_finished=False, alive=None, b=3, length=12, s=4, eos=5):
    """Runs ops.beam_alive + ops.beam_step on CPU tensors (ops/reference.py) and on the GPU; returns both states."""
    cv, ci, lse, rseq, seq, rs, sc, fin = bi.random_step_inputs(seed, b, k, length, ties, all_finished)
    inv_pen = ref.beam_inv_pen(length, lp)
    out = []
    for dev in ("cpu", DEV):
        st = dict(cv=cv, ci=ci, lse=lse, rseq=rseq, seq=seq, rs=rs, sc=sc, fin=fin.to(I32), inv_pen=inv_pen,
                  cur_len=torch.tensor([c], dtype=I32), slot=torch.tensor([c - 1], dtype=I32),
                  tokens=torch.full((b * k, 1), 77, dtype=I32), positions=torch.arange(b * k, dtype=I32)[:, None] + 3,
                  alive=torch.tensor([1], dtype=I32), beam_idx=torch.full((b * k,), -1, dtype=I32))
        st = {n: t.clone().to(dev) for n, t in st.items()}
        if alive is None:
            ops.beam_alive(st["rs"], st["sc"], st["fin"], st["inv_pen"], st["cur_len"], st["alive"], length, s, early, lp)
        else:
            st["alive"].fill_(alive)
        ops.beam_step(st["cv"], st["ci"], st["lse"], st["rseq"], st["seq"], st["rs"], st["sc"], st["fin"],
                      st["inv_pen"], st["cur_len"], st["slot"], st["tokens"], st["positions"], st["alive"],
                      st["beam_idx"], s, eos, early)
        out.append({n: t.cpu() for n, t in st.items()})
    torch.cuda.synchronize()
    return out


def _assert_same(cpu, gpu):
    for n in cpu:
        assert torch.equal(cpu[n], gpu[n]), n


@pytest.mark.parametrize("k", [2, 3, 4, 8])
@pytest.mark.parametrize("ties", [False, True])
def test_beam_step_is_the_reference(k, ties):
    """Random inputs and exact ties across beams and ranks (eos = 5 is among the 12 candidate tokens), every
    early_stopping mode and penalty, c from the first step to L - 1, with the loop condition evaluated on the device."""
    changed = 0
    for seed in range(12):
        early = [False, True, "never"][seed % 3]
        lp = [0.0, 1.0, 2.0][(seed // 3) % 3]
        c = [4, 6, 11][seed % 3] if seed < 9 else 11
        cpu, gpu = _step_both(100 * k + seed, k, c, ties, early, lp)
        _assert_same(cpu, gpu)
        changed += int(cpu["alive"])
        assert int(cpu["cur_len"]) == c + int(cpu["alive"]) and int(cpu["slot"]) == c - 1 + int(cpu["alive"])
    assert changed >= 3  # (c == S always runs)
    ops.check_bounds()


@pytest.mark.parametrize("early", [False, True])
def test_beam_step_all_finished_item(early):
    for k in (2, 4):
        for seed in range(4):
            # alive forced to 1: the step itself must apply (or not) the all-finished penalty
            cpu, gpu = _step_both(seed, k, 7, seed % 2 == 0, early, 1.0, all_finished=True, alive=1)
            _assert_same(cpu, gpu)
            assert int(cpu["cur_len"]) == 8
    # ... and the loop condition sees it: early_stopping=True stops, False goes by the scores
    cpu, gpu = _step_both(1, 2, 7, False, early, 1.0, all_finished=True)
    _assert_same(cpu, gpu)
    if early:
        assert int(gpu["alive"]) == 0


@pytest.mark.parametrize("k", [2, 8])
def test_beam_step_not_alive_changes_nothing(k):
    cv, ci, lse, rseq, seq, rs, sc, fin = bi.random_step_inputs(5, 3, k, 12, False)
    cpu, gpu = _step_both(5, k, 7, False, False, 1.0, alive=0)
    _assert_same(cpu, gpu)
    assert torch.equal(gpu["rseq"], rseq) and torch.equal(gpu["seq"], seq) and torch.equal(gpu["rs"], rs)
    assert torch.equal(gpu["sc"], sc) and torch.equal(gpu["fin"], fin.to(I32))
    assert int(gpu["cur_len"]) == 7 and int(gpu["slot"]) == 6 and bool((gpu["tokens"] == 77).all())
    assert torch.equal(gpu["positions"][:, 0], torch.arange(3 * k, dtype=I32) + 3)
    assert gpu["beam_idx"].tolist() == list(range(k)) * 3
    # cur_len == L: the loop condition is false on the device, and the step is the same no-op
    cpu, gpu = _step_both(5, k, 12, False, False, 1.0)
    _assert_same(cpu, gpu)
    assert int(gpu["alive"]) == 0 and int(gpu["cur_len"]) == 12 and torch.equal(gpu["rseq"], rseq)


# ----------------------------------------------------------------------------------
# 3. the engine on the scripted model
# ----------------------------------------------------------------------------------
_MODELS = {}


def _scripted(fmt="bf16"):
    if fmt not in _MODELS:
        cfg = li.config()
        params = meta_state_dict_to_params(bi.state_dict(), cfg.num_hidden_layers)
        _MODELS[fmt] = LLaMAForCausalLM(cfg, device=DEV, _do_init=False).load_params(params)
        _MODELS[fmt].set_kv_cache_format(fmt)
    return _MODELS[fmt]


def _gc(k, eos, lp, early, nrs=1, max_length=bi.MAX_LENGTH):
    return GenerationConfig(max_length=max_length, num_beams=k, pad_token_id=bi.PAD, eos_token_id=eos,
                            length_penalty=lp, early_stopping=early, num_return_sequences=nrs)


def _run(eng, toks, mask, gc):
    seqs, scores = eng.run(toks, mask, gc)
    torch.cuda.synchronize()
    return seqs.cpu().to(I32), scores.cpu()


def _check(got, name):
    seqs, scores, bound = bi.case(name)[6:9]
    assert torch.equal(got[0], seqs), name
    assert float((got[1] - scores).abs().max()) <= bound, name


@pytest.mark.parametrize("name", list(bi.CASES))
def test_engine_is_the_host_search(name):
    toks, mask, k, eos, lp, early = bi.case(name)[:6]
    model = _scripted()
    eager = _run(BeamEngine(model, 3, k, bi.MAX_LENGTH, use_graph=False), toks, mask, _gc(k, eos, lp, early))
    graph = _run(BeamEngine(model, 3, k, bi.MAX_LENGTH, use_graph=True), toks, mask, _gc(k, eos, lp, early))
    _check(eager, name)
    _check(graph, name)
    assert torch.equal(eager[0], graph[0]) and torch.equal(eager[1], graph[1])
    ops.check_bounds()


@pytest.mark.parametrize("first,second", [("k2_lp1", "k2_lp2"), ("k2_lp1", "k2_no_eos"), ("k2_lp1", "k2_early"),
                                          ("k2_lp05", "k2_never"), ("k4_lp1", "k4_lp0")])
def test_one_engine_two_runs(first, second):
    """The captured step takes eos, early_stopping and (through "never") the penalty's sign by value: a second run with
    other settings on the same engine gets its own host result, and so does the first one run again."""
    toks, mask, k = bi.case(first)[:3]
    eng = BeamEngine(_scripted(), 3, k, bi.MAX_LENGTH, use_graph=True)
    for name in (first, second, first):
        _, _, _, eos, lp, early = bi.case(name)[:6]
        _check(_run(eng, toks, mask, _gc(k, eos, lp, early)), name)


@pytest.mark.parametrize("name", ["k2_early", "k4_lp0", "k2_lp1"])
def test_check_every_does_not_change_the_output(name):
    toks, mask, k, eos, lp, early = bi.case(name)[:6]
    outs = []
    for every in (1, 16):
        eng = BeamEngine(_scripted(), 3, k, bi.MAX_LENGTH, use_graph=True, check_every=every)
        outs.append(_run(eng, toks, mask, _gc(k, eos, lp, early)))
        _check(outs[-1], name)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_generate_and_num_return_sequences():
    toks, mask, k, eos, lp, early, seqs, scores, bound = bi.case("k4_lp1", nrs=3)[:9]
    out = _scripted().generate(toks, attention_mask=mask, generation_config=_gc(k, eos, lp, early, nrs=3))
    assert torch.equal(out.sequences.cpu().to(I32), seqs)
    assert float((out.scores.cpu() - scores).abs().max()) <= bound


def test_engine_fp8_kv_cache_is_the_host_search():
    toks, mask, k, eos, lp, early = bi.case("k4_lp1")[:6]
    eng = BeamEngine(_scripted("fp8_e4m3"), 3, k, bi.MAX_LENGTH, use_graph=True)
    assert eng.cache.kv_format == "fp8_e4m3"
    _check(_run(eng, toks, mask, _gc(k, eos, lp, early)), "k4_lp1")


# ----------------------------------------------------------------------------------
# 4. a model that reads its cache
# ----------------------------------------------------------------------------------
def _gather_reorder(cache, beam_idx, k):
    for t in ops.kv_beam_tensors(cache):
        ref.kv_beam_reorder(t, beam_idx, k, int(cache.index_t.item()))


def _no_reorder(cache, beam_idx, k):
    pass


@pytest.mark.parametrize("fmt", ["bf16", "fp8_e4m3"])
def test_cache_follows_the_beams(fmt):
    """Tiny random-init model, B = 3 left-padded prompts, K = 4: the graph engine with the kernel equals an eager
    engine whose reorder is the torch gather (sequences, scores and the valid cache slots, bit for bit); some step
    reorders for real; and without the reorder the output differs, so these inputs can tell.

    Also prints, without asserting (decode and teacher-forced numerics differ), the distance between each returned
    score at length_penalty = 0 and the sum of ``model.score``'s log-probs over the generated tokens."""
    cfg = gpu_config()
    model = build(cfg, device=DEV, seed=3)[0]
    model.set_kv_cache_format(fmt)
    s, length, k, pad = 7, 24, 4, 0
    toks, mask = li.prompts([5, 9, 130], [3, 7, 5], s, pad, seed=2)
    toks = toks % cfg.vocab_size
    gc = GenerationConfig(max_length=length, num_beams=k, pad_token_id=pad, eos_token_id=-1, length_penalty=0.0,
                          num_return_sequences=2)
    runs = {}
    for name, reorder, graph in (("gather", _gather_reorder, False), ("kernel", None, True),
                                 ("none", _no_reorder, False)):
        eng = BeamEngine(model, 3, k, length, use_graph=graph)
        if reorder is not None:
            eng.reorder = reorder
        eng.beam_idx_log = []
        seqs, scores = _run(eng, toks, mask, gc)
        n = int(eng.cache.index_t.item())
        bits = [_bits(t)[:, :, :, :n].cpu() for t in ops.kv_beam_tensors(eng.cache)]
        runs[name] = (seqs, scores, bits, eng.beam_idx_log, n)
    g, kern, none = runs["gather"], runs["kernel"], runs["none"]
    assert g[4] == kern[4] == length - 1
    ident = torch.arange(k, dtype=I32).repeat(3)
    assert any(not torch.equal(step, ident) for step in g[3])
    assert torch.equal(g[0], kern[0]) and torch.equal(g[1], kern[1])
    for a, b in zip(g[2], kern[2]):
        assert torch.equal(a, b)
    assert not torch.equal(g[0], none[0])
    ops.check_bounds()
    full_mask = torch.cat([mask.repeat_interleave(2, 0), torch.ones(6, length - s, dtype=mask.dtype)], 1)
    lp = model.score(kern[0], attention_mask=full_mask).token_logprobs.float().cpu()
    for r in range(6):
        total = float(lp[r, s - 1:].sum())
        print(f"rescoring [{fmt}] row {r}: score {float(kern[1][r]):.5f}, teacher-forced {total:.5f}, "
              f"|difference| {abs(float(kern[1][r]) - total):.2e}")
