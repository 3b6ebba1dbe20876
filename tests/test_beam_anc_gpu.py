"""The indirect beam cache on the GPU: decode attention through an ancestry table against the fp32 reference on the
gathered rows and, bit for bit, against itself on a physically gathered cache; the table's update kernel against
``ref.beam_anc_update``; and the beam engine that moves no cache row against the host search and the torch update."""
from __future__ import annotations

import functools

import pytest
import torch

import beam_inputs as bi
import loop_inputs as li
from jax_llama_amd import ops
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime.engine import BeamEngine, GenerationConfig
from helpers import build, gpu_config
from test_beam_gpu import _check, _gc, _run, _scripted
from test_kernels_gpu import _close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32, BF16 = torch.int32, torch.bfloat16
NB, K, HKV, DH = 2, 3, 2, 128  # 2 prompts x 3 beams (not a power of two)


# ----------------------------------------------------------------------------------
# 1 + 2. attn_decode_anc
# ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(rep, t, slot, masked):
    """CPU inputs and the reference output, once per shape: a random table with every beam in every column, prompt 1
    with kv_start 5, the last row with no valid key."""
    g = torch.Generator().manual_seed(1000 * rep + t)
    rows, h = NB * K, HKV * rep
    kc = torch.randn(rows, HKV, t, DH, generator=g).to(BF16)
    vc = torch.randn(rows, HKV, t, DH, generator=g).to(BF16)
    q = torch.randn(rows, 1, h, DH, generator=g).to(BF16)
    anc = torch.randint(0, K, (rows, t), generator=g, dtype=torch.uint8)
    kv_start = torch.tensor([0] * K + [5] * (K - 1) + [slot + 1], dtype=I32)
    mask = None
    if masked:
        mask = (torch.rand(rows, t, generator=g) > 0.3).to(torch.uint8)
        mask[:, slot] = 1
    expect = ref.attention_anc(q, kc, vc, slot, kv_start, anc, K, mask).reshape(rows, h * DH)
    return q, kc, vc, anc, kv_start, mask, expect


@pytest.mark.parametrize("splits", [1, 2, 3])  # 3: at (1030, 700) the last split ends in a partial chunk at every rep
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("t,slot", [(40, 17), (300, 299), (1030, 700)])
@pytest.mark.parametrize("rep", [1, 4, 8])
def test_attention_through_the_table(rep, t, slot, masked, splits):
    e = ops.ext()
    q, kc, vc, anc, kv_start, mask, expect = _inputs(rep, t, slot, masked)
    dev = [None if x is None else x.to(DEV) for x in (q, kc, vc, anc, kv_start, mask)]
    slot_t = torch.tensor([slot], dtype=I32, device=DEV)
    ident = torch.arange(K, dtype=torch.uint8).repeat(NB)[:, None].repeat(1, t).contiguous().to(DEV)

    def run(k_cache, v_cache, table):
        return ops.attention(dev[0], k_cache, v_cache, slot_t, dev[4], dev[5], beam_anc=table, num_beams=K)

    try:
        e.attn_set_anc_splits(splits)
        rc, _, _, kpg, nsplit, *_ = e.attn_decode_anc_plan_check(NB * K, HKV * rep, HKV, DH, t, masked, K)
        assert rc == 0 and nsplit == min(splits, -(-t // (32 * kpg)))  # (a pinned count: at most the chunks of T)
        got = run(dev[1], dev[2], dev[3])
        again = run(dev[1], dev[2], dev[3])
        # the same kernel on the rows the table names, moved for real, under the identity table: the indexing, exactly
        moved = run(ref.gather_anc(dev[1], dev[3], K).contiguous(), ref.gather_anc(dev[2], dev[3], K).contiguous(), ident)
        torch.cuda.synchronize()
    finally:
        e.attn_reset_knobs()
    _close(got, expect, 2e-2, 2e-2)
    assert got[-1].float().abs().max().item() == 0.0  # no valid key: exact zeros
    assert torch.equal(got, again) and torch.equal(got, moved)
    ops.check_bounds()


def test_table_values_past_the_group_are_clamped():
    q, kc, vc, anc, kv_start, _, _ = _inputs(4, 300, 299, False)
    big = torch.where(anc == K - 1, torch.full_like(anc, 200), anc)
    slot_t = torch.tensor([299], dtype=I32, device=DEV)
    out = [ops.attention(q.to(DEV), kc.to(DEV), vc.to(DEV), slot_t, kv_start.to(DEV), beam_anc=a.to(DEV), num_beams=K)
           for a in (anc, big)]
    assert torch.equal(out[0], out[1])
    assert torch.equal(ref.gather_anc(kc, big, K), ref.gather_anc(kc, anc, K))


def test_attention_with_a_table_rejects_what_it_cannot_serve():
    q, kc, vc, anc, kv_start, _, _ = [None if x is None else x.to(DEV) for x in _inputs(1, 40, 17, False)]
    slot_t = torch.tensor([17], dtype=I32, device=DEV)
    with pytest.raises(ValueError):  # S > 1
        ops.attention(q.reshape(NB * K // 2, 2, HKV, DH), kc[:3], vc[:3], slot_t, kv_start[:3], beam_anc=anc[:3],
                      num_beams=K)
    with pytest.raises(ValueError):  # an Fp8KV
        kv8 = ref.Fp8KV.zeros(NB * K, HKV, 40, device=DEV)
        ops.attention(q, kv8, kv8, slot_t, kv_start, beam_anc=anc, num_beams=K)
    assert not ops.attention_packs(q, kc, None, anc)
    assert ops.qkv_attention_splits(q, None, kc, 1, HKV, HKV, beam_anc=anc) == 0


# ----------------------------------------------------------------------------------
# 3. beam_anc_update
# ----------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [48, 40])  # 16-byte units; a row length that is no multiple of 16 (byte units)
@pytest.mark.parametrize("k", [2, 3, 8])
def test_anc_update_is_the_reference(k, t):
    g = torch.Generator().manual_seed(10 * k + t)
    b = 3
    ident = torch.arange(k, dtype=I32).repeat(b)
    for count in (0, 16, 21, t):  # nothing; a unit boundary; inside a unit; the whole row
        anc = torch.randint(0, k, (b * k, t), generator=g, dtype=torch.uint8)
        idx = torch.randint(0, k, (b * k,), generator=g, dtype=I32)
        idx[k:2 * k] = ident[:k]  # one group keeps its beams
        slot = torch.tensor([count], dtype=I32, device=DEV)
        got = anc.clone().to(DEV)
        ops.beam_anc_update(got, idx.to(DEV), k, slot)
        want = ref.beam_anc_update(anc.clone(), idx, k, count)
        assert torch.equal(got.cpu(), want), (count,)
        assert torch.equal(got.cpu()[:, count:], anc[:, count:])
        same = anc.clone().to(DEV)
        ops.beam_anc_update(same, ident.to(DEV), k, slot)
        assert torch.equal(same.cpu(), anc)
    ops.check_bounds()


# ----------------------------------------------------------------------------------
# 4. the engine
# ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(bi.CASES))
def test_indirect_engine_is_the_host_search(name):
    toks, mask, k, eos, lp, early = bi.case(name)[:6]
    model = _scripted()
    eager = _run(BeamEngine(model, 3, k, bi.MAX_LENGTH, use_graph=False, beam_cache="indirect"), toks, mask,
                 _gc(k, eos, lp, early))
    graph = _run(BeamEngine(model, 3, k, bi.MAX_LENGTH, use_graph=True, beam_cache="indirect"), toks, mask,
                 _gc(k, eos, lp, early))
    _check(eager, name)
    _check(graph, name)
    assert torch.equal(eager[0], graph[0]) and torch.equal(eager[1], graph[1])
    ops.check_bounds()


def _torch_update(cache, beam_idx, k):
    ref.beam_anc_update(cache.beam_anc, beam_idx, k, int(cache.index_t.item()))


def _no_update(cache, beam_idx, k):
    pass


def test_table_follows_the_beams():
    """The tiny random-init model of test_cache_follows_the_beams, through ``set_beam_cache``: the graph engine with the
    kernel update equals an eager engine whose update is the torch reference (sequences, scores and the table below the
    slot, bit for bit); some step permutes for real; and without the update the output differs."""
    cfg = gpu_config()
    model = build(cfg, device=DEV, seed=3)[0].set_beam_cache("indirect")
    s, length, k, pad = 7, 24, 4, 0
    toks, mask = li.prompts([5, 9, 130], [3, 7, 5], s, pad, seed=2)
    toks = toks % cfg.vocab_size
    gc = GenerationConfig(max_length=length, num_beams=k, pad_token_id=pad, eos_token_id=-1, length_penalty=0.0,
                          num_return_sequences=2)
    runs = {}
    for name, update, graph in (("torch", _torch_update, False), ("kernel", None, True), ("none", _no_update, False)):
        eng = BeamEngine(model, 3, k, length, use_graph=graph)
        assert eng.beam_cache == "indirect"
        if update is not None:
            eng.reorder = update
        eng.beam_idx_log = []
        seqs, scores = _run(eng, toks, mask, gc)
        n = int(eng.cache.index_t.item())
        runs[name] = (seqs, scores, eng.cache.beam_anc[:, :n].cpu(), eng.beam_idx_log, n)
    t, kern, none = runs["torch"], runs["kernel"], runs["none"]
    assert t[4] == kern[4] == length - 1
    ident = torch.arange(k, dtype=I32).repeat(3)
    assert any(not torch.equal(step, ident) for step in t[3])
    assert torch.equal(t[0], kern[0]) and torch.equal(t[1], kern[1]) and torch.equal(t[2], kern[2])
    assert not torch.equal(t[0], none[0])
    ops.check_bounds()
