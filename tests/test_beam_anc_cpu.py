"""The indirect beam cache on the CPU: a BeamEngine that moves no cache row returns what the reordering one returns,
``ref.beam_anc_update`` is the ancestry traced in plain lists, and the public switch rejects what it cannot serve."""
from __future__ import annotations

import pytest
import torch

import beam_inputs as bi
import loop_inputs as li
from jax_llama_amd.models import LLaMAForCausalLM
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime.engine import BeamEngine, GenerationConfig
from jax_llama_amd.utils.checkpoint import meta_state_dict_to_params
from helpers import build, gpu_config


def _both_modes(model, toks, mask, gc, b, k, length):
    out = {}
    for mode in ("reorder", "indirect"):
        eng = BeamEngine(model, b, k, length, use_graph=False, beam_cache=mode)
        eng.beam_idx_log = []
        seqs, scores = eng.run(toks, mask, gc)
        out[mode] = (seqs, scores, eng.beam_idx_log)
    return out


@pytest.mark.parametrize("name", ["k2_lp1", "k4_early"])
def test_indirect_engine_is_the_reorder_engine_scripted(name):
    toks, mask, k, eos, lp, early, seqs, scores, bound = bi.case(name)[:9]
    cfg = li.config()
    model = LLaMAForCausalLM(cfg, _do_init=False).load_params(
        meta_state_dict_to_params(bi.state_dict(), cfg.num_hidden_layers))
    gc = GenerationConfig(max_length=bi.MAX_LENGTH, num_beams=k, pad_token_id=bi.PAD, eos_token_id=eos,
                          length_penalty=lp, early_stopping=early)
    out = _both_modes(model, toks, mask, gc, 3, k, bi.MAX_LENGTH)
    assert torch.equal(out["indirect"][0], out["reorder"][0]) and torch.equal(out["indirect"][1], out["reorder"][1])
    assert torch.equal(out["indirect"][0].to(torch.int32), seqs)
    assert float((out["indirect"][1] - scores).abs().max()) <= bound


def test_indirect_engine_is_the_reorder_engine_on_a_model_that_reads_its_cache():
    cfg = gpu_config()
    model = build(cfg, seed=3)[0]
    s, length, k, pad = 7, 24, 4, 0
    toks, mask = li.prompts([5, 9, 130], [3, 7, 5], s, pad, seed=2)
    toks = toks % cfg.vocab_size
    gc = GenerationConfig(max_length=length, num_beams=k, pad_token_id=pad, eos_token_id=-1, length_penalty=0.0,
                          num_return_sequences=2)
    out = _both_modes(model, toks, mask, gc, 3, k, length)
    ident = torch.arange(k, dtype=torch.int32).repeat(3)
    assert any(not torch.equal(step, ident) for step in out["reorder"][2])  # some step reorders for real
    assert torch.equal(out["indirect"][0], out["reorder"][0]) and torch.equal(out["indirect"][1], out["reorder"][1])


@pytest.mark.parametrize("k", [2, 3, 8])
def test_anc_update_is_the_traced_ancestry(k):
    """Each logical row's history as a list of (physical beam) per slot, permuted and extended step by step."""
    b, s, t = 2, 5, 19
    g = torch.Generator().manual_seed(k)
    anc = ref.beam_anc_init(b, k, t, s)
    hist = [[[0] * s for _ in range(k)] for _ in range(b)]  # the prompt: beam 0's row
    for n in range(s + 1, t + 1):  # the slot counter after each step
        idx = torch.randint(0, k, (b, k), generator=g, dtype=torch.int32)
        for i in range(b):
            written = [h + [j] for j, h in enumerate(hist[i])]  # every row wrote slot n - 1 into its own row
            hist[i] = [list(written[int(idx[i, j])]) for j in range(k)]
        ref.beam_anc_update(anc, idx.reshape(-1), k, n)
        want = torch.tensor([h for i in range(b) for h in hist[i]], dtype=torch.uint8)
        assert torch.equal(anc[:, :n], want)
        assert torch.equal(anc[:, n:], ref.beam_anc_init(b, k, t, s)[:, n:])  # untouched: still the identity


def test_set_beam_cache_rejects_what_it_cannot_serve():
    model = build(gpu_config(), seed=0)[0]
    assert model.beam_cache == "reorder"
    with pytest.raises(ValueError):
        model.set_beam_cache("paged")
    assert model.set_beam_cache("indirect").beam_cache == "indirect"
    model.set_kv_cache_format("fp8_e4m3")
    with pytest.raises(ValueError):
        BeamEngine(model, 1, 2, 16, use_graph=False)
