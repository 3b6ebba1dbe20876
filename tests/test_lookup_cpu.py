"""Prompt-lookup decoding on the CPU: the reference loop against plain greedy, and generate's validation."""
import dataclasses

import pytest
import torch

from jax_llama_amd.runtime.engine import GenerationConfig
from jax_llama_amd.ops import reference as ref

from helpers import build, left_padded_batch, tiny_config

GC = dict(max_length=40, do_sample=False, pad_token_id=2, eos_token_id=2)


@pytest.fixture(scope="module")
def model():
    return build(tiny_config(), seed=3)[0]


@pytest.mark.parametrize("batch,k", [(1, 3), (4, 3), (3, 7)])
def test_lookup_cpu_matches_plain_greedy(model, batch, k):
    lens = [max(2, 11 - (3 * i) % 9) for i in range(batch)]
    toks, mask = left_padded_batch(lens, 11, model.config.vocab_size, pad=2, seed=4)
    gc = GenerationConfig(prompt_lookup_num_tokens=k, **GC)
    before = dataclasses.asdict(gc)
    got = model.generate(toks, attention_mask=mask, generation_config=gc).sequences
    want = model.generate(toks, attention_mask=mask, generation_config=GenerationConfig(**GC)).sequences
    assert dataclasses.asdict(gc) == before  # generate works on a copy
    assert got.shape == want.shape
    assert (got.long() == want.long()).float().mean().item() > 0.97
    assert torch.equal(got[:, :11], toks)


@pytest.mark.parametrize("kw,exc", [
    (dict(prompt_lookup_num_tokens=0), ValueError),
    (dict(prompt_lookup_num_tokens=16), ValueError),  # (k + 1) x rep = 34 > 32 at rep 2
    (dict(prompt_lookup_num_tokens=3, max_matching_ngram_size=0), ValueError),
    (dict(prompt_lookup_num_tokens=3, do_sample=True), ValueError),
    (dict(prompt_lookup_num_tokens=3, num_beams=2), ValueError),
    (dict(prompt_lookup_num_tokens=3, repetition_penalty=1.2), ValueError),
    (dict(prompt_lookup_num_tokens=3, do_sample=True, min_p=0.1), ValueError),
])
def test_lookup_validation(model, kw, exc):
    toks, mask = left_padded_batch([5], 5, model.config.vocab_size, pad=2, seed=1)
    with pytest.raises(exc):
        model.generate(toks, attention_mask=mask, generation_config=GenerationConfig(**{**GC, **kw}))


def test_lookup_validation_batch_and_tp(model):
    toks = torch.full((65, 4), 5, dtype=torch.int32)
    with pytest.raises(ValueError):
        model.generate(toks, generation_config=GenerationConfig(prompt_lookup_num_tokens=3, **GC))
    comm = model.comm
    model.comm = type("TP2", (), {"size": 2, "rank": 0})()
    try:
        with pytest.raises(NotImplementedError):
            model.generate(toks[:1], generation_config=GenerationConfig(prompt_lookup_num_tokens=3, **GC))
    finally:
        model.comm = comm


def test_reference_rules():
    # history 7 8 9 7 8 5 7 8: the 2-gram (7 8) matches at 0 and 3 -> the earliest, continuation 9 7 8
    seq = torch.tensor([[7, 8, 9, 7, 8, 5, 7, 8, 0, 0]], dtype=torch.int32)
    hs = torch.zeros(1, dtype=torch.int32)
    assert ref.prompt_lookup(seq, 8, hs, 3, 2).tolist() == [[9, 7, 8]]
    # the history starts at 1: the match at 0 is padding, the one at 3 has the continuation 5 7 8
    assert ref.prompt_lookup(seq, 8, hs + 1, 3, 2).tolist() == [[5, 7, 8]]
    # history from 4 on (8 5 7 8): no 2-gram, the 1-gram (8) at 4, continuation 5 7 8 of which cur_len cuts nothing
    assert ref.prompt_lookup(seq, 8, hs + 4, 4, 2).tolist() == [[5, 7, 8, 8]]
    assert ref.prompt_lookup(seq, 3, hs, 2, 2).tolist() == [[9, 9]]  # no match: the last token
