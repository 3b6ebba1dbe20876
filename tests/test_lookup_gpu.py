"""Prompt-lookup decoding on the GPU: the two state kernels (csrc/kernels/spec.hip) against their references, exactly, and
the loop end to end against plain greedy generation."""
from __future__ import annotations

import pytest
import torch

from jax_llama_amd import ops
from jax_llama_amd.models import LLaMAForCausalLM
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime.engine import GenerationConfig, LookupEngine

from helpers import build, gpu_config, left_padded_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32 = torch.int32

# rows of one history buffer (cur_len 8), each hitting one rule of ref.prompt_lookup
HIST = [
    ([7, 8, 9, 7, 8, 5, 7, 8], 0),  # the 2-gram (7 8) at 0 and at 3: the earliest
    ([7, 8, 9, 7, 8, 5, 7, 8], 1),  # the history starts inside the left padding: only the match at 3 counts
    ([1, 2, 3, 4, 8, 5, 6, 8], 0),  # no 2-gram match, the 1-gram (8) at 4
    ([1, 2, 3, 4, 5, 9, 6, 9], 0),  # a match at 5 whose continuation (6 9) is shorter than k
    ([1, 2, 3, 4, 5, 6, 7, 8], 0),  # no match: the last token
]


@pytest.mark.parametrize("k,max_ngram", [(3, 2), (5, 1), (2, 3)])
def test_prompt_lookup_kernel(k, max_ngram):
    seq = torch.zeros(len(HIST), 12, dtype=I32)
    seq[:, :8] = torch.tensor([h for h, _ in HIST], dtype=I32)
    hs = torch.tensor([s for _, s in HIST], dtype=I32)
    want = ref.prompt_lookup(seq, 8, hs, k, max_ngram)
    tokens = torch.full((len(HIST), k + 1), -5, dtype=I32, device=DEV)
    ops.prompt_lookup(seq.to(DEV), torch.tensor([8], dtype=I32, device=DEV), hs.to(DEV), tokens, max_ngram)
    assert torch.equal(tokens[:, 1:].cpu(), want)
    assert bool((tokens[:, 0] == -5).all())


# (drafts, tgt, finished, cur_len): k = 3, L = 12, pad 0, stop ids {2, 9}
ACCEPT = {
    "accept_0": ([[5, 6, 7], [5, 6, 7]], [[4, 6, 7, 8], [5, 6, 7, 8]], [0, 0], 6),
    "accept_some": ([[5, 6, 7], [5, 6, 7]], [[5, 6, 1, 8], [5, 6, 7, 8]], [0, 0], 6),
    "accept_all": ([[5, 6, 7], [5, 6, 7]], [[5, 6, 7, 8], [5, 6, 7, 3]], [0, 0], 6),
    "finished_row_ignored": ([[5, 6, 7], [1, 1, 1]], [[5, 6, 7, 8], [4, 4, 4, 4]], [0, 1], 6),
    "stop_inside_run": ([[5, 9, 7], [5, 6, 7]], [[5, 9, 7, 8], [5, 6, 7, 8]], [0, 0], 6),
    "clamp_at_max_length": ([[5, 6, 7], [5, 6, 7]], [[5, 6, 7, 8], [5, 6, 7, 8]], [0, 0], 10),
    "buffer_full": ([[5, 6, 7], [5, 6, 7]], [[5, 6, 7, 8], [5, 6, 7, 8]], [0, 0], 12),
}


@pytest.mark.parametrize("case", list(ACCEPT))
def test_spec_accept_kernel(case):
    drafts, tgt, fin, cl = ACCEPT[case]
    drafts, tgt = torch.tensor(drafts, dtype=I32), torch.tensor(tgt, dtype=I32)
    b, k, length, pad = drafts.shape[0], drafts.shape[1], 12, 0
    stop = ops.id_buffer([2, 9], ops.PROC_MAX_STOP, "cpu")
    seq = torch.arange(b * length, dtype=I32).reshape(b, length) + 100
    want_seq, want_fin = seq.clone(), torch.tensor(fin, dtype=I32)
    n = ref.spec_accept(drafts, tgt, want_fin, want_seq, cl, pad, stop.tolist())
    tokens = torch.cat([torch.full((b, 1), 77, dtype=I32), drafts], 1).to(DEV)
    pos = (torch.tensor([[20], [30]], dtype=I32) + torch.arange(k + 1, dtype=I32)).to(DEV)
    finished, seq_d = torch.tensor(fin, dtype=I32, device=DEV), seq.to(DEV)
    cur_len, slot = torch.tensor([cl], dtype=I32, device=DEV), torch.tensor([cl - 1], dtype=I32, device=DEV)
    ops.spec_accept(tgt.to(DEV), finished, seq_d, cur_len, tokens, pos, slot, pad, stop.to(DEV))
    assert torch.equal(seq_d.cpu(), want_seq) and torch.equal(finished.cpu(), want_fin)
    assert (int(cur_len), int(slot)) == (cl + n, cl - 1 + n)
    assert pos.cpu().tolist() == [[20 + n + s for s in range(k + 1)], [30 + n + s for s in range(k + 1)]]
    assert tokens[:, 0].cpu().tolist() == ([77, 77] if n == 0 else want_seq[:, cl + n - 1].tolist())


@pytest.fixture(scope="module")
def model():
    cfg = gpu_config()
    params = build(cfg, seed=3)[3]
    return LLaMAForCausalLM(cfg, device=DEV, _do_init=False).load_params(params)


@pytest.mark.parametrize("batch", [1, 4])
def test_lookup_generate_matches_plain_greedy(model, batch):
    lens = [max(2, 11 - (3 * i) % 9) for i in range(batch)]
    toks, mask = left_padded_batch(lens, 11, model.config.vocab_size, pad=2, seed=4)
    gc = dict(max_length=40, do_sample=False, pad_token_id=2, eos_token_id=2)
    got = model.generate(toks, attention_mask=mask,
                         generation_config=GenerationConfig(prompt_lookup_num_tokens=3, **gc)).sequences.cpu()
    want = model.generate(toks, attention_mask=mask, generation_config=GenerationConfig(**gc)).sequences.cpu()
    # the same rounding points, another summation order across M: near-ties may flip
    assert (got.long() == want.long()).float().mean().item() > 0.97
    assert torch.equal(got[:, :11], toks)


def test_lookup_graph_replay_matches_eager(model):
    toks, mask = left_padded_batch([5, 8], 8, model.config.vocab_size, pad=2, seed=6)
    gc = GenerationConfig(max_length=48, do_sample=False, pad_token_id=2, eos_token_id=2, prompt_lookup_num_tokens=3)
    a = LookupEngine(model, 2, 48, 3, use_graph=True).run(toks, mask, gc).clone()
    b = LookupEngine(model, 2, 48, 3, use_graph=False).run(toks, mask, gc).clone()
    assert torch.equal(a, b)
