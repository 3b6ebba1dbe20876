"""min_p and typical_p in ``ref.nucleus_sample``: the defaults are the definition as it was, the survivor sets are HF's
two warpers in lists and loops, the GPU tests' rows meet their margins, and ``generate`` takes the options."""
from __future__ import annotations

import math

import pytest
import torch

import loop_inputs as li
import nucleus_inputs as ni
import truncation_inputs as ti
from jax_llama_amd import ops
from jax_llama_amd.models import LLaMAForCausalLM
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime.engine import GenerationConfig, _min_p_typical, _sampler_route, generate
from jax_llama_amd.utils.checkpoint import meta_state_dict_to_params


def test_defaults_are_the_definition_as_it_was():
    x, _ = ni.gap_rows(8, 1025, 63, 0, 0.6, 0.9, seed=4)
    for top_k, top_p in ((0, 0.9), (65, 0.9), (0, 1.0)):
        was = ref.nucleus_sample(x, top_k, 0.6, top_p, 7, 2, True)
        now = ref.nucleus_sample(x, top_k, 0.6, top_p, 7, 2, True, min_p=0.0, typical_p=1.0)
        assert torch.equal(was[0], now[0]) and torch.equal(was[1], now[1])


def _warpers(l, min_p, typical_p):
    """HF's MinPLogitsWarper, then TypicalLogitsWarper, on one row of scaled logits: the surviving indices."""
    z = sum(math.exp(v - max(l)) for v in l)
    alive = [i for i in range(len(l)) if math.exp(l[i] - max(l)) / z >= min_p * (1 / z)]
    if typical_p < 1.0:
        z = sum(math.exp(l[i]) for i in alive)
        logp = {i: l[i] - math.log(z) for i in alive}
        ent = -sum(math.exp(v) * v for v in logp.values() if v > -math.inf)  # (nansum: a banned token adds 0)
        by_d = sorted(alive, key=lambda i: (abs(-logp[i] - ent), i))
        cum, last_ind = 0.0, 0
        for i in by_d:  # last_ind = (cumulative probs < mass).sum(), the position of the last token kept
            cum += math.exp(logp[i])
            last_ind += cum < typical_p
        alive = by_d[:min(last_ind, len(by_d) - 1) + 1]
    return sorted(alive)


@pytest.mark.parametrize("min_p,typical_p", [(0.1, 1.0), (0.0, 0.2), (0.0, 0.88), (0.1, 0.88), (1.0, 1.0)])
def test_survivors_are_hfs_warpers(min_p, typical_p):
    x = ti.rows(37, 1.0, 3)
    x[2, 5:9] = float(x[2].max())  # min_p = 1 keeps the equal maxima
    got = ref.nucleus_scores(x, 0, 1.0, 1.0, 1, 0, min_p, typical_p)
    assert [idx.tolist() for idx, _ in got] == [_warpers(row, min_p, typical_p) for row in x.double().tolist()]


@pytest.mark.parametrize("combo", ti.COMBOS)
def test_gpu_rows_meet_their_margins(combo):  # (case asserts them; the larger V hold the same head)
    assert all(ti.case("head", v, *combo)[3].min() >= 1 for v in (1023, 1024, 4100)) and ti.case("dead", 61, *combo)
    assert [int(ti.case("restream", 16384, 0, 1.0, 0.0, t)[3][0]) for t in (0.75, 0.88)] == [16376, 16377]


@pytest.mark.parametrize("min_p,typical_p", [(0.1, 1.0), (0.0, 0.2), (0.1, 0.88)])
def test_torch_path_keeps_the_definitions_survivors(min_p, typical_p):
    x = ti.rows(37, 1.0, 3)
    vals, idx = torch.sort(x, dim=-1, descending=True, stable=True)
    kept = _min_p_typical(vals, GenerationConfig(min_p=min_p, typical_p=typical_p)) > -math.inf
    want = ref.nucleus_scores(x, 0, 1.0, 1.0, 1, 0, min_p, typical_p)
    assert [sorted(idx[r][kept[r]].tolist()) for r in range(3)] == [i.tolist() for i, _ in want]


def test_generate_takes_the_options_and_routes_them_to_the_full_sampler():
    cfg = li.config()
    params = meta_state_dict_to_params(li.state_dict(li.SAMPLE_LEVELS), cfg.num_hidden_layers)
    model = LLaMAForCausalLM(cfg, device="cpu", _do_init=False).load_params(params)
    toks, mask = li.sample_batch(0)
    gc = GenerationConfig(max_length=20, do_sample=True, top_k=40, temperature=1.0, seed=2, pad_token_id=0,
                          eos_token_id=-1)
    assert _sampler_route(gc, 300, 1, True, True) == "topk"
    for opt in (dict(min_p=0.1), dict(typical_p=0.5)):
        assert _sampler_route(GenerationConfig(top_k=40, **opt), 300, 1, True, True) == "nucleus"
        got, tok = generate(model, toks, mask, gc, **opt).sequences, toks[:, -1].to(torch.int32)
        for cur in range(toks.shape[1], 20):  # the host loop over the definition
            tok = ref.nucleus_sample(li.analytic_logits(tok, li.SAMPLE_LEVELS), 40, 1.0, 1.0, 2, cur, **opt)
            assert torch.equal(got[:, cur].cpu().to(torch.int32), tok)
    for bad in (dict(min_p=1.5), dict(typical_p=None), dict(min_p=0.1, num_beams=2, do_sample=False)):
        with pytest.raises(ValueError):
            generate(model, toks, mask, gc, **bad)
    with pytest.raises(ValueError):
        ops.nucleus_sample(torch.zeros(1, 8), 0, 1.0, 1.0, 0, torch.zeros(1, dtype=torch.int32), typical_p=1.5)
