"""Beam search without a GPU: ``ops/reference.py``'s tensor form of the step and the loop condition equal the literal
per-item transcription (tests/beam_inputs.py) bit for bit, the scripted cases hit what they are listed for, and
``model.generate(num_beams=K)`` on the CPU model path equals the host search (sequences exactly, scores within the
derived bound)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import beam_inputs as bi
import loop_inputs as li
from jax_llama_amd.models import LLaMAForCausalLM
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime import engine as eng_mod
from jax_llama_amd.runtime.engine import GenerationConfig
from jax_llama_amd.utils.checkpoint import meta_state_dict_to_params

_MODEL = []


def _model():
    if not _MODEL:
        cfg = li.config()
        _MODEL.append(LLaMAForCausalLM(cfg, device="cpu", _do_init=False).load_params(
            meta_state_dict_to_params(bi.state_dict(), cfg.num_hidden_layers)))
    return _MODEL[0]


def test_scripted_logits_are_the_analytic_rows():
    model = _model()
    toks, mask = li.prompts([0, 1, 77, bi.END], [3, 9, 5, 9], 9, pad=2, seed=1)
    pos = mask.cumsum(-1) - 1
    want = bi.analytic_logits(toks[:, -1])
    got = model(toks, attention_mask=mask, position_ids=pos).logits[:, -1].float()
    on = want != 0
    assert torch.all(got[~on] == 0)
    assert float(((got[on] - want[on]).abs() / want[on]).max()) < bi.LOGIT_FACTOR


@pytest.mark.parametrize("seed", range(24))
def test_reference_step_is_the_transcription(seed):
    """Random inputs and tie-laden small integers (equal scores across beams and ranks, eos among the candidates,
    items whose slots are all finished), every early_stopping mode and length penalty, c up to L - 1."""
    k, b, length, s, eos = [2, 3, 4, 8][seed % 4], 3, 12, 4, 5
    c = [4, 7, 11][seed % 3]
    ties = seed % 2 == 0
    early = [False, True, "never"][(seed // 2) % 3]
    lp = [0.0, 1.0, 2.0][(seed // 3) % 3]
    cv, ci, lse, rseq, seq, rs, sc, fin = bi.random_step_inputs(seed, b, k, length, ties, all_finished=seed % 5 == 0)
    inv_pen = ref.beam_inv_pen(length, lp)
    table = bi.inv_pen_table(length, lp)
    assert np.array_equal(np.asarray(table, dtype=np.float32), inv_pen.numpy())
    out = ref.beam_step(cv, ci, lse, rseq, seq, rs, sc, fin, inv_pen, c, s, eos, early)
    items = bi.items_from_tensors(rseq, seq, rs, sc, fin)
    for i, st in enumerate(items):
        cands = [[(np.float32(cv[i * k + j, n]), int(ci[i * k + j, n])) for n in range(2 * k)] for j in range(k)]
        lses = [np.float32(lse[i * k + j]) for j in range(k)]
        beam_idx, toks = bi.item_step(st, cands, lses, c, s, eos, early, table)
        assert out[0][i].tolist() == st.running_seq and out[1][i].tolist() == st.seq
        assert np.array_equal(out[2][i].numpy(), np.asarray(st.running_score, dtype=np.float32))
        assert np.array_equal(out[3][i].numpy(), np.asarray(st.score, dtype=np.float32))
        assert out[4][i].tolist() == st.is_finished
        assert out[5][i].tolist() == beam_idx and out[6][i].tolist() == toks
    for cc in (s, c, length):
        fresh = bi.items_from_tensors(rseq, seq, rs, sc, fin)
        assert (ref.beam_continue(rs, sc, fin, inv_pen, cc, s, length, early, lp) ==
                bi.search_continues(fresh, cc, s, length, early, lp, table))


def test_cases_hit_what_they_are_listed_for():
    steps = {name: bi.case(name)[9] for name in bi.CASES}
    full = bi.MAX_LENGTH - bi.S
    # a beam finishes on eos mid-run while others go on, and a finished hypothesis is later displaced
    for name in ("k2_lp1", "k4_lp1"):
        trace, k = bi.case(name)[10], bi.case(name)[2]
        mid = displaced = False
        for item in range(3):
            prev = set()
            for t, (_, rec) in enumerate(trace):
                _, fin, score = rec[item]
                real = {float(v) for v, f in zip(score, fin) if f}
                mid |= bool(real - prev) and t < len(trace) - 2 and len(real) < k
                displaced |= bool(prev - real)
                prev = real
        assert mid and displaced and steps[name] == full
    # length_penalty 0 / 1 / 2: three winners
    winners = {name: bi.case(name)[6].tolist() for name in ("k2_lp0", "k2_lp1", "k2_lp2")}
    assert len({str(w) for w in winners.values()}) == 3
    assert len({str(bi.case(n)[6].tolist()) for n in ("k4_lp0", "k4_lp1")}) == 2
    # early_stopping=True ends a run early; "never" runs longer than False
    assert steps["k2_early"] < full and steps["k4_early"] < full
    assert steps["k2_lp05"] < steps["k2_never"]
    # nothing finishes without an eos: the running beams are returned at max_length
    for name in ("k2_no_eos", "k4_no_eos"):
        assert steps[name] == full and not any(any(fin) for _, rec in bi.case(name)[10] for _, fin, _ in rec)
        assert int((bi.case(name)[6] == bi.PAD)[:, bi.S:].sum()) == 0


@pytest.mark.parametrize("name", list(bi.CASES))
def test_cpu_generate_is_the_host_search(name):
    toks, mask, k, eos, lp, early, seqs, scores, bound = bi.case(name)[:9]
    out = _model().generate(toks, attention_mask=mask, generation_config=GenerationConfig(
        max_length=bi.MAX_LENGTH, num_beams=k, pad_token_id=bi.PAD, eos_token_id=eos, length_penalty=lp,
        early_stopping=early))
    assert torch.equal(out.sequences.to(torch.int32), seqs)
    assert float((out.scores - scores).abs().max()) <= bound


def test_num_return_sequences():
    toks, mask, k, eos, lp, early, seqs, scores, bound = bi.case("k4_lp1", nrs=3)[:9]
    out = _model().generate(toks, attention_mask=mask, generation_config=GenerationConfig(
        max_length=bi.MAX_LENGTH, num_beams=k, pad_token_id=bi.PAD, eos_token_id=eos, num_return_sequences=3))
    assert out.sequences.shape == (9, bi.MAX_LENGTH) and out.scores.shape == (9,)
    assert torch.equal(out.sequences.to(torch.int32), seqs)
    assert float((out.scores - scores).abs().max()) <= bound
    one = bi.case("k4_lp1")[6]
    assert torch.equal(seqs[::3], one)  # the first of each prompt's three is the single best
    assert bool((out.scores.view(3, 3)[:, :-1] >= out.scores.view(3, 3)[:, 1:]).all())


def test_errors():
    model = _model()
    toks, mask = bi.batch(bi.LAST_TOKENS[2])

    def gen(**kw):
        return model.generate(toks, attention_mask=mask, generation_config=GenerationConfig(
            max_length=bi.MAX_LENGTH, pad_token_id=bi.PAD, eos_token_id=bi.END, **kw))

    for kw in (dict(num_beams=2, do_sample=True), dict(num_beams=9), dict(num_beams=0), dict(num_beams=-2),
               dict(num_beams=2, num_return_sequences=3), dict(num_beams=2, num_return_sequences=0),
               dict(num_beams=2, early_stopping="always")):
        with pytest.raises(ValueError):
            gen(**kw)

    class TwoRanks:
        size = 2

    comm = model.comm
    try:
        model.comm = TwoRanks()
        with pytest.raises(NotImplementedError):
            gen(num_beams=2)
    finally:
        model.comm = comm
    from jax_llama_amd.generation import LLaMA
    with pytest.raises(ValueError):  # beams with a temperature
        LLaMA(None, model, None).generate(toks, mask, 4, temperature=0.8, num_beams=2)


def test_one_beam_is_todays_path():
    model = _model()
    toks, mask = bi.batch(bi.LAST_TOKENS[2])
    for kw in (dict(do_sample=False), dict(do_sample=True, seed=3, top_k=8)):
        base = dict(max_length=bi.MAX_LENGTH, pad_token_id=bi.PAD, eos_token_id=bi.END, **kw)
        a = model.generate(toks, attention_mask=mask, generation_config=GenerationConfig(**base))
        b = model.generate(toks, attention_mask=mask, generation_config=GenerationConfig(num_beams=1, **base))
        assert torch.equal(a.sequences, b.sequences) and a.scores is None and b.scores is None
        assert type(eng_mod.get_engine(model, 3, bi.MAX_LENGTH)) is eng_mod.DecodeEngine
