"""The scripted decode-loop fixture (tests/loop_inputs.py) validated without a GPU: the CPU model path and the fp32
oracle give the analytic logits, ``model.generate`` on the CPU equals the plain host loop token for token, the chosen
sampling seeds keep the margins the GPU tests rely on, and the reference sampler draws from the true distribution at
the sampler's real sizes."""
from __future__ import annotations

import pytest
import torch

import loop_inputs as li
from jax_llama_amd.models import LLaMAForCausalLM
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime.engine import GenerationConfig
from jax_llama_amd.utils.checkpoint import meta_state_dict_to_params
from oracle import OracleLLaMA

_MODELS = {}


def _model(levels):
    if levels not in _MODELS:
        cfg = li.config()
        sd = li.state_dict(levels)
        model = LLaMAForCausalLM(cfg, device="cpu", _do_init=False).load_params(
            meta_state_dict_to_params(sd, cfg.num_hidden_layers))
        oracle = OracleLLaMA(sd, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.num_key_value_heads,
                             cfg.rms_norm_eps, cfg.rope_theta)
        _MODELS[levels] = (model, oracle)
    return _MODELS[levels]


def test_fixture_algebra():
    h = li.hadamard()
    assert torch.equal(h @ h.t(), 256 * torch.eye(256, dtype=torch.float64))
    x = torch.arange(256)
    for j in range(4):
        assert sorted(li.succ(x, j).tolist()) == list(range(256))  # every level: one predecessor per token
    assert len({int(li.succ(torch.tensor(7), j)) for j in range(4)}) == 4
    seen, t = set(), 0
    for _ in range(256):
        seen.add(t)
        t = int(li.succ(t))
    assert len(seen) == 256 and t == 0  # successor 0 is one 256-cycle: a greedy row meets eos when the test says
    assert li.pred(int(li.succ(li.succ(99))), 2) == 99


@pytest.mark.parametrize("levels", [li.GREEDY_LEVELS, li.SAMPLE_LEVELS])
def test_logits_are_the_analytic_rows(levels):
    """Exact zeros off the successors and the levels within 1e-4 relative, from the CPU model path (bf16 rounding
    points: the normed row is the +-1 row, every product and partial sum of the lm_head is exact) and from the fp32
    oracle with eps = 0 (the same: rsqrt(1 + 0) = 1, and there the levels are exact too).

    The oracle at the config's eps = 1e-5 cannot give exact zeros: its normed row is +-fl32(1 / sqrt(1 + 1e-5)) =
    +-0.99999499, a 24-bit number whose multiples (256 terms of up to 26 / 256 of it per logit) do not add up exactly
    in fp32; measured 6.7e-8 (one level) and 1.0e-7 (four levels). Its zeros are held to the fp32 summation bound
    (n + 1) * 2^-24 * sum|terms| = 257 * 2^-24 * 26 = 4e-4, five orders below a misplaced level."""
    model, oracle = _model(levels)
    toks, mask = li.prompts([0, 1, 77, 255], [3, 9, 5, 9], 9, pad=2, seed=1)
    pos = mask.cumsum(-1) - 1
    want = li.analytic_logits(toks[:, -1], levels)
    on = want != 0
    assert int(on.sum()) == 4 * len(levels)
    exact = OracleLLaMA(oracle.sd, oracle.L, oracle.H, oracle.Hkv, 0.0, li.config().rope_theta)
    eps_oracle = oracle.forward(toks, mask, pos)[:, -1].float()
    for got in (model(toks, attention_mask=mask, position_ids=pos).logits[:, -1].float(),
                exact.forward(toks, mask, pos)[:, -1].float(), eps_oracle):
        if got is eps_oracle:
            assert float(got[~on].abs().max()) <= 257 * 2.0 ** -24 * sum(levels)
        else:
            assert torch.all(got[~on] == 0)
        assert float(((got[on] - want[on]).abs() / want[on]).max()) < 1e-4
    assert torch.equal(exact.forward(toks, mask, pos)[:, -1].float(), want)


def _cases():
    """(name, last tokens, lengths, S, max_length, pad, eos): rows that meet eos at their 1st, 3rd and last new token,
    a row that never does, eos = -1, pad == eos and pad != eos, max_length = S + 1."""
    eos = 200
    last = [li.pred(eos, 1), li.pred(eos, 3), li.pred(eos, 7), li.pred(eos, 100)]
    yield "pad_is_eos", last, [2, 6, 4, 6], 6, 13, eos, eos
    yield "pad_not_eos", last, [2, 6, 4, 6], 6, 13, 0, eos
    yield "no_eos", last, [6, 1, 3, 2], 6, 13, 0, -1
    yield "one_token", last, [2, 6, 4, 6], 6, 7, 0, eos
    yield "single_row", last[1:2], [5], 5, 12, 2, eos


@pytest.mark.parametrize("case", list(_cases()), ids=lambda c: c[0])
def test_cpu_greedy_generate_is_the_host_loop(case):
    _, last, lengths, s, max_length, pad, eos = case
    model, _ = _model(li.GREEDY_LEVELS)
    toks, mask = li.prompts(last, lengths, s, pad, seed=3)
    want = li.host_generate(li.GREEDY_LEVELS, toks, mask, max_length, pad, eos)
    gc = GenerationConfig(max_length=max_length, do_sample=False, pad_token_id=pad, eos_token_id=eos)
    got = model.generate(toks, attention_mask=mask, generation_config=gc).sequences
    assert torch.equal(got.cpu().to(torch.int32), want)
    if eos >= 0 and max_length == s + 7 and len(last) == 4:  # the script did what the case says
        new = want[:, s:]
        assert int(new[0, 0]) == eos and int(new[1, 2]) == eos and int(new[2, 6]) == eos
        assert torch.all(new[0, 1:] == pad) and torch.all(new[1, 3:] == pad)
        assert not bool((new[:, :6] == eos)[2].any()) and not bool((new[3] == eos).any())


SAMPLE_SETTINGS = sorted({s for pair in li.SAMPLE_PAIRS.values() for s in pair})


@pytest.mark.parametrize("sample", SAMPLE_SETTINGS)
@pytest.mark.parametrize("eos_at,pad_is_eos,max_length", [(0, True, 16), (2, False, 16), (9, False, 16),
                                                          (None, False, 16), (0, False, 7)])
def test_cpu_sampled_generate_is_the_host_loop(sample, eos_at, pad_is_eos, max_length):
    """eos = the token row 0 draws as its (eos_at + 1)-th new one in a run without eos: 1st, 3rd and last. The
    guarded host loop asserts the seeds' margins (score lead >= 1e-2, top_p distance >= 1e-3) on every draw."""
    model, _ = _model(li.SAMPLE_LEVELS)
    s = li.SAMPLE_S
    eos = -1 if eos_at is None else li.sampled_eos(sample, eos_at)
    pad = eos if pad_is_eos else 0
    toks, mask = li.sample_batch(pad)
    want = li.guarded_host_generate(toks, mask, max_length, pad, eos, sample)
    if eos_at is not None:
        assert int(want[0, s + eos_at]) == eos and torch.all(want[0, s + eos_at + 1:] == pad)
        assert not bool((want[0, s:s + eos_at] == eos).any())
    k, t, p, seed = sample
    gc = GenerationConfig(max_length=max_length, do_sample=True, top_k=k, temperature=t, top_p=p, seed=seed,
                          pad_token_id=pad, eos_token_id=eos)
    got = model.generate(toks, attention_mask=mask, generation_config=gc).sequences
    assert torch.equal(got.cpu().to(torch.int32), want)


def test_sampled_rows_take_several_successors_and_settings_differ():
    """The sampling script is not greedy in disguise (the guarded run takes lower-level successors too), and every
    variant of the settings changes the tokens: a run that replays stale settings cannot pass by coincidence."""
    toks, mask = li.sample_batch()
    s = li.SAMPLE_S
    seq = li.guarded_host_generate(toks, mask, 26, 0, -1, li.SAMPLE_BASE)
    prev, new = seq[:, s - 1:-1].long(), seq[:, s:].long()
    ranks = {j for j in range(4) if bool((new == li.succ(prev, j)).any())}
    assert len(ranks) >= 3
    for name, (first, second) in li.SAMPLE_PAIRS.items():
        one = li.guarded_host_generate(toks, mask, 26, 0, -1, first)
        two = li.guarded_host_generate(toks, mask, 26, 0, -1, second)
        assert not torch.equal(one[:, s + 2:], two[:, s + 2:]), name


def test_sample_detail_is_the_reference():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(64, 2000, generator=g) * 2
    for k, t, p in [(50, 0.8, 0.9), (50, 1.0, 1.0), (64, 1.3, 0.5), (1, 1.0, 0.9)]:
        tok, lead, dist = li.sample_detail(x, k, t, p, 9, 3)
        assert torch.equal(tok, ref.topk_sample(x, k, t, p, 9, 3))
        assert bool((lead >= 0).all()) and bool((dist >= 0).all())


@pytest.mark.parametrize("k,temperature,top_p", [(50, 0.8, 0.9), (50, 1.0, 1.0)])
def test_reference_sampler_draws_the_true_distribution(k, temperature, top_p):
    """4096 identical rows are 4096 independent draws (the row index is a Philox counter word)."""
    g = torch.Generator().manual_seed(21)
    row = torch.randn(2000, generator=g) * 2
    draws = ref.topk_sample(row.expand(4096, 2000), k, temperature, top_p, 1234, 7)
    chi, df = li.check_draws(draws, row, k, temperature, top_p)
    print(f"chi-square {chi:.1f} at df {df} (bound {li.chi2_bound(df):.1f})")
    assert df >= 10


def test_reference_top_p_at_a_cumulative_sum_excludes_the_candidate():
    row = li.top_p_boundary_row()
    draws = ref.topk_sample(row.expand(4096, row.numel()), 4, 1.0, 0.5, 77, 3)
    assert sorted(set(draws.tolist())) == [1, 3]
    ids, q = li.true_distribution(row, 4, 1.0, 0.5)
    assert ids.tolist() == [1, 3] and q.tolist() == [0.5, 0.5]
    li.check_draws(draws, row, 4, 1.0, 0.5)


def test_chi2_bound():
    assert 85.0 < li.chi2_bound(33) < 89.0
