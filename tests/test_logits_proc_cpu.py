"""The logits processors without a GPU: ``ops/reference.py`` against the host transcription of
tests/logits_proc_inputs.py bit for bit, the CPU engine against the host loop on the scripted model (which also checks
that every scenario of the GPU tests meets its conditions), the validation errors, and a world-2 gloo run."""
from __future__ import annotations

import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import logits_proc_inputs as lp
import loop_inputs as li
from jax_llama_amd import ops
from jax_llama_amd.models import LLaMAForCausalLM
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime.engine import DecodeEngine, GenerationConfig
from jax_llama_amd.utils.checkpoint import meta_state_dict_to_params, random_meta_state_dict
from helpers import gpu_config

I32 = torch.int32
_NEG_INF = float("-inf")


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal, and the signs of the zeros too."""
    return torch.equal(a, b) and np.array_equal(np.signbit(a.numpy()), np.signbit(b.numpy()))


def _both(x, seq, cur_len, start, col_offset, vocab, p, n, suppress, stop, min_len):
    want = lp.process(x, seq, cur_len, start.tolist(), col_offset, vocab, p, n, suppress, stop, min_len)
    cfg = ref.LogitsProcessors(p, n, suppress, stop, min_len, vocab)
    got = ref.process_logits(x.clone(), seq, cur_len, start, col_offset, cfg)
    return got, want


OPTIONS = [dict(p=1.3), dict(p=0.7), dict(n=1), dict(n=2), dict(n=3), dict(suppress=[3, 17, 255, 256, 999]),
           dict(stop=[4, 200], min_len=1000), dict(stop=[4, 200], min_len=1),
           dict(p=1.25, n=2, suppress=[9, 300], stop=[5, 6, 7], min_len=1000)]


@pytest.mark.parametrize("opt", OPTIONS, ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()).replace(" ", ""))
@pytest.mark.parametrize("b,v,hist_len,kind", [(3, 300, 40, "random"), (2, 64, 200, "random"), (3, 300, 100, "same"),
                                               (2, 300, 101, "two")])
def test_reference_is_the_transcription(b, v, hist_len, kind, opt):
    """Random rows with +0.0, -0.0 and -inf at history tokens, ids outside the vocabulary in the history, a token
    repeated 100 times and two alternating ones."""
    x, seq, cur_len, start = lp.kernel_case(b, v, hist_len, kind=kind, seed=1)
    o = dict(p=1.0, n=0, suppress=[], stop=[], min_len=0)
    o.update(opt)
    got, want = _both(x, seq, cur_len, start, 0, v, **o)
    assert _same(got, want)
    assert _same(got, x) == (opt.get("min_len") == 1)  # every option but the lapsed minimum length changes something


def test_a_repeated_token_is_penalised_once():
    x = torch.tensor([[4.0, -4.0, 2.0, 0.0, -0.0, _NEG_INF, 1.0, 1.0]])
    seq = torch.tensor([[0] * 100 + [1] * 100 + [3, 4, 5, 3, 4, 5, 6]], dtype=I32)
    got, want = _both(x, seq, 207, torch.zeros(1, dtype=I32), 0, 8, 1.6, 0, [], [], 0)
    assert _same(got, want)
    inv = np.float32(1 / 1.6)
    assert got[0].tolist() == [float(np.float32(4.0) * inv), float(np.float32(-4.0) * np.float32(1.6)), 2.0, 0.0, -0.0,
                               _NEG_INF, float(inv), 1.0]
    assert not np.signbit(got.numpy()[0, 3]) and np.signbit(got.numpy()[0, 4])


@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_ngram_ban_starts_at_history_length_n(n):
    """History lengths n - 2, n - 1 (nothing is banned) and n (the first length with an earlier n-gram: it bans only
    where the first n - 1 tokens equal the last n - 1, which a constant history does)."""
    for length in (n - 2, n - 1, n, n + 3):
        if length < 0:
            continue
        x = torch.zeros(2, 16)
        seq = torch.full((2, 12), 7, dtype=I32)
        seq[1] = torch.arange(12, dtype=I32)  # no repeated (n - 1)-gram: nothing to ban for n >= 2
        start = torch.full((2,), 2, dtype=I32)
        got, want = _both(x, seq, 2 + length, start, 0, 16, 1.0, n, [], [], 0)
        assert _same(got, want)
        banned0 = (got[0] == _NEG_INF).nonzero().reshape(-1).tolist()
        banned1 = (got[1] == _NEG_INF).nonzero().reshape(-1).tolist()
        assert banned0 == ([7] if length >= n else [])
        assert banned1 == (list(range(2, 2 + length)) if n == 1 else [])


def test_empty_history_changes_nothing():
    x, seq, cur_len, _ = lp.kernel_case(3, 100, 20, seed=2)
    start = torch.full((3,), cur_len, dtype=I32)
    got, want = _both(x, seq, cur_len, start, 0, 100, 1.5, 2, [], [7], 0)
    assert _same(got, want) and _same(got, x)
    got, _ = _both(x, seq, cur_len, start + 5, 0, 100, 1.5, 1, [], [], 0)  # a start past cur_len: empty too
    assert _same(got, x)


@pytest.mark.parametrize("shards", [2, 4])
def test_col_offset_shards_make_the_unsharded_result(shards):
    v = 256
    x, seq, cur_len, start = lp.kernel_case(3, v, 150, seed=3)
    o = dict(p=1.25, n=2, suppress=[0, 63, 64, 127, 128, 255], stop=[64, 191], min_len=1000)
    whole, want = _both(x, seq, cur_len, start, 0, v, **o)
    assert _same(whole, want)
    vl = v // shards
    parts = []
    for r in range(shards):
        got, want = _both(x[:, r * vl:(r + 1) * vl].contiguous(), seq, cur_len, start, r * vl, v, **o)
        assert _same(got, want)
        parts.append(got)
    assert _same(torch.cat(parts, 1), whole)


def test_ops_process_logits_on_cpu_tensors_is_the_reference():
    x, seq, cur_len, start = lp.kernel_case(3, 300, 60, seed=4)
    want = lp.process(x, seq, cur_len, start.tolist(), 0, 300, 1.3, 2, [5], [6, 7], 1000)
    got = ops.process_logits(x.clone(), seq, torch.tensor([cur_len], dtype=I32), start, 0, 300, 1.3, 2,
                             ops.id_buffer([5], 64, "cpu"), ops.id_buffer([6, 7], 8, "cpu"),
                             torch.tensor([1000], dtype=I32))
    assert _same(got, want)
    with pytest.raises(ValueError):  # fp32 rows only
        ops.process_logits(x.double(), seq, torch.tensor([cur_len], dtype=I32), start, 0, 300, 1.3, 2,
                           ops.id_buffer([5], 64, "cpu"), ops.id_buffer([6, 7], 8, "cpu"), torch.tensor([0], dtype=I32))


# ----------------------------------------------------------------------------------
# the CPU engine on the scripted model
# ----------------------------------------------------------------------------------
_MODEL = []


def _model():
    if not _MODEL:
        cfg = li.config()
        _MODEL.append(LLaMAForCausalLM(cfg, device="cpu", _do_init=False).load_params(
            meta_state_dict_to_params(li.state_dict(li.SAMPLE_LEVELS), cfg.num_hidden_layers)))
    return _MODEL[0]


gc_of = lp.generation_config


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("name", lp.GREEDY_SCENARIOS + ("sampled",))
def test_cpu_engine_is_the_host_loop(name, b, variant):
    sc = lp.scenario(name, b, variant)
    want = lp.expected(sc)  # asserts the scenario's conditions
    got = _model().generate(sc.toks, attention_mask=sc.mask, generation_config=gc_of(sc)).sequences
    assert torch.equal(got.to(I32), want)


def test_padding_is_not_history():
    """The penalty scenario's pad token is the third token row 1 generates: an engine that counted the padding as
    history (the host loop with every column attended shows what it would give) would change that row."""
    sc = lp.scenario("penalty", 3)
    want = lp.expected(sc)
    counted = lp.host_generate(li.SAMPLE_LEVELS, sc.toks, torch.ones_like(sc.mask), sc.max_length, sc.pad, sc.proc)
    assert not torch.equal(counted[1], want[1]) and torch.equal(counted[0], want[0])
    eng = DecodeEngine(_model(), 3, sc.max_length)
    got = eng.run(sc.toks, sc.mask, gc_of(sc)).to(I32)
    assert eng.hist_start.tolist() == lp.first_attended(sc.mask) == [0, 2, 1]
    assert torch.equal(got, want) and not torch.equal(got[1], counted[1])


@pytest.mark.parametrize("name", sorted(lp.STALE))
def test_one_cpu_engine_two_runs(name):
    """lp.two_runs asserts that run 2 gives other tokens with any of run 1's values it must not keep (lp.STALE); one
    engine then runs both."""
    first, want1, second, want2 = lp.two_runs(name)
    eng = DecodeEngine(_model(), 3, first.max_length)
    assert torch.equal(eng.run(first.toks, first.mask, gc_of(first)).to(I32), want1)
    assert torch.equal(eng.run(second.toks, second.mask, gc_of(second)).to(I32), want2)


def test_a_hole_after_the_first_attended_column_is_history():
    sc = lp.scenario("penalty", 1)
    holed = sc.mask.clone()
    first = lp.first_attended(sc.mask)[0]
    holed[0, first + 1] = 0
    assert lp.first_attended(holed) == [first]
    eng = DecodeEngine(_model(), 1, sc.max_length)
    eng.run(sc.toks, holed, gc_of(sc))
    assert eng.hist_start.tolist() == [first]
    eng.run(sc.toks, torch.zeros_like(holed), gc_of(sc))
    assert eng.hist_start.tolist() == [sc.toks.shape[1]]  # fully masked: the history starts with the first new token


def test_min_length_counts_the_prompt():
    sc = lp.scenario("min_new", 1)
    s = sc.toks.shape[1]
    a = _model().generate(sc.toks, attention_mask=sc.mask, generation_config=gc_of(sc)).sequences
    sc.proc = lp.Proc(min_length=s + sc.proc.min_new_tokens, stop=sc.proc.stop)
    b = _model().generate(sc.toks, attention_mask=sc.mask, generation_config=gc_of(sc)).sequences
    assert torch.equal(a, b) and torch.equal(b.to(I32), lp.expected(sc))


def test_single_id_stop_list_is_the_single_eos():
    sc = lp.scenario("min_new", 1)
    eos = sc.proc.stop[0]
    a = _model().generate(sc.toks, attention_mask=sc.mask, generation_config=gc_of(sc, single_eos=eos)).sequences
    b = _model().generate(sc.toks, attention_mask=sc.mask, generation_config=gc_of(sc, single_eos=[eos])).sequences
    assert torch.equal(a, b) and torch.equal(a.to(I32), lp.expected(sc))


def test_default_options_keep_the_fused_argmax_and_the_graph_key():
    model = _model()
    eng = DecodeEngine(model, 1, 12)
    sc = lp.scenario("penalty", 1)
    eng.run(sc.toks[:, :4], None, GenerationConfig(max_length=12, pad_token_id=0, eos_token_id=7))
    assert eng._logits_mode() == "argmax" and not eng._processors and not eng._stop_set
    key = eng._graph_state()
    assert len(key) == 11 and key[9] == 7
    eng.run(sc.toks[:, :4], None, GenerationConfig(max_length=12, pad_token_id=0, eos_token_id=7,
                                                   repetition_penalty=1.1))
    assert eng._logits_mode() == "last" and eng._graph_state()[-1] == (1.1, 0)
    eng.run(sc.toks[:, :4], None, GenerationConfig(max_length=12, pad_token_id=0, eos_token_id=[7, 8]))
    assert eng._logits_mode() == "argmax" and eng._graph_state()[-2:] == (True, None)


# ----------------------------------------------------------------------------------
# the public interface
# ----------------------------------------------------------------------------------
def test_generate_kwargs_are_no_longer_dropped():
    sc = lp.scenario("penalty", 1)
    model = _model()
    plain = model.generate(sc.toks, attention_mask=sc.mask, max_length=sc.max_length, pad_token_id=0,
                           eos_token_id=-1).sequences
    got = model.generate(sc.toks, attention_mask=sc.mask, max_length=sc.max_length, pad_token_id=0, eos_token_id=-1,
                         repetition_penalty=1.25).sequences
    assert not torch.equal(got, plain)
    assert torch.equal(got.to(I32), lp.expected(sc))
    for kw in (dict(no_repeat_ngram_size=1), dict(suppress_tokens=[int(plain[0, sc.toks.shape[1]])]),
               dict(bad_words_ids=[[int(plain[0, sc.toks.shape[1]])]])):
        other = model.generate(sc.toks, attention_mask=sc.mask, max_length=sc.max_length, pad_token_id=0,
                               eos_token_id=-1, **kw).sequences
        assert not torch.equal(other, plain)


@pytest.mark.parametrize("kw", [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0),
                                dict(no_repeat_ngram_size=-1), dict(min_length=-1), dict(min_new_tokens=-2),
                                dict(eos_token_id=list(range(9))), dict(eos_token_id=[]), dict(eos_token_id=[256]),
                                dict(eos_token_id=[3, -1]), dict(suppress_tokens=list(range(65))),
                                dict(suppress_tokens=[256]), dict(suppress_tokens=[-1]),
                                dict(bad_words_ids=[[256]]),
                                dict(num_beams=2, repetition_penalty=1.2), dict(num_beams=2, no_repeat_ngram_size=2),
                                dict(num_beams=2, eos_token_id=[3, 4]), dict(num_beams=2, min_new_tokens=2),
                                dict(num_beams=2, min_length=2), dict(num_beams=2, suppress_tokens=[5]),
                                dict(num_beams=2, bad_words_ids=[[5]])],
                         ids=lambda kw: "-".join(kw))
def test_validation_errors(kw):
    toks = torch.tensor([[1, 2, 3]], dtype=I32)
    with pytest.raises(ValueError):
        _model().generate(toks, max_length=8, pad_token_id=0, **({"eos_token_id": 5} | kw))


def test_multi_token_bad_words_are_not_implemented():
    with pytest.raises(NotImplementedError):
        _model().generate(torch.tensor([[1, 2, 3]], dtype=I32), max_length=8, pad_token_id=0, eos_token_id=5,
                          bad_words_ids=[[4, 5]])


class _Tok:
    bos_id, eos_id = 1, 2

    def encode(self, s, bos, eos):
        return ([1] if bos else []) + [int(t) for t in s.split()]

    def decode(self, t):
        return " ".join(str(x) for x in t)


def test_generate_from_str_cuts_at_any_stop_token():
    from jax_llama_amd import LLaMA
    sc = lp.scenario("stop_set", 3)
    want = lp.expected(sc)
    llama = LLaMA(None, _model(), _Tok())
    prompts = [" ".join(str(int(t)) for t, m in zip(row, mrow) if m) for row, mrow in zip(sc.toks.tolist(),
                                                                                          sc.mask.tolist())]
    width = 1 + max(len(p.split()) for p in prompts)
    gen = sc.max_length - width
    out = llama.generate_from_str(prompts, gen, temperature=0.0, stop_token_ids=sc.proc.stop)
    s = sc.toks.shape[1]
    for r, text in enumerate(out):
        toks = [int(t) for t in text.split()]
        new = toks[1 + len(prompts[r].split()):]
        full = [int(t) for t in want[r, s:].tolist()]
        stop_at = min(i for i, t in enumerate(full) if t in sc.proc.stop)
        assert new == full[:stop_at] and len(new) < gen
    # without a stop list: as before, one eos
    plain = llama.generate_from_str(prompts, gen, temperature=0.0)
    assert all(len(t.split()) == 1 + len(p.split()) + gen for t, p in zip(plain, prompts))
    with pytest.raises(ValueError):
        llama.generate_from_str(prompts, gen, temperature=0.0, num_beams=2, stop_token_ids=sc.proc.stop)


# ----------------------------------------------------------------------------------
# vocab-parallel TP (gloo)
# ----------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _tp_state_dict(cfg):
    """The scripted model with two kv heads (one per rank): attention's weights are random in it anyway."""
    sd = random_meta_state_dict(cfg, seed=0)
    base = li.state_dict(li.SAMPLE_LEVELS)
    for k, t in base.items():
        if sd[k].shape == t.shape:
            sd[k] = t
    return sd


def _worker(rank, world, port, names, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        from jax_llama_amd.parallel import TPComm, init_distributed
        ctx = init_distributed(backend="gloo", device_type="cpu")
        ctx.setup_mesh(tp=world)
        comm = TPComm.from_context(ctx)
        cfg = gpu_config(vocab_size=li.V, hidden_size=li.V, num_key_value_heads=2)
        model = LLaMAForCausalLM(cfg, comm=comm, _do_init=False).load_params(
            meta_state_dict_to_params(_tp_state_dict(cfg), cfg.num_hidden_layers))
        outs = []
        for name in names:
            sc = lp.scenario(name, 3)
            outs.append(model.generate(sc.toks, attention_mask=sc.mask, generation_config=gc_of(sc)).sequences)
        if rank == 0:
            q.put(("ok", outs))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # pragma: no cover - surfaced in the parent
        import traceback
        q.put(("err", traceback.format_exc()))


def test_world_2_gloo_is_the_single_process_run():
    """Every rank processes its own half of the vocabulary (col_offset); the tokens are the host loop's, which the
    single-process engine's are (test_cpu_engine_is_the_host_loop)."""
    names = ("all", "sampled")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, names, q)) for r in range(2)]
    for p in procs:
        p.start()
    status, outs = q.get(timeout=240)
    for p in procs:
        p.join(timeout=120)
    assert status == "ok", outs
    for name, got in zip(names, outs):
        assert torch.equal(got.to(I32), lp.expected(lp.scenario(name, 3))), name
