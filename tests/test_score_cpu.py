"""Scoring on the CPU path (ops/reference.py): ``LLaMAForCausalLM.score``, ``LLaMA.loglikelihood``, the shard combine
and a gloo world-2 run. The GPU kernels behind the same API are tested in test_logprob_gpu.py."""
from __future__ import annotations

import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import build, left_padded_batch, tiny_config
from jax_llama_amd import LLaMA, LLaMAForCausalLM, ScoreOutput, ops
from jax_llama_amd.utils.checkpoint import meta_state_dict_to_params, random_meta_state_dict
from test_tokenizers_checkpoint import llama3_tok  # noqa: F401  (fixture)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gathered(logits, labels):
    """log_softmax + gather in float64: entry [b, t-1] for labels[b, t] (clamped; the caller masks)."""
    v = logits.shape[-1]
    return torch.log_softmax(logits.double(), -1)[:, :-1].gather(-1, labels[:, 1:].long().clamp(0, v - 1)[..., None])[..., 0]


def _padded_case(seed=0):
    cfg = tiny_config()
    model, oracle, _, _ = build(cfg, seed=seed)
    toks, mask = left_padded_batch([12, 7, 3], 12, cfg.vocab_size, pad=0, seed=1)
    pos = mask.cumsum(-1) - 1
    own = model(toks, attention_mask=mask, position_ids=pos).logits.float()
    ref_logits = oracle.forward(toks, mask, pos).float()
    bound = 2 * float((own - ref_logits)[mask.bool()].abs().max())  # a log-prob cannot be off by more
    return cfg, model, toks, mask, own, ref_logits, bound


def test_score_matches_oracle():
    cfg, model, toks, mask, own, ref_logits, bound = _padded_case()
    out = model.score(toks, attention_mask=mask)
    assert isinstance(out, ScoreOutput) and out[0] is out.token_logprobs and out["mask"] is out.mask
    b, s = toks.shape
    assert out.token_logprobs.shape == out.is_greedy.shape == out.mask.shape == (b, s - 1)
    assert out.token_logprobs.dtype == torch.float32 and out.is_greedy.dtype == out.mask.dtype == torch.bool
    valid = (mask[:, :-1] != 0) & (mask[:, 1:] != 0)
    assert torch.equal(out.mask, valid) and 0 < int(valid.sum()) < valid.numel()
    lp = out.token_logprobs.double()
    err = float((lp - _gathered(ref_logits, toks))[valid].abs().max())
    print(f"score vs oracle {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert float((lp - _gathered(own, toks))[valid].abs().max()) <= 1e-5  # the same fp32 logits on this path
    assert torch.equal(out.is_greedy[valid], (own[:, :-1].argmax(-1) == toks[:, 1:])[valid])
    # masked entries: 0, true, false
    assert bool((out.token_logprobs[~valid] == 0).all()) and bool(out.is_greedy[~valid].all())
    # perplexity-style use: every entry is a log-probability
    assert float(lp[valid].max()) <= 0


def test_score_chunked_rows(monkeypatch):
    cfg, model, toks, mask, own, _, _ = _padded_case()
    whole = model.score(toks, attention_mask=mask)
    from jax_llama_amd.runtime import engine
    monkeypatch.setattr(engine, "PREFILL_TOKENS", 2 * toks.shape[1])  # rows 0-1, then row 2
    parts = model.score(toks, attention_mask=mask)
    assert torch.equal(parts.mask, whole.mask) and torch.equal(parts.is_greedy, whole.is_greedy)
    assert float((parts.token_logprobs - whole.token_logprobs).abs().max()) <= 1e-5


def test_score_labels_and_ignore_index():
    cfg, model, toks, mask, own, _, _ = _padded_case()
    g = torch.Generator().manual_seed(7)
    labels = torch.randint(0, cfg.vocab_size, toks.shape, generator=g)
    labels[0, 3] = labels[1, -1] = -100
    labels[2, 1] = cfg.vocab_size + 5  # a masked position's label is never looked at
    out = model.score(toks, attention_mask=mask, labels=labels)
    valid = (mask[:, :-1] != 0) & (mask[:, 1:] != 0) & (labels[:, 1:] != -100)
    assert torch.equal(out.mask, valid) and not bool(out.mask[0, 2]) and not bool(out.mask[1, -1])
    assert float((out.token_logprobs.double() - _gathered(own, labels))[valid].abs().max()) <= 1e-5
    assert bool((out.token_logprobs[~valid] == 0).all()) and bool(out.is_greedy[~valid].all())
    # another ignore_index: -100 is then an ordinary (illegal) label
    with pytest.raises(ValueError):
        model.score(toks, attention_mask=mask, labels=labels, ignore_index=-1)
    lab2 = labels.clone()
    lab2[labels == -100] = -1
    out2 = model.score(toks, attention_mask=mask, labels=lab2, ignore_index=-1)
    assert torch.equal(out2.mask, out.mask) and torch.equal(out2.token_logprobs, out.token_logprobs)
    # no mask: every position but the first has an entry
    full = model.score(toks)
    assert bool(full.mask.all())


def test_score_value_errors():
    cfg, model, toks, mask, *_ = _padded_case()
    bad = toks.clone().long()
    bad[0, 5] = cfg.vocab_size
    with pytest.raises(ValueError):
        model.score(toks, attention_mask=mask, labels=bad)
    bad[0, 5] = -3
    with pytest.raises(ValueError):
        model.score(toks, attention_mask=mask, labels=bad)
    with pytest.raises(ValueError):
        model.score(toks[:, :1])
    with pytest.raises(ValueError):
        model.score(toks, attention_mask=mask, labels=toks[:, :-1])
    with pytest.raises(ValueError):
        model.score(toks, attention_mask=mask[:, :-1])
    with pytest.raises(ValueError):
        model.forward_tokens(toks, None, None, 0, None, logits_mode="logprob")  # no targets


def test_logprob_combine_shards():
    """Column shards of one logits matrix, an empty shard among them: the combined log-prob is the unsplit one."""
    g = torch.Generator().manual_seed(3)
    m, v = 9, 96
    logits = torch.randn(m, v, generator=g) * 6
    tg = torch.randint(0, v, (m,), generator=g, dtype=torch.int32)
    tg[0], tg[1] = -1, v  # ignored
    whole = ops.logprob(logits, tg)
    lp, lse, is_max = ops.logprob_combine(*whole)
    want = torch.logsumexp(logits.double(), -1)
    assert float((lse.double() - want).abs().max()) <= 1e-5
    parts = [ops.logprob(logits[:, c0:c0 + 32], tg, col_offset=c0) for c0 in (0, 32, 64)]
    m_inf, zero = torch.full((m,), float("-inf")), torch.zeros(m)
    parts.insert(1, (zero, m_inf, zero))  # a shard with no column: the identity
    stacked = [torch.stack([p[i] for p in parts]) for i in range(3)]
    lp2, lse2, is_max2 = ops.logprob_combine(*stacked)
    assert torch.equal(stacked[0].sum(0), whole[0]) and torch.equal(is_max2, is_max)
    assert float((lse2.double() - want).abs().max()) <= 1e-5 and bool(torch.isfinite(lp2).all())
    ok = (tg >= 0) & (tg < v)
    picked = logits.gather(1, tg.long().clamp(0, v - 1)[:, None])[:, 0]
    assert float((lp2.double() - (picked.double() - want))[ok].abs().max()) <= 1e-5
    assert torch.equal(is_max[ok], (picked == logits.max(-1).values)[ok])
    # nothing but empty shards: -inf, never NaN
    e_lp, e_lse, _ = ops.logprob_combine(zero, m_inf, zero)
    assert bool((e_lse == float("-inf")).all()) and not bool(torch.isnan(e_lp).any())


def test_loglikelihood(llama3_tok):
    tok = llama3_tok
    cfg = tiny_config(vocab_size=len(tok), num_hidden_layers=2, bos_token_id=tok.bos_id, eos_token_id=tok.eos_id)
    model, *_ = build(cfg, seed=9)
    gen = LLaMA(None, model, tok)
    pairs = [("The quick brown", " fox jumps"), ("hello", " world"), ("The", " quick brown fox")]
    res = gen.loglikelihood(pairs)
    assert len(res) == 3 and all(isinstance(v, float) and isinstance(f, bool) and v < 0 for v, f in res)
    # the sum is the slice of score over the continuation's tokens: the same left-padded, length-masked batch
    enc = [(tok.encode(c, bos=True, eos=False), tok.encode(x, bos=False, eos=False)) for c, x in pairs]
    width = max(len(c) + len(x) for c, x in enc)
    toks = torch.zeros(len(enc), width, dtype=torch.int32)
    mask = torch.zeros(len(enc), width, dtype=torch.int32)
    for i, (c, x) in enumerate(enc):
        toks[i, width - len(c) - len(x):] = torch.tensor(c + x, dtype=torch.int32)
        mask[i, width - len(c) - len(x):] = 1
    out = model.score(toks, attention_mask=mask)
    for i, ((c, x), (v, f)) in enumerate(zip(enc, res)):
        assert len(x) > 0 and bool(out.mask[i, width - 1 - len(x):].all())
        assert abs(v - float(out.token_logprobs[i, width - 1 - len(x):].double().sum())) <= 1e-9
        assert f == bool(out.is_greedy[i, width - 1 - len(x):].all())
    assert gen.loglikelihood([]) == []
    assert gen.loglikelihood([("hello", "")]) == [(0.0, True)]
    with pytest.raises(ValueError):
        gen.loglikelihood([("hello " * cfg.max_sequence_length, " world")])


def _chain_model(cfg, chain, seed=9):
    """A model whose greedy next token is planted: the layers add nothing to the residual stream (wo = w2 = 0), so the
    hidden state at a position is its token's embedding, and the lm_head row of ``b`` points along the embedding of
    ``a`` for every ``(a, b)`` of ``chain`` (every other row is 0: logit 0 against 2 sqrt(D) for the planted one)."""
    sd = random_meta_state_dict(cfg, seed=seed)
    for i in range(cfg.num_hidden_layers):
        sd[f"layers.{i}.attention.wo.weight"] = torch.zeros_like(sd[f"layers.{i}.attention.wo.weight"])
        sd[f"layers.{i}.feed_forward.w2.weight"] = torch.zeros_like(sd[f"layers.{i}.feed_forward.w2.weight"])
    emb = sd["tok_embeddings.weight"].float()
    head = torch.zeros_like(sd["output.weight"])
    for a, b in chain:
        head[b] = (2 * emb[a] / emb[a].norm()).to(head.dtype)
    sd["output.weight"] = head
    sd["norm.weight"] = torch.ones_like(sd["norm.weight"])
    return LLaMAForCausalLM(cfg, _do_init=False).load_params(meta_state_dict_to_params(sd, cfg.num_hidden_layers))


def test_loglikelihood_greedy_flag(llama3_tok):
    """The flag is true for the continuation ``generate_from_str(..., temperature=0.0)`` produces and false as soon as
    one continuation token is not the greedy one. The model is planted (``_chain_model``) so that greedy decoding
    after "The" gives the ordinary text tokens of " quick", which survive decode / encode."""
    tok = llama3_tok
    cfg = tiny_config(vocab_size=len(tok), num_hidden_layers=2, bos_token_id=tok.bos_id, eos_token_id=tok.eos_id)
    prompt, cont, other = "The", " quick", " fox"
    c, x, y = (tok.encode(t, bos=b, eos=False) for t, b in ((prompt, True), (cont, False), (other, False)))
    assert len(x) == len(y) == 2 and x[0] == y[0] and x[1] != y[1]  # (" ", "quick") and (" ", "fox")
    assert len({c[-1], x[0]}) == 2  # the next token is a function of the current one
    gen = LLaMA(None, _chain_model(cfg, [(c[-1], x[0]), (x[0], x[1])]), tok)
    out, = gen.generate_from_str([prompt], max_gen_len=len(x), temperature=0.0)
    head = tok.decode([tok.bos_id]) + prompt
    assert out.startswith(head) and out[len(head):] == cont, out
    (v, f), (v2, f2) = gen.loglikelihood([(prompt, cont), (prompt, other)])
    assert f is True and f2 is False  # (other: its first token is the greedy one, its second is not)
    assert v2 < v < 0
    # in one batch with other lengths (left padding) the flags stay
    res = gen.loglikelihood([(prompt + cont, other), (prompt, cont), (prompt, other)])
    assert [r[1] for r in res] == [False, True, False] and abs(res[1][0] - v) <= 1e-5


def _worker(rank, world, port, toks, mask, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank))
        from jax_llama_amd.models import LLaMAForCausalLM
        from jax_llama_amd.parallel import TPComm, init_distributed
        torch.manual_seed(0)
        ctx = init_distributed(backend="gloo", device_type="cpu")
        ctx.setup_mesh(tp=world)
        comm = TPComm.from_context(ctx)
        cfg = tiny_config(intermediate_size=128)
        _, _, _, params = build(cfg, seed=11)
        model = LLaMAForCausalLM(cfg, comm=comm, _do_init=False).load_params(params)
        out = model.score(toks, attention_mask=mask)
        q.put(("ok", rank, (out.token_logprobs, out.is_greedy, out.mask)))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:  # pragma: no cover - surfaced in the parent
        import traceback
        q.put(("err", rank, traceback.format_exc()))


def test_score_tensor_parallel_gloo():
    """Vocab-parallel lm_head over two gloo ranks: each rank scores its shard with its column offset, the triples are
    gathered and combined in rank order -- identical bits on both ranks, the single-process result within the bound."""
    cfg = tiny_config(intermediate_size=128)
    ref_model, oracle, _, _ = build(cfg, seed=11)
    toks, mask = left_padded_batch([5, 8], 8, cfg.vocab_size, pad=2, seed=2)
    pos = mask.cumsum(-1) - 1
    want = ref_model.score(toks, attention_mask=mask)
    own = ref_model(toks, attention_mask=mask, position_ids=pos).logits.float()
    bound = 2 * float((own - oracle.forward(toks, mask, pos).float())[mask.bool()].abs().max())
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, toks, mask, q)) for r in range(world)]
    for p in procs:
        p.start()
    outs = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
    for status, rank, payload in outs:
        assert status == "ok", payload
    res = {rank: payload for _, rank, payload in outs}
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    lp, greedy, valid = res[0]
    assert torch.equal(valid, want.mask)
    err = float((lp - want.token_logprobs).abs().max())
    print(f"TP2 vs single process {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert bool((lp[~valid] == 0).all()) and bool(greedy[~valid].all())
