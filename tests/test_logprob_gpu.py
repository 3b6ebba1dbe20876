"""Scoring on the GPU: the lm_head GEMM's log-sum-exp epilogue (``gemm_logprob``, MODE_LOGPROB in gemm.hip), the
unfused row kernel (``logprob_rows``, sample.hip), the op-layer dispatch and shard combine, ``LLaMAForCausalLM.score``.

The kernel tests compare against fp32 logits stored by the plain gemm4 store epilogue (tile 7, the same main loop and
row scale): the target logit and the row maximum bit for bit, the log-sum-exp within LSE_TOL of a float64 logsumexp of
those stored logits. LSE_TOL = 1e-4 is derived, not measured on the device: a CPU emulation of the worst merge order
(128-column fp32 partials merged sequentially, fp32 random logits at N = 128256 with a standard deviation up to 12)
gives at most 3.7e-6; the bound leaves about 25x for the device's exp."""
from __future__ import annotations

import functools

import pytest
import torch

from helpers import build, gpu_config, left_padded_batch
from jax_llama_amd import LLaMAConfig, LLaMAForCausalLM, ops
from jax_llama_amd.models import mask_to_kv_start
from jax_llama_amd.models.kv_cache import KVCache
from jax_llama_amd.models.weights import PackedLinear

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
LSE_TOL = 1e-4
INF = float("inf")

SHAPES = [(256, 272, 64), (300, 400, 128), (700, 2560, 1024)]
NORMS = [(-1.0, False), (1e-5, False), (1e-5, True)]  # (rms_eps, the precomputed row statistic's scratch)


def _planted(n):
    """Target columns at the wave-block and tile boundaries, then two ignored labels."""
    return [0, 127, 128, 255, 256, n - 1, -1, n]


@functools.lru_cache(maxsize=None)
def _case(m, n, k):
    """Shared, read-only: x (bf16), packed W, the dense W, int32 targets (device)."""
    g = torch.Generator().manual_seed(m + n + k)
    x = torch.randn(m, k, generator=g).to(BF16)
    w = (torch.randn(n, k, generator=g) * (4.0 / k ** 0.5)).to(BF16)  # logits of standard deviation ~4
    tg = torch.randint(0, n, (m,), generator=g, dtype=torch.int32)
    tg[:8] = torch.tensor(_planted(n), dtype=torch.int32)
    return x.to(DEV), PackedLinear.from_dense(w, DEV), w, tg.to(DEV)


@functools.lru_cache(maxsize=None)
def _stored(m, n, k, eps, scratch):
    """Shared, read-only: the fp32 logits of the plain store epilogue on gemm4's 256 x 256 tile."""
    e = ops.ext()
    x, pw, _, _ = _case(m, n, k)
    rw = torch.empty(m, device=DEV) if scratch else None
    assert e.gemm_plan_check(m, n, k, ops.MODE_STORE, eps >= 0, 1, 7, scratch) == 0
    out = torch.empty(m, n, dtype=torch.float32, device=DEV)
    e.gemm(x, pw.weight, n, k, out, ops.MODE_STORE, True, None, 1, None, eps, 7, None, rw)
    torch.cuda.synchronize()
    return out


def _want(logits, tg):
    """(tgt, mx, float64 lse) of stored logits on the host."""
    lg = logits.cpu()
    col = tg.cpu().long()
    ok = (col >= 0) & (col < lg.shape[1])
    picked = lg.gather(1, col.clamp(0, lg.shape[1] - 1)[:, None])[:, 0]
    return torch.where(ok, picked, torch.zeros_like(picked)), lg.max(-1).values, torch.logsumexp(lg.double(), -1)


def _fused(m, n, k, eps, scratch, tg, col_offset=0, w=None):
    e = ops.ext()
    x, pw, _, _ = _case(m, n, k)
    w = pw if w is None else w
    ws = torch.full((e.gemm_logprob_workspace(m, w.n),), float("nan"), dtype=torch.float32, device=DEV)
    out = torch.full((3, m), float("nan"), dtype=torch.float32, device=DEV)
    rw = torch.empty(m, device=DEV) if scratch else None
    e.gemm_logprob(x, w.weight, w.n, k, ws, eps, tg, col_offset, out[0], out[1], out[2], rw)
    torch.cuda.synchronize()
    return out.cpu(), ws.cpu()


def _assert_triple(got, want, what):
    tgt, mx, se = got
    w_tgt, w_mx, w_lse = want
    assert torch.equal(tgt, w_tgt), f"{what}: tgt differs on {int((tgt != w_tgt).sum())} rows"
    assert torch.equal(mx, w_mx), f"{what}: mx differs on {int((mx != w_mx).sum())} rows"
    err = float((mx.double() + se.double().log() - w_lse).abs().max())
    print(f"{what}: max |lse - float64 logsumexp| = {err:.3e}")
    assert err <= LSE_TOL, f"{what}: lse off by {err:.3e}"


@pytest.mark.parametrize("eps,scratch", NORMS, ids=["nonorm", "inloop", "rowstat"])
@pytest.mark.parametrize("m,n,k", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_kernel_parity(m, n, k, eps, scratch):
    """N = 272: the second tile's second wave has no valid column ((-inf, 0) partial); N = 400: it has 16. Every partial
    slot is written (the workspace starts as NaN), ignored rows get exactly 0, a second call returns the same bits, and
    the row kernel on the stored logits gives the same tgt / mx bits."""
    e = ops.ext()
    assert e.gemm_plan_check(m, n, k, ops.MODE_LOGPROB, eps >= 0, 1, 0, scratch) == 0
    _, _, _, tg = _case(m, n, k)
    logits = _stored(m, n, k, eps, scratch)
    want = _want(logits, tg)
    got, ws = _fused(m, n, k, eps, scratch, tg)
    assert not bool(torch.isnan(ws).any()), "a partial slot was not written"
    assert not bool(torch.isnan(got).any())
    _assert_triple(got, want, "fused")
    assert bool((got[0][6:8] == 0).all()) and bool((want[0][:6] != 0).all())
    if n == 272:  # slots per row: 2 tiles x 2 wave columns; the last one covers columns 384..511
        part = ws.view(m, 4, 2)
        assert bool((part[:, 3, 0] == -INF).all()) and bool((part[:, 3, 1] == 0).all())
    again, _ = _fused(m, n, k, eps, scratch, tg)
    assert torch.equal(again, got), "a second call returned other bits"
    rows = torch.stack(ops.logprob(logits, tg)).cpu()
    _assert_triple(rows, want, "logprob_rows")


def test_dispatch(monkeypatch):
    """ops.linear_logprob: the fused GEMM from ARGMAX_FUSED_MIN_M rows where gemm_plan() has a MODE_LOGPROB plan; the
    GEMM + row kernel below that, at K % 64 != 0 and with gemm4 off."""
    e = ops.ext()
    calls = []
    real_fused, real_rows = e.gemm_logprob, e.logprob_rows
    monkeypatch.setattr(e, "gemm_logprob", lambda *a, **kw: (calls.append("fused"), real_fused(*a, **kw))[1])
    monkeypatch.setattr(e, "logprob_rows", lambda *a, **kw: (calls.append("rows"), real_rows(*a, **kw))[1])
    for m, n, k in SHAPES:
        x, pw, _, tg = _case(m, n, k)
        assert ops.logprob_fused(x, pw, 1e-5) and ops.logprob_fused(x, pw, None)
        calls.clear()
        got = torch.stack(ops.linear_logprob(x, pw, tg, rms_eps=1e-5)).cpu()
        assert calls == ["fused"]
        direct, _ = _fused(m, n, k, 1e-5, True, tg)
        assert torch.equal(got, direct)
    m, n, k = 48, 400, 128
    x, pw, _, tg = _case(m, n, k)
    assert not ops.logprob_fused(x, pw, 1e-5)
    calls.clear()
    got = torch.stack(ops.linear_logprob(x, pw, tg, rms_eps=1e-5)).cpu()
    assert calls == ["rows"]
    _assert_triple(got, _want(ops.linear(x, pw, 1e-5, out_dtype=torch.float32), tg), "unfused M = 48")
    x96, pw96, _, _ = _case(300, 400, 96)
    assert not ops.logprob_fused(x96, pw96, None)
    x, pw, _, tg = _case(300, 400, 128)
    try:
        e.gemm_set_g4_default(0)
        assert not ops.logprob_fused(x, pw, None)
    finally:
        e.gemm_set_g4_default(1)
    monkeypatch.setattr(ops, "LOGPROB_CHUNK_BYTES", 100 * 400 * 4)  # three row chunks of the unfused form
    monkeypatch.setattr(ops, "ARGMAX_FUSED_MIN_M", 1 << 30)
    calls.clear()
    got = torch.stack(ops.linear_logprob(x, pw, tg, rms_eps=None)).cpu()
    assert calls == ["rows"] * 3
    chunks = torch.cat([ops.linear(x[r0:r0 + 100], pw, None, out_dtype=torch.float32) for r0 in (0, 100, 200)])
    _assert_triple(got, _want(chunks, tg), "unfused, chunked")


# ---- exact answers --------------------------------------------------------------------
def test_exact_needle():
    """Integer-valued bf16 x and W: every logit is exactly 0 except one needle of exactly 40 per row, whose column
    cycles over the boundary columns. log p(needle) = -log1p((N - 1) e^-40) = 0 and log p(other) = -40 to 1.7e-15."""
    m, n, k = 300, 400, 64
    cols = _planted(n)[:6]
    x = torch.zeros(m, k)
    w = torch.zeros(n, k)
    r = torch.arange(m)
    x[r, r % 6] = 5.0
    for j, c in enumerate(cols):
        w[c, j] = 8.0
    needle = torch.tensor(cols)[r % 6]
    tg = needle.clone()
    other = r % 2 == 1
    tg[other] = (needle[other] + 1 + (r[other] % 7)) % n  # never the needle: 1..7 columns to its right
    assert bool((tg[other] != needle[other]).all())
    xd, pw, tgd = x.to(BF16).to(DEV), PackedLinear.from_dense(w.to(BF16), DEV), tg.to(torch.int32).to(DEV)
    assert ops.logprob_fused(xd, pw, None)
    lp, lse, is_max = (t.cpu() for t in ops.logprob_combine(*ops.linear_logprob(xd, pw, tgd)))
    print("needle max |lp|", float(lp[~other].abs().max()), "other max |lp + 40|", float((lp[other] + 40).abs().max()))
    assert float(lp[~other].abs().max()) <= 1e-6
    assert float((lp[other] + 40).abs().max()) <= 1e-4
    assert torch.equal(is_max, ~other)
    # all-zero W: a uniform row, lse = ln N
    zero = PackedLinear.from_dense(torch.zeros(n, k, dtype=BF16), DEV)
    lp0, lse0, _ = (t.cpu() for t in ops.logprob_combine(*ops.linear_logprob(xd, zero, tgd)))
    want = torch.log(torch.tensor(float(n), dtype=torch.float64))
    print("uniform max |lse - ln N|", float((lse0.double() - want).abs().max()))
    assert float((lse0.double() - want).abs().max()) <= 1e-5
    assert float((lp0.double() + want).abs().max()) <= 1e-5


# ---- shard combine --------------------------------------------------------------------
def test_shard_combine():
    """W cut into two column halves, run with col_offset 0 and N / 2 (vocab-parallel ranks): after logprob_combine the
    target logit and the maximum are those of the unsplit run bit for bit, the lse within the bound."""
    m, n, k = 700, 2560, 1024
    x, pw, w, tg = _case(m, n, k)
    halves = [PackedLinear.from_dense(w[: n // 2], DEV), PackedLinear.from_dense(w[n // 2:], DEV)]
    whole = ops.linear_logprob(x, pw, tg, rms_eps=1e-5)
    parts = [ops.linear_logprob(x, h, tg, rms_eps=1e-5, col_offset=r * (n // 2)) for r, h in enumerate(halves)]
    own = (tg >= 0) & (tg < n // 2)
    assert bool((parts[1][0][own] == 0).all()) and bool((parts[0][0][(tg >= n // 2) & (tg < n)] == 0).all())
    stacked = [torch.stack([p[i] for p in parts]) for i in range(3)]
    lp, lse, is_max = ops.logprob_combine(*stacked)
    lp1, lse1, is_max1 = ops.logprob_combine(*whole)
    assert torch.equal(stacked[0].sum(0), whole[0]) and torch.equal(stacked[1].max(0).values, whole[1])
    assert torch.equal(is_max, is_max1)
    w_tgt, w_mx, w_lse = _want(_stored(m, n, k, 1e-5, True), tg)
    assert torch.equal(stacked[0].sum(0).cpu(), w_tgt) and torch.equal(stacked[1].max(0).values.cpu(), w_mx)
    for name, v in (("split", lse), ("whole", lse1)):
        err = float((v.cpu().double() - w_lse).abs().max())
        print(f"{name}: max |lse - float64 logsumexp| = {err:.3e}")
        assert err <= LSE_TOL
    assert float((lp.cpu().double() - (w_tgt.double() - w_lse)).abs().max()) <= LSE_TOL


# ---- model ----------------------------------------------------------------------------
def test_score_model(monkeypatch):
    """score against log_softmax + gather of this model's own fp32 logits (1e-4) and against the fp32 oracle (twice
    the maximum logit error between those logits and the oracle's, computed here: a log-prob cannot be off by more)."""
    cfg = gpu_config()
    model, oracle, _, _ = build(cfg, device=DEV, seed=5)
    b, s = 3, 100
    toks, mask = left_padded_batch([100, 63, 17], s, cfg.vocab_size, pad=0, seed=4)
    pos = (mask.cumsum(-1) - 1).to(torch.int32)
    out = model.score(toks, attention_mask=mask)
    torch.cuda.synchronize()
    assert out.token_logprobs.shape == out.is_greedy.shape == out.mask.shape == (b, s - 1)
    valid = (mask[:, :-1] != 0) & (mask[:, 1:] != 0)
    assert torch.equal(out.mask.cpu(), valid)
    kv_start, key_mask = mask_to_kv_start(mask, model.device)
    assert key_mask is None

    def own_logits(chunks):
        """The model's own fp32 logits, the way score runs the forward: the same row chunks, a transient cache each."""
        parts = []
        for b0, b1 in chunks:
            cache = KVCache(cfg.num_hidden_layers, b1 - b0, model.n_kv_heads, s, model.head_dim, model.device)
            lg, *_ = model.forward_tokens(toks[b0:b1].to(DEV), pos[b0:b1].to(DEV), cache, 0, kv_start[b0:b1], None,
                                          logits_mode="all")
            parts.append(lg.float().cpu().reshape(b1 - b0, s, -1))
        return torch.cat(parts)

    logits = own_logits([(0, b)])
    nxt = toks[:, 1:].long()

    def gathered(lg):
        return torch.log_softmax(lg.double(), -1)[:, :-1].gather(-1, nxt[..., None])[..., 0]

    lp = out.token_logprobs.cpu().double()
    own = gathered(logits)
    err_own = float((lp - own)[valid].abs().max())
    ref_logits = oracle.forward(toks, mask, pos).float().cpu()
    bound = 2 * float((logits - ref_logits)[mask.bool()].abs().max())
    err_ref = float((lp - gathered(ref_logits))[valid].abs().max())
    print(f"score vs own logits {err_own:.3e}; vs oracle {err_ref:.3e} (bound {bound:.3e})")
    assert err_own <= 1e-4
    assert err_ref <= bound
    top2 = logits[:, :-1].topk(2, -1).values
    clear = valid & (top2[..., 0] - top2[..., 1] > 1e-4)  # (a near-tie may go either way between two GEMM plans)
    greedy = logits[:, :-1].argmax(-1) == nxt
    assert torch.equal(out.is_greedy.cpu()[clear], greedy[clear]) and int(clear.sum()) > int(valid.sum()) // 2
    # masked entries: 0, true, false
    assert bool((out.token_logprobs.cpu()[~valid] == 0).all()) and bool(out.is_greedy.cpu()[~valid].all())
    assert not bool(out.mask.cpu()[~valid].any()) and int((~valid).sum()) > 0
    # two row chunks (2 rows: M = 200, the unfused form; then 1 row)
    from jax_llama_amd.runtime import engine
    monkeypatch.setattr(engine, "PREFILL_TOKENS", 2 * s)
    out2 = model.score(toks, attention_mask=mask)
    lp2 = out2.token_logprobs.cpu().double()
    logits2 = own_logits([(0, 2), (2, 3)])
    bound2 = 2 * float((logits2 - ref_logits)[mask.bool()].abs().max())
    err_own2, err_ref2 = float((lp2 - gathered(logits2))[valid].abs().max()), float((lp2 - gathered(ref_logits))[valid].abs().max())
    print(f"chunked: vs own logits {err_own2:.3e}; vs oracle {err_ref2:.3e} (bound {bound2:.3e})")
    assert err_own2 <= 1e-4
    assert err_ref2 <= bound2
    assert torch.equal(out2.mask.cpu(), valid) and bool((out2.token_logprobs.cpu()[~valid] == 0).all())


def test_score_fused_chunks(monkeypatch):
    """Six rows in two chunks of three: every chunk has M = 300 and takes the fused GEMM (the two-chunk run of
    test_score_model has chunks below ARGMAX_FUSED_MIN_M). Same bounds: 1e-4 against this model's own fp32 logits run in
    the same chunks, twice the maximum logit error against the fp32 oracle."""
    from jax_llama_amd.runtime import engine
    cfg = gpu_config()
    model, oracle, _, _ = build(cfg, device=DEV, seed=5)
    b, s = 6, 100
    toks, mask = left_padded_batch([100, 63, 17, 2, 99, 40], s, cfg.vocab_size, pad=0, seed=6)
    pos = (mask.cumsum(-1) - 1).to(torch.int32)
    kv_start, key_mask = mask_to_kv_start(mask, model.device)
    assert key_mask is None
    e = ops.ext()
    calls = []
    real = e.gemm_logprob
    monkeypatch.setattr(e, "gemm_logprob", lambda *a, **kw: (calls.append(a[0].shape[0]), real(*a, **kw))[1])
    monkeypatch.setattr(engine, "PREFILL_TOKENS", 3 * s)
    out = model.score(toks, attention_mask=mask)
    torch.cuda.synchronize()
    assert calls == [300, 300]
    parts = []
    for b0 in (0, 3):
        cache = KVCache(cfg.num_hidden_layers, 3, model.n_kv_heads, s, model.head_dim, model.device)
        lg, *_ = model.forward_tokens(toks[b0:b0 + 3].to(DEV), pos[b0:b0 + 3].to(DEV), cache, 0, kv_start[b0:b0 + 3],
                                      None, logits_mode="all")
        parts.append(lg.float().cpu().reshape(3, s, -1))
    logits = torch.cat(parts)
    ref_logits = oracle.forward(toks, mask, pos).float().cpu()
    valid = (mask[:, :-1] != 0) & (mask[:, 1:] != 0)
    nxt = toks[:, 1:].long()

    def gathered(lg):
        return torch.log_softmax(lg.double(), -1)[:, :-1].gather(-1, nxt[..., None])[..., 0]

    lp = out.token_logprobs.cpu().double()
    bound = 2 * float((logits - ref_logits)[mask.bool()].abs().max())
    err_own, err_ref = float((lp - gathered(logits))[valid].abs().max()), float((lp - gathered(ref_logits))[valid].abs().max())
    print(f"fused chunks: vs own logits {err_own:.3e}; vs oracle {err_ref:.3e} (bound {bound:.3e})")
    assert err_own <= 1e-4
    assert err_ref <= bound
    assert torch.equal(out.mask.cpu(), valid) and bool((out.token_logprobs.cpu()[~valid] == 0).all())
    assert bool(out.is_greedy.cpu()[~valid].all())


def test_score_memory():
    """Llama-3's vocabulary: no logits tensor is materialised. Peak allocated bytes during score, above the level
    before the call, stay below a quarter of M * V * 4 (2.1 GB) -- a condition, not a measurement: the partials are
    33 MB and the cache 2 MB, so only a materialised logits tensor can break it."""
    cfg = LLaMAConfig(vocab_size=128256, hidden_size=256, intermediate_size=512, num_hidden_layers=1,
                      num_attention_heads=2, num_key_value_heads=1, max_sequence_length=1024, rms_norm_eps=1e-5)
    model = LLaMAForCausalLM(cfg, device=DEV, seed=3)
    b, s = 4, 1024
    toks = torch.randint(0, cfg.vocab_size, (b, s), generator=torch.Generator().manual_seed(1), dtype=torch.int32)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = model.score(toks)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak above the start: {peak / 2**20:.1f} MiB; logits would be {b * s * cfg.vocab_size * 4 / 2**20:.0f} MiB")
    assert peak < b * s * cfg.vocab_size * 4 // 4
    lp = out.token_logprobs
    assert lp.shape == (b, s - 1) and bool(torch.isfinite(lp).all()) and float(lp.max()) <= 0
    assert bool(out.mask.all())
