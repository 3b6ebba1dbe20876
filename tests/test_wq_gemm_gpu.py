"""The quantised-weight GEMM (csrc/kernels/gemm5q.h; ``model.set_quantized_gemm("direct")``): calls of 65 .. 512 rows on
an Fp8Linear / Mxfp4Linear stream the quantised bytes. Contract: the bits of gemm5 (tiles 11 / 12) on ``W_deq``."""
from __future__ import annotations

import functools

import pytest
import torch

import exact_inputs as xi
from jax_llama_amd import ops
from jax_llama_amd.models import LLaMAForCausalLM
from jax_llama_amd.models.kv_cache import KVCache
from jax_llama_amd.models.weights import Fp8Linear, Mxfp4Linear, PackedLinear
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime.engine import DecodeEngine, GenerationConfig
from helpers import build, gpu_config, left_padded_batch, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
STORE, RESID, SWIGLU, QKV = ops.MODE_STORE, ops.MODE_RESIDUAL, ops.MODE_SWIGLU, ops.MODE_QKV
LINEAR = {"fp8": Fp8Linear, "mxfp4": Mxfp4Linear}
FMTS = ("fp8", "mxfp4")


@pytest.fixture(autouse=True)
def _default_plan():
    yield
    ops.WQ_GEMM_PLAN = None


def _direct(x, w, mode, eps=None):
    """The call under test must be one the quantised-weight GEMM takes (else the test would pass on the dequant path)."""
    assert ops._wq_direct(ops.ext(), x, w, mode, eps)


@functools.lru_cache(maxsize=None)
def _rand_weight(fmt, n, k):
    """Random weights with the per-row exponents of ``test_dequant_kernel_bit_equal`` and one all-zero row, marked
    direct."""
    g = torch.Generator().manual_seed(n + k)
    w = (torch.randn(n, k, generator=g) * 2.0 ** torch.randint(-12, 6, (n, 1), generator=g).float()).to(BF16)
    w[n // 2] = 0
    lin = LINEAR[fmt].from_dense(w, DEV)
    lin.gemm_direct = True
    return lin


def _gemm5(x, w, out, mode, acc, mirror, ks, tile, eps):
    """gemm5 on the dequantised copy: the other side of the contract."""
    e = ops.ext()
    fused = eps is not None and mode != RESID
    m = x.shape[0]
    ws = torch.empty(e.gemm5_ksplit(w.k, ks) * m * (w.n + 1), dtype=torch.float32, device=DEV)
    e.gemm(ops._tiled_input(x, eps, fused), ops.bf16_weight(w).weight, w.n, w.k, out, mode, acc, mirror, ks, ws,
           float(eps) if fused else -1.0, tile)


# (m, n, k, tile, ksplit). M: 65 the 128-row form with clamped rows, 128, 129 the 256-row form, 256, 257 two m-tiles.
# N: 16 one n-tile (three waves idle, clamped n-tiles), 272 a clamped tail past one workgroup, 288 the SwiGLU shape.
# K: 128 fewer stages than the ring, 384 under split 2 kc = 3 (an MXFP4 split starts mid-block), 2176 34 stages.
BIT_CASES = [(65, 16, 128, 11, 1), (128, 272, 384, 12, 2), (129, 272, 2176, 11, 5), (256, 16, 2176, 12, 1),
             (257, 288, 384, 11, 2), (129, 288, 128, 12, 5)]


@pytest.mark.parametrize("m,n,k,tile,ks", BIT_CASES)
@pytest.mark.parametrize("fmt", FMTS)
def test_bit_equal_gemm5_on_wdeq(fmt, m, n, k, tile, ks):
    w = _rand_weight(fmt, n, k)
    ops.WQ_GEMM_PLAN = (tile, ks)
    g = torch.Generator().manual_seed(m)
    x = torch.randn(m, k, generator=g).to(BF16).to(DEV)
    h0 = torch.randn(m, n, generator=g).to(DEV)
    for eps in (None, 1e-5):
        _direct(x, w, STORE, eps)
        want = torch.empty(m, n, dtype=torch.float32, device=DEV)
        _gemm5(x, w, want, STORE, True, None, ks, tile, eps)
        assert torch.equal(ops.linear(x, w, rms_eps=eps, out_dtype=torch.float32), want), f"STORE eps={eps}"
        for acc in (True, False):
            _direct(x, w, RESID, eps)
            ha, hb = h0.clone(), h0.clone()
            ma, mb = [torch.full((m, n), 7.0, dtype=BF16, device=DEV) for _ in range(2)]
            ops.linear_residual(x, w, ha, rms_eps=eps, accumulate=acc, mirror=ma)
            _gemm5(x, w, hb, RESID, acc, mb, ks, tile, eps)
            assert torch.equal(ha, hb) and torch.equal(ma, mb), f"RESIDUAL accumulate={acc} eps={eps}"
        if n % 32 == 0:
            _direct(x, w, SWIGLU, eps)
            want = torch.empty(m, n // 2, dtype=BF16, device=DEV)
            _gemm5(x, w, want, SWIGLU, True, None, ks, tile, eps)
            assert torch.equal(ops.linear_swiglu(x, w, rms_eps=eps), want), f"SWIGLU eps={eps}"


@pytest.mark.parametrize("m,s,k,tile,ks", [(130, 2, 384, 12, 2), (256, 1, 2176, 11, 5)])
@pytest.mark.parametrize("fmt", FMTS)
def test_bit_equal_gemm5_qkv(fmt, m, s, k, tile, ks):
    h, hkv, dh, t = 2, 1, 128, 8
    n, b = (h + 2 * hkv) * dh, m // s
    w = _rand_weight(fmt, n, k)
    ops.WQ_GEMM_PLAN = (tile, ks)
    g = torch.Generator().manual_seed(m)
    x = torch.randn(m, k, generator=g).to(BF16).to(DEV)
    table = ref.rope_table(dh, 64, 10000.0).to(DEV)
    pos = torch.randint(0, 40, (m,), dtype=torch.int32, generator=g).to(DEV)
    slot = torch.tensor([2], dtype=torch.int32, device=DEV)
    e = ops.ext()
    for eps in (None, 1e-5):
        _direct(x, w, QKV, eps)
        ka, va, kb, vb = [torch.zeros(b, hkv, t, dh, dtype=BF16, device=DEV) for _ in range(4)]
        qa = ops.linear_qkv_rope(x, w, eps, table, pos, ka, va, slot, s, h, hkv, dh)
        qb = torch.empty_like(qa)
        ws = torch.empty(e.gemm5_ksplit(k, ks) * m * (n + 1), dtype=torch.float32, device=DEV)
        e.gemm_qkv(ops._tiled_input(x, eps, eps is not None), ops.bf16_weight(w).weight, n, k, table, pos, kb, vb, slot,
                   s, h, hkv, dh, qb, ks, ws, -1.0 if eps is None else eps, tile)
        assert torch.equal(qa, qb) and torch.equal(ka, kb) and torch.equal(va, vb), f"QKV eps={eps}"


# ---------------------------------------------------------------------------------- exact answers, default plan
@pytest.mark.parametrize("m", [65, 200])
@pytest.mark.parametrize("fmt,n,k", [("fp8", 48, 192), ("fp8", 272, 2176), ("mxfp4", 272, 2176)])
def test_int_gemm_exact(fmt, n, k, m):
    x, w, y = xi.int_gemm_inputs(m, n, k, seed=m + n + k, amp=2, plant=True)
    assert int(y.abs().max()) > 256 and bool(xi.bf16_ties(y)[m - 1, :4].all())
    p = 2.0 ** torch.randint(-3, 4, (n,), generator=torch.Generator().manual_seed(n + k)).double()
    wd = (w.double() * p[:, None]).float().to(BF16)
    lin = LINEAR[fmt].from_dense(wd, DEV)
    assert torch.equal(lin.dense().cpu(), wd)  # integers in [-2, 2] x powers of two quantise exactly
    lin.gemm_direct = True
    ys = y.double() * p[None, :]
    xg = x.to(BF16).to(DEV)
    _direct(xg, lin, STORE)
    o32 = ops.linear(xg, lin, out_dtype=torch.float32)
    assert torch.equal(o32.cpu().double(), ys), f"STORE fp32: {int((o32.cpu().double() != ys).sum())} elements differ"
    assert torch.equal(ops.linear(xg, lin).cpu(), ys.float().to(BF16)), "STORE bf16 is not the RNE of the exact sum"
    h0 = xi.int_residual(m, n, m + n)
    for acc in (True, False):
        _direct(xg, lin, RESID)
        hg = h0.float().to(DEV)
        mir = torch.full((m, n), 7.0, dtype=BF16, device=DEV)
        ops.linear_residual(xg, lin, hg, accumulate=acc, mirror=mir)
        want64 = h0.double() + ys if acc else ys
        want = want64.float()
        assert torch.equal(want.double(), want64)  # (the sum is exact in fp32)
        assert torch.equal(hg.cpu(), want), f"RESIDUAL accumulate={acc}"
        assert torch.equal(mir.cpu(), want.to(BF16)), f"mirror accumulate={acc}"


# ---------------------------------------------------------------------------------- tiny model
@functools.lru_cache(maxsize=None)
def _models(fmt):
    """(config, quantised model, bf16 model holding W_deq), on the GPU."""
    cfg = gpu_config()
    _, _, _, params = build(cfg, seed=0)
    qm, deq = [LLaMAForCausalLM(cfg, device=DEV, _do_init=False).load_params(params) for _ in range(2)]
    qm.quantize_weights_("fp8_e4m3" if fmt == "fp8" else "mxfp4")
    for lq, ld in zip(qm.layers, deq.layers):
        for name in ("qkv", "o", "gu", "down"):
            setattr(ld, name, PackedLinear.from_dense(getattr(lq, name).dense(), DEV))
    return cfg, qm, deq


def _prefill(model, toks):
    b, s = toks.shape
    cache = KVCache(model.config.num_hidden_layers, b, model.n_kv_heads, s + 4, model.head_dim, DEV)
    pos = torch.arange(s, dtype=torch.int32).expand(b, s).contiguous().to(DEV)
    kvs = torch.zeros(b, dtype=torch.int32, device=DEV)
    logits, *_ = model.forward_tokens(toks.to(DEV), pos, cache, 0, kvs, None, logits_mode="last")
    return logits, cache, kvs


@pytest.mark.parametrize("fmt", FMTS)
def test_model_direct(fmt):
    cfg, qm, deq = _models(fmt)
    b, s = 72, 3
    g = torch.Generator().manual_seed(b)
    toks = torch.randint(0, cfg.vocab_size, (b, s), dtype=torch.int32, generator=g)
    (_, cq, kvs), (_, cd, _) = _prefill(qm, toks), _prefill(deq, toks)  # (dequant setting: the same caches)
    try:
        assert qm.set_quantized_gemm("direct").quantized_gemm == "direct"
        x = torch.zeros(b, cfg.hidden_size, dtype=BF16, device=DEV)
        _direct(x, qm.layers[0].qkv, QKV, cfg.rms_norm_eps)
        _direct(x, qm.layers[1].o, RESID)
        _direct(x, qm.layers[0].gu, SWIGLU, cfg.rms_norm_eps)
        # one decode step of 72 rows: gemm5's summation order against the tuned bf16 plan's on W_deq, so the
        # whole-model tolerance of the quantised-weight tests
        nxt = torch.randint(0, cfg.vocab_size, (b, 1), dtype=torch.int32, generator=g).to(DEV)
        pos = torch.full((b, 1), s, dtype=torch.int32, device=DEV)
        slot = torch.tensor([s], dtype=torch.int32, device=DEV)
        dq, *_ = qm.forward_tokens(nxt, pos, cq, slot, kvs, None, logits_mode="last")
        dd, *_ = deq.forward_tokens(nxt, pos, cd, slot, kvs, None, logits_mode="last")
        assert bool(torch.isfinite(dq).all()) and rel_err(dq, dd) < 2e-2
        ptoks, mask = left_padded_batch([5, 8] * 36, 8, cfg.vocab_size, pad=2, seed=6)
        gc = GenerationConfig(max_length=24, do_sample=False, pad_token_id=2, eos_token_id=2)
        ga = DecodeEngine(qm, b, 24, use_graph=True).run(ptoks, mask, gc).clone()
        gb = DecodeEngine(qm, b, 24, use_graph=False).run(ptoks, mask, gc).clone()
        assert torch.equal(ga, gb)
    finally:
        qm.set_quantized_gemm("dequant")
    assert qm.quantized_gemm == "dequant" and not ops._wq_direct(ops.ext(), x, qm.layers[0].qkv, QKV, 1e-5)
    ptoks = torch.randint(0, cfg.vocab_size, (40, 5), dtype=torch.int32, generator=g)  # a 200-row prefill
    assert torch.equal(_prefill(qm, ptoks)[0], _prefill(deq, ptoks)[0])
