"""MXFP4 weight-only linears on the MI355X: the dequant kernel, the MXFP4-weight decode GEMV on exact-answer and random
inputs, the dequant path (the bf16 kernels on W_deq), and a quantised model against the bf16 model that holds the
dequantised weights."""
from __future__ import annotations

import functools

import pytest
import torch

import exact_inputs as xi
from jax_llama_amd import ops
from jax_llama_amd.models import LLaMAForCausalLM
from jax_llama_amd.models.kv_cache import KVCache
from jax_llama_amd.models.weights import Mxfp4Linear, PackedLinear
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime.benchmark import graph_kernels
from jax_llama_amd.runtime.engine import DecodeEngine, GenerationConfig
from helpers import build, gpu_config, left_padded_batch, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
DH = xi.DH
STORE, RESID, SWIGLU, QKV = ops.MODE_STORE, ops.MODE_RESIDUAL, ops.MODE_SWIGLU, ops.MODE_QKV
MS = [1, 16, 17, 33, 64]


def _close(a, b, rtol, atol):  # (tests/test_fp8_gpu.py's measure)
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item()
    assert err <= atol + rtol * scale, f"max err {err:.3e} (ref max {scale:.3e})"


def _fast(x, w, mode):
    """The call under test must be one the MXFP4 GEMV takes (else the test would pass on the dequant path)."""
    assert ops._w4_fast(ops.ext(), x, w, mode)


# ---------------------------------------------------------------------------------- dequant kernel
@pytest.mark.parametrize("n,k", [(16, 128), (48, 384), (4096, 256)])
def test_dequant_kernel_bit_equal(n, k):
    """Settles the nibble order of the layout: the kernel converts byte i of a dword into elements 2 i, 2 i + 1 of the
    fragment in the order the conversion instruction emits them."""
    g = torch.Generator().manual_seed(n + k)
    w = (torch.randn(n, k, generator=g) * 2.0 ** torch.randint(-12, 6, (n, 1), generator=g).float()).to(BF16)
    w[n // 2] = 0  # (a zero row: scale bytes 127)
    cpu = Mxfp4Linear.from_dense(w, "cpu")
    gpu = Mxfp4Linear.from_dense(w, DEV)
    assert gpu.qweight.dtype == torch.uint8 and tuple(gpu.qweight.shape) == (n // 16, k // 128, 64, 16)
    assert gpu.scale.dtype == torch.uint8 and tuple(gpu.scale.shape) == (n // 16, k // 128, 16, 4)
    assert torch.equal(gpu.q().cpu(), cpu.q()) and torch.equal(gpu.e8m0().cpu(), cpu.e8m0())
    got = ops.bf16_weight(gpu)
    assert (got.n, got.k) == (n, k)
    want = ref.pack_frag16x32(cpu.dense())
    assert torch.equal(got.weight.cpu().view(torch.int16), want.view(torch.int16))
    assert torch.equal(gpu.dense().cpu().view(torch.int16), cpu.dense().view(torch.int16))


def test_bf16_weight_is_identity_for_packed():
    pw = PackedLinear.from_dense(torch.randn(32, 128).to(BF16), DEV)
    gen = ops.workspace.generation
    assert ops.bf16_weight(pw) is pw and ops.workspace.generation == gen


def test_bindings_refuse_wrong_layouts():
    f4 = Mxfp4Linear.from_dense(torch.randn(32, 256).to(BF16), DEV)
    x = torch.zeros(1, 256, dtype=BF16, device=DEV)
    out = torch.empty(1, 32, dtype=BF16, device=DEV)
    e = ops.ext()
    with pytest.raises(RuntimeError):
        e.linear_skinny_w4(x, f4.qweight, f4.scale, 64, 128, out, STORE, -1.0, True)  # (n, k) that is not the tensor's
    with pytest.raises(RuntimeError):
        e.linear_skinny_w4(x, f4.qweight, f4.scale.reshape(2, 2, 4, 16), 32, 256, out, STORE, -1.0, True)
    with pytest.raises(RuntimeError):
        e.linear_skinny_w4(x.float(), f4.qweight, f4.scale, 32, 256, out, STORE, -1.0, True)  # fp32 x
    with pytest.raises(RuntimeError):
        e.dequant_fp4(f4.qweight, f4.scale, 32, 256, torch.empty(2, 4, 64, 8, dtype=BF16, device=DEV))
    assert e.gemv_w4_plan_check(1, 32, 192, STORE, False)[0] != 0  # K % 128
    assert e.gemv_w4_plan_check(65, 32, 256, STORE, False)[0] != 0
    assert e.gemv_w4_plan_check(1, 48, 256, SWIGLU, False)[0] != 0  # SwiGLU: N % 32
    assert e.gemv_w4_plan_check(1, 32, 256, 8, False)[0] != 0  # (MODE_ARGMAX: no such epilogue here)
    assert e.gemv_w4_plan_check(1, 32, 256, STORE, True)[0] != 0  # fp32 x


# ---------------------------------------------------------------------------------- exact-answer GEMV
def _int_gemm_inputs(m, n, k, seed, plant):
    """``xi.int_gemm_inputs(amp=2)``. Its own bound (K amp^2 <= 16384) is a round figure far below the 2^24 that
    exactness needs; K = 4224 (16896) is built here from the same pieces, with the same planted ties."""
    if k * 4 <= 16384:
        return xi.int_gemm_inputs(m, n, k, seed=seed, amp=2, plant=plant)
    assert k * 4 < 2 ** 24
    x = xi.int_matrix(m, k, 2, seed * 2 + 1)
    w = xi.int_matrix(n, k, 2, seed * 2 + 2)
    if plant:
        x[m - 1, :] = 2
        x[m - 1, 0] = 1
        w[:4, :] = 0
        w[:4, 0] = 1
        w[:4, 1:65] = 2
        w[1, 65] = w[3, 65] = 1
        w[2:4] = -w[2:4]
    return x, w, x @ w.t()


def _block_pow2(n, k, seed):
    """int64 [n, k / 32] exponents in -3 .. 3: each (row, 32-block) of the weight is multiplied by 2^e, so the block
    scales differ inside one dot product."""
    return torch.randint(-3, 4, (n, k // 32), generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _int_case(m, n, k, blocks):
    """Shared, read-only: x (bf16, device), the Mxfp4Linear of W (``blocks``: times 2^e per (row, 32-block)), and the
    exact y = x W^T in fp64."""
    plant = k >= 66 and n >= 4
    x, w, y = _int_gemm_inputs(m, n, k, m + n + k, plant)
    if plant:
        assert int(y.abs().max()) > 256 and bool(xi.bf16_ties(y)[m - 1, :4].all())
    ys = y.double()
    wd = w.double()
    if blocks:
        p = (2.0 ** _block_pow2(n, k, n + k).double()).repeat_interleave(32, dim=1)
        wd = wd * p
        ys = x.double() @ wd.t()  # multiples of 2^-3 below 4 * 4224 * 8 units: exact in fp64 and in fp32, any order
        assert float(ys.abs().max()) * 8 < 2 ** 24
    wb = wd.float().to(BF16)
    f4 = Mxfp4Linear.from_dense(wb, DEV)
    assert torch.equal(f4.dense().cpu(), wb)  # integers in [-2, 2] x powers of two quantise exactly
    return x.to(BF16).to(DEV), f4, ys


# (16, 128): one block, most waves idle; (48, 384): fewer blocks than waves; (256, 4224): 33 blocks, the ring wraps with
# a ragged tail on 4 and on 8 waves; (32768, 128): the two-tile rule; (4112, 256): 257 column tiles; (32784, 128): 2049
# tiles under the two-tile rule, so the last workgroup's second tile is the clamped one
W4_SHAPES = [(16, 128), (48, 384), (256, 4224), (32768, 128), (4112, 256), (32784, 128)]


@pytest.mark.parametrize("blocks", [False, True])
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("n,k", W4_SHAPES)
def test_int_gemv_w4_store_residual(n, k, m, blocks):
    xg, f4, ys = _int_case(m, n, k, blocks)
    _fast(xg, f4, STORE)
    assert ops.ext().gemv_w4_plan_check(m, n, k, STORE, False)[2] == (2 if n // 16 >= 2048 else 1)
    o32 = ops.linear(xg, f4, out_dtype=torch.float32)
    assert torch.equal(o32.cpu().double(), ys), f"STORE fp32: {int((o32.cpu().double() != ys).sum())} elements differ"
    ob = ops.linear(xg, f4)
    assert torch.equal(ob.cpu(), ys.float().to(BF16)), "STORE bf16 is not the round-to-nearest-even of the exact sum"
    h0 = xi.int_residual(m, n, m + n)
    for acc in (True, False):
        hg = h0.float().to(DEV)
        mir = torch.full((m, n), 7.0, dtype=BF16, device=DEV)
        mp = ops.packed_empty(m, n, DEV) if n % 32 == 0 else None
        ops.linear_residual(xg, f4, hg, accumulate=acc, mirror=mir, mirror_packed=mp)
        want64 = h0.double() + ys if acc else ys
        want = want64.float()
        assert torch.equal(want.double(), want64)  # (the sum is exact in fp32)
        assert torch.equal(hg.cpu(), want), f"RESIDUAL accumulate={acc}"
        assert torch.equal(mir.cpu(), want.to(BF16)), f"mirror accumulate={acc}"
        if mp is not None:
            assert torch.equal(ref.unpack_act(mp.cpu(), m), mir.cpu())


def _row_pow2(n, seed):
    return torch.randint(-3, 4, (n,), generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _swiglu_case(m, f, k):
    """Entries in {-1, 0, 1} (as tests/test_exact_gpu.py), gate / up rows times 2^e: x, the interleaved Mxfp4Linear,
    (want, tol) of silu(g) * u per ``swiglu_exact``."""
    x = xi.int_matrix(m, k, 1, m + k)
    w1, w3 = xi.int_matrix(f, k, 1, f + k), xi.int_matrix(f, k, 1, f + k + 1)
    p1, p3 = 2.0 ** _row_pow2(f, f + 1).double(), 2.0 ** _row_pow2(f, f + 2).double()
    g, u = (x @ w1.t()).double() * p1[None, :], (x @ w3.t()).double() * p3[None, :]
    gu = ref.interleave_gate_up((w1.double() * p1[:, None]).float().to(BF16), (w3.double() * p3[:, None]).float().to(BF16))
    f4 = Mxfp4Linear.from_dense(gu, DEV)
    assert torch.equal(f4.dense().cpu(), gu)
    return x.to(BF16).to(DEV), f4, xi.swiglu_exact(g, u)


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("f,k", [(32, 128), (128, 2176), (16384, 128)])
def test_int_gemv_w4_swiglu(f, k, m):
    xg, f4, (want, tol) = _swiglu_case(m, f, k)
    _fast(xg, f4, SWIGLU)
    ap = ops.packed_empty(m, f, DEV)
    got = ops.linear_swiglu(xg, f4, None, out_packed=ap)
    err = (got.cpu().float() - want.float()).abs()
    assert bool((err <= tol).all()), f"SwiGLU: {int((err > tol).sum())} elements beyond one bf16 ulp, max {float(err.max())}"
    assert torch.equal(ref.unpack_act(ap.cpu(), m), got.cpu())


NPOS = 1024


@pytest.mark.parametrize("m,s", [(1, 1), (16, 1), (17, 1), (33, 3), (64, 4)])
@pytest.mark.parametrize("k", [128, 2176])
def test_qkv_rope_w4_epilogue_exact(k, m, s):
    h, hkv, t, slot0 = 4, 2, 40, 7
    b = m // s
    n = (h + 2 * hkv) * DH
    xg, f4, ys = _int_case(m, n, k, True)
    _fast(xg, f4, QKV)
    pos = torch.randperm(NPOS, generator=torch.Generator().manual_seed(m))[:m].to(torch.int32)
    want = xi.qkv_rope_exact(ys, pos, NPOS, b, s, h, hkv, t, slot0)
    kg = torch.zeros(b, hkv, t, DH, dtype=BF16, device=DEV)
    vg = torch.zeros_like(kg)
    qg = ops.linear_qkv_rope(xg, f4, None, xi.quarter_table(NPOS).to(DEV), pos.to(DEV), kg, vg,
                             torch.tensor([slot0], dtype=torch.int32, device=DEV), s, h, hkv, DH)
    for name, a, w_ in zip(("q", "K cache", "V cache"), (qg, kg, vg), want):
        assert torch.equal(a.cpu(), w_), f"{name}: {int((a.cpu() != w_).sum())} elements differ"


# ---------------------------------------------------------------------------------- random-data GEMV
@functools.lru_cache(maxsize=None)
def _rand_linear(n, k, seed=0):
    w = (torch.randn(n, k, generator=torch.Generator().manual_seed(seed + n + k)) * 0.05).to(BF16)
    f4 = Mxfp4Linear.from_dense(w, DEV)
    return f4, Mxfp4Linear.from_dense(w, "cpu").dense()


@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("m", [1, 17, 64])
@pytest.mark.parametrize("n,k", [(256, 512), (4096, 384)])
def test_w4_random_store_residual(n, k, m, rms):
    g = torch.Generator().manual_seed(m)
    x = (torch.randn(m, k, generator=g) * 2).to(BF16)
    f4, wdeq = _rand_linear(n, k)
    eps = 1e-5 if rms else None
    xg = x.to(DEV)
    _fast(xg, f4, STORE)
    expect = ref.linear(x, wdeq, eps, torch.float32)
    _close(ops.linear(xg, f4, rms_eps=eps, out_dtype=torch.float32), expect, 1e-2, 1e-3)
    _close(ops.linear(xg, f4, rms_eps=eps), expect, 2e-2, 2e-2)
    h = torch.randn(m, n, generator=g)
    for acc in (True, False):
        hg = h.to(DEV)
        mir = torch.empty(m, n, dtype=BF16, device=DEV)
        ops.linear_residual(xg, f4, hg, rms_eps=eps, accumulate=acc, mirror=mir)
        _close(hg, ref.linear_residual(x, wdeq, h.clone(), eps, accumulate=acc), 1e-2, 1e-3)
        assert torch.equal(mir.cpu(), hg.cpu().to(BF16))


@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("m", [1, 17, 64])
def test_w4_random_swiglu(m, rms):
    f, k = 352, 640
    g = torch.Generator().manual_seed(m)
    w1, w3 = [(torch.randn(f, k, generator=g) * 0.05).to(BF16) for _ in range(2)]
    f4 = Mxfp4Linear.from_dense(ref.interleave_gate_up(w1, w3), DEV)
    d1, d3 = [ref.dequantize_mxfp4(*ref.quantize_mxfp4(w)) for w in (w1, w3)]
    x = torch.randn(m, k, generator=g).to(BF16)
    eps = 1e-5 if rms else None
    _fast(x.to(DEV), f4, SWIGLU)
    y = ops.linear_swiglu(x.to(DEV), f4, rms_eps=eps)
    gg, uu = ref.linear(x, d1, eps, torch.float32), ref.linear(x, d3, eps, torch.float32)
    _close(y, torch.nn.functional.silu(gg) * uu, 3e-2, 3e-2)


@pytest.mark.parametrize("rms", [False, True])
@pytest.mark.parametrize("m,s", [(1, 1), (6, 3), (17, 1), (64, 1)])  # (17: two m-tiles, the hand-counted ring)
def test_w4_random_qkv_rope(m, s, rms):
    h, hkv, dh, t, k = 4, 2, 128, 24, 384
    b = m // s
    n = (h + 2 * hkv) * dh
    f4, wdeq = _rand_linear(n, k, seed=1)
    g = torch.Generator().manual_seed(m)
    x = torch.randn(m, k, generator=g).to(BF16)
    table = ref.rope_table(dh, 64, 10000.0)
    pos = torch.randint(0, 40, (m,), dtype=torch.int32, generator=g)
    eps = 1e-5 if rms else None
    kc = torch.zeros(b, hkv, t, dh, dtype=BF16)
    vc = torch.zeros_like(kc)
    q = ref.linear_qkv_rope(x, wdeq, eps, table, pos, kc, vc, 3, s, h, hkv, dh)
    kg, vg = torch.zeros_like(kc, device=DEV), torch.zeros_like(vc, device=DEV)
    _fast(x.to(DEV), f4, QKV)
    qg = ops.linear_qkv_rope(x.to(DEV), f4, eps, table.to(DEV), pos.to(DEV), kg, vg,
                             torch.tensor([3], dtype=torch.int32, device=DEV), s, h, hkv, dh)
    _close(qg, q, 2e-2, 2e-2)
    _close(kg, kc, 2e-2, 2e-2)
    _close(vg, vc, 2e-2, 2e-2)


# ---------------------------------------------------------------------------------- the dequant path is the bf16 path
@functools.lru_cache(maxsize=None)
def _pair(n, k):
    f4, wdeq = _rand_linear(n, k, seed=2)
    return f4, PackedLinear.from_dense(wdeq, DEV)


@pytest.mark.parametrize("m,xdt", [(65, BF16), (200, BF16), (5, torch.float32)])
def test_dequant_path_equals_bf16_kernels(m, xdt):
    n, k = 512, 1024
    f4, pw = _pair(n, k)
    x = torch.randn(m, k, generator=torch.Generator().manual_seed(m)).to(xdt).to(DEV)
    assert not ops._w4_fast(ops.ext(), x, f4, STORE)
    for eps in (None, 1e-5):
        assert torch.equal(ops.linear(x, f4, rms_eps=eps, out_dtype=torch.float32),
                           ops.linear(x, pw, rms_eps=eps, out_dtype=torch.float32))
        assert torch.equal(ops.linear_swiglu(x, f4, rms_eps=eps), ops.linear_swiglu(x, pw, rms_eps=eps))
    h = torch.randn(m, n, generator=torch.Generator().manual_seed(m + 1))
    ha, hb = h.to(DEV), h.to(DEV)
    ma, mb = [torch.empty(m, n, dtype=BF16, device=DEV) for _ in range(2)]
    ops.linear_residual(x, f4, ha, mirror=ma)
    ops.linear_residual(x, pw, hb, mirror=mb)
    assert torch.equal(ha, hb) and torch.equal(ma, mb)


@pytest.mark.parametrize("m", [3, 70, 300])
def test_dequant_path_argmax_logprob(m):
    n, k = 1024, 512
    f4, pw = _pair(n, k)
    g = torch.Generator().manual_seed(m)
    x = torch.randn(m, k, generator=g).to(BF16).to(DEV)
    ia, va = ops.linear_argmax(x, f4, rms_eps=1e-5)
    ib, vb = ops.linear_argmax(x, pw, rms_eps=1e-5)
    assert torch.equal(ia, ib) and torch.equal(va, vb)
    tg = torch.randint(0, n, (m,), dtype=torch.int32, generator=g).to(DEV)
    for a, b in zip(ops.linear_logprob(x, f4, tg, rms_eps=1e-5), ops.linear_logprob(x, pw, tg, rms_eps=1e-5)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("m,s", [(70, 2), (256, 1)])
def test_dequant_path_qkv_rope(m, s):
    h, hkv, dh, t, k = 4, 2, 128, 8, 512
    b = m // s
    f4, pw = _pair((h + 2 * hkv) * dh, k)
    g = torch.Generator().manual_seed(m)
    x = torch.randn(m, k, generator=g).to(BF16).to(DEV)
    table = ref.rope_table(dh, 64, 10000.0).to(DEV)
    pos = torch.randint(0, 40, (m,), dtype=torch.int32, generator=g).to(DEV)
    outs = []
    for w in (f4, pw):
        kg = torch.zeros(b, hkv, t, dh, dtype=BF16, device=DEV)
        vg = torch.zeros_like(kg)
        q = ops.linear_qkv_rope(x, w, 1e-5, table, pos, kg, vg, torch.tensor([2], dtype=torch.int32, device=DEV), s, h,
                                hkv, dh)
        outs.append((q, kg, vg))
    for a, b_ in zip(*outs):
        assert torch.equal(a, b_)


def test_fused_launches_decline_mxfp4():
    f4, pw = _pair(1280, 512)
    x = torch.randn(1, 512).to(BF16).to(DEV)
    kc = torch.zeros(1, 1, 64, 128, dtype=BF16, device=DEV)
    assert ops.qkv_attention_splits(x, f4, kc, 1, 8, 1) == 0
    assert ops.qkv_attention_o_groups(x, f4, 8, 1) == 0


# ---------------------------------------------------------------------------------- tiny model
@functools.lru_cache(maxsize=None)
def _models(seed=0):
    """(config, quantised model, bf16 model holding W_deq, the original bf16 model), on the GPU."""
    cfg = gpu_config()
    _, _, _, params = build(cfg, seed=seed)
    q4, deq, orig = [LLaMAForCausalLM(cfg, device=DEV, _do_init=False).load_params(params) for _ in range(3)]
    q4.quantize_weights_("mxfp4")
    for lq, ld in zip(q4.layers, deq.layers):
        for name in ("qkv", "o", "gu", "down"):
            setattr(ld, name, PackedLinear.from_dense(getattr(lq, name).dense(), DEV))
    return cfg, q4, deq, orig


def _prefill(model, toks, kv_format="bf16"):
    b, s = toks.shape
    cache = KVCache(model.config.num_hidden_layers, b, model.n_kv_heads, s + 4, model.head_dim, DEV,
                    kv_format=kv_format)
    pos = torch.arange(s, dtype=torch.int32).expand(b, s).contiguous().to(DEV)
    kvs = torch.zeros(b, dtype=torch.int32, device=DEV)
    logits, *_ = model.forward_tokens(toks.to(DEV), pos, cache, 0, kvs, None, logits_mode="last")
    return logits, cache, kvs


@pytest.mark.parametrize("b,s", [(2, 40), (40, 5)])
def test_model_prefill_exact_and_decode_close(b, s):
    cfg, q4, deq, orig = _models()
    assert q4.weight_format == "mxfp4" and all(lw.qkv.packed for lw in q4.layers)
    toks = torch.randint(0, cfg.vocab_size, (b, s), dtype=torch.int32, generator=torch.Generator().manual_seed(b))
    assert b * s > 64  # every GEMM of the prefill is on the dequant path: the same kernels on the same bits
    lq, cq, kvs = _prefill(q4, toks)
    ld, cd, _ = _prefill(deq, toks)
    lo, _, _ = _prefill(orig, toks)
    assert torch.equal(lq, ld)
    rel = (lq - lo).abs() / lo.abs().max()
    print(f"mxfp4 vs bf16 last-token logits (B={b}, S={s}): max rel err {float(rel.max()):.4f}, "
          f"mean rel err {float(rel.mean()):.5f}")
    # one decode step of b rows on the MXFP4 GEMV (b <= 64) against the bf16 kernels on W_deq: a different summation
    # order, so the whole-model tolerance of tests/test_fp8_gpu.py; tokens are not compared (near-ties)
    nxt = torch.randint(0, cfg.vocab_size, (b, 1), dtype=torch.int32, generator=torch.Generator().manual_seed(b + 1))
    pos = torch.full((b, 1), s, dtype=torch.int32, device=DEV)
    slot = torch.tensor([s], dtype=torch.int32, device=DEV)
    dq, *_ = q4.forward_tokens(nxt.to(DEV), pos, cq, slot, kvs, None, logits_mode="last")
    dd, *_ = deq.forward_tokens(nxt.to(DEV), pos, cd, slot, kvs, None, logits_mode="last")
    assert bool(torch.isfinite(dq).all()) and rel_err(dq, dd) < 2e-2


def test_model_prefill_with_fp8_kv_cache():
    """The quantising KV write follows the bf16 projection output, whatever the weight format."""
    cfg, q4, deq, _ = _models()
    toks = torch.randint(0, cfg.vocab_size, (2, 40), dtype=torch.int32, generator=torch.Generator().manual_seed(3))
    lq, cq, _ = _prefill(q4, toks, "fp8_e4m3")
    ld, cd, _ = _prefill(deq, toks, "fp8_e4m3")
    assert cq.kv_format == "fp8_e4m3"
    assert torch.equal(lq, ld)
    for i in range(cfg.num_hidden_layers):
        for a, b in zip(cq.layer(i), cd.layer(i)):
            assert torch.equal(a.q, b.q) and torch.equal(a.scale, b.scale)


def test_model_graph_replay_matches_eager():
    cfg, q4, _, _ = _models()
    toks, mask = left_padded_batch([5, 8], 8, cfg.vocab_size, pad=2, seed=6)
    gc = GenerationConfig(max_length=48, do_sample=False, pad_token_id=2, eos_token_id=2)
    a = DecodeEngine(q4, 2, 48, use_graph=True).run(toks, mask, gc).clone()
    b = DecodeEngine(q4, 2, 48, use_graph=False).run(toks, mask, gc).clone()
    assert torch.equal(a, b)
    gs = dict(max_length=30, do_sample=True, temperature=0.8, top_p=0.95, pad_token_id=2, eos_token_id=2)
    s1 = q4.generate(toks, mask, GenerationConfig(seed=11, **gs)).sequences
    s2 = q4.generate(toks, mask, GenerationConfig(seed=11, **gs)).sequences
    assert torch.equal(s1, s2) and int(s1.min()) >= 0 and int(s1.max()) < cfg.vocab_size


def test_model_score_and_checkpoint(tmp_path):
    cfg, q4, deq, _ = _models()
    toks = torch.randint(0, cfg.vocab_size, (3, 30), dtype=torch.int32, generator=torch.Generator().manual_seed(9))
    sq, sd = q4.score(toks), deq.score(toks)  # 90 rows: the dequant path
    assert torch.equal(sq.token_logprobs, sd.token_logprobs) and torch.equal(sq.is_greedy, sd.is_greedy)
    q4.save_pretrained(str(tmp_path))
    back = LLaMAForCausalLM.from_pretrained(str(tmp_path), device=DEV)
    assert back.weight_format == "mxfp4"
    for la, lb in zip(q4.layers, back.layers):
        for name in ("qkv", "o", "gu", "down"):
            a, b = getattr(la, name), getattr(lb, name)
            assert torch.equal(a.qweight, b.qweight) and torch.equal(a.scale, b.scale)


# ---------------------------------------------------------------------------------- nothing changes for bf16
def _decode_graph_kernels(model, batch):
    gc = GenerationConfig(max_length=24, do_sample=False, pad_token_id=0, eos_token_id=-1)
    eng = DecodeEngine(model, batch, 24, use_graph=True)
    eng.gc = gc
    g = torch.Generator().manual_seed(batch)
    eng.prefill(torch.randint(3, model.config.vocab_size, (batch, 8), generator=g, dtype=torch.int32), None)
    eng._decode_step()
    eng.keep_graph = True
    eng._ensure_graph()
    return graph_kernels(eng._graph)


# Kernel nodes of the captured decode step of the bf16 tiny model (2 layers) with the default decode GEMV pinned (as
# tests/test_fp8_gpu.py counts them): embedding, per layer qkv GEMV + attention + o GEMV + w1|w3 GEMV + w2 GEMV, the
# lm_head GEMV with its argmax partials + their reduce, and the state update.
BF16_DECODE_KERNELS = 14


@pytest.mark.parametrize("batch", [2, 40])
def test_bf16_decode_graph_is_unchanged(batch):
    cfg, q4, deq, orig = _models()
    try:
        ops.GEMV_VARIANT = 1
        n_bf16 = _decode_graph_kernels(orig, batch)
        n_fp4 = _decode_graph_kernels(q4, batch)
    finally:
        ops.GEMV_VARIANT = 0
    print(f"decode graph kernel nodes at B={batch}: bf16 {n_bf16}, mxfp4 {n_fp4}")
    assert n_bf16 == BF16_DECODE_KERNELS
    assert n_fp4 == n_bf16  # (the MXFP4 GEMV is one launch per projection, like the bf16 GEMV)
