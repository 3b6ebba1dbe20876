"""MXFP4 (e2m1 codes, one e8m0 scale per row and 32 K elements) weight-only linears on the CPU path: the quantiser's
defined numerics, the 16 x 128 block layout and the scale layout, and that a quantised model computes exactly what a
bf16 model loaded with the dequantised weights computes."""
from __future__ import annotations

import json
import os

import pytest
import torch

from jax_llama_amd.models import LLaMAForCausalLM
from jax_llama_amd.models.weights import Fp8Linear, Mxfp4Linear, PackedLinear
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime import engine as eng_mod
from jax_llama_amd.runtime.engine import GenerationConfig
from helpers import build, gpu_config

BF16 = torch.bfloat16
VALUES = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)


def _gauss(n, k, std, seed):
    return (torch.randn(n, k, generator=torch.Generator().manual_seed(seed)) * std).to(BF16)


def _scales(e8m0):
    """fp64 [N, K/32] block scales 2^(b - 127)."""
    return torch.ldexp(torch.ones(e8m0.shape, dtype=torch.float64), e8m0.to(torch.int32) - 127)


def _per_elem(s, k):
    return s.repeat_interleave(32, dim=1)[:, :k]


def _value(codes):
    """fp64 value of every code, from the format's definition (not from ``ref``'s table)."""
    return VALUES[(codes & 7).long()] * torch.where(codes >= 8, -1.0, 1.0).double()


# ---------------------------------------------------------------------------------- quantiser
@pytest.mark.parametrize("std", [1e-4, 0.02, 1.0, 37.0])
def test_quantiser_bounds(std):
    w = _gauss(64, 512, std, 1)
    codes, e8 = ref.quantize_mxfp4(w)
    assert codes.dtype == torch.uint8 and codes.shape == w.shape and int(codes.max()) <= 15
    assert e8.dtype == torch.uint8 and e8.shape == (64, 16)
    s = _scales(e8)  # (a power of two by construction: one e8m0 byte)
    assert int(e8.min()) >= 27 and int(e8.max()) <= 227
    # the scale is the defined power of two: the smallest one that brings the block maximum to <= 6
    amax = w.double().abs().reshape(64, 16, 32).amax(2)
    assert bool((amax > 0).all())
    r = amax / s
    assert bool((r <= 6).all()) and bool((r > 3).all())
    # W_deq is exact in bf16
    deq64 = _value(codes) * _per_elem(s, 512)
    deq = ref.dequantize_mxfp4(codes, e8)
    assert deq.dtype == BF16 and torch.equal(deq.double(), deq64)
    # element-wise error: half an e2m1 step. From |w| / s = 1 up a step is at most half the value (2^-2 relative);
    # below it the step is 0.5 (2^-2 s absolute)
    se = _per_elem(s, 512)
    ratio = w.double().abs() / se
    err = (deq64 - w.double()).abs()
    big = ratio >= 1
    assert bool((err[big] <= 2.0 ** -2 * w.double().abs()[big]).all())
    assert bool((err[~big] <= 2.0 ** -2 * se[~big]).all())


@pytest.mark.parametrize("std", [1e-4, 0.02, 37.0])
def test_quantiser_value_idempotent(std):
    """Quantising W_deq again gives W_deq (the scale may drop by one power of two when a block maximum rounds down to
    3: values are compared, not bytes)."""
    w = _gauss(48, 256, std, 2)
    deq = ref.dequantize_mxfp4(*ref.quantize_mxfp4(w))
    assert torch.equal(ref.dequantize_mxfp4(*ref.quantize_mxfp4(deq)), deq)


def test_quantiser_zero_block_and_integers():
    g = torch.Generator().manual_seed(3)
    ints = torch.randint(-2, 3, (32, 128), generator=g).float()
    ints[:, 0::32] = 2.0  # (every block holds its maximum)
    pw = 2.0 ** torch.randint(-3, 4, (32, 4), generator=g).float()
    w = (ints * pw.repeat_interleave(32, dim=1)).to(BF16)
    w[5, 32:64] = 0
    codes, e8 = ref.quantize_mxfp4(w)
    assert int(e8[5, 1]) == 127 and bool((codes[5, 32:64] == 0).all())
    assert torch.equal(ref.dequantize_mxfp4(codes, e8), w)  # integers in [-2, 2] x per-block powers of two: exact


def test_quantiser_block_maximum_at_the_scale_boundary():
    """amax = 1.5 = 6 * 2^-2 maps onto 6 exactly; just above it the scale doubles and the maximum lands on 3."""
    w = torch.zeros(2, 64)
    w[0, 3], w[1, 3] = 1.5, 1.5001
    w[:, 7] = -0.25
    w[:, 40] = 1.0  # (the second block of each row has its own scale)
    codes, e8 = ref.quantize_mxfp4(w)
    assert e8[:, 0].tolist() == [125, 126]
    assert codes[:, 3].tolist() == [7, 5]
    assert codes[:, 7].tolist() == [8 | 2, 8 | 1]  # -0.25 / 2^-2 = -1, -0.25 / 2^-1 = -0.5
    assert e8[:, 1].tolist() == [125, 125] and codes[:, 40].tolist() == [6, 6]  # 1.0 = 4 * 2^-2


def test_rounding_ties_to_even_and_signs():
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    want = torch.tensor([0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0], dtype=torch.float64)
    got = ref.e2m1_rne(ties)
    assert torch.equal(_value(got), want) and bool((got & 1 == 0).all())  # every tie lands on an even code
    assert torch.equal(_value(ref.e2m1_rne(-ties)), -want) and bool((ref.e2m1_rne(-ties) >= 8).all())
    # just off a tie: to the nearer value
    eps = 2.0 ** -10
    assert _value(ref.e2m1_rne(ties + eps)).tolist() == [0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    assert _value(ref.e2m1_rne(ties - eps)).tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0]
    # every representable value is a fixed point, with its sign bit; -0.0 keeps its sign bit
    for sgn in (1.0, -1.0):
        v = (VALUES * sgn).float()
        c = ref.e2m1_rne(v)
        assert c.tolist() == [i + (8 if sgn < 0 else 0) for i in range(8)]
    # through the quantiser: a block whose maximum is 6 has scale 1, so the ties are taken as they are
    w = torch.zeros(16, 128)
    w[0, 0] = 6.0
    w[0, 1:8] = ties
    w[0, 8:15] = -ties
    w[0, 15] = -0.0
    codes, e8 = ref.quantize_mxfp4(w)
    assert int(e8[0, 0]) == 127
    assert codes[0, :16].tolist() == [7, 0, 2, 2, 4, 4, 6, 6, 8, 10, 10, 12, 12, 14, 14, 8]
    deq = ref.dequantize_mxfp4(codes, e8)
    assert bool(torch.signbit(deq[0, 15].float())) and float(deq[0, 15]) == 0.0


def test_quantiser_exponent_clamp():
    w = torch.zeros(2, 32)
    w[0, 0], w[1, 0] = 1e-38, 3e38
    codes, e8 = ref.quantize_mxfp4(w)
    assert e8[:, 0].tolist() == [27, 227]
    deq = ref.dequantize_mxfp4(codes, e8)
    assert not bool(torch.isnan(deq.float()).any()) and bool(torch.isfinite(deq.float()).all())
    assert codes[:, 0].tolist() == [0, 7]


# ---------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("n,k", [(16, 128), (48, 384), (64, 4096)])
def test_pack_roundtrip_and_lane_order(n, k):
    g = torch.Generator().manual_seed(n + k)
    codes = torch.randint(0, 16, (n, k), dtype=torch.uint8, generator=g)
    p = ref.pack_mxfp4_16x128(codes)
    assert p.dtype == torch.uint8 and p.shape == (n // 16, k // 128, 64, 16)
    assert torch.equal(ref.unpack_mxfp4_16x128(p, n, k), codes)
    # the definition, element by element on a few (block, lane) pairs
    for nt, kb, lane in ((0, 0, 0), (n // 16 - 1, k // 128 - 1, 63), (0, k // 128 - 1, 37), (n // 16 - 1, 0, 18)):
        row = nt * 16 + (lane & 15)
        for j in range(4):
            col = kb * 128 + 32 * j + 8 * (lane >> 4)
            for e in range(8):
                byte = int(p[nt, kb, lane, 4 * j + e // 2])
                assert (byte >> 4 if e & 1 else byte & 15) == int(codes[row, col + e]), (nt, kb, lane, j, e)
    # dword j of every lane holds, in order, the elements of the bf16 fragment of k-step 4 kb + j
    frag = ref.pack_frag16x32(codes)  # [n/16, k/32, 64, 8] in the same element order
    lo, hi = p & 15, p >> 4
    elems = torch.stack([lo, hi], -1).reshape(n // 16, k // 128, 64, 4, 8)  # [.., lane, dword j, element]
    for j in range(4):
        assert torch.equal(elems[:, :, :, j], frag[:, j::4])
    # the scales: one dword per (row, 128-deep block), byte j the scale of k-step 4 kb + j
    e8 = torch.randint(0, 256, (n, k // 32), dtype=torch.uint8, generator=g)
    sp = ref.pack_mxfp4_scales(e8)
    assert sp.dtype == torch.uint8 and sp.shape == (n // 16, k // 128, 16, 4)
    assert torch.equal(ref.unpack_mxfp4_scales(sp, n, k), e8)
    for nt, kb, r, j in ((0, 0, 0, 0), (n // 16 - 1, k // 128 - 1, 15, 3), (0, k // 128 - 1, 5, 2)):
        assert int(sp[nt, kb, r, j]) == int(e8[16 * nt + r, 4 * kb + j])


@pytest.mark.parametrize("n,k", [(8, 128), (16, 64), (16, 192), (24, 128)])
def test_layout_refuses_other_shapes(n, k):
    codes = torch.zeros(n, k, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ref.pack_mxfp4_16x128(codes)
    with pytest.raises(ValueError):
        ref.unpack_mxfp4_16x128(codes.reshape(-1)[: n * k // 2], n, k)
    with pytest.raises(ValueError):
        ref.pack_mxfp4_scales(torch.zeros(n, k // 32, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ref.unpack_mxfp4_scales(torch.zeros(n * (k // 32), dtype=torch.uint8), n, k)
    with pytest.raises(ValueError):
        Mxfp4Linear.from_dense(torch.zeros(n, k, dtype=BF16), "cpu")


def test_container_surface():
    w = _gauss(32, 256, 0.05, 4)
    fold = 1.0 + 0.1 * torch.randn(256, generator=torch.Generator().manual_seed(5))
    f4 = Mxfp4Linear.from_dense(w, "cpu", fold=fold)
    folded = PackedLinear.from_dense(w, "cpu", fold=fold).dense()  # quantised after the fold
    assert torch.equal(f4.dense(), ref.dequantize_mxfp4(*ref.quantize_mxfp4(folded)))
    assert (f4.n, f4.k, f4.device.type, f4.packed) == (32, 256, "cpu", False)
    assert f4.nbytes() == 32 * 256 // 2 + 32 * 256 // 32
    assert getattr(f4, "mxfp4", False) and not getattr(f4, "fp8", False)
    assert torch.equal(Mxfp4Linear.from_linear(PackedLinear.from_dense(folded, "cpu")).dense(), f4.dense())
    back = Mxfp4Linear.from_q(f4.q(), f4.e8m0(), "cpu")
    assert torch.equal(back.q(), f4.q()) and torch.equal(back.e8m0(), f4.e8m0())
    with pytest.raises(ValueError):
        Mxfp4Linear.from_q(f4.q(), f4.e8m0()[:, :-1], "cpu")
    # scale bytes the quantiser never writes (the CPU and kernel definitions part there) and codes past 15 are refused
    for bad in (0, 26, 228, 255):
        e8 = f4.e8m0().clone()
        e8[3, 1] = bad
        with pytest.raises(ValueError):
            Mxfp4Linear.from_q(f4.q(), e8, "cpu")
    for good in (27, 227):
        e8 = f4.e8m0().clone()
        e8[3, 1] = good
        Mxfp4Linear.from_q(f4.q(), e8, "cpu")
    codes = f4.q().clone()
    codes[0, 0] = 16
    with pytest.raises(ValueError):
        Mxfp4Linear.from_q(codes, f4.e8m0(), "cpu")


# ---------------------------------------------------------------------------------- model
def _models(seed=0):
    """(mxfp4 model, bf16 model holding W_deq, the original bf16 model) on the CPU: 2 layers, hidden 256, 4 q / 2 kv
    heads, ffn 512, vocab 512."""
    cfg = gpu_config(num_attention_heads=4, num_key_value_heads=2)
    q4, _, _, params = build(cfg, seed=seed)
    orig = LLaMAForCausalLM(cfg, _do_init=False).load_params(params)
    deq = LLaMAForCausalLM(cfg, _do_init=False).load_params(params)
    q4.quantize_weights_("mxfp4")
    for lq, ld in zip(q4.layers, deq.layers):
        for name in ("qkv", "o", "gu", "down"):
            setattr(ld, name, PackedLinear.from_dense(getattr(lq, name).dense(), "cpu"))
    return cfg, q4, deq, orig


@pytest.fixture(scope="module")
def models():
    return _models()


def test_model_is_the_bf16_model_on_wdeq(models):
    cfg, q4, deq, orig = models
    assert q4.weight_format == "mxfp4" and deq.weight_format == "bf16"
    assert all(isinstance(getattr(lw, n), Mxfp4Linear) for lw in q4.layers for n in ("qkv", "o", "gu", "down"))
    assert isinstance(q4.lm_head, PackedLinear)  # lm_head (and wte) keep their format
    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, cfg.vocab_size, (3, 12), dtype=torch.int32, generator=g)
    lq, ld, lo = q4(toks).logits, deq(toks).logits, orig(toks).logits
    assert torch.equal(lq, ld)
    sq, sd = q4.score(toks), deq.score(toks)
    assert torch.equal(sq.token_logprobs, sd.token_logprobs) and torch.equal(sq.is_greedy, sd.is_greedy)
    gc = GenerationConfig(max_length=24, do_sample=False, pad_token_id=2, eos_token_id=-1)
    assert torch.equal(q4.generate(toks, generation_config=gc).sequences,
                       deq.generate(toks, generation_config=gc).sequences)
    # model quality against the original bf16 weights (recorded, no threshold: the element-wise bounds are the contract)
    rel = (lq - lo).abs() / lo.abs().max()
    print(f"mxfp4 vs bf16 logits, tiny random-init model: max rel err {float(rel.max()):.4f}, "
          f"mean rel err {float(rel.mean()):.5f}")
    assert bool(torch.isfinite(lq).all())


def test_quantise_twice_and_unknown_format(models):
    _, q4, deq, _ = models
    with pytest.raises(RuntimeError):
        q4.quantize_weights_("mxfp4")
    with pytest.raises(RuntimeError):
        q4.quantize_weights_("fp8_e4m3")
    with pytest.raises(ValueError):
        deq.quantize_weights_("int4")
    assert deq.weight_format == "bf16"
    assert "mxfp4" in LLaMAForCausalLM.WEIGHT_FORMATS and "fp8_e4m3" in LLaMAForCausalLM.WEIGHT_FORMATS


def test_refused_model_shape_leaves_the_model_bf16():
    """A K that is no multiple of 128 (here the down projection's, ffn 320) is refused, and nothing was replaced."""
    cfg = gpu_config(num_attention_heads=4, num_key_value_heads=2, intermediate_size=320)
    model, *_ = build(cfg, seed=1)
    with pytest.raises(ValueError):
        model.quantize_weights_("mxfp4")
    assert model.weight_format == "bf16"
    assert all(isinstance(getattr(lw, n), PackedLinear) for lw in model.layers for n in ("qkv", "o", "gu", "down"))


def test_weight_bytes(models):
    cfg, q4, deq, _ = models
    d, f, v, hd = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.head_dim
    nqkv = (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * hd
    shapes = [(nqkv, d), (d, cfg.num_attention_heads * hd), (2 * f, d), (d, f)]
    per_layer = sum(n * k // 2 + n * k // 32 for n, k in shapes)
    assert q4.weight_bytes() == 2 * v * d + 2 * v * d + cfg.num_hidden_layers * per_layer
    assert q4.streamed_weight_bytes_per_token() == 2 * v * d + cfg.num_hidden_layers * per_layer
    assert deq.weight_bytes() == 2 * v * d + 2 * v * d + cfg.num_hidden_layers * sum(2 * n * k for n, k in shapes)


def test_checkpoint_roundtrip(models, tmp_path):
    cfg, q4, deq, _ = models
    q4.save_pretrained(str(tmp_path / "q4"))
    with open(os.path.join(tmp_path / "q4", "jla_native.json")) as fh:
        assert json.load(fh)["weights"] == "mxfp4"
    from safetensors import safe_open
    with safe_open(os.path.join(tmp_path / "q4", "model-rank00-of-01.safetensors"), framework="pt") as f:
        lin = q4.layers[0].qkv
        stored = f.get_tensor("h.0.qkv.q")
        assert stored.dtype == torch.uint8 and tuple(stored.shape) == (lin.n, lin.k // 2)  # two codes per byte
        assert torch.equal(stored & 15, lin.q()[:, 0::2]) and torch.equal(stored >> 4, lin.q()[:, 1::2])
        assert torch.equal(f.get_tensor("h.0.qkv.scale"), lin.e8m0())
    back = LLaMAForCausalLM.from_pretrained(str(tmp_path / "q4"))
    assert back.weight_format == "mxfp4"
    for la, lb in zip(q4.layers, back.layers):
        for name in ("qkv", "o", "gu", "down"):
            a, b = getattr(la, name), getattr(lb, name)
            assert isinstance(b, Mxfp4Linear)
            assert torch.equal(a.q(), b.q()) and torch.equal(a.e8m0(), b.e8m0())
    toks = torch.randint(0, cfg.vocab_size, (2, 9), dtype=torch.int32, generator=torch.Generator().manual_seed(2))
    assert torch.equal(back(toks).logits, q4(toks).logits)
    # a bf16 checkpoint carries no marker and reloads as bf16
    deq.save_pretrained(str(tmp_path / "bf16"))
    with open(os.path.join(tmp_path / "bf16", "jla_native.json")) as fh:
        assert "weights" not in json.load(fh)
    assert LLaMAForCausalLM.from_pretrained(str(tmp_path / "bf16")).weight_format == "bf16"


def test_shard_then_quantise_equals_quantise_then_shard():
    """A K shard is a multiple of 32, so the blocks of a shard are blocks of the whole matrix."""
    w = _gauss(32, 512, 0.05, 6)
    codes, e8 = ref.quantize_mxfp4(w)
    for r in range(4):
        c, s = ref.quantize_mxfp4(w[:, 128 * r:128 * (r + 1)].contiguous())
        assert torch.equal(c, codes[:, 128 * r:128 * (r + 1)]) and torch.equal(s, e8[:, 4 * r:4 * (r + 1)])


# ---------------------------------------------------------------------------------- engine cache
@pytest.mark.parametrize("fmt,cls", [("mxfp4", Mxfp4Linear), ("fp8_e4m3", Fp8Linear)])
def test_quantising_drops_the_cached_engines(fmt, cls):
    """An engine from before ``quantize_weights_`` holds a graph captured on the weights the call frees: the next
    ``get_engine`` must build a new one. Other models' engines stay."""
    cfg = gpu_config(num_attention_heads=4, num_key_value_heads=2)
    model, *_ = build(cfg, seed=2)
    other, *_ = build(cfg, seed=3)
    eng_mod._ENGINES.clear()
    try:
        toks = torch.randint(3, cfg.vocab_size, (2, 5), dtype=torch.int32, generator=torch.Generator().manual_seed(4))
        gc = GenerationConfig(max_length=12, do_sample=False, pad_token_id=0, eos_token_id=-1)
        model.generate(toks, generation_config=gc)
        before = eng_mod.get_engine(model, 2, 12)
        assert eng_mod.get_engine(model, 2, 12) is before  # (the engine generate() used is cached)
        kept = eng_mod.get_engine(other, 2, 12)
        model.quantize_weights_(fmt)
        after = eng_mod.get_engine(model, 2, 12)
        assert after is not before
        assert eng_mod.get_engine(other, 2, 12) is kept
        assert isinstance(model.layers[0].qkv, cls)
        seq = model.generate(toks, generation_config=gc).sequences
        assert seq.shape == (2, 12) and torch.equal(seq[:, :5], toks)
    finally:
        eng_mod._ENGINES.clear()
