"""FP8 (OCP e4m3fn) weight-only linears on the CPU path: the quantiser's defined numerics, the 16 x 64 block layout,
and that a quantised model computes exactly what a bf16 model loaded with the dequantised weights computes."""
from __future__ import annotations

import json
import os

import pytest
import torch

from jax_llama_amd.models import LLaMAForCausalLM
from jax_llama_amd.models.weights import Fp8Linear, PackedLinear
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime.engine import GenerationConfig
from helpers import build, gpu_config

BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn


def _gauss(n, k, std, seed):
    return (torch.randn(n, k, generator=torch.Generator().manual_seed(seed)) * std).to(BF16)


# ---------------------------------------------------------------------------------- quantiser
@pytest.mark.parametrize("std", [1e-4, 0.02, 1.0, 37.0])
def test_quantiser_bounds(std):
    w = _gauss(64, 512, std, 1)
    q, s = ref.quantize_fp8_rows(w)
    assert q.dtype == FP8 and q.shape == w.shape and s.dtype == torch.float32 and s.shape == (64,)
    qf = q.float()
    assert not bool(torch.isnan(qf).any()) and float(qf.abs().max()) <= 448.0
    # the scale is the defined power of two: the smallest one that brings the row maximum to <= 448
    e = torch.log2(s.double())
    assert torch.equal(e, e.round())
    amax = w.double().abs().amax(1)
    assert bool((amax / s.double() <= 448).all()) and bool((amax / (s.double() / 2) > 448).all())
    # W_deq is exact in bf16
    deq64 = q.double() * s.double()[:, None]
    deq = ref.dequantize_fp8_rows(q, s)
    assert deq.dtype == BF16 and torch.equal(deq.double(), deq64)
    # element-wise error: half an e4m3 ulp (2^-4 relative) in the normal range, half a subnormal step (2^-10 s) below
    r = w.double().abs() / s.double()[:, None]
    err = (deq64 - w.double()).abs()
    normal = r >= 2.0 ** -6
    assert bool((err[normal] <= 2.0 ** -4 * w.double().abs()[normal]).all())
    assert bool((err[~normal] <= 2.0 ** -10 * s.double()[:, None].expand_as(err)[~normal]).all())


@pytest.mark.parametrize("std", [1e-4, 0.02, 37.0])
def test_quantiser_value_idempotent(std):
    """Quantising W_deq again gives W_deq (the scale may drop by one power of two when a row maximum rounds down to
    224: values are compared, not bytes)."""
    w = _gauss(48, 256, std, 2)
    deq = ref.dequantize_fp8_rows(*ref.quantize_fp8_rows(w))
    assert torch.equal(ref.dequantize_fp8_rows(*ref.quantize_fp8_rows(deq)), deq)


def test_quantiser_zero_row_and_integers():
    g = torch.Generator().manual_seed(3)
    ints = torch.randint(-2, 3, (32, 128), generator=g).float()
    ints[:, 0] = 2.0  # (every row holds its maximum)
    pw = 2.0 ** torch.randint(-3, 4, (32,), generator=g).float()
    w = (ints * pw[:, None]).to(BF16)
    w[5] = 0
    q, s = ref.quantize_fp8_rows(w)
    assert float(s[5]) == 1.0 and bool((q[5].float() == 0).all())
    assert torch.equal(ref.dequantize_fp8_rows(q, s), w)  # integers in [-2, 2] x per-row powers of two: exact


def test_quantiser_row_maximum_at_the_scale_boundary():
    """amax = 3.5 = 448 * 2^-7 maps onto 448 exactly; just above it the scale doubles and the maximum lands on 224."""
    w = torch.zeros(2, 64)
    w[0, 3], w[1, 3] = 3.5, 3.5001
    w[:, 7] = -1.0
    q, s = ref.quantize_fp8_rows(w)
    assert s.tolist() == [2.0 ** -7, 2.0 ** -6]
    assert q.float()[:, 3].tolist() == [448.0, 224.0] and q.float()[:, 7].tolist() == [-128.0, -64.0]


def test_quantiser_exponent_clamp():
    w = torch.zeros(2, 64)
    w[0, 0], w[1, 0] = 1e-38, 3e38
    q, s = ref.quantize_fp8_rows(w)
    assert s.tolist() == [2.0 ** -100, 2.0 ** 100]
    assert not bool(torch.isnan(q.float()).any()) and float(q.float().abs().max()) <= 448.0


# ---------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("n,k", [(16, 64), (48, 192), (64, 4096)])
def test_pack_roundtrip_and_lane_order(n, k):
    q = torch.randint(0, 256, (n, k), dtype=torch.uint8, generator=torch.Generator().manual_seed(n + k))
    p = ref.pack_fp8_16x64(q.view(FP8))
    assert p.dtype == torch.uint8 and p.shape == (n // 16, k // 64, 64, 16)
    assert torch.equal(ref.unpack_fp8_16x64(p, n, k).view(torch.uint8), q)
    # the definition, element by element on a few (block, lane) pairs
    for nt, kb, lane in ((0, 0, 0), (n // 16 - 1, k // 64 - 1, 63), (0, k // 64 - 1, 37), (n // 16 - 1, 0, 18)):
        row, col = nt * 16 + (lane & 15), kb * 64 + 8 * (lane >> 4)
        assert torch.equal(p[nt, kb, lane, :8], q[row, col:col + 8])
        assert torch.equal(p[nt, kb, lane, 8:], q[row, col + 32:col + 40])
    # bytes 0-7 / 8-15 of every lane are the bf16 fragments of k-steps 2 kb / 2 kb + 1
    frag = ref.pack_frag16x32(q)  # [n/16, k/32, 64, 8] in the same element order
    assert torch.equal(p[..., :8], frag[:, 0::2]) and torch.equal(p[..., 8:], frag[:, 1::2])


@pytest.mark.parametrize("n,k", [(8, 64), (16, 32), (16, 96), (24, 128)])
def test_layout_refuses_other_shapes(n, k):
    q = torch.zeros(n, k, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ref.pack_fp8_16x64(q)
    with pytest.raises(ValueError):
        ref.unpack_fp8_16x64(q.reshape(-1), n, k)
    with pytest.raises(ValueError):
        Fp8Linear.from_dense(torch.zeros(n, k, dtype=BF16), "cpu")


def test_container_surface():
    w = _gauss(32, 128, 0.05, 4)
    fold = 1.0 + 0.1 * torch.randn(128, generator=torch.Generator().manual_seed(5))
    f8 = Fp8Linear.from_dense(w, "cpu", fold=fold)
    folded = PackedLinear.from_dense(w, "cpu", fold=fold).dense()  # quantised after the fold
    assert torch.equal(f8.dense(), ref.dequantize_fp8_rows(*ref.quantize_fp8_rows(folded)))
    assert (f8.n, f8.k, f8.device.type, f8.nbytes()) == (32, 128, "cpu", 32 * 128 + 4 * 32)
    assert torch.equal(Fp8Linear.from_linear(PackedLinear.from_dense(folded, "cpu")).dense(), f8.dense())


# ---------------------------------------------------------------------------------- model
def _models(seed=0):
    """(fp8 model, bf16 model holding W_deq, the original bf16 model) on the CPU: 2 layers, hidden 256, 4 q / 2 kv
    heads, ffn 512, vocab 512."""
    cfg = gpu_config(num_attention_heads=4, num_key_value_heads=2)
    q8, _, _, params = build(cfg, seed=seed)
    orig = LLaMAForCausalLM(cfg, _do_init=False).load_params(params)
    deq = LLaMAForCausalLM(cfg, _do_init=False).load_params(params)
    q8.quantize_weights_("fp8_e4m3")
    for lq, ld in zip(q8.layers, deq.layers):
        for name in ("qkv", "o", "gu", "down"):
            setattr(ld, name, PackedLinear.from_dense(getattr(lq, name).dense(), "cpu"))
    return cfg, q8, deq, orig


@pytest.fixture(scope="module")
def models():
    return _models()


def test_model_is_the_bf16_model_on_wdeq(models):
    cfg, q8, deq, orig = models
    assert q8.weight_format == "fp8_e4m3" and deq.weight_format == "bf16"
    assert all(isinstance(getattr(lw, n), Fp8Linear) for lw in q8.layers for n in ("qkv", "o", "gu", "down"))
    assert isinstance(q8.lm_head, PackedLinear)  # lm_head (and wte) keep their format
    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, cfg.vocab_size, (3, 12), dtype=torch.int32, generator=g)
    lq, ld, lo = q8(toks).logits, deq(toks).logits, orig(toks).logits
    assert torch.equal(lq, ld)
    sq, sd = q8.score(toks), deq.score(toks)
    assert torch.equal(sq.token_logprobs, sd.token_logprobs) and torch.equal(sq.is_greedy, sd.is_greedy)
    gc = GenerationConfig(max_length=24, do_sample=False, pad_token_id=2, eos_token_id=-1)
    assert torch.equal(q8.generate(toks, generation_config=gc).sequences,
                       deq.generate(toks, generation_config=gc).sequences)
    # model quality against the original bf16 weights (recorded, no threshold: the element-wise bounds are the contract)
    rel = (lq - lo).abs() / lo.abs().max()
    print(f"fp8 vs bf16 logits, tiny random-init model: max rel err {float(rel.max()):.4f}, "
          f"mean rel err {float(rel.mean()):.5f}")
    assert bool(torch.isfinite(lq).all())


def test_quantise_twice_and_unknown_format(models):
    _, q8, deq, _ = models
    with pytest.raises(RuntimeError):
        q8.quantize_weights_("fp8_e4m3")
    with pytest.raises(ValueError):
        deq.quantize_weights_("int4")
    assert deq.weight_format == "bf16"


def test_weight_bytes(models):
    cfg, q8, deq, _ = models
    d, f, v, hd = cfg.hidden_size, cfg.intermediate_size, cfg.vocab_size, cfg.head_dim
    nqkv = (cfg.num_attention_heads + 2 * cfg.num_key_value_heads) * hd
    shapes = [(nqkv, d), (d, cfg.num_attention_heads * hd), (2 * f, d), (d, f)]
    per_layer = sum(n * k + 4 * n for n, k in shapes)
    assert q8.weight_bytes() == 2 * v * d + 2 * v * d + cfg.num_hidden_layers * per_layer
    assert q8.streamed_weight_bytes_per_token() == 2 * v * d + cfg.num_hidden_layers * per_layer
    assert deq.weight_bytes() == 2 * v * d + 2 * v * d + cfg.num_hidden_layers * sum(2 * n * k for n, k in shapes)


def test_checkpoint_roundtrip(models, tmp_path):
    cfg, q8, deq, _ = models
    q8.save_pretrained(str(tmp_path / "q8"))
    with open(os.path.join(tmp_path / "q8", "jla_native.json")) as fh:
        assert json.load(fh)["weights"] == "fp8_e4m3"
    back = LLaMAForCausalLM.from_pretrained(str(tmp_path / "q8"))
    assert back.weight_format == "fp8_e4m3"
    for la, lb in zip(q8.layers, back.layers):
        for name in ("qkv", "o", "gu", "down"):
            a, b = getattr(la, name), getattr(lb, name)
            assert isinstance(b, Fp8Linear)
            assert torch.equal(a.q().view(torch.uint8), b.q().view(torch.uint8)) and torch.equal(a.scale, b.scale)
    toks = torch.randint(0, cfg.vocab_size, (2, 9), dtype=torch.int32, generator=torch.Generator().manual_seed(2))
    assert torch.equal(back(toks).logits, q8(toks).logits)
    # a bf16 checkpoint carries no marker and reloads as bf16
    deq.save_pretrained(str(tmp_path / "bf16"))
    with open(os.path.join(tmp_path / "bf16", "jla_native.json")) as fh:
        assert "weights" not in json.load(fh)
    assert LLaMAForCausalLM.from_pretrained(str(tmp_path / "bf16")).weight_format == "bf16"
