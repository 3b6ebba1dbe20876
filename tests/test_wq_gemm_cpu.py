"""``model.set_quantized_gemm``: the setting's surface; on the CPU it changes no bit."""
from __future__ import annotations

import pytest
import torch

from helpers import build, gpu_config


@pytest.mark.parametrize("fmt", ["fp8_e4m3", "mxfp4"])
def test_set_quantized_gemm(fmt):
    cfg = gpu_config(num_attention_heads=4, num_key_value_heads=2)
    model, *_ = build(cfg, seed=0)
    with pytest.raises(RuntimeError):
        model.set_quantized_gemm("direct")  # not quantised
    model.quantize_weights_(fmt)
    assert model.quantized_gemm == "dequant"
    with pytest.raises(ValueError):
        model.set_quantized_gemm("fused")
    toks = torch.randint(0, cfg.vocab_size, (70, 3), dtype=torch.int32, generator=torch.Generator().manual_seed(1))
    want = model(toks).logits
    assert model.set_quantized_gemm("direct") is model and model.quantized_gemm == "direct"
    assert all(getattr(lw, n).gemm_direct for lw in model.layers for n in ("qkv", "o", "gu", "down"))
    assert torch.equal(model(toks).logits, want)
    assert model.set_quantized_gemm("dequant").quantized_gemm == "dequant"
    assert not any(getattr(lw, n).gemm_direct for lw in model.layers for n in ("qkv", "o", "gu", "down"))
    with pytest.raises(AttributeError):
        model.quantized_gemm = "direct"  # read-only
