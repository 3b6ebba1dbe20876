"""The FP8 (e4m3) KV cache on the CPU path: the exact-answer builders of tests/kv8_inputs.py validated against
``ops/reference.py`` alone, the row quantiser, the equivalence that defines the format (an ``Fp8KV`` cache is the bf16
cache holding the dequantised rows), and the ``KVCache`` / model plumbing."""
from __future__ import annotations

import pytest
import torch

import exact_inputs as xi
import kv8_inputs as k8
from jax_llama_amd import ops
from jax_llama_amd.models import LLaMAForCausalLM
from jax_llama_amd.models.kv_cache import KVCache
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime import engine as eng_mod
from jax_llama_amd.runtime.engine import GenerationConfig
from helpers import build, gpu_config, left_padded_batch, tiny_config

BF16 = torch.bfloat16
DH = xi.DH


def _kvs(slot):
    return torch.tensor([0, 37, slot + 1], dtype=torch.int32)


# ---------------------------------------------------------------------------------- builders against the reference
@pytest.mark.parametrize("t,slot,masked", [(40, 17, False), (300, 299, True), (1030, 700, False)])
def test_census_on_fp8kv_is_the_reference(t, slot, masked):
    b, hkv, rep = 3, 2, 4
    kv_start = _kvs(slot)
    mask = xi.edge_mask(b, t, slot, seed=t + slot) if masked else None
    count, n = xi.census_counts(b, hkv, t, slot, 1, kv_start, mask)
    kq, vq = k8.census_kv8(b, hkv, t, seed=t)
    q = torch.zeros(b, 1, hkv * rep, DH, dtype=BF16)
    out = ref.attention(q, kq, vq, slot, kv_start, mask).reshape(b, -1)
    assert xi.census_mismatch(out, count, n, rep) is None
    c2, n2 = xi.census_counts(b, hkv, t, slot - 1, 1, kv_start, mask)
    assert xi.census_mismatch(out, c2, n2, rep) is not None  # (the check has teeth)
    # ops.attention takes the handle on the CPU too
    assert torch.equal(ops.attention(q, kq, vq, slot, kv_start, mask), out)


@pytest.mark.parametrize("variant", ["pm1", "vgrid", "kpow2"])
@pytest.mark.parametrize("t,slot0,s,masked", [(40, 17, 1, False), (300, 299, 1, True), (1030, 700, 1, False),
                                              (135, 0, 130, True)])
def test_needles_on_fp8kv_exactly_one_hot(variant, t, slot0, s, masked):
    b, hkv, rep = (3, 2, 4) if s == 1 else (2, 2, 2)
    h = hkv * rep
    kv_start = _kvs(slot0) if s == 1 else torch.tensor([0, slot0 + s // 3], dtype=torch.int32)
    mask = xi.edge_mask(b, t, slot0 + s - 1, seed=t) if masked else None
    q, kq, vq, jstar, want = k8.needle_kv8(variant, b, hkv, rep, t, slot0, s, kv_start, mask, seed=t + s)
    out, p = ref.attention(q, kq, vq, slot0, kv_start, mask, return_weights=True)
    onehot = torch.nn.functional.one_hot(jstar.clamp_min(0), slot0 + s).float() * (jstar >= 0)[..., None]
    assert torch.equal(p, onehot.permute(0, 2, 1, 3))
    assert torch.equal(out.reshape(b * s, h * DH), want)
    if variant == "kpow2":  # the K scales differ per key, and all three magnitudes occur
        assert len(kq.scale.unique()) == 3
    if variant == "vgrid":  # V scales over many octaves
        assert len(vq.scale.unique()) > 8


def test_kpow2_needle_has_three_key_magnitudes():
    """The "kpow2" builder's own claim: the stored codes are +-256 for every key and the magnitudes 1 / 2 / 4 apart live
    in the K scales alone."""
    kv_start = _kvs(17)
    q, kq, vq, jstar, want = k8.needle_kv8("kpow2", 3, 2, 4, 40, 17, 1, kv_start, None, seed=3)
    mags = kq.dequant().float().abs().amax(-1)
    assert set(mags.unique().tolist()) == {0.25, 0.5, 1.0}
    assert torch.equal(kq.scale, mags * 2.0 ** -8) and set(kq.q.unique().tolist()) == {0x78, 0xF8}


# ---------------------------------------------------------------------------------- the quantiser
def test_grid_values_round_trip_exactly():
    g = torch.Generator().manual_seed(1)
    for lo, hi in ((-8, 8), (-60, -40), (40, 60)):
        rows = k8.fp8_grid_rows((64,), g, lo, hi)
        q, scale = ref.quantize_fp8_rows(rows)
        assert torch.equal(ref.dequantize_fp8_rows(q, scale), rows)
        m, x = torch.frexp(scale)
        assert bool((m == 0.5).all())  # powers of two


def test_zero_row_has_scale_one():
    kv = ref.Fp8KV.zeros(1, 1, 4)
    rows = torch.zeros(1, 1, 2, DH, dtype=BF16)
    rows[0, 0, 1, 5] = 3.0
    kv.store(rows, 1)
    assert kv.scale[0, 0].tolist() == [0.0, 1.0, 2.0 ** -7, 0.0]  # unwritten 0; zero row 1; amax 3 = 0.75 * 2^2
    assert int(kv.q[0, 0, 1].max()) == 0 and int(kv.q[0, 0, 0].max()) == 0
    assert torch.equal(kv.dequant()[0, 0, 1:3], rows[0, 0])
    assert float(kv.dequant()[0, 0, 0].abs().max()) == 0 and float(kv.dequant()[0, 0, 3].abs().max()) == 0


@pytest.mark.parametrize("e", [-20, 0, 7])
def test_tie_row_rounds_to_even(e):
    row, codes, scale = k8.tie_row(e)
    q, s = ref.quantize_fp8_rows(row[None])
    assert float(s[0]) == scale
    assert torch.equal(q.view(torch.uint8)[0], codes)
    # the ties are ties: each midpoint is as far from the code below as from the code above
    val = codes.view(k8.FP8).double() * scale
    assert bool((codes[1:127] % 2 == 0).all())
    d = (row.double() - val).abs()[1:127]
    grid = torch.arange(0, 0x7F, dtype=torch.uint8).view(k8.FP8).double() * scale
    assert torch.equal(d, (grid[1:] - grid[:-1]) / 2)


# ---------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("b,s,slot0,h,hkv", [(2, 1, 5, 4, 2), (3, 7, 0, 8, 2), (2, 9, 3, 2, 2)])
def test_fp8_cache_is_the_bf16_cache_of_dequantised_rows(b, s, slot0, h, hkv):
    t = slot0 + s + 3
    g = torch.Generator().manual_seed(b + s)
    m = b * s
    qkv = (torch.randn(m, (h + 2 * hkv) * DH, generator=g) * 3).to(BF16)
    table = ref.rope_table(DH, 64, 10000.0)
    pos = torch.randint(0, 64, (m,), generator=g, dtype=torch.int32)
    kv_start = torch.zeros(b, dtype=torch.int32)
    # the bf16 caches, then their rows replaced by q * scale
    kc, vc = torch.zeros(b, hkv, t, DH, dtype=BF16), torch.zeros(b, hkv, t, DH, dtype=BF16)
    q_ref = ref.rope_kv_write(qkv, table, pos, kc, vc, slot0, s, h, hkv, DH)
    kd, vd = k8.quantize_kv(kc).dequant(), k8.quantize_kv(vc).dequant()
    kq, vq = ref.Fp8KV.zeros(b, hkv, t), ref.Fp8KV.zeros(b, hkv, t)
    q8 = ops.rope_kv_write(qkv, table, pos, kq, vq, slot0, s, h, hkv, DH)
    assert torch.equal(q8, q_ref)  # q is never quantised
    assert torch.equal(kq.dequant(), kd) and torch.equal(vq.dequant(), vd)
    assert int(kq.scale[:, :, :slot0].abs().max() if slot0 else 0) == 0 and float(kq.scale[:, :, slot0 + s:].max()) == 0
    q4 = q8.reshape(b, s, h, DH)
    assert torch.equal(ref.attention(q4, kq, vq, slot0, kv_start), ref.attention(q4, kd, vd, slot0, kv_start))
    # the relative error of a dequantised row is fp8's: 2^-4 of the row's amax at most
    assert float((kd.float() - kc.float()).abs().max()) <= 2.0 ** -4 * float(kc.float().abs().max())


def test_linear_qkv_rope_with_fp8kv_quantises_the_bf16_projection():
    from jax_llama_amd.models.weights import PackedLinear
    b, s, h, hkv, k, slot0 = 2, 3, 4, 2, 64, 1
    g = torch.Generator().manual_seed(0)
    w = PackedLinear.from_dense((torch.randn((h + 2 * hkv) * DH, k, generator=g) * 0.1).to(BF16), "cpu")
    x = torch.randn(b * s, k, generator=g).to(BF16)
    table = ref.rope_table(DH, 32, 10000.0)
    pos = torch.arange(s, dtype=torch.int32).repeat(b)
    kq, vq = ref.Fp8KV.zeros(b, hkv, 8), ref.Fp8KV.zeros(b, hkv, 8)
    q = ops.linear_qkv_rope(x, w, 1e-5, table, pos, kq, vq, slot0, s, h, hkv, DH)
    k2, v2 = ref.Fp8KV.zeros(b, hkv, 8), ref.Fp8KV.zeros(b, hkv, 8)
    q2 = ref.rope_kv_write(ref.linear(x, w.dense(), 1e-5), table, pos, k2, v2, slot0, s, h, hkv, DH)
    assert torch.equal(q, q2) and torch.equal(kq.q, k2.q) and torch.equal(vq.scale, v2.scale)
    assert int(kq.q[:, :, slot0:slot0 + s].max()) > 0


# ---------------------------------------------------------------------------------- KVCache and the model
def test_kvcache_fp8_layout_and_bytes():
    nl, b, hkv, t = 3, 4, 2, 10
    c = KVCache(nl, b, hkv, t, DH, "cpu", kv_format="fp8_e4m3")
    assert c.nbytes() == nl * b * hkv * t * 2 * 132
    assert KVCache(nl, b, hkv, t, DH, "cpu").nbytes() == nl * b * hkv * t * 2 * 256
    kq, vq = c.layer(1)
    assert isinstance(kq, ops.Fp8KV) and tuple(kq.shape) == (b, hkv, t, DH) and kq.device.type == "cpu"
    rows = torch.randn(b, hkv, 2, DH).to(BF16)
    kq.store(rows, 4)  # a view of the cache: the write lands in it
    assert int(c.k[1, :, :, 4:6].max()) > 0 and float(c.k_scale[1, :, :, 4:6].min()) > 0
    r = c.rows(1, 3)
    rk, rv = r.layer(1)
    assert tuple(rk.shape) == (2, hkv, t, DH) and torch.equal(rk.q, kq.q[1:3]) and rk.q.is_contiguous()
    assert r.kv_format == "fp8_e4m3" and r.index_t is c.index_t
    d = c.as_dict()
    assert d["1"]["cached_key"].dtype == BF16 and tuple(d["1"]["cached_key"].shape) == (b, t, hkv, DH)
    assert torch.equal(d["1"]["cached_key"].permute(0, 2, 1, 3), kq.dequant())
    assert float(d["0"]["cached_value"].abs().max()) == 0
    c.advance(3)
    c.zero_()
    assert int(c.k.max()) == 0 and float(c.k_scale.abs().max()) == 0 and c.index == 3
    bf = KVCache(1, 1, 1, 4, DH, "cpu")
    bf.k.fill_(1.0)
    bf.zero_()
    assert float(bf.k.abs().max()) == 0 and bf.kv_format == "bf16"
    with pytest.raises(ValueError):
        KVCache(1, 1, 1, 4, DH, "cpu", kv_format="int4")
    with pytest.raises(ValueError):
        KVCache(1, 1, 1, 4, 64, "cpu", kv_format="fp8_e4m3")


def test_set_kv_cache_format_errors_and_state():
    m = LLaMAForCausalLM(gpu_config(), device="cpu", seed=0)
    assert m.kv_cache_format == "bf16"
    assert m.init_cache(1, 8).kv_format == "bf16"
    assert m.init_cache(1, 8, kv_format="fp8_e4m3").kv_format == "fp8_e4m3"
    with pytest.raises(ValueError):
        m.set_kv_cache_format("fp4")
    with pytest.raises(ValueError):
        m.init_cache(1, 8, kv_format="fp4")
    assert m.set_kv_cache_format("fp8_e4m3") is m and m.kv_cache_format == "fp8_e4m3"
    assert m.init_cache(1, 8).kv_format == "fp8_e4m3" and m.init_cache(1, 8, kv_format="bf16").kv_format == "bf16"
    m.set_kv_cache_format("bf16")
    assert m.kv_cache_format == "bf16"
    with pytest.raises(ValueError):  # head_dim 8
        LLaMAForCausalLM(tiny_config(), device="cpu", seed=0).set_kv_cache_format("fp8_e4m3")
    with pytest.raises(ValueError):  # 16 query heads per kv head
        LLaMAForCausalLM(gpu_config(hidden_size=2048, num_attention_heads=16, num_key_value_heads=1,
                                    num_hidden_layers=1), device="cpu", seed=0).set_kv_cache_format("fp8_e4m3")
    with pytest.raises(ValueError):  # 3 query heads per kv head
        LLaMAForCausalLM(gpu_config(hidden_size=384, num_attention_heads=3, num_key_value_heads=1,
                                    num_hidden_layers=1), device="cpu", seed=0).set_kv_cache_format("fp8_e4m3")


def test_model_prefill_decode_sees_the_teacher_forced_keys():
    """Every attention reads the dequantised rows, a prefill reading its own keys included: prefill + decode steps give
    the logits of one teacher-forced forward over the same tokens, with a left-padded batch;
    and the fp8 cache moves the logits off the bf16 cache's by a small, non-zero amount."""
    cfg = gpu_config(num_attention_heads=4, num_key_value_heads=2, hidden_size=512)
    model, *_ = build(cfg, seed=1)
    toks, mask = left_padded_batch([4, 9], 9, cfg.vocab_size, pad=2, seed=2)
    full_mask = torch.cat([mask, torch.ones(2, 3, dtype=mask.dtype)], 1)
    extra = torch.randint(3, cfg.vocab_size, (2, 3), dtype=torch.int32, generator=torch.Generator().manual_seed(3))
    seq = torch.cat([toks, extra], 1)
    pos = full_mask.cumsum(-1) - 1
    bf16_logits = model(seq, attention_mask=full_mask, position_ids=pos).logits
    model.set_kv_cache_format("fp8_e4m3")
    forced = model(seq, attention_mask=full_mask, position_ids=pos).logits
    cache = model.init_cache(2, 12)
    assert cache.kv_format == "fp8_e4m3"
    out = model(toks, attention_mask=full_mask, position_ids=pos[:, :9], past_key_values=cache)
    steps = [out.logits]
    for i in range(3):
        out = model(seq[:, 9 + i:10 + i], attention_mask=full_mask, position_ids=pos[:, 9 + i:10 + i],
                    past_key_values=cache)
        steps.append(out.logits)
    got = torch.cat(steps, 1)
    m = full_mask.bool()
    # the same computation at another M per GEMM, so the CPU BLAS may sum in another order: fp32 noise (2e-7 of the
    # logit scale measured, for the bf16 cache as well), and where that noise flips the bf16 rounding of an activation,
    # one bf16 ulp (2^-7) of that value, diluted over a K >= 256 sum: a few 1e-4 of the logit scale per flip. A prefill
    # that read its own keys unquantised would move the logits by the whole fp8-vs-bf16 shift (7e-3, below).
    assert float((got[m] - forced[m]).abs().max() / forced[m].abs().max()) < 2e-3
    shift = float((forced[m] - bf16_logits[m]).abs().max() / bf16_logits[m].abs().max())
    assert 0 < shift < 0.1, shift
    # score() builds its transient caches in the model's format
    sc8 = model.score(seq, attention_mask=full_mask)
    model.set_kv_cache_format("bf16")
    sc16 = model.score(seq, attention_mask=full_mask)
    d = (sc8.token_logprobs - sc16.token_logprobs).abs().max()
    assert 0 < float(d) < 0.5


def test_engine_cache_key_and_budget_follow_the_format(monkeypatch):
    cfg = gpu_config()
    model = LLaMAForCausalLM(cfg, device="cpu", seed=0)
    eng_mod._ENGINES.clear()
    try:
        e16 = eng_mod.get_engine(model, 2, 16)
        model.set_kv_cache_format("fp8_e4m3")
        e8 = eng_mod.get_engine(model, 2, 16)
        assert e8 is not e16 and e8.cache.kv_format == "fp8_e4m3" and e16.cache.kv_format == "bf16"
        assert eng_mod.get_engine(model, 2, 16) is e8
        assert e8.cache.nbytes() * 256 == e16.cache.nbytes() * 132
        # the budget counts the format's bytes: room for the fp8 engine's cache, not for a bf16 one of the same shape
        eng_mod._ENGINES.clear()
        need8 = cfg.num_hidden_layers * 2 * 2 * model.n_kv_heads * 32 * 132
        monkeypatch.setenv("JLA_ENGINE_CACHE_GB", str((e8.cache.nbytes() + need8) / (1 << 30)))
        eng_mod._ENGINES[("held",)] = e8
        eng_mod.get_engine(model, 2, 32)
        assert ("held",) in eng_mod._ENGINES  # fits: nothing evicted
        toks = torch.randint(3, cfg.vocab_size, (2, 5), dtype=torch.int32)
        gc = GenerationConfig(max_length=12, do_sample=False, pad_token_id=0, eos_token_id=-1)
        seq = model.generate(toks, generation_config=gc).sequences
        assert seq.shape == (2, 12) and torch.equal(seq[:, :5], toks)
    finally:
        eng_mod._ENGINES.clear()
