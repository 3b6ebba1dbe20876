"""The few-query decode attention (csrc/kernels/attn_verify.hip, ``ops.attention(few_query=True)``) against the fp32
reference, and the shapes its plan declines against the launch they get without the flag."""
from __future__ import annotations

import pytest
import torch

from jax_llama_amd import ops
from jax_llama_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
B, HKV, DH = 3, 2, 128


def _close(a, b):  # test_attention_decode_mfma_v6's tolerance: the same math against the same reference
    a, b = a.float().cpu(), b.float().cpu()
    err, scale = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= 2e-2 + 2e-2 * scale, f"max err {err:.3e} (ref max {scale:.3e})"


def _inputs(rep, s, t, slot0, seed=0):
    g = torch.Generator().manual_seed(seed)
    kc = (torch.randn(B, HKV, t, DH, generator=g) * 0.5).to(BF16)
    vc = torch.randn(B, HKV, t, DH, generator=g).to(BF16)
    q = torch.randn(B, s, HKV * rep, DH, generator=g).to(BF16)
    # padding that starts inside a 32-key step; row 2: query positions 0 and 1 have no valid key (zeros)
    kv_start = torch.tensor([0, 37, slot0 + 2], dtype=torch.int32)
    return q, kc, vc, kv_start


def _run(q, kc, vc, slot0, kv_start, **kw):
    sl = torch.tensor([slot0], dtype=torch.int32, device=DEV)
    out = ops.attention(q.to(DEV), kc.to(DEV), vc.to(DEV), sl, kv_start.to(DEV), **kw)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("rep,s", [(1, 2), (1, 16), (4, 4), (4, 8), (8, 2), (8, 4), (2, 5)])
@pytest.mark.parametrize("t,slot0", [(40, 17), (384, 200), (1030, 1020)])
def test_attn_verify(rep, s, t, slot0):
    """One column tile, two full tiles and a ragged second tile; the causal edge inside a 32-key step and at the
    cache's end. (S = 16 at slot 1020 of a 1030-slot cache would put queries past the cache, which the reference does
    not define: there the first query sits at T - S, so the last one is the cache's last slot.)"""
    slot0 = min(slot0, t - s)
    q, kc, vc, kv_start = _inputs(rep, s, t, slot0)
    assert ops.ext().attn_verify_plan_check(B, s, HKV * rep, HKV, DH, t)[0] == 0
    want = ref.attention(q, kc, vc, slot0, kv_start).reshape(B * s, -1)
    got = _run(q, kc, vc, slot0, kv_start, few_query=True)
    _close(got, want)
    assert torch.equal(got[2 * s:2 * s + 2], torch.zeros_like(got[:2]))  # row 2, positions 0 and 1: no valid key
    assert torch.equal(got, _run(q, kc, vc, slot0, kv_start, few_query=True))


@pytest.mark.parametrize("nsplit", [1, 2, 5])
@pytest.mark.parametrize("rep,s", [(4, 8), (2, 5)])
def test_attn_verify_forced_splits(rep, s, nsplit):
    e = ops.ext()
    t, slot0 = 1030, 1020
    q, kc, vc, kv_start = _inputs(rep, s, t, slot0, seed=1)
    want = ref.attention(q, kc, vc, slot0, kv_start).reshape(B * s, -1)
    try:
        e.attn_set_verify_splits(nsplit)
        assert e.attn_verify_plan_check(B, s, HKV * rep, HKV, DH, t)[3] == nsplit
        got = _run(q, kc, vc, slot0, kv_start, few_query=True)
        again = _run(q, kc, vc, slot0, kv_start, few_query=True)
    finally:
        e.attn_set_verify_splits(0)
    _close(got, want)
    assert torch.equal(got, again)


@pytest.mark.parametrize("case", ["fp8", "mask", "cols40"])
def test_attn_verify_declined_runs_the_old_kernel(case):
    rep, s, t, slot0 = (8, 5, 384, 200) if case == "cols40" else (4, 4, 384, 200)
    q, kc, vc, kv_start = _inputs(rep, s, t, slot0, seed=2)
    kw = {}
    if case == "mask":
        mask = (torch.rand(B, t) > 0.3).to(torch.uint8)
        kw["key_mask"] = mask.to(DEV)
    if case == "fp8":
        kc, vc = ops.Fp8KV.zeros(B, HKV, t, DEV), ops.Fp8KV.zeros(B, HKV, t, DEV)
        for c in (kc, vc):
            c.q.copy_(torch.randint(0, 0x78, c.q.shape, dtype=torch.uint8))
            c.scale.fill_(0.125)
        sl = torch.tensor([slot0], dtype=torch.int32, device=DEV)
        a = ops.attention(q.to(DEV), kc, vc, sl, kv_start.to(DEV), few_query=True).cpu()
        b = ops.attention(q.to(DEV), kc, vc, sl, kv_start.to(DEV)).cpu()
    else:
        a = _run(q, kc, vc, slot0, kv_start, few_query=True, **kw)
        b = _run(q, kc, vc, slot0, kv_start, **kw)
    assert ops.ext().attn_verify_plan_check(B, s, HKV * rep, HKV, DH, t, case == "fp8", case == "mask")[0] != 0
    assert torch.equal(a, b)
