"""S > 1 attention straight on the FP8 KV cache (csrc/kernels/attn_prefill.hip, the Q8 instantiations of the flash prefill
kernel): the direct launch writes the bits ``attn_prefill`` with the same impl writes on the dequantised rows, reads no
row a query cannot see as anything but finite filler, takes no scratch, and is routed by ``attn_prefill_q8_plan``."""
from __future__ import annotations

import pytest
import torch

import kv8_inputs as k8
from jax_llama_amd import ops
from jax_llama_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
DH = 128


@pytest.fixture(autouse=True)
def _restore():
    e = ops.ext()
    e.attn_set_q8_prefill(-1)  # (without the direct launch: every test fails here)
    yield
    e.attn_set_q8_prefill(-1)
    e.attn_prefill_set_impl(2)


def _inputs(b, hkv, rep, s, slot0, t, seed, masked=False):
    """q on the device, (K, V) ``Fp8KV`` on the host with per-row magnitudes 2^[-4, 4], kv_start, key mask or None."""
    g = torch.Generator().manual_seed(seed)
    mag = lambda: 2.0 ** torch.randint(-4, 5, (b, hkv, t, 1), generator=g).float()  # noqa: E731
    kq = k8.quantize_kv((torch.randn(b, hkv, t, DH, generator=g) * 0.25 * mag()).to(BF16))
    vq = k8.quantize_kv((torch.randn(b, hkv, t, DH, generator=g) * mag()).to(BF16))
    q = (torch.randn(b, s, hkv * rep, DH, generator=g) * 0.5).to(BF16).to(DEV)
    kv_start = torch.tensor([0] + [slot0 + s // 3] * (b - 1), dtype=torch.int32)
    mask = (torch.rand(b, t, generator=g) > 0.2).to(torch.uint8) if masked else None
    return q, kq, vq, kv_start, mask


def _dev(x):
    return None if x is None else x.to(DEV)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("rep", [1, 4, 8])
# (192, 0): kv_start 64 makes two key tiles, and at rep 1 / 4 the waves of queries 0 .. 63 are idle from the first one
@pytest.mark.parametrize("s,slot0", [(7, 0), (70, 10), (200, 57), (192, 0)])
@pytest.mark.parametrize("impl", [8, 7, 9, 13])
def test_direct_is_the_same_impl_on_the_dequantised_rows(impl, s, slot0, rep, masked):
    b, hkv = 2, 2
    q, kq, vq, kv_start, mask = _inputs(b, hkv, rep, s, slot0, slot0 + s + 5, 1000 * s + 10 * rep + masked, masked)
    e = ops.ext()
    e.attn_prefill_set_impl(impl)
    e.attn_set_q8_prefill(1)
    got = ops.attention(q, k8.to_device(kq, DEV), k8.to_device(vq, DEV), slot0, kv_start.to(DEV), _dev(mask))
    want = ops.attention(q, kq.dequant().to(DEV), vq.dequant().to(DEV), slot0, kv_start.to(DEV), _dev(mask))
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    exp = ref.attention(q.cpu(), kq, vq, slot0, kv_start, mask).reshape(b * s, -1)
    # (the measure and tolerance of test_kv8_gpu.py's dequant-path test: max error against 2e-2 + 2e-2 x the largest value)
    err, top = (got.cpu().float() - exp.float()).abs().max().item(), exp.float().abs().max().item()
    assert err <= 2e-2 + 2e-2 * top, f"max err {err:.3e} (ref max {top:.3e})"


@pytest.mark.parametrize("b,hkv,rep", [(1, 1, 4), (4, 8, 8)])  # impl 2 resolves to 7, to 13
def test_default_dispatch_bits(b, hkv, rep):
    s = 520
    q, kq, vq, kv_start, _ = _inputs(b, hkv, rep, s, 0, s + 5, b)
    ops.ext().attn_set_q8_prefill(1)
    got = ops.attention(q, k8.to_device(kq, DEV), k8.to_device(vq, DEV), 0, kv_start.to(DEV))
    want = ops.attention(q, kq.dequant().to(DEV), vq.dequant().to(DEV), 0, kv_start.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def _raises(*_a, **_k):
    raise AssertionError("kv8_dequant called")


@pytest.mark.parametrize("s,slot0,rep", [(64, 10, 4), (320, 57, 8), (70, 10, 4), (300, 57, 8)])
def test_unseen_rows_and_no_scratch(s, slot0, rep, monkeypatch):
    """S a multiple of 32 (every wave holds 32 real queries): the bits of the same call on a cache cut to slot0 + S
    rows. At S = 70 / 300 the comparison with a cut cache is not defined bit for bit, for either cache format: the v2
    kernel's padding lanes past S (clamped copies of the last query, never stored) do see the rows past slot0 + S, and
    their tile maximum can take the wave-uniform lazy-rescale branch, which moves the real lanes' running maximum by a
    rounding (measured: max difference 0.031 in 4 / 23 rows, identical on the direct and the dequantised route, 0 with
    zero filler). There the check is the contract itself: the bits of the dequantised route on the same full cache."""
    b, hkv, n = 2, 2, slot0 + s
    q, kq, vq, kv_start, _ = _inputs(b, hkv, rep, s, slot0, 4 * n, s)
    for kv in (kq, vq):  # every row no query sees: the largest finite code at a large scale
        kv.q[:, :, n:] = 0x7E
        kv.scale[:, :, n:] = 2.0 ** 20
    cut = lambda kv: ref.Fp8KV(kv.q[:, :, :n].contiguous().to(DEV), kv.scale[:, :, :n].contiguous().to(DEV))  # noqa: E731
    slot = torch.tensor([slot0], dtype=torch.int32, device=DEV)
    e = ops.ext()
    e.attn_set_q8_prefill(1)
    if s % 32 == 0:
        want = ops.attention(q, cut(kq), cut(vq), slot, kv_start.to(DEV))
    else:
        e.attn_set_q8_prefill(0)
        want = ops.attention(q, k8.to_device(kq, DEV), k8.to_device(vq, DEV), slot, kv_start.to(DEV)).clone()
        e.attn_set_q8_prefill(1)
    monkeypatch.setattr(ops, "kv8_dequant", _raises)
    got = ops.attention(q, k8.to_device(kq, DEV), k8.to_device(vq, DEV), slot, kv_start.to(DEV))
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all() and torch.equal(got, want)
    e.attn_set_q8_prefill(0)  # the switch is wired: the dequant route is taken
    with pytest.raises(AssertionError, match="kv8_dequant called"):
        ops.attention(q, k8.to_device(kq, DEV), k8.to_device(vq, DEV), slot, kv_start.to(DEV))


@pytest.mark.parametrize("b,hkv,rep,s,slot0,t", [(2, 2, 4, 7, 0, 64), (1, 8, 4, 16, 4096, 8192),
                                                  (1, 2, 4, 300, 0, 320), (1, 1, 4, 300, 32468, 32768)])
def test_route_follows_the_plan(b, hkv, rep, s, slot0, t, monkeypatch):
    q, _kq, _vq, kv_start, _ = _inputs(b, hkv, rep, s, 0, 8, 0)
    kz = ops.Fp8KV.zeros(b, hkv, t, DEV)
    calls, real = [], ops.kv8_dequant
    monkeypatch.setattr(ops, "kv8_dequant", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    rc, _why, direct = ops.ext().attn_prefill_q8_plan_check(b, hkv * rep, hkv, s, slot0 + s)
    ops.attention(q, kz, kz, slot0, torch.zeros(b, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert rc == 0 and len(calls) == (0 if direct else 1)
