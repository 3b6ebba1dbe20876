"""The FP8 (e4m3) KV cache on the MI355X (csrc/kernels/kv8.hip): the quantising RoPE + cache write bit for bit against
``ref.quantize_fp8_rows``, the dequantiser, the decode attention on the fp8 bytes in both wave forms on the exact-answer
inputs of tests/kv8_inputs.py and on random ones, the S > 1 path (the bf16 prefill kernel on the dequantised rows), the
routing, and a model with the FP8 cache against the CPU path of the same definition."""
from __future__ import annotations

import contextlib
import functools
import glob
import json
import os
import subprocess
import sys

import pytest
import torch

import exact_inputs as xi
import kv8_inputs as k8
from jax_llama_amd import ops
from jax_llama_amd.models import LLaMAForCausalLM
from jax_llama_amd.models.weights import PackedLinear
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime.benchmark import graph_kernels
from jax_llama_amd.runtime.engine import DecodeEngine, GenerationConfig
from helpers import build, gpu_config, left_padded_batch, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
DH = xi.DH
SENTINEL_BYTE, SENTINEL_SCALE = 0x5A, -3.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(a, b, rtol, atol):  # (tests/test_kernels_gpu.py's measure)
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item()
    assert err <= atol + rtol * scale, f"max err {err:.3e} (ref max {scale:.3e})"


def _sentinel_kv(b, hkv, t):
    return ops.Fp8KV(torch.full((b, hkv, t, DH), SENTINEL_BYTE, dtype=torch.uint8, device=DEV),
                     torch.full((b, hkv, t), SENTINEL_SCALE, dtype=torch.float32, device=DEV))


def _assert_outside_untouched(kv, slot0, s):
    q, sc = kv.q.cpu(), kv.scale.cpu()
    for part_q, part_s in ((q[:, :, :slot0], sc[:, :, :slot0]), (q[:, :, slot0 + s:], sc[:, :, slot0 + s:])):
        assert bool((part_q == SENTINEL_BYTE).all()) and bool((part_s == SENTINEL_SCALE).all())


# ---------------------------------------------------------------------------------- the write kernel
@pytest.mark.parametrize("h,hkv", [(4, 1), (8, 2)])
@pytest.mark.parametrize("m,s", [(1, 1), (16, 1), (6, 3), (130, 65)])
def test_write_kernel(m, s, h, hkv):
    b, slot0 = m // s, 2
    t = slot0 + s + 3
    g = torch.Generator().manual_seed(m + h)
    n = (h + 2 * hkv) * DH
    qkv = (torch.randn(m, n, generator=g) * 2.0 ** torch.randint(-10, 8, (m, 1), generator=g).float()).to(BF16)
    voff = (h + hkv) * DH
    # V rows with known answers: the tie rows (subnormal codes included) at three exponents, and a zero row
    ties = {}
    for i, e in enumerate((-20, 0, 7)):
        row, codes, scale = k8.tie_row(e)
        mi, hi = (i * 5) % m, i % hkv
        qkv[mi, voff + hi * DH: voff + (hi + 1) * DH] = row
        ties[(mi, hi)] = (codes, scale)
    zrow = (m - 1, hkv - 1)
    if zrow not in ties:
        qkv[zrow[0], voff + zrow[1] * DH: voff + (zrow[1] + 1) * DH] = 0
    table = ref.rope_table(DH, 256, 500000.0)
    pos = torch.randint(0, 256, (m,), generator=g, dtype=torch.int32)
    kr, vr = ref.Fp8KV.zeros(b, hkv, t), ref.Fp8KV.zeros(b, hkv, t)
    q_ref = ref.rope_kv_write(qkv, table, pos, kr, vr, slot0, s, h, hkv, DH)
    kg, vg = _sentinel_kv(b, hkv, t), _sentinel_kv(b, hkv, t)
    slot = torch.tensor([slot0], dtype=torch.int32, device=DEV)
    q_gpu = ops.rope_kv_write(qkv.to(DEV), table.to(DEV), pos.to(DEV), kg, vg, slot, s, h, hkv, DH)
    torch.cuda.synchronize()
    w = slice(slot0, slot0 + s)
    # V: no rotation, so the bytes and the scales are the reference quantiser's, bit for bit
    assert torch.equal(vg.scale.cpu()[:, :, w], vr.scale[:, :, w])
    assert torch.equal(vg.q.cpu()[:, :, w], vr.q[:, :, w])
    for (mi, hi), (codes, scale) in ties.items():
        bi, si = mi // s, mi % s
        assert torch.equal(vg.q[bi, hi, slot0 + si].cpu(), codes) and float(vg.scale[bi, hi, slot0 + si]) == scale
    if zrow not in ties:
        bi, si = zrow[0] // s, zrow[0] % s
        assert float(vg.scale[bi, zrow[1], slot0 + si]) == 1.0 and int(vg.q[bi, zrow[1], slot0 + si].max()) == 0
    # K: the rotation's fp32 arithmetic may round a bf16 value the other way (test_kernels_gpu.py's measures)
    _close(q_gpu, q_ref, 1e-2, 1e-2)
    _close(k8.to_device(kg, "cpu").dequant()[:, :, w], kr.dequant()[:, :, w], 2e-2, 2e-2)
    _assert_outside_untouched(kg, slot0, s)
    _assert_outside_untouched(vg, slot0, s)

    # integers and quarter turns: the rotation is exact, so K is bit-equal too
    npos = 64
    ys = xi.int_matrix(m, n, 100, m + 1).to(BF16)
    pos2 = torch.randint(0, npos, (m,), generator=g, dtype=torch.int32)
    qt = xi.quarter_table(npos)
    kr2, vr2 = ref.Fp8KV.zeros(b, hkv, t), ref.Fp8KV.zeros(b, hkv, t)
    q_ref2 = ref.rope_kv_write(ys, qt, pos2, kr2, vr2, slot0, s, h, hkv, DH)
    kg2, vg2 = _sentinel_kv(b, hkv, t), _sentinel_kv(b, hkv, t)
    q_gpu2 = ops.rope_kv_write(ys.to(DEV), qt.to(DEV), pos2.to(DEV), kg2, vg2, slot, s, h, hkv, DH)
    torch.cuda.synchronize()
    assert torch.equal(q_gpu2.cpu(), q_ref2)
    for got, want in ((kg2, kr2), (vg2, vr2)):
        assert torch.equal(got.q.cpu()[:, :, w], want.q[:, :, w])
        assert torch.equal(got.scale.cpu()[:, :, w], want.scale[:, :, w])
        _assert_outside_untouched(got, slot0, s)


def test_write_kernel_bounds_flag_is_wired():
    """The bounds-checked build's flag bits reach the new kernels through ops.bounds_error(): the release build reports
    0 (the debug build's own tests cover the bits); a slot past the cache writes nothing."""
    b, hkv, h, t = 2, 1, 2, 4
    qkv = torch.randn(b, (h + 2 * hkv) * DH).to(BF16).to(DEV)
    table = ref.rope_table(DH, 16, 10000.0).to(DEV)
    pos = torch.zeros(b, dtype=torch.int32, device=DEV)
    kg, vg = _sentinel_kv(b, hkv, t), _sentinel_kv(b, hkv, t)
    ops.rope_kv_write(qkv, table, pos, kg, vg, torch.tensor([t], dtype=torch.int32, device=DEV), 1, h, hkv, DH)
    torch.cuda.synchronize()
    _assert_outside_untouched(kg, 0, 0)
    _assert_outside_untouched(vg, 0, 0)
    if not ops.ext().DEBUG_BOUNDS:
        assert ops.bounds_error() == 0


BOUNDS_CHILD = r"""
import json, torch
from jax_llama_amd import ops
from jax_llama_amd.ops import reference as ref
e = ops.ext()
dev = "cuda"
res = {"debug": bool(e.DEBUG_BOUNDS)}
B, S, H, Hkv, Dh, T = 1, 2, 4, 2, 128, 8
qkv = torch.randn(B * S, (H + 2 * Hkv) * Dh, device=dev).to(torch.bfloat16)
rope = ref.rope_table(Dh, 64, 10000.0).to(dev)
pos = torch.arange(S, dtype=torch.int32, device=dev)
kc, vc = ops.Fp8KV.zeros(B, Hkv, T, dev), ops.Fp8KV.zeros(B, Hkv, T, dev)
ops.bounds_error(reset=True)
ops.rope_kv_write(qkv, rope, pos, kc, vc, 0, S, H, Hkv, Dh)
torch.cuda.synchronize()
res["clean"] = ops.bounds_error(reset=True)
ops.rope_kv_write(qkv, rope, pos, kc, vc, T - 1, S, H, Hkv, Dh)  # the second row lands at slot T: skipped, recorded
torch.cuda.synchronize()
res["kv"] = ops.bounds_error(reset=True)
res["slot_T_minus_1_written"] = bool(kc.scale[0, :, T - 1].min().item() > 0)
ops.rope_kv_write(qkv, rope, pos + 63, kc, vc, 2, S, H, Hkv, Dh)  # position 64 of a 64-row table: clamped, recorded
torch.cuda.synchronize()
res["rope"] = ops.bounds_error(reset=True)
q = torch.randn(B, 1, H, Dh, device=dev).to(torch.bfloat16)
kvs = torch.zeros(B, dtype=torch.int32, device=dev)
for waves in (8, 1):
    e.attn_set_q8_waves(waves)
    out = ops.attention(q, kc, vc, T, kvs)  # slot T: the keys past the cache are never read, and it is recorded
    torch.cuda.synchronize()
    res["attn%d" % waves] = ops.bounds_error(reset=True)
    res["finite%d" % waves] = bool(torch.isfinite(out).all())
e.attn_reset_knobs()
print("RESULT " + json.dumps(res))
"""


@pytest.mark.skipif(not glob.glob(os.path.join(ROOT, "jax_llama_amd", "_C_dbg*.so")),
                    reason="debug build absent (python build.py --debug-bounds)")
def test_debug_build_flags_are_wired_to_the_new_kernels():
    """The bounds-checked build (a child process, as tests/test_debug_bounds_gpu.py): the existing JLA_BOUNDS_* bits set
    by the quantising write (KV slot, RoPE position) and by the fp8 decode attention (slot past the cache). Every bad
    index here is one the kernels clamp or skip."""
    env = dict(os.environ, JLA_DEBUG_BOUNDS="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", BOUNDS_CHILD], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["debug"] and res["clean"] == 0
    assert res["kv"] == 1 << 1 and res["slot_T_minus_1_written"]
    assert res["rope"] == 1 << 4
    assert res["attn8"] == 1 << 3 and res["attn1"] == 1 << 3 and res["finite8"] and res["finite1"]


# ---------------------------------------------------------------------------------- the dequant kernel
@pytest.mark.parametrize("b,hkv,t,n", [(1, 1, 3, 3), (3, 2, 70, 33), (2, 8, 257, 257)])
def test_dequant_kernel_bit_equal(b, hkv, t, n):
    g = torch.Generator().manual_seed(t)
    x = (torch.randn(b, hkv, t, DH, generator=g) * 2.0 ** torch.randint(-30, 30, (b, hkv, t, 1), generator=g).float())
    x[0, 0, 1] = 0
    kc, vc = k8.quantize_kv(x.to(BF16)), k8.quantize_kv(x.flip(2).to(BF16))
    kc.scale[0, 0, 0] = 0  # an unwritten slot: bytes 0 and scale 0
    kc.q[0, 0, 0] = 0
    kd, vd = ops.kv8_dequant(k8.to_device(kc, DEV), k8.to_device(vc, DEV), n)
    torch.cuda.synchronize()
    assert tuple(kd.shape) == (b, hkv, n, DH) and kd.dtype == BF16
    assert torch.equal(kd.cpu().view(torch.int16), kc.dequant(n).view(torch.int16))
    assert torch.equal(vd.cpu().view(torch.int16), vc.dequant(n).view(torch.int16))


# ---------------------------------------------------------------------------------- decode attention
@contextlib.contextmanager
def _waves(waves, b, hkv, rep, t, masked):
    """Pin the waves per pair and assert that the plan says so."""
    e = ops.ext()
    try:
        e.attn_set_q8_waves(waves)
        rc, why, w, kpg, r = e.attn_decode_q8_plan_check(b, hkv * rep, hkv, DH, t, masked)
        assert rc == 0 and (w, r) == (waves, rep) and rep * kpg <= 16, (rc, why, w, kpg, r)
        yield
    finally:
        e.attn_reset_knobs()


def _kv_start(b, slot):
    ks = torch.randint(0, max(1, slot // 2), (b,), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
    ks[:3] = torch.tensor([0, 37, slot + 1], dtype=torch.int32)[:min(b, 3)]  # inside a chunk; a row with no valid key
    return ks


@functools.lru_cache(maxsize=None)
def _decode_case(b, hkv, rep, t, slot, masked):
    """Shared, read-only: every input of one decode shape with its expected output, device tensors for the kernel."""
    kv_start = _kv_start(b, slot)
    mask = xi.edge_mask(b, t, slot, seed=t + slot) if masked else None
    h = hkv * rep
    case = {"kvs": kv_start.to(DEV), "mask": None if mask is None else mask.to(DEV)}
    count, n = xi.census_counts(b, hkv, t, slot, 1, kv_start, mask)
    ck, cv = k8.census_kv8(b, hkv, t, seed=t)
    case["census"] = (count, n, k8.to_device(ck, DEV), k8.to_device(cv, DEV))
    base = xi.needle_inputs(b, hkv, rep, t, slot, 1, kv_start, mask, t + slot)
    for variant in ("pm1", "vgrid", "kpow2"):
        q, kq, vq, _, want = k8.needle_kv8(variant, b, hkv, rep, t, slot, 1, kv_start, mask, seed=t + slot, base=base)
        case[variant] = (q.to(DEV), k8.to_device(kq, DEV), k8.to_device(vq, DEV), want)
    g = torch.Generator().manual_seed(t + rep)
    mag = lambda: 2.0 ** torch.randint(-6, 7, (b, hkv, t, 1), generator=g).float()  # noqa: E731
    kq = k8.quantize_kv((torch.randn(b, hkv, t, DH, generator=g) * 0.25 * mag()).to(BF16))
    vq = k8.quantize_kv((torch.randn(b, hkv, t, DH, generator=g) * mag()).to(BF16))
    q = (torch.randn(b, 1, h, DH, generator=g) * 0.5).to(BF16)
    want = ref.attention(q, kq.dequant(), vq.dequant(), slot, kv_start, mask).reshape(b, h * DH)
    case["random"] = (q.to(DEV), k8.to_device(kq, DEV), k8.to_device(vq, DEV), want)
    return case


def _attend(q, kq, vq, slot, kvs, mask, max_kv=None):
    sl = torch.tensor([slot], dtype=torch.int32, device=DEV)
    out = ops.attention(q, kq, vq, sl, kvs, mask, max_kv=max_kv)
    torch.cuda.synchronize()
    return out


def _check_decode_case(case, b, hkv, rep, slot):
    kvs, mask = case["kvs"], case["mask"]
    count, n, ck, cv = case["census"]
    out = _attend(torch.zeros(b, 1, hkv * rep, DH, dtype=BF16, device=DEV), ck, cv, slot, kvs, mask)
    msg = xi.census_mismatch(out, count, n, rep)
    assert msg is None, msg
    for variant in ("pm1", "vgrid", "kpow2"):
        q, kq, vq, want = case[variant]
        out = _attend(q, kq, vq, slot, kvs, mask)
        assert torch.equal(out.cpu(), want), variant
    q, kq, vq, want = case["random"]
    out = _attend(q, kq, vq, slot, kvs, mask)
    assert bool(torch.isfinite(out).all())
    _close(out, want, 2e-2, 2e-2)
    assert float(out[2].abs().max()) == 0  # the row with no valid key


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("t,slot", [(40, 17), (300, 299), (1030, 700)])
@pytest.mark.parametrize("rep", [1, 2, 4, 8])
@pytest.mark.parametrize("waves", [8, 1])
def test_decode_attention(waves, rep, t, slot, masked):
    b, hkv = 3, 2
    case = _decode_case(b, hkv, rep, t, slot, masked)
    with _waves(waves, b, hkv, rep, t, masked):
        _check_decode_case(case, b, hkv, rep, slot)


@functools.lru_cache(maxsize=None)
def _ladder_case(b, hkv, rep, t, slot, masked):
    """Shared, read-only: the ladder of tests/exact_inputs.py on an fp8 cache (its keys are 0 / +-1 and its V rows unit
    vectors: the quantiser loses nothing), per profile (q, K) on the device and the fp64 softmax; V, kv_start, mask."""
    kv_start = _kv_start(b, slot)
    mask = xi.edge_mask(b, t, slot, seed=t + slot) if masked else None
    prof = {}
    for profile in xi.LADDER_PROFILES:
        q, kc, levels, gain = xi.ladder_inputs(b, hkv, rep, t, 1, profile, seed=t + slot)
        kq = k8.quantize_kv(kc)
        assert torch.equal(kq.dequant(), kc)
        prof[profile] = (q.to(DEV), k8.to_device(kq, DEV),
                         xi.ladder_expected(b, hkv, rep, t, slot, 1, kv_start, mask, levels, gain))
    vq = k8.quantize_kv(xi.census_v(b, hkv, t))
    return prof, k8.to_device(vq, DEV), kv_start.to(DEV), None if mask is None else mask.to(DEV)


def _check_ladder_case(case, rep, slot, tag):
    """Every element within u + 2^-12 of the fp64 softmax (fp32 P and fp32 FMAs; u is the bf16 rounding of the output),
    the row without a valid key exactly 0. Prints the worst relative error in units of u = 2^-8."""
    prof, vq, kvs, mask = case
    results = [(profile, _attend(q, kq, vq, slot, kvs, mask), want) for profile, (q, kq, want) in prof.items()]
    worst = {p: xi.ladder_worst_u(out, want) for p, out, want in results}
    print(f"ladder {tag}: worst relative error {max(worst.values()):.3f} u of the bound "
          f"{xi.LADDER_RTOL_FMA / xi.U_BF16:.4f} u", worst)
    for profile, out, want in results:
        msg = xi.ladder_mismatch(out, want, rep, xi.LADDER_RTOL_FMA)
        assert msg is None, f"{profile}: {msg}"
    assert float(results[0][2][2].abs().max()) == 0  # (row 2 has no valid key)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("t,slot", xi.LADDER_DECODE_TS)
@pytest.mark.parametrize("rep", [1, 2, 4, 8])
@pytest.mark.parametrize("waves", [8, 1])
def test_decode_attention_ladder(waves, rep, t, slot, masked):
    """Scores with a real range (up to 181 nats between two keys, gains of both signs within a kv group) on the fp8
    cache, both wave forms: the running maximum moves in every chunk and the wave merge weighs partials whose maxima
    are far apart. The census above has equal weights and the needles a single one."""
    b, hkv = 3, 2
    case = _ladder_case(b, hkv, rep, t, slot, masked)
    with _waves(waves, b, hkv, rep, t, masked):
        _check_ladder_case(case, rep, slot, f"fp8 decode waves {waves}")


def test_decode_attention_one_wave_1024_pairs():
    b, hkv, rep, t, slot = 128, 8, 4, 300, 299
    case = _decode_case(b, hkv, rep, t, slot, False)
    with _waves(1, b, hkv, rep, t, False):
        _check_decode_case(case, b, hkv, rep, slot)


@pytest.mark.parametrize("waves", [8, 1])
def test_decode_attention_long_context(waves):
    b, hkv, rep, t, slot = 3, 2, 4, 8192, 8000
    case = _decode_case(b, hkv, rep, t, slot, False)
    with _waves(waves, b, hkv, rep, t, False):
        _check_decode_case(case, b, hkv, rep, slot)


def test_decode_attention_honours_max_kv():
    """t_cap below the slot: the keys from t_cap on are not attended (as the bf16 kernels treat max_kv)."""
    b, hkv, rep, t, slot, cap = 3, 2, 4, 300, 299, 150
    case = _decode_case(b, hkv, rep, t, slot, False)
    q, kq, vq, _ = case["random"]
    kvs = case["kvs"].clone()
    kvs[2] = 5
    want = ref.attention(q.cpu(), k8.to_device(kq, "cpu"), k8.to_device(vq, "cpu"), cap - 1, kvs.cpu()).reshape(b, -1)
    for waves in (8, 1):
        with _waves(waves, b, hkv, rep, cap, False):
            _close(_attend(q, kq, vq, slot, kvs, None, max_kv=cap), want, 2e-2, 2e-2)


def test_plan_rules():
    e = ops.ext()
    assert e.attn_decode_q8_plan_check(2, 32, 8, 64, 100, False)[0] != 0   # head dim
    assert e.attn_decode_q8_plan_check(2, 16, 1, DH, 100, False)[0] != 0   # rep 16
    assert e.attn_decode_q8_plan_check(2, 3, 1, DH, 100, False)[0] != 0    # rep 3
    # one wave per pair from 2048 (row, kv head) pairs, 8 waves below, whatever the rep, the context or a mask
    assert e.attn_decode_q8_plan_check(64, 32, 8, DH, 8192, False)[2] == 8
    assert e.attn_decode_q8_plan_check(255, 32, 8, DH, 384, False)[2] == 8
    assert e.attn_decode_q8_plan_check(256, 32, 8, DH, 384, False)[2] == 1
    assert e.attn_decode_q8_plan_check(256, 64, 8, DH, 384, True)[2] == 1    # rep 8, 2048 pairs
    assert e.attn_decode_q8_plan_check(32, 64, 8, DH, 384, False)[2] == 8
    assert e.attn_decode_q8_plan_check(2048, 8, 1, DH, 384, False)[2] == 1   # one kv head: by pairs, not by rows
    with pytest.raises(RuntimeError, match="no plan"):
        kv = ops.Fp8KV.zeros(1, 1, 8, DEV)
        ops.attention(torch.zeros(1, 1, 16, DH, dtype=BF16, device=DEV), kv, kv, 0,
                      torch.zeros(1, dtype=torch.int32, device=DEV))


# ---------------------------------------------------------------------------------- S > 1
@pytest.mark.parametrize("slot_on_device", [False, True])
@pytest.mark.parametrize("slot0", [0, 10])
@pytest.mark.parametrize("s", [7, 130])
def test_prefill_is_the_bf16_kernel_on_the_dequantised_rows(s, slot0, slot_on_device):
    b, hkv, rep = 2, 2, 4
    t = slot0 + s + 5
    g = torch.Generator().manual_seed(s + slot0)
    kv_start = torch.tensor([0, slot0 + s // 3], dtype=torch.int32)
    mag = lambda: 2.0 ** torch.randint(-4, 5, (b, hkv, t, 1), generator=g).float()  # noqa: E731
    kq = k8.quantize_kv((torch.randn(b, hkv, t, DH, generator=g) * 0.25 * mag()).to(BF16))
    vq = k8.quantize_kv((torch.randn(b, hkv, t, DH, generator=g) * mag()).to(BF16))
    q = (torch.randn(b, s, hkv * rep, DH, generator=g) * 0.5).to(BF16).to(DEV)
    slot = torch.tensor([slot0], dtype=torch.int32, device=DEV) if slot_on_device else slot0
    got = ops.attention(q, k8.to_device(kq, DEV), k8.to_device(vq, DEV), slot, kv_start.to(DEV))
    want = ops.attention(q, kq.dequant().to(DEV), vq.dequant().to(DEV), slot, kv_start.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(got, want)  # the same kernel on the same bits
    _close(got, ref.attention(q.cpu(), kq, vq, slot0, kv_start).reshape(b * s, -1), 2e-2, 2e-2)


# ---------------------------------------------------------------------------------- routing
def test_fused_launches_and_packs_decline_fp8kv():
    h, hkv, k = 8, 1, 512
    pw = PackedLinear.from_dense(torch.randn((h + 2 * hkv) * DH, k).to(BF16), DEV)
    po = PackedLinear.from_dense(torch.randn(k, h * DH).to(BF16), DEV)
    x = torch.randn(1, k).to(BF16).to(DEV)
    kc = torch.zeros(1, hkv, 64, DH, dtype=BF16, device=DEV)
    k8v = ops.Fp8KV.zeros(1, hkv, 64, DEV)
    q4 = torch.zeros(1, 1, h, DH, dtype=BF16, device=DEV)
    assert ops.qkv_attention_splits(x, pw, kc, 1, h, hkv) > 0 and ops.attention_packs(q4, kc)  # bf16: both apply here
    assert ops.qkv_attention_splits(x, pw, k8v, 1, h, hkv) == 0
    assert ops.attention_packs(q4, k8v) is False
    saved = ops.QKV_ATTN_O
    try:
        ops.QKV_ATTN_O = 1
        assert ops.qkv_attention_o_groups(x, po, h, hkv, kc) == ops.qkv_attention_o_groups(x, po, h, hkv) > 0
        assert ops.qkv_attention_o_groups(x, po, h, hkv, k8v) == 0
    finally:
        ops.QKV_ATTN_O = saved
    with pytest.raises(ValueError):
        ops.attention(q4, k8v, k8v, 0, torch.zeros(1, dtype=torch.int32, device=DEV),
                      out_packed=ops.packed_empty(1, h * DH, DEV))


@pytest.mark.parametrize("m", [1, 40, 130])
def test_linear_qkv_rope_is_store_plus_write(m):
    """linear_qkv_rope with an Fp8KV: exactly linear() followed by rope_kv_write (no RoPE epilogue quantises)."""
    h, hkv, k, s = 4, 2, 256, 1
    g = torch.Generator().manual_seed(m)
    pw = PackedLinear.from_dense((torch.randn((h + 2 * hkv) * DH, k, generator=g) * 0.05).to(BF16), DEV)
    x = torch.randn(m, k, generator=g).to(BF16).to(DEV)
    table = ref.rope_table(DH, 64, 10000.0).to(DEV)
    pos = torch.randint(0, 64, (m,), generator=g, dtype=torch.int32).to(DEV)
    slot = torch.tensor([1], dtype=torch.int32, device=DEV)
    k1, v1, k2, v2 = [ops.Fp8KV.zeros(m, hkv, 4, DEV) for _ in range(4)]
    q1 = ops.linear_qkv_rope(x, pw, 1e-5, table, pos, k1, v1, slot, s, h, hkv, DH)
    q2 = ops.rope_kv_write(ops.linear(x, pw, rms_eps=1e-5), table, pos, k2, v2, slot, s, h, hkv, DH)
    torch.cuda.synchronize()
    assert torch.equal(q1, q2) and torch.equal(k1.q, k2.q) and torch.equal(v1.q, v2.q)
    assert torch.equal(k1.scale, k2.scale) and torch.equal(v1.scale, v2.scale) and int(k1.q[:, :, 1].max()) > 0


# ---------------------------------------------------------------------------------- the model
@functools.lru_cache(maxsize=None)
def _models(weights):
    """(config, CPU model, GPU model) with the fp8 KV cache set, bf16 or Fp8Linear weights."""
    cfg = gpu_config()
    cpu, _, _, params = build(cfg, seed=21)
    gpu = LLaMAForCausalLM(cfg, device=DEV, _do_init=False).load_params(params)
    if weights == "fp8":
        cpu.quantize_weights_("fp8_e4m3")
        gpu.quantize_weights_("fp8_e4m3")
    return cfg, cpu, gpu


def _prefill_and_decode(model, toks, mask, extra, fmt):
    """Logits of the prefill and of 3 decode steps ([B, S + 3, V]) with a cache of ``fmt``, and the cache."""
    b, s = toks.shape
    full = torch.cat([mask, torch.ones(b, 3, dtype=mask.dtype)], 1)
    pos = (full.cumsum(-1) - 1).to(torch.int32)
    cache = model.init_cache(b, s + 4, kv_format=fmt)
    outs = [model(toks, attention_mask=full, position_ids=pos[:, :s], past_key_values=cache).logits]
    for i in range(3):
        outs.append(model(extra[:, i:i + 1], attention_mask=full, position_ids=pos[:, s + i:s + i + 1],
                          past_key_values=cache).logits)
    return torch.cat(outs, 1).float().cpu(), cache, full.bool()


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
@pytest.mark.parametrize("b", [2, 40])
def test_model_gpu_vs_cpu_same_definition(b, weights):
    """Prefill + 3 decode steps, left-padded batch. GPU logits against the CPU path of the same definition: rel_err <
    2e-2, the project's GPU-vs-CPU number (tests/test_model_gpu.py)."""
    cfg, cpu, gpu = _models(weights)
    s = 9
    lens = [max(2, s - (3 * i) % 8) for i in range(b)]
    toks, mask = left_padded_batch(lens, s, cfg.vocab_size, pad=2, seed=b)
    extra = torch.randint(3, cfg.vocab_size, (b, 3), dtype=torch.int32, generator=torch.Generator().manual_seed(b + 1))
    g8, gc8, m = _prefill_and_decode(gpu, toks, mask, extra, "fp8_e4m3")
    c8, cc8, _ = _prefill_and_decode(cpu, toks, mask, extra, "fp8_e4m3")
    g16, _, _ = _prefill_and_decode(gpu, toks, mask, extra, "bf16")
    c16, _, _ = _prefill_and_decode(cpu, toks, mask, extra, "bf16")
    assert gc8.kv_format == "fp8_e4m3" and gc8.index == s + 3
    err8, err16 = rel_err(g8[m], c8[m]), rel_err(g16[m], c16[m])
    written = torch.zeros(b, s + 4, dtype=torch.bool)
    written[:, :s + 3] = True
    sel = written[None, :, None, :].expand(cfg.num_hidden_layers, b, gpu.n_kv_heads, s + 4)
    diff = sum(int((a.cpu()[sel] != c[sel]).sum()) for a, c in ((gc8.k, cc8.k), (gc8.v, cc8.v)))
    sdiff = sum(int((a.cpu()[sel] != c[sel]).sum()) for a, c in ((gc8.k_scale, cc8.k_scale), (gc8.v_scale, cc8.v_scale)))
    total = 2 * int(sel.sum()) * DH
    shift = rel_err(g8[m], g16[m])
    print(f"B={b} weights={weights}: GPU vs CPU rel_err fp8 cache {err8:.4f}, bf16 cache {err16:.4f}; fp8 codes that "
          f"differ between the GPU and CPU caches {diff} of {total} ({sdiff} row scales); fp8-cache vs bf16-cache "
          f"logits on the GPU: rel shift {shift:.4f}")
    assert bool(torch.isfinite(g8).all())
    assert err8 < 2e-2


def test_model_graph_replay_sampling_and_kernel_count():
    cfg, _, gpu = _models("bf16")
    toks, mask = left_padded_batch([5, 8], 8, cfg.vocab_size, pad=2, seed=6)
    gc = GenerationConfig(max_length=48, do_sample=False, pad_token_id=2, eos_token_id=2)
    try:
        gpu.set_kv_cache_format("fp8_e4m3")
        e1 = DecodeEngine(gpu, 2, 48, use_graph=True)
        assert e1.cache.kv_format == "fp8_e4m3"
        a = e1.run(toks, mask, gc).clone()
        b = DecodeEngine(gpu, 2, 48, use_graph=False).run(toks, mask, gc).clone()
        assert torch.equal(a, b)
        gs = dict(max_length=30, do_sample=True, temperature=0.8, top_p=0.95, pad_token_id=2, eos_token_id=2)
        s1 = gpu.generate(toks, mask, GenerationConfig(seed=11, **gs)).sequences
        s2 = gpu.generate(toks, mask, GenerationConfig(seed=11, **gs)).sequences
        assert torch.equal(s1, s2) and int(s1.min()) >= 0 and int(s1.max()) < cfg.vocab_size
    finally:
        gpu.set_kv_cache_format("bf16")


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


BF16_DECODE_KERNELS = 14  # (tests/test_fp8_gpu.py: the bf16 tiny model's captured decode step, default GEMV pinned)


@pytest.mark.parametrize("batch", [2, 40])
def test_decode_graph_has_one_more_kernel_per_layer(batch):
    cfg, _, gpu = _models("bf16")
    try:
        ops.GEMV_VARIANT = 1
        n_bf16 = _decode_graph_kernels(gpu, batch)
        gpu.set_kv_cache_format("fp8_e4m3")
        n_fp8 = _decode_graph_kernels(gpu, batch)
    finally:
        ops.GEMV_VARIANT = 0
        gpu.set_kv_cache_format("bf16")
    print(f"decode graph kernel nodes at B={batch}: bf16 cache {n_bf16}, fp8 cache {n_fp8}")
    assert n_bf16 == BF16_DECODE_KERNELS  # nothing changes for the bf16 cache
    assert n_fp8 == BF16_DECODE_KERNELS + cfg.num_hidden_layers  # the write kernel
