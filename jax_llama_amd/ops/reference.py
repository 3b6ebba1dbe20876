"""Pure-PyTorch reference implementations of every fused op.

These are (a) the CPU execution path of the framework (used by CPU tests, the gloo
multi-rank tests and the JAX-CPU-equivalent "plumbing" config) and (b) the numerics oracle
the HIP kernels are tested against. Each function reproduces the *rounding points* of the
corresponding kernel (bf16 operands, fp32 accumulation) so CPU and GPU runs agree to
bf16 rounding.

Reference semantics being reproduced (``/root/reference/jax_llama/model.py``):
  * RMSNorm ``x * rsqrt(mean(x^2) + eps) * w``                        (:28-48)
  * interleaved (complex-pair) RoPE                                  (:50-92)
  * causal + padding masked softmax attention with a KV cache        (:169-291)
  * SwiGLU ``w2(silu(w1 x) * w3 x)``                                  (:337-340)
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16


# ----------------------------------------------------------------------------------
# Weight packing (MFMA fragment layout, see ops/linear.py for the rationale)
# ----------------------------------------------------------------------------------
def pack_frag16x32(w: torch.Tensor) -> torch.Tensor:
    """Pack a row-major ``[N, K]`` weight into the 16x16x32-MFMA B-fragment layout.

    ``P[nt, ks, lane, e] = W[16*nt + (lane & 15), 32*ks + 8*(lane >> 4) + e]`` so one
    wave's 64 x 16-byte fragment load of a 16(n) x 32(k) block is 1 KiB contiguous.
    """
    n, k = w.shape
    assert n % 16 == 0 and k % 32 == 0, (n, k)
    return (w.reshape(n // 16, 16, k // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()
            .reshape(n // 16, k // 32, 64, 8))


def pack_act(x: torch.Tensor, rows: int) -> torch.Tensor:
    """Packed-layout copy of a decode activation ``x [M, K]`` (csrc/kernels/common.h pack_off): rows zero-padded to
    ``rows`` (a multiple of 16), then the weights' fragment order; returned as ``[rows, K]`` (flat order
    ``[rows/16][K/32][64][8]``)."""
    m, k = x.shape
    xp = torch.zeros(rows, k, dtype=x.dtype, device=x.device)
    xp[:m] = x
    return pack_frag16x32(xp).reshape(rows, k)


def unpack_act(p: torch.Tensor, m: int) -> torch.Tensor:
    """Inverse of ``pack_act`` (first ``m`` rows)."""
    rows, k = p.shape
    return unpack_frag16x32(p.reshape(rows // 16, k // 32, 64, 8), rows, k)[:m]


def unpack_frag16x32(p: torch.Tensor, n: int, k: int) -> torch.Tensor:
    return (p.reshape(n // 16, k // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).contiguous()
            .reshape(n, k))


# ----------------------------------------------------------------------------------
# FP8 (OCP e4m3fn) weight-only quantisation: one power-of-two scale per output row
# ----------------------------------------------------------------------------------
FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
FP8_EXP_CLAMP = 100


def quantize_fp8_rows(w: torch.Tensor):
    """``[N, K]`` weight -> ``(q float8_e4m3fn [N, K], scale fp32 [N])`` with ``scale[n] = 2^e[n]``,
    ``e[n] = ceil(log2(amax_n / 448))`` clamped to [-100, 100] (0 for an all-zero row) and ``q = fp8_rne(w / scale)``.
    The scale is a power of two, so ``dequantize_fp8_rows`` (``q * scale``) is exact in bf16.

    The exponent comes from ``frexp`` (no rounded logarithm): ``amax = m 2^x`` with ``m`` in [0.5, 1) and
    ``448 = 0.875 * 2^9``, so ``e = x - 9`` where ``m <= 0.875`` and ``x - 8`` above."""
    if w.dim() != 2:
        raise ValueError(f"quantize_fp8_rows: a [N, K] matrix, got {tuple(w.shape)}")
    wf = w.float()
    amax = wf.abs().amax(1)
    m, x = torch.frexp(amax)
    e = torch.where(m <= 0.875, x - 9, x - 8)
    e = torch.where(amax == 0, torch.zeros_like(e), e).clamp(-FP8_EXP_CLAMP, FP8_EXP_CLAMP)
    scale = torch.ldexp(torch.ones_like(amax), e)
    q = (wf / scale[:, None]).clamp(-FP8_MAX, FP8_MAX).to(FP8)  # (the clamp acts only where e was clamped)
    return q, scale


def dequantize_fp8_rows(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """``W_deq = q * scale`` as bf16 (exact)."""
    return (q.float() * scale.float()[:, None]).to(BF16)


KV8_DH = 128  # the head dim of the FP8 KV cache (the attention kernels' only head dim)


class Fp8KV:
    """One layer's K (post-RoPE) or V in the FP8 KV-cache format. A *row* is the 128 values of one (batch row, kv
    head, slot), quantised by ``quantize_fp8_rows``: ``q`` uint8 ``[B, Hkv, T, 128]`` holds the e4m3fn bytes in natural
    element order (``q.view(torch.float8_e4m3fn)`` is readable), ``scale`` fp32 ``[B, Hkv, T]`` the power-of-two row
    scales. 132 bytes per row instead of bf16's 256. Unwritten slots are bytes 0 and scale 0 (they dequantise to 0).
    Accepted wherever ``rope_kv_write`` / ``linear_qkv_rope`` / ``attention`` take a cache tensor; the model then
    computes what the bf16 model computes when every K / V row is replaced by ``q * scale`` (exact in bf16) at the
    moment it is written."""

    __slots__ = ("q", "scale")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        if q.dtype != torch.uint8 or q.dim() != 4 or q.shape[-1] != KV8_DH:
            raise ValueError(f"Fp8KV: q must be uint8 [B, Hkv, T, {KV8_DH}], got {q.dtype} {tuple(q.shape)}")
        if scale.dtype != torch.float32 or tuple(scale.shape) != tuple(q.shape[:3]) or scale.device != q.device:
            raise ValueError(f"Fp8KV: scale must be fp32 {tuple(q.shape[:3])} on {q.device}, got {scale.dtype} "
                             f"{tuple(scale.shape)} on {scale.device}")
        self.q, self.scale = q, scale

    @classmethod
    def zeros(cls, batch: int, n_kv_heads: int, max_length: int, device="cpu") -> "Fp8KV":
        return cls(torch.zeros(batch, n_kv_heads, max_length, KV8_DH, dtype=torch.uint8, device=device),
                   torch.zeros(batch, n_kv_heads, max_length, dtype=torch.float32, device=device))

    @property
    def shape(self):
        return self.q.shape

    @property
    def device(self):
        return self.q.device

    def nbytes(self) -> int:
        return self.q.numel() + 4 * self.scale.numel()

    def dequant(self, n: Optional[int] = None) -> torch.Tensor:
        """Slots ``[0, n)`` (default: all) as bf16 ``[B, Hkv, n, 128]``: ``q * scale``, exact."""
        n = self.q.shape[2] if n is None else n
        return (self.q[:, :, :n].view(FP8).float() * self.scale[:, :, :n, None]).to(BF16)

    def store(self, rows: torch.Tensor, slot0: int) -> None:
        """Quantise bf16 rows ``[B, Hkv, S, 128]`` into slots ``slot0 .. slot0 + S - 1``."""
        b, hkv, s, dh = rows.shape
        q, scale = quantize_fp8_rows(rows.to(BF16).reshape(-1, dh))
        self.q[:, :, slot0:slot0 + s] = q.view(torch.uint8).reshape(b, hkv, s, dh)
        self.scale[:, :, slot0:slot0 + s] = scale.reshape(b, hkv, s)

    def zero_(self) -> "Fp8KV":
        self.q.zero_()
        self.scale.zero_()
        return self


def is_fp8_kv(cache) -> bool:
    return isinstance(cache, Fp8KV)


def _kv_store(cache, rows: torch.Tensor, slot0: int) -> None:
    """``rows [B, Hkv, S, Dh]`` into cache slots ``slot0 ..``: a cast for a tensor cache, a quantising store of the
    bf16 rows for an ``Fp8KV``."""
    if is_fp8_kv(cache):
        cache.store(rows, slot0)
    else:
        cache[:, :, slot0:slot0 + rows.shape[2]] = rows.to(cache.dtype)


def _check_fp8_shape(n: int, k: int):
    if n <= 0 or k <= 0 or n % 16 or k % 64:
        raise ValueError(f"FP8 linear weights need N % 16 == 0 and K % 64 == 0, got {n}x{k}")


def pack_fp8_16x64(q: torch.Tensor) -> torch.Tensor:
    """``[N, K]`` float8 (or its uint8 bytes) -> uint8 ``[N/16, K/64, 64 lanes, 16 bytes]``: lane ``l`` of block
    ``(nt, kb)`` holds ``q[16 nt + (l & 15), 64 kb + 8 (l >> 4) + 0..7]`` in bytes 0-7 (the element order of the bf16
    fragment of k-step ``2 kb``, ``pack_frag16x32``) and the same at ``k + 32`` in bytes 8-15 (k-step ``2 kb + 1``)."""
    if q.dim() != 2:
        raise ValueError(f"pack_fp8_16x64: a [N, K] matrix, got {tuple(q.shape)}")
    n, k = q.shape
    _check_fp8_shape(n, k)
    b = q if q.dtype == torch.uint8 else q.view(torch.uint8)
    return (b.reshape(n // 16, 16, k // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5).contiguous()
            .reshape(n // 16, k // 64, 64, 16))


def unpack_fp8_16x64(p: torch.Tensor, n: int, k: int) -> torch.Tensor:
    """Inverse of ``pack_fp8_16x64``: the ``[n, k]`` float8 matrix."""
    _check_fp8_shape(n, k)
    if p.dtype != torch.uint8 or p.numel() != n * k:
        raise ValueError(f"unpack_fp8_16x64: uint8 with {n * k} bytes, got {p.dtype} {tuple(p.shape)}")
    return (p.reshape(n // 16, k // 64, 4, 16, 2, 8).permute(0, 3, 1, 4, 2, 5).contiguous()
            .reshape(n, k).view(FP8))


# ----------------------------------------------------------------------------------
# MXFP4 weight-only quantisation: e2m1 codes, one e8m0 (power-of-two) scale per output row and 32 K elements
# ----------------------------------------------------------------------------------
MXFP4_BLOCK = 32
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # the magnitudes of codes 0..7; bit 3 of a code is the sign
MXFP4_EXP_CLAMP = 100
E8M0_BIAS = 127


def e2m1_rne(v: torch.Tensor) -> torch.Tensor:
    """fp32 values -> e2m1 codes (uint8, 0..15): round to nearest, ties to the even code (the tie points 0.25 / 0.75 /
    1.25 / 1.75 / 2.5 / 3.5 / 5 go to 0 / 1 / 1 / 2 / 2 / 4 / 4), saturating at 6; the sign bit is the input's (also
    of -0.0)."""
    a = v.abs()
    mag = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8)
           + (a >= 1.75).to(torch.uint8) + (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8)
           + (a > 5.0).to(torch.uint8))
    return mag | (torch.signbit(v).to(torch.uint8) << 3)


def quantize_mxfp4(w: torch.Tensor):
    """``[N, K]`` weight (K % 32 == 0) -> ``(codes uint8 [N, K] in 0..15, e8m0 uint8 [N, K/32])``. The storage format is
    OCP MX (e2m1 elements, one e8m0 scale ``2^(b - 127)`` per 32 consecutive K elements of a row); the scale rule is
    the one of ``quantize_fp8_rows`` with 6 in place of 448 and a block in place of a row: ``e = ceil(log2(amax_block /
    6))`` clamped to [-100, 100] (0 for an all-zero block), ``code = e2m1_rne(w / 2^e)``. Nothing saturates except
    where the clamp acted -- unlike OCP's ``floor`` rule, which can clip the block maximum.

    The exponent comes from ``frexp`` (no rounded logarithm): ``amax = m 2^x`` with ``m`` in [0.5, 1) and
    ``6 = 0.75 * 2^3``, so ``e = x - 3`` where ``m <= 0.75`` and ``x - 2`` above."""
    if w.dim() != 2 or w.shape[1] % MXFP4_BLOCK:
        raise ValueError(f"quantize_mxfp4: a [N, K] matrix with K % 32 == 0, got {tuple(w.shape)}")
    n, k = w.shape
    wf = w.float().reshape(n, k // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = wf.abs().amax(2)
    m, x = torch.frexp(amax)
    e = torch.where(m <= 0.75, x - 3, x - 2)
    e = torch.where(amax == 0, torch.zeros_like(e), e).clamp(-MXFP4_EXP_CLAMP, MXFP4_EXP_CLAMP)
    scale = torch.ldexp(torch.ones_like(amax), e)
    codes = e2m1_rne(wf / scale[:, :, None]).reshape(n, k)
    return codes, (e + E8M0_BIAS).to(torch.uint8)


def dequantize_mxfp4(codes: torch.Tensor, e8m0: torch.Tensor) -> torch.Tensor:
    """``W_deq = value(code) * 2^(e8m0 - 127)`` as bf16 ``[N, K]`` (exact: three significant bits times a power of
    two)."""
    n, k = codes.shape
    lut = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32, device=codes.device)
    val = lut[codes.long()].reshape(n, k // MXFP4_BLOCK, MXFP4_BLOCK)
    scale = torch.ldexp(torch.ones(e8m0.shape, dtype=torch.float32, device=codes.device),
                        e8m0.to(torch.int32) - E8M0_BIAS)
    return (val * scale.reshape(n, k // MXFP4_BLOCK, 1)).reshape(n, k).to(BF16)


def _check_mxfp4_shape(n: int, k: int):
    if n <= 0 or k <= 0 or n % 16 or k % 128:
        raise ValueError(f"MXFP4 linear weights need N % 16 == 0 and K % 128 == 0, got {n}x{k}")


def pack_mxfp4_16x128(codes: torch.Tensor) -> torch.Tensor:
    """``[N, K]`` e2m1 codes (uint8, 0..15) -> uint8 ``[N/16, K/128, 64 lanes, 16 bytes]``: lane ``l`` of block
    ``(nt, kb)`` owns row ``16 nt + (l & 15)``, and its dword ``j`` (bytes ``4 j .. 4 j + 3``) holds the eight codes at
    ``k = 128 kb + 32 j + 8 (l >> 4) + 0..7``, two per byte -- the element order of the bf16 fragment of k-step
    ``4 kb + j`` (``pack_frag16x32``). The lower ``k`` of a byte is in the LOW nibble: byte ``i`` of a dword is the
    pair the conversion instruction's byte select ``i`` turns into one packed bf16 pair, low nibble first (settled by
    the GPU dequant kernel's bit-equality test against ``pack_frag16x32(W_deq)``)."""
    if codes.dim() != 2:
        raise ValueError(f"pack_mxfp4_16x128: a [N, K] matrix, got {tuple(codes.shape)}")
    n, k = codes.shape
    _check_mxfp4_shape(n, k)
    if codes.dtype != torch.uint8:
        raise ValueError(f"pack_mxfp4_16x128: uint8 codes, got {codes.dtype}")
    c = codes.reshape(n // 16, 16, k // 128, 4, 4, 4, 2)  # [nt, row, kb, j, l >> 4, byte, nibble]
    b = (c[..., 0] & 15) | (c[..., 1] << 4)
    return b.permute(0, 2, 4, 1, 3, 5).contiguous().reshape(n // 16, k // 128, 64, 16)


def unpack_mxfp4_16x128(p: torch.Tensor, n: int, k: int) -> torch.Tensor:
    """Inverse of ``pack_mxfp4_16x128``: the ``[n, k]`` codes."""
    _check_mxfp4_shape(n, k)
    if p.dtype != torch.uint8 or p.numel() != n * k // 2:
        raise ValueError(f"unpack_mxfp4_16x128: uint8 with {n * k // 2} bytes, got {p.dtype} {tuple(p.shape)}")
    b = p.reshape(n // 16, k // 128, 4, 16, 4, 4).permute(0, 3, 1, 4, 2, 5)  # [nt, row, kb, j, l >> 4, byte]
    return torch.stack([b & 15, b >> 4], -1).contiguous().reshape(n, k)


def pack_mxfp4_scales(e8m0: torch.Tensor) -> torch.Tensor:
    """``[N, K/32]`` e8m0 bytes -> uint8 ``[N/16, K/128, 16 rows, 4]``: one dword per (row, 128-deep block), byte ``j``
    the scale of k-step ``4 kb + j``; lane ``l`` of the block reads dword ``l & 15`` (64 bytes per block)."""
    if e8m0.dim() != 2:
        raise ValueError(f"pack_mxfp4_scales: a [N, K/32] matrix, got {tuple(e8m0.shape)}")
    n, k = e8m0.shape[0], e8m0.shape[1] * MXFP4_BLOCK
    _check_mxfp4_shape(n, k)
    if e8m0.dtype != torch.uint8:
        raise ValueError(f"pack_mxfp4_scales: uint8 scale bytes, got {e8m0.dtype}")
    return e8m0.reshape(n // 16, 16, k // 128, 4).permute(0, 2, 1, 3).contiguous()


def unpack_mxfp4_scales(p: torch.Tensor, n: int, k: int) -> torch.Tensor:
    """Inverse of ``pack_mxfp4_scales``: the ``[n, k/32]`` e8m0 bytes."""
    _check_mxfp4_shape(n, k)
    if p.dtype != torch.uint8 or p.numel() != n * k // MXFP4_BLOCK:
        raise ValueError(f"unpack_mxfp4_scales: uint8 with {n * k // MXFP4_BLOCK} bytes, got {p.dtype} {tuple(p.shape)}")
    return p.reshape(n // 16, k // 128, 16, 4).permute(0, 2, 1, 3).contiguous().reshape(n, k // MXFP4_BLOCK)


def nibble_pairs(codes: torch.Tensor) -> torch.Tensor:
    """``[N, K]`` codes -> uint8 ``[N, K/2]`` in natural order, the even ``k`` in the low nibble (the checkpoint form)."""
    return (codes[:, 0::2] & 15) | (codes[:, 1::2] << 4)


def nibble_unpairs(b: torch.Tensor) -> torch.Tensor:
    """Inverse of ``nibble_pairs``."""
    return torch.stack([b & 15, b >> 4], -1).reshape(b.shape[0], 2 * b.shape[1])


# ----------------------------------------------------------------------------------
# Elementwise / normalisation
# ----------------------------------------------------------------------------------
def embedding(ids: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    return table[ids.long().clamp(0, table.shape[0] - 1)].float()


def inv_rms(x: torch.Tensor, eps: float) -> torch.Tensor:
    x = x.float()
    return torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)


def rms_scale(x: torch.Tensor, eps: float) -> torch.Tensor:
    """``bf16(x * rsqrt(mean(x^2)+eps))`` — the norm weight is folded into the next GEMM."""
    return (x.float() * inv_rms(x, eps)).to(BF16)


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    """Un-fused RMSNorm exactly as the reference module (fp32 math)."""
    return x.float() * inv_rms(x, eps) * weight.float()


# ----------------------------------------------------------------------------------
# Linear layers (x @ W^T with W stored [N, K]); fp32 accumulate over bf16 operands
# ----------------------------------------------------------------------------------
def _mm(x: torch.Tensor, w_dense: torch.Tensor, rms_eps: Optional[float]) -> torch.Tensor:
    y = x.to(BF16).float() @ w_dense.float().t()
    if rms_eps is not None:
        y = y * inv_rms(x, rms_eps)
    return y


def linear(x, w_dense, rms_eps=None, out_dtype=BF16):
    return _mm(x, w_dense, rms_eps).to(out_dtype)


def linear_residual(x, w_dense, residual, rms_eps=None, accumulate=True):
    y = _mm(x, w_dense, rms_eps)
    if accumulate:
        residual.add_(y)
    else:
        residual.copy_(y)
    return residual


def linear_swiglu(x, w_dense_interleaved, rms_eps=None):
    """``w_dense_interleaved`` rows are 16-row tiles alternating gate (w1) / up (w3)."""
    y = _mm(x, w_dense_interleaved, rms_eps)
    m, n2 = y.shape
    y = y.reshape(m, n2 // 32, 2, 16)
    g, u = y[:, :, 0, :], y[:, :, 1, :]
    return (F.silu(g) * u).reshape(m, n2 // 2).to(BF16)


def interleave_gate_up(w1: torch.Tensor, w3: torch.Tensor) -> torch.Tensor:
    f, k = w1.shape
    assert f % 16 == 0
    return torch.stack([w1.reshape(f // 16, 16, k), w3.reshape(f // 16, 16, k)], 1).reshape(2 * f, k)


# ----------------------------------------------------------------------------------
# RoPE (interleaved pairs) + KV cache write
# ----------------------------------------------------------------------------------
def _llama31_scale(freqs: torch.Tensor) -> torch.Tensor:
    """Llama-3.1 ``use_scaled_rope`` frequency remap (factor 8, low/high 1/4, 8192 ctx)."""
    factor, low, high, old_ctx = 8.0, 1.0, 4.0, 8192.0
    wavelen = 2 * math.pi / freqs
    smooth = (old_ctx / wavelen - low) / (high - low)
    mid = (1 - smooth) * freqs / factor + smooth * freqs
    out = torch.where(wavelen < old_ctx / high, freqs, mid)
    return torch.where(wavelen > old_ctx / low, freqs / factor, out)


def rope_table(head_dim: int, end: int, theta: float, scaled: bool = False) -> torch.Tensor:
    """fp32 ``[end, head_dim/2, 2]`` (cos, sin) table (reference ``precompute_freqs_cis``,
    computed in fp64 and rounded once; the reference never stores it in bf16)."""
    i = torch.arange(0, head_dim, 2, dtype=torch.float64)[: head_dim // 2]
    freqs = 1.0 / (theta ** (i / head_dim))
    if scaled:
        freqs = _llama31_scale(freqs)
    t = torch.arange(end, dtype=torch.float64)
    ang = torch.outer(t, freqs)
    return torch.stack([torch.cos(ang), torch.sin(ang)], -1).float().contiguous()


def apply_rope(x: torch.Tensor, table: torch.Tensor, positions: torch.Tensor) -> torch.Tensor:
    """x: [M, nh, Dh]; positions: [M] (clamped into the table like the kernel)."""
    pos = positions.reshape(-1).long().clamp(0, table.shape[0] - 1)
    cs = table[pos]  # [M, Dh/2, 2]
    c, s = cs[..., 0][:, None, :], cs[..., 1][:, None, :]
    xf = x.float().reshape(*x.shape[:-1], -1, 2)
    xr, xi = xf[..., 0], xf[..., 1]
    out = torch.stack([xr * c - xi * s, xr * s + xi * c], -1)
    return out.reshape(x.shape)


def rope_kv_write(qkv, table, positions, k_cache, v_cache, slot0: int, seq_len: int,
                  n_heads: int, n_kv_heads: int, head_dim: int) -> torch.Tensor:
    """Split fused qkv ``[B*S, (H+2Hkv)*Dh]``, rotate q and k, store k/v at cache slots
    ``slot0 .. slot0+S-1`` of ``[B, Hkv, T, Dh]`` caches. Returns rotated q ``[B*S, H, Dh]``."""
    m = qkv.shape[0]
    b = m // seq_len
    q = qkv[:, : n_heads * head_dim].reshape(m, n_heads, head_dim)
    k = qkv[:, n_heads * head_dim:(n_heads + n_kv_heads) * head_dim].reshape(m, n_kv_heads, head_dim)
    v = qkv[:, (n_heads + n_kv_heads) * head_dim:].reshape(m, n_kv_heads, head_dim)
    qr = apply_rope(q, table, positions).to(BF16)
    kr = apply_rope(k, table, positions).to(BF16)
    kr = kr.reshape(b, seq_len, n_kv_heads, head_dim).permute(0, 2, 1, 3)
    vv = v.reshape(b, seq_len, n_kv_heads, head_dim).permute(0, 2, 1, 3)
    _kv_store(k_cache, kr, slot0)  # (an Fp8KV: the bf16 rows, quantised)
    _kv_store(v_cache, vv, slot0)
    return qr


def linear_qkv_rope(x, w_dense, rms_eps, table, positions, k_cache, v_cache, slot0: int, seq_len: int,
                    n_heads: int, n_kv_heads: int, head_dim: int) -> torch.Tensor:
    """Fused-kernel rounding points: fp32 projection -> fp32 RoPE -> one bf16 rounding. With ``Fp8KV`` caches the
    projection is a plain bf16 store followed by ``rope_kv_write`` (the rows that get quantised are defined from the
    bf16 projection output)."""
    if is_fp8_kv(k_cache) or is_fp8_kv(v_cache):
        return rope_kv_write(linear(x, w_dense, rms_eps), table, positions, k_cache, v_cache, slot0, seq_len,
                             n_heads, n_kv_heads, head_dim)
    y = _mm(x, w_dense, rms_eps)  # fp32 [M, (H+2Hkv)*Dh]
    m = y.shape[0]
    b = m // seq_len
    hq, hk = n_heads * head_dim, n_kv_heads * head_dim
    q = apply_rope(y[:, :hq].reshape(m, n_heads, head_dim), table, positions).to(BF16)
    k = apply_rope(y[:, hq:hq + hk].reshape(m, n_kv_heads, head_dim), table, positions)
    v = y[:, hq + hk:].reshape(m, n_kv_heads, head_dim)
    k_cache[:, :, slot0:slot0 + seq_len] = k.reshape(b, seq_len, n_kv_heads, head_dim).permute(0, 2, 1, 3).to(
        k_cache.dtype)
    v_cache[:, :, slot0:slot0 + seq_len] = v.reshape(b, seq_len, n_kv_heads, head_dim).permute(0, 2, 1, 3).to(
        v_cache.dtype)
    return q


# ----------------------------------------------------------------------------------
# Attention over the cache
# ----------------------------------------------------------------------------------
def attention(q, k_cache, v_cache, slot0: int, kv_start: torch.Tensor,
              key_mask: Optional[torch.Tensor] = None, return_weights: bool = False):
    """q: [B, S, H, Dh] (already rotated) for cache slots ``slot0+s``; caches
    ``[B, Hkv, T, Dh]``. Query at slot i attends keys j with ``kv_start[b] <= j <= i`` and
    ``key_mask[b, j]`` (if given). Rows with no valid key produce 0. Returns
    ``[B, S, H*Dh]`` bf16 (and fp32 weights ``[B, H, S, slot0+S]`` if requested). ``Fp8KV`` caches are read through
    their dequantised rows (q is never quantised)."""
    bsz, s, h, dh = q.shape
    t_len = slot0 + s
    if is_fp8_kv(k_cache):
        k_cache = k_cache.dequant(t_len)
    if is_fp8_kv(v_cache):
        v_cache = v_cache.dequant(t_len)
    hkv = k_cache.shape[1]
    rep = h // hkv
    k = k_cache[:, :, :t_len].float().repeat_interleave(rep, dim=1)  # [B,H,T,Dh]
    v = v_cache[:, :, :t_len].float().repeat_interleave(rep, dim=1)
    qf = q.float().permute(0, 2, 1, 3)  # [B,H,S,Dh]
    scores = qf @ k.transpose(-1, -2) / math.sqrt(dh)  # [B,H,S,T]
    qi = torch.arange(slot0, slot0 + s, device=q.device)[:, None]
    kj = torch.arange(t_len, device=q.device)[None, :]
    valid = (kj <= qi)[None]  # [1,S,T]
    valid = valid & (kj[None] >= kv_start.long().reshape(bsz, 1, 1))
    if key_mask is not None:
        valid = valid & key_mask[:, None, :t_len].bool()
    valid = valid[:, None]  # [B,1,S,T]
    scores = scores.masked_fill(~valid, float("-inf"))
    mx = scores.amax(-1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    p = torch.exp(scores - mx)
    denom = p.sum(-1, keepdim=True)
    p = torch.where(denom > 0, p / denom.clamp_min(1e-30), torch.zeros_like(p))
    out = (p @ v).permute(0, 2, 1, 3).reshape(bsz, s, h * dh).to(BF16)
    if return_weights:
        return out, p
    return out


# ----------------------------------------------------------------------------------
# Sampling (HF FlaxGenerationMixin semantics: temperature -> top-k -> top-p -> categorical)
# ----------------------------------------------------------------------------------
def argmax(logits: torch.Tensor) -> torch.Tensor:
    return logits.float().argmax(-1).to(torch.int32)  # first max index, like jnp.argmax


def logprob(logits: torch.Tensor, targets: torch.Tensor, col_offset: int = 0):
    """Scoring triple of one vocab shard's logits ``[M, V]``: ``tgt`` = the logit at column ``targets - col_offset``
    (0 where that is outside ``[0, V)``: an ignored label, another rank's shard), ``mx`` = the row maximum, ``se`` =
    ``sum exp(logit - mx)``; fp32 ``[M]`` each. ``log p(target) = sum_r tgt_r - lse`` (``ops.logprob_combine``)."""
    x = logits.float()
    col = targets.to(torch.int64).reshape(-1) - int(col_offset)
    ok = (col >= 0) & (col < x.shape[1])
    picked = x.gather(1, col.clamp(0, x.shape[1] - 1).unsqueeze(1)).squeeze(1)
    tgt = torch.where(ok, picked, torch.zeros_like(picked))
    mx = x.max(-1).values
    se = torch.exp(x - mx.unsqueeze(1)).sum(-1)
    return tgt, mx, se


def linear_logprob(x, w_dense, targets, rms_eps=None, col_offset: int = 0):
    """fp32 ``linear`` followed by the scoring triple."""
    return logprob(linear(x, w_dense, rms_eps, torch.float32), targets, col_offset)


def top_k_top_p_filter(logits: torch.Tensor, temperature: float, top_k: int, top_p: float) -> torch.Tensor:
    """Returns warped logits with filtered entries at -inf (FlaxTemperature/TopK/TopP)."""
    x = logits.float()
    if temperature is not None and temperature != 1.0:
        x = x / temperature
    if top_k is not None and top_k != 0:
        k = min(top_k, x.shape[-1])
        vals, idx = torch.topk(x, k, dim=-1)
        y = torch.full_like(x, float("-inf"))
        x = y.scatter(-1, idx, vals)
    if top_p is not None and top_p < 1.0:
        vals, idx = torch.sort(x, dim=-1, descending=True)
        cum = torch.softmax(vals, -1).cumsum(-1)
        keep = cum < top_p
        keep = torch.roll(keep, 1, dims=-1)
        keep[:, 0] = True
        vals = torch.where(keep, vals, torch.full_like(vals, float("-inf")))
        x = torch.full_like(x, float("-inf")).scatter(-1, idx, vals)
    return x


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) on uint32 numpy arrays: ``counter`` [..., 4], ``key``
    [2]. Bit-exact twin of ``philox4x32_10`` in csrc/kernels/topk_sample.hip."""
    import numpy as np
    c = [np.asarray(counter[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    m0, m1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & mask
        hi1, lo1 = p1 >> np.uint64(32), p1 & mask
        c = [(hi1 ^ c[1] ^ k0) & mask, lo1, (hi0 ^ c[3] ^ k1) & mask, lo0]
        k0 = (k0 + np.uint64(0x9E3779B9)) & mask
        k1 = (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack([x.astype(np.uint32) for x in c], -1)


def topk_sorted(logits: torch.Tensor, k: int):
    """Top-k values (descending) and indices, ties broken by the lower index (lax.top_k order)."""
    import numpy as np
    x = logits.float().cpu().numpy()
    vals, idxs = [], []
    for row in x:
        order = np.lexsort((np.arange(row.size), -row))[:k]
        vals.append(row[order])
        idxs.append(order)
    return torch.from_numpy(np.stack(vals)), torch.from_numpy(np.stack(idxs).astype(np.int32))


def topk_sample(logits: torch.Tensor, k: int, temperature: float, top_p: float, seed: int, step: int) -> torch.Tensor:
    """Reference of the on-device sampler: temperature -> top-k -> top-p (HF keep rule) ->
    Gumbel-max with Philox(seed; counter = (rank-in-top-k, row, step, 0))."""
    import numpy as np
    vals, idx = topk_sorted(logits, k)
    v = vals.numpy().astype(np.float32) / np.float32(temperature)
    p = np.exp(v - v[:, :1])
    p = p / p.sum(-1, keepdims=True)
    excl = np.cumsum(p, -1) - p
    keep = excl < np.float32(top_p)
    keep[:, 0] = True
    b = v.shape[0]
    ctr = np.zeros((b, k, 4), dtype=np.uint32)
    ctr[..., 0] = np.arange(k, dtype=np.uint32)[None]
    ctr[..., 1] = np.arange(b, dtype=np.uint32)[:, None]
    ctr[..., 2] = np.uint32(step)
    r = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))[..., 0]
    u = ((r >> 8).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    g = -np.log(-np.log(u))
    score = np.where(keep, v + g, -np.inf)
    choice = score.argmax(-1)
    return idx[torch.arange(b), torch.from_numpy(choice)].to(torch.int32)


# ----------------------------------------------------------------------------------
# Beam search (HF Flax ``_beam_search`` semantics; the README's "Beam search" section is the definition)
# ----------------------------------------------------------------------------------
BEAM_NEG = -1.0e7
BEAM_MAX = 8  # num_beams <= 8: K x 2K <= 128 candidates per batch item (ranked by counting in the kernel)


def beam_early_code(early_stopping) -> int:
    """``early_stopping`` as the kernels take it: False -> 0, True -> 1, "never" -> 2."""
    if early_stopping is True:
        return 1
    if early_stopping is False:
        return 0
    if early_stopping == "never":
        return 2
    raise ValueError(f"early_stopping must be True, False or 'never', got {early_stopping!r}")


def beam_inv_pen(max_length: int, length_penalty: float) -> torch.Tensor:
    """fp32 ``[max_length + 1]``: ``1 / t ** length_penalty`` computed in fp64 and rounded once (entry 0 is unused).
    Every score is multiplied by an entry of this table, so the CPU and the GPU do the same IEEE multiply; HF
    divides by the power instead, which differs by at most one rounding."""
    import numpy as np
    t = np.arange(max_length + 1, dtype=np.float64)
    t[0] = 1.0
    return torch.from_numpy((1.0 / t ** float(length_penalty)).astype(np.float32))


def _order_desc(x: torch.Tensor) -> torch.Tensor:
    """int64 ``[B, n]``: the columns of each row of ``x`` by value descending, ties to the lower column."""
    import numpy as np
    v = x.float().cpu().numpy()
    idx = np.broadcast_to(np.arange(v.shape[1]), v.shape)
    return torch.from_numpy(np.lexsort((idx, -v), axis=-1).astype(np.int64))


def beam_step(cand_v, cand_i, lse, running_seq, seq, running_score, score, is_finished, inv_pen, cur_len: int,
              prompt_len: int, eos: int, early_stopping):
    """One beam-search step at ``cur_len = c`` for B items of K beams. ``cand_v`` / ``cand_i`` ``[B*K, 2K]``: each
    running beam's sorted top-2K logits and their token ids; ``lse`` fp32 ``[B*K]``; ``running_seq`` / ``seq`` int32
    ``[B, K, L]``; ``running_score`` / ``score`` fp32 ``[B, K]``; ``is_finished`` bool ``[B, K]``. Returns the next
    ``(running_seq, seq, running_score, score, is_finished, beam_idx int32 [B, K], tokens int32 [B, K])``; the inputs
    are left as they are. All arithmetic is fp32, one rounding per add / multiply. The penalty of a finished-pool
    candidate is ONE addition of -1e7, made where the candidate did not just finish or where every slot of its item
    was already finished under ``early_stopping=True`` (HF's ``add_penalty`` is the OR of the two)."""
    b, k, length = running_seq.shape
    k2, c = 2 * k, int(cur_len)
    assert prompt_len <= c < length and cand_v.shape == (b * k, k2), (prompt_len, c, length, cand_v.shape)
    neg = torch.tensor(BEAM_NEG, dtype=torch.float32)
    lp = running_score.float().unsqueeze(-1) + (cand_v.float().view(b, k, k2) - lse.float().view(b, k, 1))
    flat = lp.reshape(b, k * k2)
    order = _order_desc(flat)[:, :k2]
    top_lp = flat.gather(1, order)
    parent = order // k2
    token = cand_i.reshape(b, k * k2).gather(1, order).to(torch.int32)
    just = token == int(eos)
    run_lp = torch.where(just, neg + top_lp, top_lp)
    rorder = _order_desc(run_lp)[:, :k]
    beam_idx = parent.gather(1, rorder).to(torch.int32)
    tokens = token.gather(1, rorder)
    cand_seq = running_seq.gather(1, parent[:, :, None].expand(b, k2, length)).clone()
    cand_seq[:, :, c] = token
    new_running_seq = cand_seq.gather(1, rorder[:, :, None].expand(b, k, length))
    new_running_score = run_lp.gather(1, rorder)
    fin_lp = top_lp * inv_pen[c + 1 - prompt_len]
    all_fin = is_finished.bool().all(1, keepdim=True) & (early_stopping is True)
    fin_lp = torch.where(~just | all_fin, fin_lp + neg, fin_lp)
    m_score = torch.cat([score.float(), fin_lp], 1)
    m_seq = torch.cat([seq, cand_seq], 1)
    m_fin = torch.cat([is_finished.bool(), just], 1)
    forder = _order_desc(m_score)[:, :k]
    return (new_running_seq, m_seq.gather(1, forder[:, :, None].expand(b, k, length)), new_running_score,
            m_score.gather(1, forder), m_fin.gather(1, forder), beam_idx, tokens)


def beam_continue(running_score, score, is_finished, inv_pen, cur_len: int, prompt_len: int, max_length: int,
                  early_stopping, length_penalty: float) -> bool:
    """The loop condition, evaluated before the step at ``cur_len`` and global over the batch."""
    c = int(cur_len)
    fin = is_finished.bool()
    if c >= max_length:
        return False
    if early_stopping is True and bool(fin.all()):
        return False
    if c == prompt_len:  # the first step always runs
        return True
    d = max_length - prompt_len if (early_stopping == "never" and length_penalty > 0.0) else c - prompt_len
    best_running = running_score.float()[:, 0] * inv_pen[d]
    neg = torch.tensor(BEAM_NEG, dtype=torch.float32)
    worst_finished = torch.where(fin.any(1), score.float().min(1).values, neg)
    return bool((best_running > worst_finished).any())


def kv_beam_reorder(t: torch.Tensor, beam_idx: torch.Tensor, k: int, count: int) -> torch.Tensor:
    """In place on one cache tensor ``[L, B*K, Hkv, T, ...]`` (values or scales): slots ``[0, count)`` of row
    ``b*K + j`` become those of row ``b*K + beam_idx[b, j]``; later slots keep their content."""
    rows = t.shape[1]
    b = rows // k
    src = (torch.arange(b, device=t.device)[:, None] * k + beam_idx.reshape(b, k).long().to(t.device)).reshape(-1)
    n = max(0, min(int(count), t.shape[3]))
    t[:, :, :, :n] = t.index_select(1, src)[:, :, :, :n]
    return t


# ----------------------------------------------------------------------------------
# Logits processors (the README's "Logits processors" section is the definition)
# ----------------------------------------------------------------------------------
PROC_MAX_STOP = 8       # stop ids per call (eos_token_id as a list)
PROC_MAX_SUPPRESS = 64  # always-banned ids per call


@dataclass
class LogitsProcessors:
    """What ``process_logits`` applies, resolved for one call: ``min_len`` is ``max(min_length, S + min_new_tokens)``
    (the stop ids are banned while ``cur_len < min_len``), ``vocab`` the whole vocabulary (history tokens outside
    ``[0, vocab)`` are skipped; None: no upper limit)."""

    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    suppress_tokens: Sequence[int] = ()
    stop_ids: Sequence[int] = ()
    min_len: int = 0
    vocab: Optional[int] = None

    def active(self) -> bool:
        return (float(self.repetition_penalty) != 1.0 or self.no_repeat_ngram_size > 0 or len(self.suppress_tokens) > 0
                or (self.min_len > 0 and len(self.stop_ids) > 0))


def inv_penalty(p: float) -> float:
    """``fp32(1 / p)``, computed in fp64 and rounded once: positive logits are multiplied by it where HF divides by
    ``p`` (at most one rounding apart), so the CPU and the GPU do the same IEEE multiply."""
    import numpy as np
    return float(np.float32(1.0 / float(p)))


def process_logits(logits: torch.Tensor, sequences: torch.Tensor, cur_len: int, hist_start: torch.Tensor,
                   col_offset: int, cfg: LogitsProcessors) -> torch.Tensor:
    """In place on fp32 ``logits [B, V_local]`` (columns ``[col_offset, col_offset + V_local)`` of the vocabulary), per
    row b over the history ``H = sequences[b, hist_start[b] : cur_len]``: the repetition penalty (each distinct token
    of H once: ``l > 0 -> l * fp32(1 / p)``, else ``l * p``), then the masks, which store ``-inf``: the token that
    would complete a repeated n-gram, the suppressed ids, and the stop ids while ``cur_len < min_len``."""
    assert logits.dtype == torch.float32 and logits.dim() == 2
    b, v = logits.shape
    length = sequences.shape[1]
    cl = max(0, min(int(cur_len), length))
    p, n = float(cfg.repetition_penalty), int(cfg.no_repeat_ngram_size)
    p32 = torch.tensor(p, dtype=torch.float32)
    inv32 = torch.tensor(inv_penalty(p), dtype=torch.float32)
    hi = cfg.vocab if cfg.vocab is not None else (1 << 62)

    def local(tok: torch.Tensor) -> torch.Tensor:  # this shard's columns of the in-vocabulary tokens of `tok`
        tok = tok[(tok >= 0) & (tok < hi)] - col_offset
        return tok[(tok >= 0) & (tok < v)]

    always = local(torch.as_tensor(list(cfg.suppress_tokens), dtype=torch.int64))
    stops = local(torch.as_tensor(list(cfg.stop_ids), dtype=torch.int64))
    for r in range(b):
        hs = max(0, min(int(hist_start[r]), cl))
        h = sequences[r, hs:cl].to(torch.int64).cpu()
        row = logits[r]
        if p != 1.0 and h.numel():
            cols = torch.unique(local(h))
            x = row[cols]
            row[cols] = torch.where(x > 0, x * inv32, x * p32)
        if n >= 1 and h.numel() >= n:
            windows = h.unfold(0, n, 1)  # [len - n + 1, n]
            match = (windows[:, :n - 1] == h[h.numel() - n + 1:]).all(1)
            row[local(windows[match, n - 1])] = -math.inf
        row[always] = -math.inf
        if int(cur_len) < cfg.min_len:
            row[stops] = -math.inf
    return logits
