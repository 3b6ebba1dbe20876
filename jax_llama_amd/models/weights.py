"""Weight containers.

On the GPU every linear weight lives in the *MFMA fragment-packed* layout
(``ops.reference.pack_frag16x32``): a ``[N, K]`` matrix becomes
``[N/16][K/32][64 lanes][8 bf16]`` so that each 16(n) x 32(k) block — exactly the B
operand of one ``v_mfma_f32_16x16x32_bf16`` — is one contiguous 1 KiB run that a wave loads
with a single ``global_load_dwordx4`` (16 B/lane, perfectly coalesced) and that an LDS-DMA
copy lands lane-linearly (bank-conflict-free ``ds_read_b128``). Both the decode GEMV-like
kernel and the prefill GEMM consume this one layout, so weights are stored once.

Norm weights are folded into the following projection at load time
(``W'[n, k] = W[n, k] * g[k]``), so RMSNorm reduces to a per-row ``inv_rms`` scale that the
GEMM applies in its epilogue (reference RMSNorm: ``model.py:28-48``).

On the CPU (test/oracle path) the same object simply holds the dense ``[N, K]`` bf16 matrix.
"""
from __future__ import annotations

from typing import Optional

import torch

from ..ops import reference as ref

BF16 = torch.bfloat16


class PackedLinear:
    """``y = x @ W^T`` with ``W`` logically ``[n, k]`` (Meta ``[out, in]`` orientation)."""

    def __init__(self, weight: torch.Tensor, n: int, k: int):
        self.weight = weight
        self.n = n
        self.k = k

    @property
    def device(self) -> torch.device:
        return self.weight.device

    @property
    def packed(self) -> bool:
        return self.weight.dim() == 4

    @classmethod
    def from_dense(cls, w: torch.Tensor, device, fold: Optional[torch.Tensor] = None) -> "PackedLinear":
        n, k = w.shape
        device = torch.device(device)
        src = w.to(device)
        if fold is not None:
            src = (src.float() * fold.to(device).float()[None, :])
        src = src.to(BF16)
        if device.type == "cuda":
            if n % 16 or k % 32:
                raise ValueError(f"GPU linear weights need N%16==0 and K%32==0, got {n}x{k}")
            return cls(ref.pack_frag16x32(src), n, k)
        return cls(src.contiguous(), n, k)

    @classmethod
    def random(cls, n: int, k: int, device, std: float = 0.02, generator=None) -> "PackedLinear":
        """Random-init directly in the on-device layout (synthetic benchmarks)."""
        device = torch.device(device)
        if device.type == "cuda":
            w = torch.empty(n // 16, k // 32, 64, 8, dtype=BF16, device=device)
        else:
            w = torch.empty(n, k, dtype=BF16, device=device)
        w.normal_(0.0, std, generator=generator)
        return cls(w, n, k)

    def dense(self) -> torch.Tensor:
        """The ``[n, k]`` bf16 matrix (unpacks on the GPU; used for debugging / oracles)."""
        if self.packed:
            return ref.unpack_frag16x32(self.weight, self.n, self.k)
        return self.weight

    def nbytes(self) -> int:
        return self.weight.numel() * self.weight.element_size()


class Fp8Linear:
    """FP8 (OCP e4m3fn) weight-only linear with ``PackedLinear``'s surface: ``q [n, k]`` fp8 plus one power-of-two fp32
    scale per output row (``ops.reference.quantize_fp8_rows``). ``W_deq = q * scale`` is exact in bf16, and the layer is
    by definition the bf16 linear on ``W_deq`` (``dense()``).

    On the GPU ``qweight`` is the uint8 block layout ``[n/16, k/64, 64, 16]`` (``ops.reference.pack_fp8_16x64``) that the
    FP8 decode GEMV streams; every other kernel reads the bf16 copy ``ops`` dequantises into a workspace. On the CPU
    it is the dense fp8 ``[n, k]`` and every op goes through ``dense()``."""

    fp8 = True

    def __init__(self, qweight: torch.Tensor, scale: torch.Tensor, n: int, k: int):
        self.qweight = qweight
        self.scale = scale
        self.n = n
        self.k = k

    @property
    def device(self) -> torch.device:
        return self.qweight.device

    @property
    def packed(self) -> bool:
        return self.qweight.dim() == 4

    @classmethod
    def from_q(cls, q: torch.Tensor, scale: torch.Tensor, device) -> "Fp8Linear":
        """From the dense fp8 values and their row scales (a checkpoint's tensors)."""
        n, k = q.shape
        device = torch.device(device)
        if n % 16 or k % 64:
            raise ValueError(f"FP8 linear weights need N%16==0 and K%64==0, got {n}x{k}")
        if q.dtype != ref.FP8 or scale.numel() != n:
            raise ValueError(f"Fp8Linear: float8_e4m3fn [N, K] and fp32 [N], got {q.dtype} and {tuple(scale.shape)}")
        scale = scale.reshape(n).to(device, torch.float32).contiguous()
        if device.type == "cuda":
            return cls(ref.pack_fp8_16x64(q.contiguous()).to(device), scale, n, k)
        return cls(q.to(device).contiguous(), scale, n, k)

    @classmethod
    def from_dense(cls, w: torch.Tensor, device, fold: Optional[torch.Tensor] = None) -> "Fp8Linear":
        """Quantise a ``[n, k]`` weight (after the optional norm fold and its bf16 rounding, as ``PackedLinear``)."""
        src = w if fold is None else w.float() * fold.to(w.device).float()[None, :]
        q, scale = ref.quantize_fp8_rows(src.to(BF16))
        return cls.from_q(q, scale, device)

    @classmethod
    def from_linear(cls, lin: PackedLinear) -> "Fp8Linear":
        return cls.from_dense(lin.dense(), lin.device)

    def q(self) -> torch.Tensor:
        """The dense ``[n, k]`` fp8 values."""
        if self.packed:
            return ref.unpack_fp8_16x64(self.qweight, self.n, self.k)
        return self.qweight

    def dense(self) -> torch.Tensor:
        """``W_deq`` as the ``[n, k]`` bf16 matrix."""
        return ref.dequantize_fp8_rows(self.q(), self.scale)

    def nbytes(self) -> int:
        return self.n * self.k + 4 * self.n


class Mxfp4Linear:
    """MXFP4 weight-only linear with ``PackedLinear``'s surface: e2m1 codes ``[n, k]`` plus one e8m0 scale byte per
    output row and 32 consecutive K elements (``ops.reference.quantize_mxfp4``), 4.25 bits per weight. ``W_deq =
    value(code) * 2^(e8m0 - 127)`` is exact in bf16, and the layer is by definition the bf16 linear on ``W_deq``
    (``dense()``).

    On the GPU ``qweight`` is the uint8 block layout ``[n/16, k/128, 64, 16]`` (``ops.reference.pack_mxfp4_16x128``)
    and ``scale`` the uint8 ``[n/16, k/128, 16, 4]`` (``pack_mxfp4_scales``) that the MXFP4 decode GEMV streams; every
    other kernel reads the bf16 copy ``ops`` dequantises into a workspace. On the CPU they are the dense codes
    ``[n, k]`` and scale bytes ``[n, k/32]`` and every op goes through ``dense()``."""

    mxfp4 = True

    def __init__(self, qweight: torch.Tensor, scale: torch.Tensor, n: int, k: int):
        self.qweight = qweight
        self.scale = scale
        self.n = n
        self.k = k

    @property
    def device(self) -> torch.device:
        return self.qweight.device

    @property
    def packed(self) -> bool:
        return self.qweight.dim() == 4

    @classmethod
    def from_q(cls, codes: torch.Tensor, e8m0: torch.Tensor, device) -> "Mxfp4Linear":
        """From the dense codes ``[n, k]`` (uint8, 0..15) and their scale bytes ``[n, k/32]`` (a checkpoint's tensors).
        Scale bytes outside 27..227, which ``quantize_mxfp4`` never writes, raise ``ValueError``."""
        if codes.dim() != 2:
            raise ValueError(f"Mxfp4Linear: a [N, K] code matrix, got {tuple(codes.shape)}")
        n, k = codes.shape
        device = torch.device(device)
        if n % 16 or k % 128 or n == 0 or k == 0:
            raise ValueError(f"MXFP4 linear weights need N%16==0 and K%128==0, got {n}x{k}")
        if codes.dtype != torch.uint8 or e8m0.dtype != torch.uint8 or tuple(e8m0.shape) != (n, k // 32):
            raise ValueError(f"Mxfp4Linear: uint8 codes [N, K] and uint8 scales [N, K/32], got {codes.dtype} and "
                             f"{e8m0.dtype} {tuple(e8m0.shape)}")
        # only the quantiser's range: outside it the definitions part (byte 0 is 2^-127 here and 0.0 as the kernel's
        # fp32 scale operand, byte 255 is a NaN in e8m0 and Inf as that operand)
        lo, hi = ref.E8M0_BIAS - ref.MXFP4_EXP_CLAMP, ref.E8M0_BIAS + ref.MXFP4_EXP_CLAMP
        if int(codes.max()) > 15 or int(e8m0.min()) < lo or int(e8m0.max()) > hi:
            raise ValueError(f"Mxfp4Linear: codes in 0..15 and scale bytes in {lo}..{hi} (quantize_mxfp4's range)")
        if device.type == "cuda":
            return cls(ref.pack_mxfp4_16x128(codes.contiguous()).to(device),
                       ref.pack_mxfp4_scales(e8m0.contiguous()).to(device), n, k)
        return cls(codes.to(device).contiguous(), e8m0.to(device).contiguous(), n, k)

    @classmethod
    def from_dense(cls, w: torch.Tensor, device, fold: Optional[torch.Tensor] = None) -> "Mxfp4Linear":
        """Quantise a ``[n, k]`` weight (after the optional norm fold and its bf16 rounding, as ``PackedLinear``)."""
        n, k = w.shape
        if n % 16 or k % 128 or n == 0 or k == 0:
            raise ValueError(f"MXFP4 linear weights need N%16==0 and K%128==0, got {n}x{k}")
        src = w if fold is None else w.float() * fold.to(w.device).float()[None, :]
        codes, e8m0 = ref.quantize_mxfp4(src.to(BF16))
        return cls.from_q(codes, e8m0, device)

    @classmethod
    def from_linear(cls, lin: PackedLinear) -> "Mxfp4Linear":
        return cls.from_dense(lin.dense(), lin.device)

    def q(self) -> torch.Tensor:
        """The dense ``[n, k]`` e2m1 codes."""
        if self.packed:
            return ref.unpack_mxfp4_16x128(self.qweight, self.n, self.k)
        return self.qweight

    def e8m0(self) -> torch.Tensor:
        """The dense ``[n, k/32]`` scale bytes."""
        if self.packed:
            return ref.unpack_mxfp4_scales(self.scale, self.n, self.k)
        return self.scale

    def dense(self) -> torch.Tensor:
        """``W_deq`` as the ``[n, k]`` bf16 matrix."""
        return ref.dequantize_mxfp4(self.q(), self.e8m0())

    def nbytes(self) -> int:
        return self.n * self.k // 2 + self.n * self.k // 32
