"""Static, pre-allocated KV cache.

Reference: Flax ``"cache"`` collection created by ``init_cache`` (``model.py:459-476``) and
updated by ``_concatenate_to_cache`` (``model.py:169-199``): per layer ``cached_key`` /
``cached_value`` of shape ``(B, T_max, Hkv, Dh)`` holding post-RoPE keys, plus a scalar
``cache_index`` advanced by the number of tokens written.

Here: two tensors ``[L, B, Hkv_local, T_max, Dh]`` (bf16) so that one (b, kv-head)'s keys
are a single contiguous ``T x 256 B`` run — the decode attention kernel streams it with
1 KiB-per-wave-instruction loads — and the slot index is mirrored in a device int32 so
hipGraph-captured decode steps read/advance it without host round trips. No forward pass
is run to create it (unlike the reference's ``module.init`` trick).

``kv_format="fp8_e4m3"``: the same layout in the FP8 KV-cache format (``ops.Fp8KV``): e4m3 bytes
``[L, B, Hkv, T, 128]`` plus one power-of-two fp32 scale per (layer, row, kv head, slot), for K and for V --
132 bytes per 128-value row instead of 256. ``layer(i)`` then returns ``Fp8KV`` pairs.
"""
from __future__ import annotations

import torch

from ..ops.reference import KV8_DH, Fp8KV

KV_FORMATS = ("bf16", "fp8_e4m3")


def kv_row_bytes(kv_format: str, head_dim: int) -> int:
    """Bytes one (row, kv head, slot) of K or of V takes: bf16 values, or e4m3 bytes plus the fp32 scale."""
    return head_dim + 4 if kv_format == "fp8_e4m3" else 2 * head_dim


class KVCache:
    def __init__(self, num_layers: int, batch_size: int, num_kv_heads: int, max_length: int,
                 head_dim: int, device, dtype=torch.bfloat16, kv_format: str = "bf16"):
        device = torch.device(device)
        if kv_format not in KV_FORMATS:
            raise ValueError(f"KVCache: unknown kv_format {kv_format!r} (one of {KV_FORMATS})")
        self.kv_format = kv_format
        shape = (num_layers, batch_size, num_kv_heads, max_length, head_dim)
        if kv_format == "fp8_e4m3":
            if head_dim != KV8_DH:
                raise ValueError(f"KVCache: the fp8_e4m3 format needs head_dim == {KV8_DH}, got {head_dim}")
            self.k = torch.zeros(shape, dtype=torch.uint8, device=device)
            self.v = torch.zeros(shape, dtype=torch.uint8, device=device)
            self.k_scale = torch.zeros(shape[:4], dtype=torch.float32, device=device)
            self.v_scale = torch.zeros(shape[:4], dtype=torch.float32, device=device)
        else:
            self.k = torch.zeros(shape, dtype=dtype, device=device)
            self.v = torch.zeros(shape, dtype=dtype, device=device)
            self.k_scale = self.v_scale = None
        self.batch_size = batch_size
        self.max_length = max_length
        self.index = 0  # host mirror of the number of filled slots
        self.index_t = torch.zeros(1, dtype=torch.int32, device=device)

    @property
    def device(self):
        return self.k.device

    def _pair(self, i: int, b0: int, b1: int):
        if self.kv_format == "fp8_e4m3":
            return (Fp8KV(self.k[i, b0:b1], self.k_scale[i, b0:b1]), Fp8KV(self.v[i, b0:b1], self.v_scale[i, b0:b1]))
        return self.k[i, b0:b1], self.v[i, b0:b1]

    def layer(self, i: int):
        """Layer ``i``'s ``(K, V)``: bf16 tensors, or ``Fp8KV`` handles (views of this cache)."""
        return self._pair(i, 0, self.batch_size)

    def advance(self, n: int) -> None:
        self.index += n
        self.index_t.add_(n)

    def reset(self) -> None:
        self.index = 0
        self.index_t.zero_()

    def zero_(self) -> None:
        """Clear every slot (values and scales); the slot index stays."""
        self.k.zero_()
        self.v.zero_()
        if self.k_scale is not None:
            self.k_scale.zero_()
            self.v_scale.zero_()

    def rows(self, b0: int, b1: int) -> "KVCacheRows":
        """The cache of batch rows ``[b0, b1)`` (every layer): a view whose per-layer K / V are contiguous slices, for a
        prefill run in row chunks (runtime/engine.py)."""
        return KVCacheRows(self, b0, b1)

    def nbytes(self) -> int:
        n = 2 * self.k.numel() * self.k.element_size()
        if self.k_scale is not None:
            n += 2 * self.k_scale.numel() * self.k_scale.element_size()
        return n

    # Flax-cache-like view for API parity / debugging (per-layer dict, (B, T, Hkv, Dh)); an FP8 cache: dequantised bf16.
    def as_dict(self):
        def bf16(kv):
            return kv.dequant() if isinstance(kv, Fp8KV) else kv

        return {
            str(i): {
                "cached_key": bf16(self.layer(i)[0]).permute(0, 2, 1, 3),
                "cached_value": bf16(self.layer(i)[1]).permute(0, 2, 1, 3),
                "cache_index": self.index,
            }
            for i in range(self.k.shape[0])
        }


class KVCacheRows:
    """Rows ``[b0, b1)`` of a KVCache: ``layer(i)`` gives contiguous ``[b1 - b0, Hkv, T, Dh]`` views; the slot index is
    the parent's (one position for every row)."""

    def __init__(self, parent: KVCache, b0: int, b1: int):
        self.parent = parent
        self.b0, self.b1 = b0, b1
        self.batch_size = b1 - b0
        self.max_length = parent.max_length
        self.kv_format = parent.kv_format

    @property
    def device(self):
        return self.parent.device

    @property
    def index(self):
        return self.parent.index

    @property
    def index_t(self):
        return self.parent.index_t

    def layer(self, i: int):
        return self.parent._pair(i, self.b0, self.b1)
