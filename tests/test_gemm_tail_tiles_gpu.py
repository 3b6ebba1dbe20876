"""Tail-balanced gemm4 (tile configs 18 / 19, csrc/kernels/gemm.hip gemm4t_kernel): a body of 256 x 192 / 256 x 256
tiles and a tail region of 256 x 128 tiles in one launch. Every output element runs the K order and MFMA sequence of
the uniform gemm4 grids, so the results are bit-identical to tiles 17 / 16 / 14; they are also checked against the fp32
reference at the tolerances tests/test_kernels_gpu.py uses for the same epilogues. The shapes are the smallest at which
the region logic can go wrong: two m-tiles (the second partial), four K-tiles (the three-deep weight ring wraps), and
n_body pinned so that both regions exist whatever the CU count."""
from __future__ import annotations

import pytest
import torch

from jax_llama_amd import ops
from jax_llama_amd.models.weights import PackedLinear
from jax_llama_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
M, K = 300, 256


def _close(a, b, rtol, atol):
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item()
    assert err <= atol + rtol * scale, f"max err {err:.3e} (ref max {scale:.3e})"


# (N, tail-balanced tile, pinned n_body, uniform tiles of the same main loops):
#   448 = one 192 body tile + two 128 tail tiles; 416 = 192 + 128 + a ragged 96-column last tile; 640 = 256 + 3 x 128
@pytest.mark.parametrize("n,tile,n_body,uniform", [(448, 18, 1, (17, 16)), (416, 18, 1, (17, 16)),
                                                   (640, 19, 1, (17, 14))])
def test_tail_tiles_every_epilogue(n, tile, n_body, uniform):
    e = ops.ext()
    torch.manual_seed(n + tile)
    x = torch.randn(M, K).to(BF16)
    w = (torch.randn(n, K) * 0.05).to(BF16)
    gu = ref.interleave_gate_up(w[: n // 2], w[n // 2:])
    pg, gp = PackedLinear.from_dense(w, DEV), PackedLinear.from_dense(gu, DEV)
    xg = x.to(DEV)
    h0 = torch.randn(M, n)
    rw = torch.empty(M, device=DEV)

    def run(t, nb):
        o2 = torch.empty(M, n // 2, dtype=BF16, device=DEV)  # SwiGLU with the fused norm statistic
        e.gemm(xg, gp.weight, n, K, o2, ops.MODE_SWIGLU, True, None, 1, None, 1e-5, t, None, rw, nb)
        ob = torch.empty(M, n, dtype=BF16, device=DEV)
        e.gemm(xg, pg.weight, n, K, ob, ops.MODE_STORE, True, None, 1, None, -1.0, t, None, None, nb)
        o = torch.empty(M, n, dtype=torch.float32, device=DEV)
        e.gemm(xg, pg.weight, n, K, o, ops.MODE_STORE, True, None, 1, None, -1.0, t, None, None, nb)
        hg, mir = h0.to(DEV), torch.empty(M, n, dtype=BF16, device=DEV)  # residual, accumulate = 1, with a mirror
        e.gemm(xg, pg.weight, n, K, hg, ops.MODE_RESIDUAL, True, mir, 1, None, -1.0, t, None, None, nb)
        torch.cuda.synchronize()
        return [o2, ob, o, hg, mir]

    got = run(tile, n_body)
    for t in uniform:
        for i, (a, b) in enumerate(zip(got, run(t, 0))):
            assert torch.equal(a, b), f"output {i}: tile {tile} (n_body {n_body}) differs from tile {t}"
    _close(got[0], ref.linear_swiglu(x, gu, 1e-5), 3e-2, 3e-2)
    _close(got[1], ref.linear(x, w, None, torch.float32), 2e-2, 2e-2)
    _close(got[2], ref.linear(x, w, None, torch.float32), 1e-2, 2e-3)
    _close(got[3], ref.linear_residual(x, w, h0.clone()), 1e-2, 1e-3)
    torch.testing.assert_close(got[4].cpu(), got[3].cpu().to(BF16), rtol=0, atol=0)


def test_tail_split_choice():
    """gemm_tail_split: the Llama-3-8B gate_up grid at M = 2048 (8 m-tiles, N = 28672, 192-wide body, 256 CUs) becomes
    4 whole rounds of body tiles + one round of tail tiles; the regions always cover N exactly; no plan where the
    uniform grid already fills whole rounds."""
    e = ops.ext()
    assert tuple(e.gemm_tail_split(8, 28672, 192, 256)) == (128, 32)
    assert tuple(e.gemm_tail_split(8, 24576, 192, 256)) == (0, 0)  # 1024 tiles = 4 whole rounds
    assert tuple(e.gemm_tail_split(8, 8192, 256, 256)) == (0, 0)   # 256 tiles = one round
    offered = 0
    for tm in (1, 2, 4, 8, 13):
        for width in (192, 256):
            for n in range(160, 30000, 1232):  # (multiples of 16)
                nb, nt = e.gemm_tail_split(tm, n, width, 256)
                if nb == 0:
                    assert nt == 0
                    continue
                offered += 1
                tail = n - nb * width  # the tail's columns: at least one, in nt tiles of 128 (the last may be ragged)
                assert nb > 0 and tail > 0 and (nt - 1) * 128 < tail <= nt * 128, (tm, n, width, nb, nt)
    assert offered > 0


def test_tail_tiles_not_offered_is_an_error():
    """Tiles 18 / 19 without a pinned n_body on a shape whose uniform grid already fills whole rounds: an error, not
    another plan run silently."""
    e = ops.ext()
    n = 192  # one body tile per m-tile: nothing for a tail
    x = torch.randn(M, K).to(BF16).to(DEV)
    pg = PackedLinear.from_dense((torch.randn(n, K) * 0.05).to(BF16), DEV)
    o = torch.empty(M, n, dtype=BF16, device=DEV)
    with pytest.raises(RuntimeError):
        e.gemm(x, pg.weight, n, K, o, ops.MODE_STORE, True, None, 1, None, -1.0, 18)
