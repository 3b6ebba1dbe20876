#!/usr/bin/env python3
"""The quantised-weight GEMM (``set_quantized_gemm("direct")``, csrc/kernels/gemm5q.h) against the dequant path and the
bf16 GEMM, at the layer shapes of Llama-3-8B and the Llama-3-70B MP 8 shard, for decode batches of 65 .. 512 rows.

One process, interleaved: per (shape, M, format) every contender is captured into one hipGraph over weight copies that
rotate through more than twice the 256 MiB Infinity Cache in every format, and the graphs are replayed alternately
for ``--rounds`` rounds. Contenders: ``dequant`` (the dequant pass + the tuned bf16 plan), ``direct`` (gemm_wq_plan()'s
default plan), ``direct_<tile>_<ksplit>`` for every ``--pinned`` plan, ``bf16`` (the tuned bf16 plan on bf16 weights).
One JSON line per point: min / median / max microseconds of each and the ratios to ``direct`` (> 1: direct is faster).

  python tools/bench_gemm_wq.py [--m 96 128 256 512] [--formats fp8 mxfp4] [--pinned 11:1 12:2 ...] [--ops qkv ...]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from jax_llama_amd import ops  # noqa: E402
from jax_llama_amd.models.weights import Fp8Linear, Mxfp4Linear, PackedLinear  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16
H, HKV, HD = 32, 8, 128  # (the qkv epilogue's heads: Llama-3-8B's; the shard's qkv is timed as a plain store)
# name: (N, K, mode)
SHAPES = {"qkv": (6144, 4096, ops.MODE_QKV), "o": (4096, 4096, ops.MODE_RESIDUAL),
          "gate_up": (28672, 4096, ops.MODE_SWIGLU), "down": (4096, 14336, ops.MODE_RESIDUAL),
          "tp8_qkv": (1280, 8192, ops.MODE_STORE), "tp8_gate_up": (7168, 8192, ops.MODE_SWIGLU)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, nargs="+", default=[96, 128, 256, 512])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--ops", nargs="+", default=None, help=f"subset of {' '.join(SHAPES)}")
    ap.add_argument("--formats", nargs="+", choices=["fp8", "mxfp4"], default=["fp8", "mxfp4"])
    ap.add_argument("--pinned", nargs="*", default=["11:1", "11:2", "11:4", "12:1", "12:2", "12:4"],
                    help="tile:ksplit plans of the direct path to time beside its default")
    args = ap.parse_args()
    pinned = [tuple(int(v) for v in p.split(":")) for p in args.pinned]
    e = ops.ext()
    for name, (n, k, mode) in SHAPES.items():
        if args.ops and name not in args.ops:
            continue
        for fmt in args.formats:
            cls = Fp8Linear if fmt == "fp8" else Mxfp4Linear
            # the copies of the quantised format alone exceed 2x the Infinity Cache
            copies = max(2, ((1200 if fmt == "mxfp4" else 600) << 20) // (n * k) + 1)
            wb = [PackedLinear.random(n, k, DEV) for _ in range(copies)]
            wq = [cls.from_linear(w) for w in wb]
            for m in args.m:
                x = torch.randn(m, k, device=DEV).to(BF16)
                if mode == ops.MODE_QKV:
                    table = torch.randn(4096, HD // 2, 2, device=DEV)
                    pos = torch.zeros(m, dtype=torch.int32, device=DEV)
                    kc = torch.zeros(m, HKV, 64, HD, dtype=BF16, device=DEV)
                    vc = torch.zeros_like(kc)
                    slot = torch.zeros(1, dtype=torch.int32, device=DEV)

                    def run(w):
                        ops.linear_qkv_rope(x, w, 1e-5, table, pos, kc, vc, slot, 1, H, HKV, HD)
                elif mode == ops.MODE_RESIDUAL:
                    out = torch.zeros(m, n, device=DEV)
                    mir = torch.zeros(m, n, dtype=BF16, device=DEV)

                    def run(w):
                        ops.linear_residual(x, w, out, mirror=mir)
                elif mode == ops.MODE_SWIGLU:
                    def run(w):
                        ops.linear_swiglu(x, w, rms_eps=1e-5)
                else:
                    def run(w):
                        ops.linear(x, w, rms_eps=1e-5)
                # contender: (weights, direct?, pinned plan)
                sides = {"dequant": (wq, False, None), "direct": (wq, True, None), "bf16": (wb, False, None)}
                for tile, ks in pinned:
                    sides[f"direct_{tile}_{ks}"] = (wq, True, (tile, ks))
                graphs = {}
                # every contender eagerly first (tunes the bf16 plans, sizes the shared workspaces to their largest), then
                # the captures: no graph is left holding a workspace a later contender outgrew
                for capture in (False, True):
                    for tag, (ws, direct, plan) in sides.items():
                        for w in wq:
                            w.gemm_direct = direct
                        ops.WQ_GEMM_PLAN = plan
                        if not capture:
                            assert not direct or ops._wq_direct(e, x, ws[0], mode,
                                                                None if mode == ops.MODE_RESIDUAL else 1e-5)
                            run(ws[0])
                            torch.cuda.synchronize()
                            continue
                        g = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(g):
                            for i in range(2 * copies):
                                run(ws[i % copies])
                        graphs[tag] = g
                ops.WQ_GEMM_PLAN = None
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                times = {tag: [] for tag in sides}
                for r in range(args.rounds + 1):
                    for tag in sides:
                        ev0.record()
                        graphs[tag].replay()
                        ev1.record()
                        ev1.synchronize()
                        if r:  # (round 0 warms the graphs)
                            times[tag].append(ev0.elapsed_time(ev1) * 1000.0 / (2 * copies))
                rec = {"op": name, "fmt": fmt, "n": n, "k": k, "m": m, "copies": copies, "rounds": args.rounds}
                for tag, t in times.items():
                    rec[f"{tag}_us"] = [round(min(t), 2), round(statistics.median(t), 2), round(max(t), 2)]
                for tag in ("dequant", "bf16"):
                    rec[f"{tag}_over_direct"] = round(rec[f"{tag}_us"][1] / rec["direct_us"][1], 3)
                print(json.dumps(rec), flush=True)
                del graphs
            del wb, wq
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
