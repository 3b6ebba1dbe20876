#!/usr/bin/env python3
"""FP8-weight and MXFP4-weight decode GEMVs against the bf16 decode GEMV (default form, variant 1) at the layer shapes of
a model.

One process, interleaved: per (projection, M) the kernels are captured into one hipGraph each (decode GEMVs run
below the host's launch rate) over weight copies that rotate through more than twice the 256 MiB Infinity Cache, so
every call streams from HBM; the graphs are replayed alternately for ``--rounds`` rounds. One JSON line per point:
microseconds (min and median of the rounds) and effective TB/s of each kernel (its own bytes over its own time), and
bf16 / fp8, bf16 / mxfp4 and fp8 / mxfp4 (> 1: the second is faster).

  python tools/bench_gemv_w8.py [--model llama3-8b] [--m 1 16 64] [--rounds 9] [--formats bf16 fp8 mxfp4]
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
from jax_llama_amd.config import get_preset  # noqa: E402
from jax_llama_amd.models.weights import Fp8Linear, Mxfp4Linear, PackedLinear  # noqa: E402

DEV = "cuda"
BF16 = torch.bfloat16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--m", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--ops", nargs="+", default=None, help="subset of qkv o gate_up down")
    ap.add_argument("--formats", nargs="+", choices=["bf16", "fp8", "mxfp4"], default=["bf16", "fp8", "mxfp4"])
    args = ap.parse_args()
    cfg = get_preset(args.model)
    d, f, hd = cfg.hidden_size, cfg.intermediate_size, cfg.head_dim
    h, hkv = cfg.num_attention_heads, cfg.num_key_value_heads
    shapes = {"qkv": ((h + 2 * hkv) * hd, d, ops.MODE_QKV), "o": (d, h * hd, ops.MODE_RESIDUAL),
              "gate_up": (2 * f, d, ops.MODE_SWIGLU), "down": (d, f, ops.MODE_RESIDUAL)}
    for name, (n, k, mode) in shapes.items():
        if args.ops and name not in args.ops:
            continue
        # the copies of the smallest format alone exceed 2x the Infinity Cache (fp8: 1 byte, mxfp4: 17 / 32 per weight)
        copies = max(2, ((1200 if "mxfp4" in args.formats else 600) << 20) // (n * k) + 1)
        wb = [PackedLinear.random(n, k, DEV) for _ in range(copies)]
        sides = {"bf16": wb}
        if "fp8" in args.formats:
            sides["fp8"] = [Fp8Linear.from_linear(w) for w in wb]
        if "mxfp4" in args.formats:
            sides["mxfp4"] = [Mxfp4Linear.from_linear(w) for w in wb]
        if "bf16" not in args.formats:
            del sides["bf16"]
        nbytes = {"bf16": 2 * n * k, "fp8": n * k + 4 * n, "mxfp4": n * k // 2 + n * k // 32}
        for m in args.m:
            x = torch.randn(m, k, device=DEV).to(BF16)
            if mode == ops.MODE_QKV:
                table = torch.randn(4096, hd // 2, 2, device=DEV)
                pos = torch.zeros(m, dtype=torch.int32, device=DEV)
                kc = torch.zeros(m, hkv, 512, hd, dtype=BF16, device=DEV)
                vc = torch.zeros_like(kc)
                slot = torch.zeros(1, dtype=torch.int32, device=DEV)

                def run(w):
                    ops.linear_qkv_rope(x, w, 1e-5, table, pos, kc, vc, slot, 1, h, hkv, hd)
            elif mode == ops.MODE_RESIDUAL:
                out = torch.zeros(m, n, device=DEV)
                mir = torch.zeros(m, n, dtype=BF16, device=DEV)

                def run(w):
                    ops.linear_residual(x, w, out, mirror=mir)
            else:
                def run(w):
                    ops.linear_swiglu(x, w, rms_eps=1e-5)
            e = ops.ext()
            assert "fp8" not in sides or ops._w8_fast(e, x, sides["fp8"][0], mode), "the fp8 side must run the FP8 GEMV"
            assert "mxfp4" not in sides or ops._w4_fast(e, x, sides["mxfp4"][0], mode), "the MXFP4 GEMV must run"
            ops.GEMV_VARIANT = 1  # the bf16 side: the untouched default form (not the tuner's pick)
            graphs = {}
            for tag, ws in sides.items():
                for i in range(2):
                    run(ws[i])
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    for i in range(2 * copies):
                        run(ws[i % copies])
                graphs[tag] = g
            ops.GEMV_VARIANT = 0
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
            rec = {"op": name, "n": n, "k": k, "m": m, "copies": copies, "rounds": args.rounds}
            for tag in sides:
                t = times[tag]
                rec[f"{tag}_us_min"] = round(min(t), 2)
                rec[f"{tag}_us_median"] = round(statistics.median(t), 2)
                rec[f"{tag}_us_max"] = round(max(t), 2)
                rec[f"{tag}_TBps"] = round(nbytes[tag] / min(t) / 1e6, 3)
            for a, b in (("bf16", "fp8"), ("bf16", "mxfp4"), ("fp8", "mxfp4")):
                if a in sides and b in sides:
                    rec[f"{a}_over_{b}"] = round(rec[f"{a}_us_median"] / rec[f"{b}_us_median"], 3)
            print(json.dumps(rec), flush=True)
            del graphs
        del sides, wb
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
