#!/usr/bin/env python3
"""Decode attention latency as a decode step sees it: hipGraph-replayed, K/V cold (a 512 MiB fill between calls
evicts L2 and the Infinity Cache, as the weight stream of a real step does). Time per call = (graph of R x
[fill, attention]) - (graph of R x [fill]) over R, min over rounds; impls interleaved in one process.

  python tools/bench_attn_decode.py --model llama3-70b --tp 8 --shapes 1x192 1x384 32x384 --impls 2 5

impl (ext.attn_set_impl / attn_set_v3_max_pairs): 2 = default dispatch; 3 = v3 (one workgroup per pair) forced;
5 = split small-batch kernel (v5) where it applies; 6 = v5 with the first merge (4 splits per load round);
7 = v4 (register ring, one split) forced; 9 = v2 (LDS-DMA ring, KPG 4, 2 slots) forced; 60 = v6 (matrix cores),
61 / 62 / 64 / 68 = v6 with 1 / 2 / 4 / 8 waves per (row, kv head) pair. Prints one JSON line per (shape, impl).

  python tools/bench_attn_decode.py --shapes 64x384 2048x384 --impls 2 --kv bf16 fp8 --q8-waves 0 1 8

--kv fp8: the FP8 (e4m3) KV cache's kernel (csrc/kernels/kv8.hip) on a cache of random codes, beside the bf16 kernels on
the bf16 cache that holds the same (dequantised) values, alternating in one process; --q8-waves pins its waves per pair
(0: the plan's choice) and --q8-splits its key splits per pair (0: the plan's choice, 1: never split, n: pinned; the
plan's resulting count goes into the record as q8_splits, the pinned value as q8_splits_pin); every (waves, splits)
combination is one run. Every record carries the median and the minimum over the rounds and GB/s (the valid K / V bytes
of the format, scales included, over the median).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from jax_llama_amd import ops  # noqa: E402
from jax_llama_amd.config import get_preset  # noqa: E402


def set_impl(e, impl):
    e.attn_reset_knobs()
    # 60: the MFMA kernel (v6) with its default waves per pair; 61 / 62 / 64 / 68: v6 with 1 / 2 / 4 / 8 waves per pair
    # 600 + d: v6 at 2 waves per pair with ablation d (attn_set_v6_diag: 1 no compute, 2 no K loads, 4 no V DMAs)
    e.attn_set_v6_diag(impl - 600 if 601 <= impl <= 607 else 0)
    if 601 <= impl <= 607:
        impl = 62
    e.attn_set_v6(2 if 60 <= impl <= 68 else 0)
    e.attn_set_v6_wpp(impl - 60 if 61 <= impl <= 68 else 0)
    if impl in (7, 9):
        # the streaming kernels at any pair count, one split: 7 = v4 register ring, 9 = v2 (LDS-DMA ring)
        e.attn_set_impl(4 if impl == 9 else 2, 1)  # waves target 1 -> one split
        e.attn_set_impl(4 if impl == 9 else 2, -1)  # v2/v4 down to 1 pair
        e.attn_set_v3_max_pairs(0)
    e.attn_set_v5_max_pairs(4096 if impl in (5, 6) else (0 if impl in (3, 7, 9) else -1))
    e.attn_set_v5_fold(4 if impl == 6 else (12 if impl == 5 else 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--tp", type=int, default=1)
    ap.add_argument("--shapes", nargs="+", default=["1x192", "1x384", "8x384", "32x384"], help="BxT (T = valid keys)")
    ap.add_argument("--cache-len", type=int, default=0, help="cache length (default: T)")
    ap.add_argument("--impls", type=int, nargs="+", default=[2, 1])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kv", nargs="+", choices=["bf16", "fp8"], default=["bf16"])
    ap.add_argument("--q8-waves", type=int, nargs="+", default=[0], help="fp8: waves per pair pinned (0: by shape)")
    ap.add_argument("--q8-splits", type=int, nargs="+", default=[0],
                    help="fp8: key splits per pair pinned (0: by shape, 1: never)")
    args = ap.parse_args()
    e = ops.ext()
    cfg = get_preset(args.model)
    h, hkv, hd = cfg.num_attention_heads // args.tp, cfg.num_key_value_heads // args.tp, cfg.head_dim
    flush = torch.empty(512 << 18, dtype=torch.int32, device="cuda")  # 512 MiB
    for shape in args.shapes:
        b, t = (int(v) for v in shape.split("x"))
        tc = max(args.cache_len, t)
        g = torch.Generator(device="cuda").manual_seed(b * 7 + t)
        k8 = v8 = None
        if "fp8" in args.kv:
            # random finite e4m3 codes (0x7F / 0xFF are NaN) at row scales 2^-9 .. 2^-7; the bf16 caches hold q * scale
            def codes():
                c = torch.randint(0, 0x7F, (b, hkv, tc, hd), device="cuda", generator=g, dtype=torch.uint8)
                return c + 0x80 * torch.randint(0, 2, c.shape, device="cuda", generator=g, dtype=torch.uint8)

            def scales():
                return 2.0 ** torch.randint(-9, -6, (b, hkv, tc), device="cuda", generator=g).float()

            k8, v8 = ops.Fp8KV(codes(), scales()), ops.Fp8KV(codes(), scales())
            kc, vc = ops.kv8_dequant(k8, v8)
        else:
            kc = torch.randn(b, hkv, tc, hd, device="cuda", generator=g).to(torch.bfloat16)
            vc = torch.randn(b, hkv, tc, hd, device="cuda", generator=g).to(torch.bfloat16)
        q = torch.randn(b, 1, h, hd, device="cuda", generator=g).to(torch.bfloat16)
        slot = torch.tensor([t - 1], dtype=torch.int32, device="cuda")
        ks = torch.zeros(b, dtype=torch.int32, device="cuda")
        res, first = {}, None
        graphs = {}
        runs = [("bf16", i) for i in args.impls if "bf16" in args.kv]
        runs += [("fp8", w, n) for w in args.q8_waves for n in args.q8_splits if k8]

        def pin(run):
            set_impl(e, run[1] if run[0] == "bf16" else 2)
            if run[0] == "fp8":
                e.attn_set_q8_waves(run[1])
                e.attn_set_q8_splits(run[2])
            return (kc, vc) if run[0] == "bf16" else (k8, v8)

        # every run once before the first capture: the workspaces (grow-only) reach the size of the largest run, so no
        # later run reallocates a buffer whose address an earlier run's graph has recorded
        for run in runs:
            ck, cv = pin(run)
            ops.attention(q, ck, cv, slot, ks)
        torch.cuda.synchronize()
        ws_generation = ops.workspace.generation
        for run in runs:
            kv, impl = run[:2]
            ck, cv = pin(run)
            out = ops.attention(q, ck, cv, slot, ks)
            torch.cuda.synchronize()
            first = out.float() if first is None else first
            diff = float((out.float() - first).abs().max())
            ga, gf = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(ga):
                for _ in range(args.reps):
                    flush.fill_(1)
                    ops.attention(q, ck, cv, slot, ks)
            with torch.cuda.graph(gf):
                for _ in range(args.reps):
                    flush.fill_(1)
            waves = e.attn_decode_q8_plan_check(b, h, hkv, hd, tc, False)[2] if kv == "fp8" else None
            nsplit = e.attn_decode_q8_split_check(b, h, hkv, hd, tc, False)[2] if kv == "fp8" else None
            graphs[run] = (ga, gf, diff, waves, nsplit)
        e.attn_set_v6_diag(0)
        e.attn_reset_knobs()
        assert ops.workspace.generation == ws_generation, "a workspace moved after a graph recorded its address"
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = {run: [] for run in runs}
        for _ in range(args.rounds):
            for run in runs:
                ga, gf = graphs[run][:2]
                tt = []
                for gr in (ga, gf):
                    gr.replay()
                    ev0.record()
                    gr.replay()
                    ev1.record()
                    ev1.synchronize()
                    tt.append(ev0.elapsed_time(ev1))
                times[run].append((tt[0] - tt[1]) * 1000.0 / args.reps)
        for run in runs:
            kv, impl = run[:2]
            ts = sorted(times[run])
            med = ts[len(ts) // 2]
            nbytes = b * hkv * t * 2 * (hd + 4 if kv == "fp8" else 2 * hd)  # the valid K and V rows of the format
            res = {"op": "attn_decode_graph", "model": args.model, "tp": args.tp, "b": b, "t": t, "cache_len": tc,
                   "kv": kv, "impl": impl if kv == "bf16" else None, "q8_waves": graphs[run][3],
                   "q8_splits": graphs[run][4], "q8_splits_pin": run[2] if kv == "fp8" else None,
                   "us": round(ts[0], 2), "us_median": round(med, 2), "kv_bytes": nbytes,
                   "us_max": round(ts[-1], 2),
                   "gbps": round(nbytes / med / 1e3, 1), "max_diff_vs_first": round(graphs[run][2], 5)}
            print(json.dumps(res), flush=True)
        del graphs, kc, vc, k8, v8


if __name__ == "__main__":
    main()
