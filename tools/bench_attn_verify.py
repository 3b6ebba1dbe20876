#!/usr/bin/env python3
"""The few-query decode attention (csrc/kernels/attn_verify.hip) against attn_prefill on the same launch, as a verify
step sees it: hipGraph-replayed, K/V cold (a 512 MiB fill between calls, its time subtracted by a fill-only graph), the
two graphs replayed alternately in one process, medians over the rounds. One JSON record per (shape, kernel).

  python tools/bench_attn_verify.py --batch 1 8 --s 4 8 --ctx 512 4096 32768 --rounds 9 [--splits 0 1 8 ...]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--s", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--ctx", type=int, nargs="+", default=[512, 4096, 32768])
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv-heads", type=int, default=8)
    ap.add_argument("--splits", type=int, nargs="+", default=[0], help="attn_set_verify_splits values (0: the plan's)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=4)
    args = ap.parse_args()
    import torch
    from jax_llama_amd import ops
    e = ops.ext()
    h, hkv, dh = args.heads, args.kv_heads, 128
    flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    for b in args.batch:
        for t in args.ctx:
            kc = (torch.randn(b, hkv, t, dh, device="cuda") * 0.5).to(torch.bfloat16)
            vc = torch.randn(b, hkv, t, dh, device="cuda").to(torch.bfloat16)
            ks = torch.zeros(b, dtype=torch.int32, device="cuda")
            for s in args.s:
                q = torch.randn(b, s, h, dh, device="cuda").to(torch.bfloat16)
                slot = torch.tensor([t - s], dtype=torch.int32, device="cuda")
                runs = [("prefill", 0)] + [("verify", n) for n in args.splits]

                def call(run):
                    e.attn_set_verify_splits(run[1])
                    return ops.attention(q, kc, vc, slot, ks, few_query=run[0] == "verify")

                for run in runs:  # the workspaces reach their largest size before the first capture
                    call(run)
                torch.cuda.synchronize()
                gen = ops.workspace.generation
                want = call(runs[0]).float()
                graphs = {}
                gf = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gf):
                    for _ in range(args.reps):
                        flush.fill_(1)
                for run in runs:
                    diff = float((call(run).float() - want).abs().max())
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        for _ in range(args.reps):
                            flush.fill_(1)
                            call(run)
                    graphs[run] = (g, diff, e.attn_verify_plan_check(b, s, h, hkv, dh, t)[3])
                e.attn_set_verify_splits(0)
                assert ops.workspace.generation == gen, "a workspace moved after a graph recorded its address"
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

                def timed(g):
                    g.replay()
                    ev0.record()
                    g.replay()
                    ev1.record()
                    ev1.synchronize()
                    return ev0.elapsed_time(ev1)

                times = {run: [] for run in runs}
                for _ in range(args.rounds):
                    for run in runs:
                        times[run].append((timed(graphs[run][0]) - timed(gf)) * 1000.0 / args.reps)
                for run in runs:
                    ts = sorted(times[run])
                    print(json.dumps({"op": "attn_verify_ab", "b": b, "s": s, "ctx": t, "h": h, "hkv": hkv,
                                      "kernel": run[0], "splits_pin": run[1] if run[0] == "verify" else None,
                                      "nsplit": graphs[run][2] if run[0] == "verify" else None,
                                      "us_median": round(ts[len(ts) // 2], 2), "us_min": round(ts[0], 2),
                                      "us_max": round(ts[-1], 2), "rounds": args.rounds,
                                      "max_diff_vs_prefill": round(graphs[run][1], 5)}), flush=True)
                del graphs
            del kc, vc


if __name__ == "__main__":
    main()
