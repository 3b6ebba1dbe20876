#!/usr/bin/env python
"""The full-vocabulary sampler's truncation rules against each other, in the method of nucleus_sample_point.py: each
setting captured into a graph, the graphs replayed alternately in one process, median ms with the min..max spread.
Settings: top_p = 0.9 alone (the kernel as it was), min_p = 0.05 alone, typical_p = 0.9 alone, all of them with
top_k = 100. One JSON line per batch.

    python tools/truncation_sample_point.py --batch 1 32 256 >> profiles/truncation_sample_points.jsonl
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SETTINGS = {"top_p": (0, 0.9, 0.0, 1.0), "min_p": (0, 1.0, 0.05, 1.0), "typical_p": (0, 1.0, 0.0, 0.9),
            "all": (100, 0.9, 0.05, 0.9)}  # (top_k, top_p, min_p, typical_p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--temperature", type=float, default=0.6)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from jax_llama_amd import ops
    dev = "cuda"
    step = torch.tensor([7], dtype=torch.int32, device=dev)
    for b in args.batch:
        x = torch.randn(b, args.vocab, device=dev, generator=torch.Generator(dev).manual_seed(b)) * 2
        graphs, kept = {}, {}
        for name, (top_k, top_p, min_p, typical_p) in SETTINGS.items():
            def fn():
                return ops.nucleus_sample(x, top_k, args.temperature, top_p, 5, step, return_kept=True, min_p=min_p,
                                          typical_p=typical_p)
            kept[name] = round(float(fn()[1].float().mean()), 1)  # (eager first)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            g.replay()
            graphs[name] = g
        torch.cuda.synchronize()
        ms = {name: [] for name in graphs}
        for _ in range(args.reps):
            for name, g in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                g.replay()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        r = {"batch": b, "vocab": args.vocab, "temperature": args.temperature, "reps": args.reps,
             "settings": SETTINGS, "mean_kept": kept}
        for name, t in ms.items():
            r[name + "_ms"] = round(statistics.median(t), 4)
            r[name + "_ms_range"] = [round(min(t), 4), round(max(t), 4)]
        print(json.dumps(r), flush=True)
        del graphs, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
