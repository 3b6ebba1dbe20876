#!/usr/bin/env python
"""The full-vocabulary sampler of this tree against the same kernel of another commit, in one process: both captured
into graphs on the same logits and replayed alternately (median ms with the min..max spread). The other commit's
kernel is a stand-alone library with the launcher it had before min_p / typical_p:

    mkdir other && git show REV:jax_llama_amd/csrc/kernels/nucleus_sample.hip > other/nucleus_sample.hip
    git show REV:jax_llama_amd/csrc/kernels/launchers.h > other/launchers.h
    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -munsafe-fp-atomics -D__HIP_PLATFORM_AMD__ \\
        -Ijax_llama_amd/csrc/kernels -shared other/nucleus_sample.hip -o other/ns.so
    python tools/nucleus_sample_ab.py --other other/ns.so >> profiles/truncation_sample_points.jsonl
"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
OLD_LAUNCHER = "_ZN3jla14nucleus_sampleEPKfiiiddmPKiPiS4_P12ihipStream_t"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True)
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    from jax_llama_amd import ops
    dev = "cuda"
    old = getattr(ctypes.CDLL(args.other, mode=ctypes.RTLD_LOCAL), OLD_LAUNCHER)
    old.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                    ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    step = torch.tensor([7], dtype=torch.int32, device=dev)
    for b in args.batch:
        x = torch.randn(b, args.vocab, device=dev, generator=torch.Generator(dev).manual_seed(b)) * 2
        nxt = torch.empty(b, dtype=torch.int32, device=dev)
        for temperature, top_p in ((0.6, 0.9), (1.0, 1.0)):
            def other():
                rc = old(x.data_ptr(), b, args.vocab, 0, temperature, top_p, 5, step.data_ptr(), nxt.data_ptr(), None,
                         torch.cuda.current_stream().cuda_stream)
                assert rc == 0, rc
                return nxt
            paths = {"other": other, "this": lambda: ops.nucleus_sample(x, 0, temperature, top_p, 5, step)}
            same = bool(torch.equal(paths["other"]().clone(), paths["this"]()))
            graphs = {}
            for name, fn in paths.items():
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
            r = {"ab": "other commit's kernel against this tree's", "batch": b, "vocab": args.vocab,
                 "temperature": temperature, "top_p": top_p, "reps": args.reps, "same_tokens": same}
            for name, t in ms.items():
                r[name + "_ms"] = round(statistics.median(t), 4)
                r[name + "_ms_range"] = [round(min(t), 4), round(max(t), 4)]
            print(json.dumps(r), flush=True)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
