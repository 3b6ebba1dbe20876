#!/usr/bin/env python3
"""Scoring lm_head: the GEMM with the log-sum-exp in its epilogue against the ways around it, at one Llama-3-8B prefill
chunk (M = 32768, N = 128256, K = 4096, fused final norm).

  a  fused      ops.linear_logprob: gemm_logprob (MODE_LOGPROB epilogue + lse_partials_kernel); no logits in HBM
  b  unfused    ops.linear (fp32 logits, 16.8 GB at the full shape) + ops.logprob (logprob_rows_kernel) -- the only way
                to these numbers without the fused form
  c  argmax     ops.linear_argmax: gemm_argmax, the greedy epilogue on the same main loop
  d  store      ops.linear with the plain bf16 MODE_STORE epilogue

The four alternate within one process, round by round; every variant is warmed up (which also settles the tuned plan
of b and d); device events time `--iters` back-to-back calls. Prints one JSON line: the median over the rounds in
microseconds per call and the (min, max) spread of each variant, plus a vs b agreement of the result.
Usage: python tools/bench_logprob.py [--m 32768 --n 128256 --k 4096] [--rounds 5] [--iters 3]
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
from jax_llama_amd.models.weights import PackedLinear  # noqa: E402

DEV = "cuda"
EPS = 1e-5


def timed(fn, iters):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(iters):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1000.0 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=32768)
    ap.add_argument("--n", type=int, default=128256)
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    m, n, k = args.m, args.n, args.k
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(m, k, device=DEV, generator=g).to(torch.bfloat16)
    w = PackedLinear.from_dense((torch.randn(n, k, device=DEV, generator=g) * 0.02).to(torch.bfloat16), DEV)
    tg = torch.randint(0, n, (m,), device=DEV, generator=g, dtype=torch.int32)
    logits = torch.empty(m, n, dtype=torch.float32, device=DEV)
    out_bf16 = torch.empty(m, n, dtype=torch.bfloat16, device=DEV)
    assert ops.logprob_fused(x, w, EPS), "no fused plan for this shape: variant a would time the unfused form"
    last = {}

    def fused():
        last["a"] = ops.linear_logprob(x, w, tg, rms_eps=EPS)

    def unfused():
        ops.linear(x, w, EPS, out_dtype=torch.float32, out=logits)
        last["b"] = ops.logprob(logits, tg)

    variants = {"a_fused_logprob": fused, "b_linear_f32_plus_logprob": unfused,
                "c_gemm_argmax": lambda: ops.linear_argmax(x, w, rms_eps=EPS),
                "d_store_bf16": lambda: ops.linear(x, w, EPS, out=out_bf16)}
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn, args.iters))
    lse = [(t[1].double() + t[2].double().log()) for t in (last["a"], last["b"])]
    print(json.dumps({
        "tool": "bench_logprob", "m": m, "n": n, "k": k, "rms_eps": EPS, "rounds": args.rounds, "iters": args.iters,
        "us": {name: round(statistics.median(v), 1) for name, v in times.items()},
        "spread_us": {name: [round(min(v), 1), round(max(v), 1)] for name, v in times.items()},
        "logits_bytes_fp32": m * n * 4,
        "a_vs_b_max_lse_diff": float((lse[0] - lse[1]).abs().max()),
        "a_vs_b_tgt_equal": bool(torch.equal(last["a"][0], last["b"][0]))}), flush=True)


if __name__ == "__main__":
    main()
