#!/usr/bin/env python3
"""One decode latency point (hipGraph-replayed steps, prefill excluded) of a synthetic model; the
unit to run under rocprofv3 for a per-kernel breakdown of small-batch decode.

  python tools/decode_point.py --model llama3-8b --batch 1 32 --steps 64
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--batch", type=int, nargs="+", default=[1])
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--gen-len", type=int, default=256)
    ap.add_argument("--sample", action="store_true")
    ap.add_argument("--tp-proxy", type=int, default=1, help="> 1: ONE rank of that MP degree on this GPU "
                    "(parallel/comm.py TPRankProxyComm; bench.py tp_rank_proxy)")
    ap.add_argument("--weights", nargs="+", choices=["bf16", "fp8", "mxfp4"], default=["bf16"],
                    help="fp8 / mxfp4: the layer projections quantised to FP8 e4m3 / MXFP4 "
                    "(LLaMAForCausalLM.quantize_weights_); `bf16 fp8 mxfp4`: one model of each in this process, "
                    "measured alternately per point")
    ap.add_argument("--kv", nargs="+", choices=["bf16", "fp8"], default=["bf16"],
                    help="KV-cache format (LLaMAForCausalLM.set_kv_cache_format; fp8: e4m3 rows with power-of-two "
                    "scales); `bf16 fp8`: the same model with each, measured alternately per point")
    ap.add_argument("--reps", type=int, default=1, help="repeats of every point (alternating over --weights and --kv)")
    ap.add_argument("--repetition-penalty", type=float, default=1.0)
    ap.add_argument("--no-repeat-ngram", type=int, default=0)
    ap.add_argument("--min-new-tokens", type=int, default=0,
                    help="with any of these three logits-processor settings every point is measured with the "
                    "processors off and on, alternately (record field `processors`)")
    ap.add_argument("--tune-report", action="store_true", help="print the decode-kernel choices and the graph-timed "
                    "microseconds of every candidate measured (ops/autotune.py)")
    args = ap.parse_args()
    import torch
    from jax_llama_amd.config import get_preset
    from jax_llama_amd.models import LLaMAForCausalLM
    from jax_llama_amd.runtime.benchmark import decode_latency
    cfg = get_preset(args.model, max_seq_len=2048)
    comm = None
    if args.tp_proxy > 1:
        from jax_llama_amd.parallel import TPRankProxyComm
        comm = TPRankProxyComm.create(args.tp_proxy, fused_hidden=cfg.hidden_size)
    models = {}
    for wf in args.weights:
        models[wf] = LLaMAForCausalLM(cfg, device="cuda", comm=comm, _do_init=False).init_random(seed=1)
        if wf != "bf16":
            models[wf].quantize_weights_("fp8_e4m3" if wf == "fp8" else "mxfp4")
    procs = [("off", None)]
    if args.repetition_penalty != 1.0 or args.no_repeat_ngram or args.min_new_tokens:
        procs.append(("on", dict(repetition_penalty=args.repetition_penalty, no_repeat_ngram_size=args.no_repeat_ngram,
                                 min_new_tokens=args.min_new_tokens)))
    for b in args.batch:
        for rep in range(args.reps):
            for wf, kv, (pname, proc) in ((wf, kv, pr) for wf in models for kv in args.kv for pr in procs):
                m = models[wf]
                m.set_kv_cache_format("fp8_e4m3" if kv == "fp8" else "bf16")
                r = decode_latency(m, b, args.prompt_len, args.gen_len, steps=args.steps, do_sample=args.sample,
                                   processors=proc)
                r["processors"] = pname
                r["model"] = args.model
                r["mp"] = args.tp_proxy
                r["weights"] = wf
                r["kv"] = kv
                r["kv_cache_gb"] = round(m.config.num_hidden_layers * 2 * b * m.n_kv_heads *
                                         (args.prompt_len + args.gen_len) *
                                         (m.head_dim + 4 if kv == "fp8" else 2 * m.head_dim) / 1e9, 2)
                r["rep"] = rep
                r["fused_row_parallel"] = comm is not None and comm.fused is not None
                r["hbm_roofline_ms"] = round(m.streamed_weight_bytes_per_token() / 6.29e12 * 1e3, 4)
                print(json.dumps(r), flush=True)
                torch.cuda.empty_cache()
    if args.tune_report:
        from jax_llama_amd.ops import autotune
        for (m, n, k, _), t in autotune.measured().items():
            print(json.dumps({"tune": "gemv", "m": m, "n": n, "k": k, "us": t, "best": min(t, key=t.get)}), flush=True)


if __name__ == "__main__":
    main()
