#!/usr/bin/env python3
"""One decode latency point (hipGraph-replayed steps, prefill excluded) of a synthetic model; the
unit to run under rocprofv3 for a per-kernel breakdown of small-batch decode.

  python tools/decode_point.py --model llama3-8b --batch 1 32 --steps 64

JLA_ATTN_Q8_WAVES=1 / 8 / 2 / 4 in the environment pins the form of the fp8 KV cache's decode attention for the whole
process (2 / 4: the matrix-core form; csrc/kernels/attn_plan.h); the records carry it as `q8_waves`.
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
    ap.add_argument("--top-k", type=int, default=50, help="with --sample: 0 = no top-k cut (the full-vocabulary sampler)")
    ap.add_argument("--top-p", type=float, default=0.95)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--tp-proxy", type=int, default=1, help="> 1: ONE rank of that MP degree on this GPU "
                    "(parallel/comm.py TPRankProxyComm; bench.py tp_rank_proxy)")
    ap.add_argument("--weights", nargs="+", choices=["bf16", "fp8", "mxfp4"], default=["bf16"],
                    help="fp8 / mxfp4: the layer projections quantised to FP8 e4m3 / MXFP4 "
                    "(LLaMAForCausalLM.quantize_weights_); `bf16 fp8 mxfp4`: one model of each in this process, "
                    "measured alternately per point")
    ap.add_argument("--quantized-gemm", nargs="+", choices=["dequant", "direct"], default=["dequant"],
                    help="quantised weights above 64 rows: the dequant pass + bf16 GEMM, or the GEMM on the quantised "
                    "bytes (LLaMAForCausalLM.set_quantized_gemm); both: every quantised point under each")
    ap.add_argument("--kv", nargs="+", choices=["bf16", "fp8"], default=["bf16"],
                    help="KV-cache format (LLaMAForCausalLM.set_kv_cache_format; fp8: e4m3 rows with power-of-two "
                    "scales); `bf16 fp8`: the same model with each, measured alternately per point")
    ap.add_argument("--reps", type=int, default=1, help="repeats of every point (alternating over --weights and --kv)")
    ap.add_argument("--repetition-penalty", type=float, default=1.0)
    ap.add_argument("--no-repeat-ngram", type=int, default=0)
    ap.add_argument("--min-new-tokens", type=int, default=0,
                    help="with any of these three logits-processor settings every point is measured with the "
                    "processors off and on, alternately (record field `processors`)")
    ap.add_argument("--min-p", type=float, default=0.0, help="with --sample: every point with min_p off and on, "
                    "alternately (record field `min_p`; on, every top_k runs the full-vocabulary sampler)")
    ap.add_argument("--prompt-lookup", type=int, default=0, metavar="K",
                    help="K > 0: after every plain point, the same model with prompt-lookup decoding "
                    "(prompt_lookup_num_tokens = K; runtime/benchmark.py lookup_latency) on a prompt that repeats a "
                    "16-token period and on a random one: ms per verify step, tokens per step, ms per token")
    ap.add_argument("--tune-report", action="store_true", help="print the decode-kernel choices and the graph-timed "
                    "microseconds of every candidate measured (ops/autotune.py)")
    args = ap.parse_args()
    import torch
    from jax_llama_amd.config import get_preset
    from jax_llama_amd.models import LLaMAForCausalLM
    from jax_llama_amd.runtime.benchmark import decode_latency, lookup_latency
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
            for wf, qg, kv, (pname, proc), min_p in ((wf, qg, kv, pr, mp) for wf in models
                                                     for qg in (args.quantized_gemm if wf != "bf16" else ["dequant"])
                                                     for kv in args.kv for pr in procs
                                                     for mp in dict.fromkeys((0.0, args.min_p))):
                m = models[wf]
                if wf != "bf16":
                    m.set_quantized_gemm(qg)
                m.set_kv_cache_format("fp8_e4m3" if kv == "fp8" else "bf16")
                r = decode_latency(m, b, args.prompt_len, args.gen_len, steps=args.steps, do_sample=args.sample,
                                   processors=proc,
                                   sampler=dict(top_k=args.top_k, top_p=args.top_p, temperature=args.temperature,
                                                min_p=min_p))
                r["top_k"], r["top_p"], r["temperature"] = args.top_k, args.top_p, args.temperature
                r["processors"] = pname
                r["min_p"] = min_p
                r["model"] = args.model
                r["mp"] = args.tp_proxy
                r["weights"] = wf
                r["quantized_gemm"] = qg
                r["kv"] = kv
                r["q8_waves"] = int(os.environ.get("JLA_ATTN_Q8_WAVES", "0")) if kv == "fp8" else None
                r["kv_cache_gb"] = round(m.config.num_hidden_layers * 2 * b * m.n_kv_heads *
                                         (args.prompt_len + args.gen_len) *
                                         (m.head_dim + 4 if kv == "fp8" else 2 * m.head_dim) / 1e9, 2)
                r["rep"] = rep
                r["fused_row_parallel"] = comm is not None and comm.fused is not None
                r["hbm_roofline_ms"] = round(m.streamed_weight_bytes_per_token() / 6.29e12 * 1e3, 4)
                print(json.dumps(r), flush=True)
                torch.cuda.empty_cache()
                if args.prompt_lookup > 0 and not args.sample and proc is None and args.tp_proxy == 1:
                    for period in (16, 0):
                        lr = lookup_latency(m, b, args.prompt_len, min(args.steps, 32), args.prompt_lookup,
                                            period=period)
                        lr.update(model=args.model, weights=wf, kv=kv, rep=rep, plain_ms_per_token=r["decode_ms_per_token"])
                        print(json.dumps(lr), flush=True)
                        torch.cuda.empty_cache()
    if args.tune_report:
        from jax_llama_amd.ops import autotune
        for (m, n, k, _), t in autotune.measured().items():
            print(json.dumps({"tune": "gemv", "m": m, "n": n, "k": k, "us": t, "best": min(t, key=t.get)}), flush=True)


if __name__ == "__main__":
    main()
