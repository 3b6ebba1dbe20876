#!/usr/bin/env python3
"""Beam-search decode points on a synthetic model, one JSON line each:

  * ``beam_decode``: ms per hipGraph-replayed step of a beam search (``--batch`` prompts x ``--beams``) against greedy
    decoding of the same number of cache rows (``batch * beams``), in one process, alternating, prefill excluded;
  * ``kv_beam_reorder``: the cache reorder alone at the model's cache shape with ``--slots`` valid slots, for an
    all-identity ``beam_idx`` (every group skipped) and a rotation (every row moves): time per call (all launches of
    one step: 2 for a bf16 cache, 4 for FP8) and GB/s over the bytes read plus written, counted from the shapes.

  python tools/beam_point.py --model llama3-8b --batch 4 --beams 4 --steps 64 --slots 160 8192
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def beam_latency(model, batch, beams, prompt_len, gen_len, steps):
    import torch
    from jax_llama_amd.runtime.benchmark import synthetic_prompts
    from jax_llama_amd.runtime.engine import BeamEngine, GenerationConfig
    max_len = prompt_len + gen_len
    eng = BeamEngine(model, batch, beams, max_len, use_graph=True)
    eng.gc = GenerationConfig(max_length=max_len, num_beams=beams, pad_token_id=0, eos_token_id=-1)
    prompts = synthetic_prompts(model.config.vocab_size, batch, prompt_len, 0)
    eng.prefill(prompts, None)
    eng._decode_step()  # eager: sizes the workspaces before capture
    eng._ensure_graph()
    eng._graph.replay()
    eng.prefill(prompts, None)
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(steps):
        eng._graph.replay()
    ev1.record()
    torch.cuda.synchronize()
    assert int(eng.alive.item()) == 1 and int(eng.cur_len.item()) == prompt_len + 1 + steps
    return ev0.elapsed_time(ev1) / steps


def reorder_points(cfg, n_kv_heads, head_dim, rows, beams, slots, kv):
    import torch
    from jax_llama_amd import ops
    from jax_llama_amd.models.kv_cache import KVCache, kv_row_bytes
    fmt = "fp8_e4m3" if kv == "fp8" else "bf16"
    t = max(slots) + 64
    cache = KVCache(cfg.num_hidden_layers, rows, n_kv_heads, t, head_dim, "cuda", kv_format=fmt)
    for x in ops.kv_beam_tensors(cache):
        x.view(torch.uint8).random_(0, 120)
    ident = torch.arange(beams, dtype=torch.int32, device="cuda").repeat(rows // beams)
    rot = ((torch.arange(beams, dtype=torch.int32, device="cuda") + 1) % beams).repeat(rows // beams)
    out = []
    for n in slots:
        cache.index_t.fill_(n)
        moved = 2 * 2 * cfg.num_hidden_layers * rows * n_kv_heads * n * kv_row_bytes(fmt, head_dim)  # read + written
        for name, idx in (("identity", ident), ("rotation", rot)):
            iters = 200 if name == "identity" or n < 1024 else 20
            for _ in range(3):
                ops.kv_beam_reorder(cache, idx, beams)
            torch.cuda.synchronize()
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(iters):
                ops.kv_beam_reorder(cache, idx, beams)
            ev1.record()
            torch.cuda.synchronize()
            ms = ev0.elapsed_time(ev1) / iters
            nbytes = moved if name == "rotation" else 0
            out.append({"what": "kv_beam_reorder", "kv": kv, "rows": rows, "beams": beams, "slots": n,
                        "cache_slots": t, "beam_idx": name, "iters": iters, "ms_per_call": round(ms, 4),
                        "bytes_moved": nbytes, "gb_per_s": round(nbytes / ms / 1e6, 1)})
    del cache
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--prompt-len", type=int, default=128)
    ap.add_argument("--gen-len", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slots", type=int, nargs="*", default=[160, 8192])
    ap.add_argument("--kv", nargs="+", choices=["bf16", "fp8"], default=["bf16"])
    args = ap.parse_args()
    import torch
    from jax_llama_amd.config import get_preset
    from jax_llama_amd.models import LLaMAForCausalLM
    from jax_llama_amd.runtime.benchmark import decode_latency
    if not torch.cuda.is_available():
        raise SystemExit("beam_point.py measures on the GPU: none found")
    cfg = get_preset(args.model, max_seq_len=2048)
    model = LLaMAForCausalLM(cfg, device="cuda", _do_init=False).init_random(seed=1)
    rows = args.batch * args.beams
    for kv in args.kv:
        model.set_kv_cache_format("fp8_e4m3" if kv == "fp8" else "bf16")
        for rep in range(args.reps):
            g = decode_latency(model, rows, args.prompt_len, args.gen_len, steps=args.steps)
            b = beam_latency(model, args.batch, args.beams, args.prompt_len, args.gen_len, args.steps)
            print(json.dumps({"what": "beam_decode", "model": args.model, "kv": kv, "rep": rep, "batch": args.batch,
                              "beams": args.beams, "prompt_len": args.prompt_len, "steps": args.steps,
                              "beam_ms_per_step": round(b, 4), "greedy_rows": rows,
                              "greedy_ms_per_step": g["decode_ms_per_token"],
                              "beam_over_greedy": round(b / g["decode_ms_per_token"], 4)}), flush=True)
            torch.cuda.empty_cache()
    heads, hd = model.n_kv_heads, model.head_dim
    for kv in args.kv:
        if args.slots:
            for r in reorder_points(cfg, heads, hd, rows, args.beams, args.slots, kv):
                r["model"] = args.model
                print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
