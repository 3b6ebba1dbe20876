#!/usr/bin/env python3
"""Prefill attention throughput (causal, GQA) at real model shapes: TFLOP/s of impl 2 (the default dispatch of the
GQA-shared 32x32x16 MFMA flash kernel, 32 queries per wave), 7 / 8 (pipelined / unpipelined, 4 waves), 9 / 13
(pipelined, 8 waves; 13 with asm LDS-DMA and interleaved next-tile scores) and impl 1 (v1). FLOPs counted for the causal triangle only:
4 * B * H * Dh * S (S + 1) / 2. Prints one JSON line per (shape, impl)."""
from __future__ import annotations

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from jax_llama_amd import ops  # noqa: E402

SHAPES = [  # (name, B, S, H, Hkv)
    ("8b_b1_s2048", 1, 2048, 32, 8), ("8b_b16_s2048", 16, 2048, 32, 8), ("8b_b1_s8192", 1, 8192, 32, 8),
    ("8b_b2048_s128", 2048, 128, 32, 8), ("70b_b1_s2048", 1, 2048, 64, 8), ("7b_b16_s2048", 16, 2048, 32, 32),
]


KV_SHAPES = [  # (name, B, S, H, Hkv, slot0, T, slot on the device)
    ("8b_b1_s2048", 1, 2048, 32, 8, 0, 2048, False), ("8b_b16_s2048", 16, 2048, 32, 8, 0, 2048, False),
    ("8b_b1_s8192", 1, 8192, 32, 8, 0, 8192, False),
    ("8b_b1_s512_at7680", 1, 512, 32, 8, 7680, 8192, False), ("8b_b8_s128_at8064", 8, 128, 32, 8, 8064, 8192, False),
    ("8b_b32_s8_at4096", 32, 8, 32, 8, 4096, 8192, False),
    ("8b_b1_s512_at7680_dev", 1, 512, 32, 8, 7680, 8192, True), ("8b_b8_s128_at8064_dev", 8, 128, 32, 8, 8064, 8192, True),
    ("8b_b32_s8_at4096_dev", 32, 8, 32, 8, 4096, 8192, True),
    ("70b_mp8_b1_s2048", 1, 2048, 8, 1, 0, 2048, False),
    # a prompt in a cache much longer than it, device-side slot: the dequant pass converts all of T
    ("8b_b1_s2048_T8192_dev", 1, 2048, 32, 8, 0, 8192, True), ("8b_b1_s2048_T32768_dev", 1, 2048, 32, 8, 0, 32768, True),
    ("8b_b1_s512_T8192_dev", 1, 512, 32, 8, 0, 8192, True), ("8b_b16_s2048_T8192_dev", 16, 2048, 32, 8, 0, 8192, True),
    ("8b_b4_s512_T32768_dev", 4, 512, 32, 8, 0, 32768, True),
    # ... and the same chunk at the end of that cache: the host cannot tell the two apart
    ("8b_b4_s512_at32256_T32768_dev", 4, 512, 32, 8, 32256, 32768, True),
    ("8b_b1_s2048_at30720_T32768_dev", 1, 2048, 32, 8, 30720, 32768, True),
]


def kv_ab(args):
    """``--kv bf16 fp8``: per shape the bf16 kernel on a bf16 cache ("bf16"), the dequant pass + the bf16 kernel on the
    scratch ("dequant") and the direct launch on the fp8 bytes ("direct"), interleaved in one process, the median of
    ``--rounds`` rounds of 5 launches each. One JSON line per shape (us)."""
    import statistics
    e = ops.ext()
    for name, b, s, h, hkv, slot0, t, on_dev in KV_SHAPES:
        if (args.shape and name != args.shape) or (args.match and args.match not in name):
            continue
        g = torch.Generator(device="cuda").manual_seed(0)
        rnd = lambda: ops.Fp8KV(  # noqa: E731  random finite codes (no 0x7f), scales 2^-8 .. 2^-5
            torch.randint(0, 0x7F, (b, hkv, t, 128), device="cuda", generator=g, dtype=torch.uint8)
            + 0x80 * torch.randint(0, 2, (b, hkv, t, 128), device="cuda", generator=g, dtype=torch.uint8),
            2.0 ** torch.randint(-8, -4, (b, hkv, t), device="cuda", generator=g).float())
        k8v, v8v = rnd(), rnd()
        kc, vc = ops.kv8_dequant(k8v, v8v)
        q = torch.randn(b, s, h, 128, device="cuda", generator=g).to(torch.bfloat16)
        ks = torch.zeros(b, dtype=torch.int32, device="cuda")
        slot = torch.tensor([slot0], dtype=torch.int32, device="cuda") if on_dev else slot0
        runs = {"bf16": (-1, kc, vc), "dequant": (0, k8v, v8v), "direct": (1, k8v, v8v)}
        outs, times = {}, {k: [] for k in runs}
        for key, (mode, kk, vv) in runs.items():  # warm-up + bits
            e.attn_set_q8_prefill(mode)
            outs[key] = ops.attention(q, kk, vv, slot, ks).clone()
        torch.cuda.synchronize()
        same = bool(torch.equal(outs["bf16"], outs["direct"]) and torch.equal(outs["dequant"], outs["direct"]))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(args.rounds):
            for key, (mode, kk, vv) in runs.items():
                e.attn_set_q8_prefill(mode)
                ev[0].record()
                for _ in range(5):
                    ops.attention(q, kk, vv, slot, ks)
                ev[1].record()
                torch.cuda.synchronize()
                times[key].append(ev[0].elapsed_time(ev[1]) * 1000 / 5)
        e.attn_set_q8_prefill(-1)
        rec = {"shape": name, "B": b, "S": s, "H": h, "Hkv": hkv, "slot0": slot0, "T": t, "device_slot": on_dev,
               "rounds": args.rounds, "bit_identical": same}
        for key in runs:
            rec[key + "_us"] = round(statistics.median(times[key]), 1)
            rec[key + "_min_max_us"] = [round(min(times[key]), 1), round(max(times[key]), 1)]
        print(json.dumps(rec), flush=True)
        del kc, vc, q, k8v, v8v, outs
        torch.cuda.empty_cache()


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--kv", nargs="*", default=None, help="'bf16 fp8': the FP8-KV-cache A/B (bf16 / dequant / direct)")
    ap.add_argument("--shape", default=None, help="run only this shape name (profiling)")
    ap.add_argument("--match", default=None, help="--kv: run only the shapes whose name contains this")
    ap.add_argument("--impl", type=int, default=None, help="run only this impl (profiling)")
    ap.add_argument("--impls", type=int, nargs="*", default=None, help="impls to compare (default 2 7 8 9 13 1)")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.kv is not None:
        if sorted(args.kv) != ["bf16", "fp8"]:
            ap.error("--kv takes 'bf16 fp8'")
        return kv_ab(args)
    e = ops.ext()
    for name, b, s, h, hkv in SHAPES:
        if args.shape and name != args.shape:
            continue
        g = torch.Generator(device="cuda").manual_seed(0)
        kc = torch.randn(b, hkv, s, 128, device="cuda", generator=g).to(torch.bfloat16)
        vc = torch.randn(b, hkv, s, 128, device="cuda", generator=g).to(torch.bfloat16)
        q = torch.randn(b, s, h, 128, device="cuda", generator=g).to(torch.bfloat16)
        ks = torch.zeros(b, dtype=torch.int32, device="cuda")
        slot = torch.zeros(1, dtype=torch.int32, device="cuda")
        flops = 4.0 * b * h * 128 * s * (s + 1) / 2
        ref = None
        impls = [i for i in (args.impls or (2, 7, 8, 9, 13, 1)) if not (i == 1 and s * s * b * h > 2048 * 2048 * 16 * 32)
                 and (args.impl is None or i == args.impl)]
        best, diffs = {i: float("inf") for i in impls}, {}
        for impl in impls:  # warm-up + correctness vs the first impl
            e.attn_prefill_set_impl(impl)
            o = ops.attention(q, kc, vc, slot, ks)
            torch.cuda.synchronize()
            diffs[impl] = 0.0 if ref is None else float((o.float() - ref.float()).abs().max())
            ref = o if ref is None else ref
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(args.rounds):  # interleaved rounds, min per impl (DVFS drift between impls)
            for impl in impls:
                e.attn_prefill_set_impl(impl)
                n = 5
                ev[0].record()
                for _ in range(n):
                    ops.attention(q, kc, vc, slot, ks)
                ev[1].record()
                torch.cuda.synchronize()
                best[impl] = min(best[impl], ev[0].elapsed_time(ev[1]) * 1000 / n)
        for impl in impls:
            us = best[impl]
            print(json.dumps({"shape": name, "impl": impl, "us": round(us, 1), "tflops": round(flops / us / 1e6, 1),
                              "max_diff_vs_first": round(diffs[impl], 5)}), flush=True)
        e.attn_prefill_set_impl(2)
        del kc, vc, q
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
