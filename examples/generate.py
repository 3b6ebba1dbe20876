#!/usr/bin/env python3
"""Text generation entry point -- the MI355X counterpart of the reference ``jax_example.py``.

Same ``load()`` / ``main()`` surface (``jax_example.py:10-40``): build the tensor-parallel layout,
the tokenizer (SentencePiece for LLaMA-1/2, tiktoken-format BPE for Llama-3), load the Meta
checkpoint and run the two fixed prompts through ``LLaMA.generate_from_str``. Differences by
design: one process per GPU (launch with ``torchrun --nproc-per-node MP``; TP degree = world size,
like the reference's ``(1, n_devices)`` mesh), each rank reads only its own slices of the
checkpoint, argparse instead of ``fire`` (not installed), and a ``--synthetic`` mode that runs a
random-init model of a named architecture with synthetic prompt ids (no checkpoint needed).

  python examples/generate.py --ckpt_dir /ckpt/8B --tokenizer_path /ckpt/tokenizer.model --is_llama3
  torchrun --nproc-per-node 8 --master-addr 127.0.0.1 examples/generate.py --ckpt_dir /ckpt/70B ...
  python examples/generate.py --synthetic --model llama3-8b --max_gen_len 32 [--weights fp8|mxfp4]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from jax_llama_amd import LLaMA, LLaMA2Tokenizer, LLaMA3Tokenizer, LLaMAForCausalLM  # noqa: E402
from jax_llama_amd.parallel import TPComm, init_distributed  # noqa: E402
from jax_llama_amd.parallel.partition import Mesh  # noqa: E402
from jax_llama_amd.utils.checkpoint import load_meta_rank  # noqa: E402

PROMPTS = ["The capital of Germany is the city of",
           "Here is my sonnet in the style of Shakespeare about an artificial intelligence:"]
WEIGHT_FORMATS = {"fp8": "fp8_e4m3", "mxfp4": "mxfp4"}  # --weights -> LLaMAForCausalLM.quantize_weights_


def load(ckpt_dir: str, tokenizer_path: str, is_llama3: bool, max_seq_len: int = 2048, weights: str = "bf16",
         kv_cache: str = "bf16", **model_kwargs) -> LLaMA:
    """Reference ``load`` (jax_example.py:10-31) on the MI355X runtime. ``weights="fp8"`` / ``"mxfp4"``: the layer
    projections are quantised to FP8 e4m3 / MXFP4 after loading (``LLaMAForCausalLM.quantize_weights_``; each rank its
    own shard).
    ``kv_cache="fp8"``: the KV caches hold FP8 e4m3 rows (``LLaMAForCausalLM.set_kv_cache_format``)."""
    ctx = init_distributed()
    ctx.setup_mesh(tp=ctx.world)
    with open(os.path.join(ckpt_dir, "params.json")) as f:
        hidden = int(json.load(f)["dim"])
    comm = TPComm.from_context(ctx, fused_hidden=hidden)
    tokenizer = LLaMA3Tokenizer(tokenizer_path) if is_llama3 else LLaMA2Tokenizer(tokenizer_path)
    params, config = load_meta_rank(ckpt_dir, tokenizer, ctx.tp_rank, ctx.tp_size, max_seq_len=max_seq_len)
    config.bos_token_id, config.eos_token_id = tokenizer.bos_id, tokenizer.eos_id
    model = LLaMAForCausalLM(config, device=ctx.device, comm=comm, _do_init=False, **model_kwargs).load_params(params, sharded=True)
    del params
    if weights != "bf16":
        model.quantize_weights_(WEIGHT_FORMATS[weights])
    if kv_cache == "fp8":
        model.set_kv_cache_format("fp8_e4m3")
    return LLaMA(None, model, tokenizer, mesh=Mesh(dp=1, mp=ctx.tp_size, rank=ctx.rank))


def main(ckpt_dir: str, tokenizer_path: str, is_llama3: bool, max_gen_len: int = 256, temperature: float = 0.8,
         top_p: float = 0.95, weights: str = "bf16", kv_cache: str = "bf16", num_beams: int = 1,
         repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, min_new_tokens: int = 0):
    """Reference ``main`` (jax_example.py:33-40). ``num_beams > 1``: beam search (temperature is then taken as 0).
    Llama-3 (without beam search) stops on any of the tokenizer's ``stop_tokens`` (end of text, end of turn)."""
    generator = load(ckpt_dir, tokenizer_path, is_llama3, weights=weights, kv_cache=kv_cache)
    if num_beams > 1:
        temperature = 0.0
    stops = sorted(generator.tokenizer.stop_tokens) if is_llama3 and num_beams == 1 else None
    results = generator.generate_from_str(PROMPTS, max_gen_len=max_gen_len, temperature=temperature, top_p=top_p,
                                          num_beams=num_beams, repetition_penalty=repetition_penalty,
                                          no_repeat_ngram_size=no_repeat_ngram_size, min_new_tokens=min_new_tokens,
                                          stop_token_ids=stops)
    if int(os.environ.get("RANK", "0")) == 0:
        for result in results:
            print(result)
            print("\n==================================\n")
    return results


def synthetic(model_name: str, batch: int, prompt_len: int, max_gen_len: int, temperature: float, top_p: float,
              weights: str = "bf16", kv_cache: str = "bf16", num_beams: int = 1, repetition_penalty: float = 1.0,
              no_repeat_ngram_size: int = 0, min_new_tokens: int = 0):
    from jax_llama_amd.config import get_preset
    from jax_llama_amd.runtime.engine import GenerationConfig
    ctx = init_distributed()
    ctx.setup_mesh(tp=ctx.world)
    cfg = get_preset(model_name, max_seq_len=max(2048, prompt_len + max_gen_len))
    comm = TPComm.from_context(ctx, fused_hidden=cfg.hidden_size)
    model = LLaMAForCausalLM(cfg, device=ctx.device, comm=comm, _do_init=False).init_random(seed=0)
    if weights != "bf16":
        model.quantize_weights_(WEIGHT_FORMATS[weights])
    if kv_cache == "fp8":
        model.set_kv_cache_format("fp8_e4m3")
    toks = torch.randint(3, cfg.vocab_size, (batch, prompt_len), generator=torch.Generator().manual_seed(0),
                         dtype=torch.int32)
    gc = GenerationConfig(max_length=prompt_len + max_gen_len, do_sample=temperature != 0.0 and num_beams == 1,
                          temperature=temperature, top_p=top_p, pad_token_id=0, eos_token_id=-1, num_beams=num_beams,
                          repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                          min_new_tokens=min_new_tokens)
    t0 = time.perf_counter()
    seq = model.generate(toks, generation_config=gc).sequences
    torch.cuda.synchronize() if torch.cuda.is_available() else None
    dt = time.perf_counter() - t0
    if ctx.rank == 0:
        print(f"{model_name} ({weights} weights, {model.weight_bytes() / 2**30:.2f} GiB; {kv_cache} KV cache): {batch} x {max_gen_len} tokens in {dt:.3f} s "
              f"({batch * max_gen_len / dt:.1f} tok/s incl. prefill + graph capture)")
        print("first row:", seq[0, prompt_len:prompt_len + 16].tolist())


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ckpt_dir")
    ap.add_argument("--tokenizer_path")
    ap.add_argument("--is_llama3", action="store_true")
    ap.add_argument("--max_gen_len", type=int, default=256)
    ap.add_argument("--temperature", type=float, default=0.8)
    ap.add_argument("--top_p", type=float, default=0.95)
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--prompt_len", type=int, default=16)
    ap.add_argument("--weights", choices=["bf16", "fp8", "mxfp4"], default="bf16",
                    help="fp8: FP8 e4m3 weight-only layer projections (one power-of-two scale per output row); "
                    "mxfp4: 4-bit e2m1 codes with one power-of-two scale per row and 32 K elements")
    ap.add_argument("--kv-cache", choices=["bf16", "fp8"], default="bf16",
                    help="fp8: KV caches of FP8 e4m3 rows (one power-of-two scale per row, kv head and slot): 132 bytes "
                    "per 128-value row instead of 256")
    ap.add_argument("--num_beams", type=int, default=1,
                    help="> 1: beam search with that many beams (2..8; no sampling, no tensor parallelism)")
    ap.add_argument("--repetition_penalty", type=float, default=1.0,
                    help="logits processor: every token already in a row's history is scaled down once (1.0: off)")
    ap.add_argument("--no_repeat_ngram_size", type=int, default=0,
                    help="logits processor: no n-gram of this size occurs twice in a row's history (0: off)")
    ap.add_argument("--min_new_tokens", type=int, default=0,
                    help="logits processor: the stop tokens are banned for this many generated tokens")
    a = ap.parse_args()
    if a.synthetic:
        synthetic(a.model, a.batch, a.prompt_len, a.max_gen_len, a.temperature, a.top_p, a.weights, a.kv_cache,
                  a.num_beams, a.repetition_penalty, a.no_repeat_ngram_size, a.min_new_tokens)
    else:
        if not (a.ckpt_dir and a.tokenizer_path):
            ap.error("--ckpt_dir and --tokenizer_path are required (or use --synthetic)")
        main(a.ckpt_dir, a.tokenizer_path, a.is_llama3, a.max_gen_len, a.temperature, a.top_p, a.weights, a.kv_cache,
             a.num_beams, a.repetition_penalty, a.no_repeat_ngram_size, a.min_new_tokens)
