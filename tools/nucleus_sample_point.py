#!/usr/bin/env python
"""The full-vocabulary sampler alone: ops.nucleus_sample against the torch chain it replaces and ops.topk_sample at
k = 50, each captured into a graph and replayed alternately in one process (medians, with the min..max spread).
One JSON line per (batch, setting); --share adds the share of rows whose first-pass boundary bin fits the kernel's
compaction list, for the last-position logits of a random-init model.

    python tools/nucleus_sample_point.py --batch 1 32 256 4096 >> profiles/nucleus_sample_points.jsonl
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def torch_chain(x, temperature, top_p):
    """runtime/engine.py::_sample's torch path at top_k = 0 (sort, softmax, cumsum, roll, rand, argmax, gather)."""
    import torch
    vals, idx = torch.sort(x / temperature if temperature != 1.0 else x, dim=-1, descending=True)
    if top_p < 1.0:
        keep = torch.roll(torch.softmax(vals, -1).cumsum(-1) < top_p, 1, dims=-1)
        keep[:, 0] = True
        vals = torch.where(keep, vals, torch.full_like(vals, float("-inf")))
    u = torch.rand(vals.shape, device=vals.device, dtype=torch.float32)
    gumbel = -torch.log(-torch.log(u.clamp_min(1e-20)).clamp_min(1e-20))
    return idx.gather(1, (vals + gumbel).argmax(-1)[:, None]).squeeze(1).to(torch.int32)


def compaction_share(x, temperature, top_p, cap=4096):
    """Share of rows whose boundary bin (the top 11 key bits of the last survivor) holds at most ``cap`` logits."""
    import torch
    vals, _ = torch.sort(x.double() / temperature, dim=-1, descending=True)
    p = torch.softmax(vals, -1)
    last = ((p.cumsum(-1) - p) < top_p).sum(-1) - 1
    t = torch.sort(x, dim=-1, descending=True)[0].gather(1, last[:, None])

    def top11(f):
        u = f.contiguous().view(torch.int32).long() & 0xFFFFFFFF
        return torch.where(u >> 31 == 1, ~u & 0xFFFFFFFF, u | 0x80000000) >> 21
    return float(((top11(x) == top11(t)).sum(-1) <= cap).float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 32, 256, 4096])
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-eager", action="store_true", help="time the torch chain eagerly: torch.sort of "
                    "[4096, 128256] is refused under stream capture")
    ap.add_argument("--share", default=None, help="a model preset: report the compaction share on its logits")
    args = ap.parse_args()
    import torch
    from jax_llama_amd import ops
    dev = "cuda"
    step = torch.tensor([7], dtype=torch.int32, device=dev)
    if args.share:
        from jax_llama_amd.config import get_preset
        from jax_llama_amd.models import LLaMAForCausalLM
        cfg = get_preset(args.share, max_seq_len=2048)
        model = LLaMAForCausalLM(cfg, device=dev, _do_init=False).init_random(seed=1)
        toks = torch.randint(3, model.config.vocab_size, (256, 16), generator=torch.Generator().manual_seed(0),
                             dtype=torch.int32)
        x = model(toks).logits[:, -1].float()
        print(json.dumps({"model": args.share, "rows": 256, "logit_std": round(float(x.std()), 3),
                          "compaction_share_T0.6_p0.9": compaction_share(x, 0.6, 0.9),
                          "compaction_share_T1_p0.95": compaction_share(x, 1.0, 0.95)}), flush=True)
        del model, x
        torch.cuda.empty_cache()
    for b in args.batch:
        x = torch.randn(b, args.vocab, device=dev, generator=torch.Generator(dev).manual_seed(b)) * 2
        for temperature, top_p in ((0.6, 0.9), (1.0, 1.0)):
            paths = {"nucleus": lambda: ops.nucleus_sample(x, 0, temperature, top_p, 5, step),
                     "torch": lambda: torch_chain(x, temperature, top_p),
                     "topk50": lambda: ops.topk_sample(x, 50, temperature, top_p, 5, step)}
            graphs = {}
            for name, fn in paths.items():
                fn()  # eager: sizes the workspaces
                torch.cuda.synchronize()
                if name == "torch" and args.torch_eager:
                    graphs[name] = fn
                    continue
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    fn()
                g.replay()
                graphs[name] = g.replay
            torch.cuda.synchronize()
            ms = {name: [] for name in graphs}
            for _ in range(args.reps):
                for name, run in graphs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run()
                    e1.record()
                    e1.synchronize()
                    ms[name].append(e0.elapsed_time(e1))
            r = {"batch": b, "vocab": args.vocab, "top_k": 0, "temperature": temperature, "top_p": top_p,
                 "reps": args.reps, "eager": [n for n, run in graphs.items() if run is paths[n]]}
            for name, t in ms.items():
                r[name + "_ms"] = round(statistics.median(t), 4)
                r[name + "_ms_range"] = [round(min(t), 4), round(max(t), 4)]
            print(json.dumps(r), flush=True)
            del graphs
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
