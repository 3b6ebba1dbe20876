"""The key-split form of the FP8 KV cache's decode attention (csrc/kernels/kv8.hip, SPLIT; the geometry and the plan in
csrc/kernels/attn_plan.h): few (row, kv head) pairs with a long context are cut into key splits, one 8-wave workgroup
each, and the last arriver of a pair merges the published partials. The exact-answer inputs of tests/kv8_inputs.py per
split count, the geometry function on the host, max_kv, ticket reset under graph replay, the plan's rules, and a model
whose default plan splits.

Why the exact inputs stay exact under splitting (tests/exact_inputs.py, tests/kv8_inputs.py): the census has q = 0, so
every p is 1 and every partial sum is a small integer times 2^-8 -- the merged numerator and denominator do not depend on
the order; a needle leads every other key by >= 158 in natural units, >= 227 in log2, so a split without the needle is
merged with the factor exp2(-227) = 0 in fp32 and the needle's split has l = 1. Both need the partials unnormalised."""
from __future__ import annotations

import contextlib
import functools

import pytest
import torch

import exact_inputs as xi
import kv8_inputs as k8
import test_kv8_gpu as base  # the shared, cached decode cases and their checks (imported, not edited)
from jax_llama_amd import ops
from jax_llama_amd.models import LLaMAForCausalLM
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime.benchmark import graph_kernels
from jax_llama_amd.runtime.engine import DecodeEngine, GenerationConfig
from helpers import build, gpu_config, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
DH = xi.DH
B, HKV = 3, 2  # 6 pairs


def _kpg(rep):
    return 8 if rep <= 2 else 16 // rep


@contextlib.contextmanager
def _splits(n):
    e = ops.ext()
    try:
        e.attn_reset_knobs()
        e.attn_set_q8_splits(n)
        yield e
    finally:
        e.attn_reset_knobs()


def _expected_pinned(t_cap, rep, n):
    """A pinned count, cut so that no split is emptier than one chunk (32 kpg keys) at t_cap."""
    ch = 32 * _kpg(rep)
    return max(1, min(n, -(-t_cap // ch)))


# ---------------------------------------------------------------------------------- exact answers per split count
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("t,slot,splits", [(40, 17, 4), (300, 299, 2), (300, 299, 3), (1030, 700, 7), (8192, 8000, 0)])
@pytest.mark.parametrize("rep", [1, 2, 4, 8])
def test_decode_attention_split(rep, t, slot, splits, masked):
    case = base._decode_case(B, HKV, rep, t, slot, masked)
    with _splits(splits) as e:
        rc, why, waves, kpg, r = e.attn_decode_q8_plan_check(B, HKV * rep, HKV, DH, t, masked)
        assert rc == 0 and (waves, kpg, r) == (8, _kpg(rep), rep), (rc, why)
        rc, why, nsplit, ws_floats, tickets = e.attn_decode_q8_split_check(B, HKV * rep, HKV, DH, t, masked)
        assert rc == 0, why
        if splits == 0:
            assert nsplit > 1  # the default plan splits this shape: the unsplit kernel would not be under test
        else:
            assert nsplit == _expected_pinned(t, rep, splits)
        assert (ws_floats, tickets) == ((B * HKV * rep * nsplit * (DH + 4), B * HKV) if nsplit > 1 else (0, 0))
        if (t, slot, splits) == (40, 17, 4):
            # fewer chunks than splits: one active split, the direct write
            assert e.attn_q8_split_ranges(0, slot + 1, kpg, splits)[0] == 1
        if (t, slot, splits) == (1030, 700, 7):
            # the rows' chunks do not divide evenly among the splits
            n_act, ranges = e.attn_q8_split_ranges(0, slot + 1, kpg, nsplit)
            assert n_act > 1 and len({b1 - b0 for b0, b1 in ranges[:n_act]}) > 1
        base._check_decode_case(case, B, HKV, rep, slot)


SPLIT_CASES = [(40, 17, 4), (300, 299, 2), (300, 299, 3), (1030, 700, 7), (8192, 8000, 0)]
assert tuple(dict.fromkeys((t, s) for t, s, _ in SPLIT_CASES)) == xi.LADDER_KV8_SPLIT_TS


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("t,slot,splits", SPLIT_CASES)
@pytest.mark.parametrize("rep", [1, 2, 4, 8])
def test_decode_attention_split_ladder(rep, t, slot, splits, masked):
    """The ladder (tests/exact_inputs.py) through the key-split merge, at the split counts of the test above: with
    ``ramp`` a negative gain puts all the weight into the first split and a positive one into the last, so every other
    partial is merged with exp2(m - M) far from 1 (the census merges equal maxima, the needle a factor of exactly 0).
    Every element within u + 2^-12 of the fp64 softmax."""
    case = base._ladder_case(B, HKV, rep, t, slot, masked)
    with _splits(splits) as e:
        rc, why, nsplit, *_ = e.attn_decode_q8_split_check(B, HKV * rep, HKV, DH, t, masked)
        assert rc == 0, why
        assert nsplit > 1 if splits == 0 else nsplit == _expected_pinned(t, rep, splits)
        base._check_ladder_case(case, rep, slot, f"fp8 split {nsplit}")


# ---------------------------------------------------------------------------------- geometry (no launch)
def test_split_geometry():
    e = ops.ext()
    checked = 0
    for kpg in (2, 4, 8):
        ch = 32 * kpg
        for lo in range(0, 131):
            his = sorted(set(list(range(lo, lo + 701, 53)) + [lo, lo + 1, lo + ch - 1, lo + ch, lo + ch + 1, lo + 700,
                                                              lo - lo % ch + ch, lo - lo % ch + 2 * ch]))
            for hi in his:
                if hi < lo:
                    continue
                for nsplit in range(1, 10):
                    n_act, ranges = e.attn_q8_split_ranges(lo, hi, kpg, nsplit)
                    ctx = (lo, hi, kpg, nsplit, n_act, ranges)
                    assert len(ranges) == nsplit and 0 <= n_act <= nsplit, ctx
                    if hi == lo:
                        assert n_act == 0, ctx
                        continue
                    assert n_act >= 1, ctx
                    act = ranges[:n_act]
                    assert all(b0 == b1 for b0, b1 in ranges[n_act:]), ctx    # inactive splits hold no key
                    assert all(b0 < b1 for b0, b1 in act), ctx                 # no active range is empty
                    assert act[0][0] == lo and act[-1][1] == hi, ctx           # the union covers [lo, hi) ...
                    assert all(act[i][1] == act[i + 1][0] for i in range(n_act - 1)), ctx  # ... disjoint, in order
                    # chunk boundaries (multiples of 32 kpg), except where clipped to [lo, hi)
                    assert all(b0 % ch == 0 for b0, _ in act[1:]) and all(b1 % ch == 0 for _, b1 in act[:-1]), ctx
                    assert act[0][0] - act[0][0] % ch == lo - lo % ch, ctx
                    # every active split but the last holds the same number of chunks
                    chunks = [-(-(b1 - (b0 - b0 % ch)) // ch) for b0, b1 in act]
                    assert len(set(chunks[:-1])) <= 1 and chunks[-1] <= chunks[0], ctx
                    checked += 1
    assert checked > 10000


# ---------------------------------------------------------------------------------- max_kv
def test_split_honours_max_kv():
    """t_cap below the slot, splits pinned: the keys from t_cap on are not attended (the existing honours_max_kv)."""
    rep, t, slot, cap = 4, 300, 299, 150
    case = base._decode_case(B, HKV, rep, t, slot, False)
    q, kq, vq, _ = case["random"]
    kvs = case["kvs"].clone()
    kvs[2] = 5
    want = ref.attention(q.cpu(), k8.to_device(kq, "cpu"), k8.to_device(vq, "cpu"), cap - 1, kvs.cpu()).reshape(B, -1)
    with _splits(3) as e:
        assert e.attn_decode_q8_split_check(B, HKV * rep, HKV, DH, cap, False)[2] == _expected_pinned(cap, rep, 3) == 2
        assert e.attn_q8_split_ranges(5, cap, _kpg(rep), 2)[0] == 2
        base._close(base._attend(q, kq, vq, slot, kvs, None, max_kv=cap), want, 2e-2, 2e-2)


# ---------------------------------------------------------------------------------- tickets reset, replay == eager
def test_split_graph_replay_equals_eager():
    rep, t, splits = 4, 1030, 4
    case = base._decode_case(B, HKV, rep, t, 700, False)
    q, kq, vq, _ = case["random"]
    kvs = case["kvs"].clone()
    kvs[2] = 3
    kpg = _kpg(rep)
    with _splits(splits) as e:
        assert e.attn_decode_q8_split_check(B, HKV * rep, HKV, DH, t, False)[2] == splits
        slot = torch.tensor([700], dtype=torch.int32, device=DEV)
        first = ops.attention(q, kq, vq, slot, kvs)  # sizes the workspaces before the capture
        second = ops.attention(q, kq, vq, slot, kvs)
        torch.cuda.synchronize()
        assert torch.equal(first, second)  # the same bits on every call
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = ops.attention(q, kq, vq, slot, kvs)
        n_acts = []
        for s in (1029, 90, 513):  # 90: every row has one active split (the direct write between two merged replays)
            slot.fill_(s)
            g.replay()
            torch.cuda.synchronize()
            got = out.clone()
            eager = ops.attention(q, kq, vq, slot, kvs)
            torch.cuda.synchronize()
            assert torch.equal(got, eager), s
            base._close(got, ref.attention(q.cpu(), k8.to_device(kq, "cpu"), k8.to_device(vq, "cpu"), s,
                                           kvs.cpu()).reshape(B, -1), 2e-2, 2e-2)
            n_acts.append([e.attn_q8_split_ranges(int(lo), s + 1, kpg, splits)[0] for lo in kvs.cpu()])
        assert max(n_acts[0]) > 1 and set(n_acts[1]) == {1} and max(n_acts[2]) > 1, n_acts


# ---------------------------------------------------------------------------------- plan rules
def test_split_plan_rules():
    e = ops.ext()
    e.attn_reset_knobs()
    try:
        # the existing answers, unchanged (tests/test_kv8_gpu.py test_plan_rules)
        assert e.attn_decode_q8_plan_check(64, 32, 8, DH, 8192, False)[2] == 8
        assert e.attn_decode_q8_plan_check(255, 32, 8, DH, 384, False)[2] == 8
        assert e.attn_decode_q8_plan_check(256, 32, 8, DH, 384, False)[2] == 1
        assert e.attn_decode_q8_plan_check(256, 64, 8, DH, 384, True)[2] == 1
        assert e.attn_decode_q8_plan_check(32, 64, 8, DH, 384, False)[2] == 8
        assert e.attn_decode_q8_plan_check(2048, 8, 1, DH, 384, False)[2] == 1
        # 256 pairs and more stay unsplit, and so do the cache lengths of the model tests
        for shape in [(64, 32, 8, DH, 8192, False), (32, 32, 8, DH, 32768, False), (256, 32, 8, DH, 8192, True),
                      (2, 2, 1, DH, 48, False), (40, 2, 1, DH, 24, False), (2, 2, 1, DH, 24, True)]:
            assert e.attn_decode_q8_split_check(*shape)[2:] == (1, 0, 0), shape
        # few pairs with a long context split, and the buffers follow the formula
        rc, why, nsplit, ws_floats, tickets = e.attn_decode_q8_split_check(1, 32, 8, DH, 8192, False)
        assert rc == 0 and nsplit > 1 and (ws_floats, tickets) == (32 * nsplit * (DH + 4), 8)
        rc, why, nsplit, ws_floats, tickets = e.attn_decode_q8_split_check(3, 16, 2, DH, 1030, True)
        assert rc == 0 and (ws_floats, tickets) == ((3 * 16 * nsplit * (DH + 4), 6) if nsplit > 1 else (0, 0))
        # a pinned q8_waves alone is the unsplit launch
        e.attn_set_q8_waves(8)
        assert e.attn_decode_q8_split_check(1, 32, 8, DH, 8192, False)[2:] == (1, 0, 0)
        e.attn_set_q8_splits(5)
        assert e.attn_decode_q8_split_check(1, 32, 8, DH, 8192, False)[2:] == (5, 32 * 5 * (DH + 4), 8)
        # pinned splits with one wave per pair: refused, with the reason; the 5-tuple says so too
        e.attn_set_q8_waves(1)
        rc, why, *_ = e.attn_decode_q8_split_check(1, 32, 8, DH, 8192, False)
        assert rc != 0 and "split" in why
        assert e.attn_decode_q8_plan_check(1, 32, 8, DH, 8192, False)[0] != 0
        # never split; and the way back
        e.attn_set_q8_waves(0)
        e.attn_set_q8_splits(1)
        assert e.attn_decode_q8_split_check(1, 32, 8, DH, 8192, False)[2:] == (1, 0, 0)
        e.attn_set_q8_splits(5)
        e.attn_reset_knobs()
        default = e.attn_decode_q8_split_check(1, 32, 8, DH, 8192, False)
        e.attn_set_q8_splits(0)
        assert e.attn_decode_q8_split_check(1, 32, 8, DH, 8192, False) == default and default[2] not in (1, 5)
        # a pinned count where the by-shape rule gives one wave per pair (2048 pairs): no splits, not refused
        e.attn_set_q8_splits(4)
        assert e.attn_decode_q8_split_check(256, 32, 8, DH, 8192, False)[:3] == (0, "", 1)
        # a pinned count is cut to the chunks of t_cap
        assert e.attn_decode_q8_split_check(3, 8, 2, DH, 300, False)[2] == 3      # rep 4: 128-key chunks
        assert e.attn_decode_q8_split_check(3, 2, 2, DH, 300, False)[2] == 2      # rep 1: 256-key chunks
        assert e.attn_decode_q8_split_check(3, 8, 2, DH, 40, False)[2] == 1
    finally:
        e.attn_reset_knobs()


def test_split_launch_checks_its_buffers():
    rep, t, slot = 4, 300, 299
    case = base._decode_case(B, HKV, rep, t, slot, False)
    q, kq, vq, want = case["random"]
    kvs = case["kvs"]
    sl = torch.tensor([slot], dtype=torch.int32, device=DEV)
    out = torch.empty(B, HKV * rep * DH, dtype=BF16, device=DEV)
    args = (q, kq.q, kq.scale, vq.q, vq.scale, sl, kvs, None, out, t)
    with _splits(3) as e:
        _, _, nsplit, ws_floats, tickets = e.attn_decode_q8_split_check(B, HKV * rep, HKV, DH, t, False)
        assert nsplit == 3
        ws = torch.empty(ws_floats, dtype=torch.float32, device=DEV)
        tk = torch.zeros(tickets, dtype=torch.int32, device=DEV)
        with pytest.raises(RuntimeError, match="ws"):
            e.attn_decode_q8(*args)  # the plan splits: the buffers are required
        with pytest.raises(RuntimeError, match="ws"):
            e.attn_decode_q8(*args, ws[:-1], tk)
        with pytest.raises(RuntimeError, match="tickets"):
            e.attn_decode_q8(*args, ws, tk[:-1])
        with pytest.raises(RuntimeError, match="ws"):
            e.attn_decode_q8(*args, ws.double(), tk)
        e.attn_decode_q8(*args, ws, tk)
        torch.cuda.synchronize()
        base._close(out, want, 2e-2, 2e-2)
        assert int(tk.abs().max()) == 0  # the last arriver of every pair reset its ticket
        e.attn_set_q8_splits(1)
        e.attn_decode_q8(*args)  # the unsplit plan keeps the old call form
        torch.cuda.synchronize()
        base._close(out, want, 2e-2, 2e-2)


# ---------------------------------------------------------------------------------- the model
MODEL_T = 2304     # the tiny model (1 kv head, rep 2: 256-key chunks) at B = 1: the default plan splits this cache
MODEL_PROMPT = 2200


@functools.lru_cache(maxsize=None)
def _long_models():
    cfg = gpu_config(max_sequence_length=MODEL_T)
    cpu, _, _, params = build(cfg, seed=21)
    gpu = LLaMAForCausalLM(cfg, device=DEV, _do_init=False).load_params(params)
    return cfg, cpu, gpu


def _prefill_and_decode(model, toks, extra):
    """Logits of the prefill and of 3 decode steps ([1, S + 3, V]) with an fp8 cache of MODEL_T slots."""
    b, s = toks.shape
    pos = torch.arange(s + 3, dtype=torch.int32)[None].expand(b, -1)
    cache = model.init_cache(b, MODEL_T, kv_format="fp8_e4m3")
    full = torch.ones(b, s + 3, dtype=torch.int32)
    outs = [model(toks, attention_mask=full, position_ids=pos[:, :s], past_key_values=cache).logits]
    for i in range(3):
        outs.append(model(extra[:, i:i + 1], attention_mask=full, position_ids=pos[:, s + i:s + i + 1],
                          past_key_values=cache).logits)
    return torch.cat(outs, 1).float().cpu()


def _graph_kernels_at(model, batch, max_length, prompt):
    gc = GenerationConfig(max_length=max_length, do_sample=False, pad_token_id=0, eos_token_id=-1)
    eng = DecodeEngine(model, batch, max_length, use_graph=True)
    eng.gc = gc
    g = torch.Generator().manual_seed(batch)
    eng.prefill(torch.randint(3, model.config.vocab_size, (batch, prompt), generator=g, dtype=torch.int32), None)
    eng._decode_step()
    eng.keep_graph = True
    eng._ensure_graph()
    return graph_kernels(eng._graph)


def test_model_whose_default_plan_splits():
    cfg, cpu, gpu = _long_models()
    e = ops.ext()
    e.attn_reset_knobs()
    h, hkv = cfg.num_attention_heads, cfg.num_key_value_heads
    g = torch.Generator().manual_seed(5)
    toks = torch.randint(3, cfg.vocab_size, (1, MODEL_PROMPT), dtype=torch.int32, generator=g)
    extra = torch.randint(3, cfg.vocab_size, (1, 3), dtype=torch.int32, generator=g)
    try:
        gpu.set_kv_cache_format("fp8_e4m3")
        nsplit = e.attn_decode_q8_split_check(1, h, hkv, DH, MODEL_T, False)[2]
        assert nsplit > 1
        assert e.attn_q8_split_ranges(0, MODEL_PROMPT + 1, _kpg(h // hkv), nsplit)[0] > 1  # the merge runs
        # graph replay and eager steps give the same sequences
        gc = GenerationConfig(max_length=MODEL_T, do_sample=False, pad_token_id=2, eos_token_id=-1)
        long_prompt = torch.randint(3, cfg.vocab_size, (1, MODEL_T - 12), dtype=torch.int32, generator=g)
        a = DecodeEngine(gpu, 1, MODEL_T, use_graph=True).run(long_prompt, None, gc).clone()
        b = DecodeEngine(gpu, 1, MODEL_T, use_graph=False).run(long_prompt, None, gc).clone()
        assert torch.equal(a, b)
        # GPU vs the CPU path of the same definition: the project's number (test_model_gpu_vs_cpu_same_definition)
        g8 = _prefill_and_decode(gpu, toks, extra)
        c8 = _prefill_and_decode(cpu, toks, extra)
        err = rel_err(g8, c8)
        print(f"B=1, cache {MODEL_T}, prompt {MODEL_PROMPT}, {nsplit} splits: GPU vs CPU rel_err {err:.4f}")
        assert bool(torch.isfinite(g8).all()) and err < 2e-2
        # one launch still: the captured decode step has the unsplit plan's kernel count
        n_split = _graph_kernels_at(gpu, 1, MODEL_T, MODEL_PROMPT)
        e.attn_set_q8_splits(1)
        n_unsplit = _graph_kernels_at(gpu, 1, MODEL_T, MODEL_PROMPT)
        assert n_split == n_unsplit > 0, (n_split, n_unsplit)
    finally:
        e.attn_reset_knobs()
        gpu.set_kv_cache_format("bf16")


@pytest.mark.parametrize("batch", [2, 40])
def test_short_cache_graph_kernel_count_is_unchanged(batch):
    """The existing B = 2 / 40, T = 24 shapes: no splits, 14 + one write kernel per layer (tests/test_kv8_gpu.py)."""
    cfg, _, gpu = base._models("bf16")
    e = ops.ext()
    e.attn_reset_knobs()
    try:
        ops.GEMV_VARIANT = 1
        gpu.set_kv_cache_format("fp8_e4m3")
        assert e.attn_decode_q8_split_check(batch, cfg.num_attention_heads, cfg.num_key_value_heads, DH, 24, False)[2] == 1
        assert base._decode_graph_kernels(gpu, batch) == base.BF16_DECODE_KERNELS + cfg.num_hidden_layers
    finally:
        ops.GEMV_VARIANT = 0
        gpu.set_kv_cache_format("bf16")
