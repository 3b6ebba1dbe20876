"""The logits processors on the MI355X: the HIP kernel (``ops.process_logits``) against ``ops/reference.py`` bit for bit,
``decode_update_set`` against a transcription, and the engine (eager and graph-replayed, one engine run twice with other
settings) on the scripted model against the host loop of tests/logits_proc_inputs.py token for token.
tests/test_logits_proc_cpu.py checks the reference, the host loop and the scenarios' conditions without a GPU."""
from __future__ import annotations

import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import logits_proc_inputs as lp
import loop_inputs as li
from jax_llama_amd import ops
from jax_llama_amd.models import LLaMAForCausalLM
from jax_llama_amd.ops import reference as ref
from jax_llama_amd.runtime.benchmark import graph_kernels
from jax_llama_amd.runtime import engine as eng_mod
from jax_llama_amd.runtime.engine import DecodeEngine, GenerationConfig
from jax_llama_amd.utils.checkpoint import meta_state_dict_to_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
I32 = torch.int32


def _same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal, and the signs of the zeros too."""
    return torch.equal(a, b) and np.array_equal(np.signbit(a.numpy()), np.signbit(b.numpy()))


# ----------------------------------------------------------------------------------
# 1. the kernel against the reference
# ----------------------------------------------------------------------------------
# each option alone, then all together (suppress and stop ids relative to col_offset; 10 ** 6 is in no vocabulary)
OPTIONS = {"penalty": dict(p=1.3), "reward": dict(p=0.75), "n1": dict(n=1), "n2": dict(n=2), "n4": dict(n=4),
           "suppress": dict(suppress=[0, 1, 31, 32, 63, 64, 200, 10 ** 6]), "min_len": dict(stop=[2, 33], min_len=10 ** 6),
           "lapsed": dict(stop=[2, 33], min_len=1),
           "all": dict(p=1.25, n=3, suppress=[5, 40, 255], stop=[2, 33, 100], min_len=10 ** 6)}


class _Buffers:
    """The device buffers of one call sequence: later launches refill them in place, as the engine does."""

    def __init__(self):
        self.suppress = torch.full((ops.PROC_MAX_SUPPRESS,), -1, dtype=I32, device=DEV)
        self.stop = torch.full((ops.PROC_MAX_STOP,), -1, dtype=I32, device=DEV)
        self.min_len = torch.zeros(1, dtype=I32, device=DEV)

    def fill(self, suppress, stop, min_len):
        self.suppress.copy_(ops.id_buffer(suppress, ops.PROC_MAX_SUPPRESS, "cpu"))
        self.stop.copy_(ops.id_buffer(stop, ops.PROC_MAX_STOP, "cpu"))
        self.min_len.fill_(min_len)


def _check(case, col_offset, vocab, opt, bufs=None):
    x, seq, cur_len, start = case
    o = dict(p=1.0, n=0, suppress=[], stop=[], min_len=0)
    o.update(opt)
    sup = [t + col_offset for t in o["suppress"]]
    stop = [t + col_offset for t in o["stop"]]
    want = ref.process_logits(x.clone(), seq, cur_len, start, col_offset,
                              ref.LogitsProcessors(o["p"], o["n"], sup, stop, o["min_len"], vocab))
    bufs = bufs or _Buffers()
    bufs.fill(sup, stop, o["min_len"])
    got = ops.process_logits(x.to(DEV), seq.to(DEV), torch.tensor([cur_len], dtype=I32, device=DEV), start.to(DEV),
                             col_offset, vocab, o["p"], o["n"], bufs.suppress, bufs.stop, bufs.min_len).cpu()
    assert _same(got, want)
    return got


@pytest.mark.parametrize("opt", sorted(OPTIONS))
@pytest.mark.parametrize("b,v", [(1, 256), (3, 1000), (70, 4096)])
def test_kernel_is_the_reference(b, v, opt):
    """History lengths around the 64-lane wave, past the 256 threads and at several strides per thread."""
    for hist_len in (1, 63, 64, 65, 1025, 2500):
        case = lp.kernel_case(b, v, hist_len, seed=3)
        got = _check(case, 0, v, OPTIONS[opt])
        if opt != "lapsed" and hist_len >= 63:
            assert not _same(got, case[0])


@pytest.mark.parametrize("opt", sorted(OPTIONS))
@pytest.mark.parametrize("hist_len", [1, 63, 64, 65, 1025, 2500])
def test_kernel_at_the_llama3_vocabulary(hist_len, opt):
    _check(lp.kernel_case(2, 128256, hist_len, seed=4), 0, 128256, OPTIONS[opt])


@pytest.mark.parametrize("kind", ["same", "two"])
@pytest.mark.parametrize("opt", ["penalty", "n1", "n2", "n4"])
def test_kernel_duplicate_heavy_histories(kind, opt):
    """Every position the same token (one owner among 2500 atomicOr callers), two tokens alternating."""
    for b, v in ((3, 1000), (2, 128256)):
        case = lp.kernel_case(b, v, 2500, kind=kind, seed=5)
        got = _check(case, 0, v, OPTIONS[opt])
        assert b <= int((got != case[0]).sum()) <= 2 * b  # one or two logits per row


@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("opt", ["penalty", "n2", "suppress", "all"])
def test_kernel_on_a_vocabulary_shard(rank, opt):
    """V_local = 64128 of 128256: the histories straddle the shard edge (kernel_case draws 40 ids either side), and the
    two shards side by side are the unsharded result."""
    vl, vocab = 64128, 128256
    for hist_len in (65, 2500):
        case = lp.kernel_case(2, vl, hist_len, col_offset=rank * vl, vocab=vocab, seed=6)
        toks = case[1][:, 3:case[2]]
        here = (toks >= rank * vl) & (toks < (rank + 1) * vl)
        assert bool(here.any()) and bool((~here & (toks >= 0) & (toks < vocab)).any())  # both shards' tokens
        _check(case, rank * vl, vocab, OPTIONS[opt])
    x, seq, cur_len, start = lp.kernel_case(2, vocab, 300, seed=7)
    seq[:, 10:40] = torch.arange(vl - 15, vl + 15, dtype=I32)  # around the edge
    whole = _check((x, seq, cur_len, start), 0, vocab, dict(p=1.3, n=1))
    half = _check((x[:, rank * vl:(rank + 1) * vl].contiguous(), seq, cur_len, start), rank * vl, vocab,
                  dict(p=1.3, n=1))
    assert _same(half, whole[:, rank * vl:(rank + 1) * vl])


def test_second_launch_reads_the_buffers_again():
    bufs = _Buffers()
    case = lp.kernel_case(3, 1000, 200, seed=8)
    a = _check(case, 0, 1000, OPTIONS["all"], bufs)
    b = _check(case, 0, 1000, dict(p=1.25, n=3, suppress=[7, 41], stop=[3, 34, 101], min_len=10 ** 6), bufs)
    c = _check(case, 0, 1000, dict(p=1.25, n=3, suppress=[7, 41], stop=[3, 34, 101], min_len=1), bufs)
    assert not _same(a, b) and not _same(b, c)


def test_empty_history_and_hist_start_past_cur_len():
    x, seq, cur_len, start = lp.kernel_case(3, 1000, 100, seed=9)
    for s in (cur_len, cur_len + 2):
        got = _check((x, seq, cur_len, torch.full_like(start, s)), 0, 1000, dict(p=1.5, n=1))
        assert _same(got, x)


def test_too_many_logits_for_the_bitmap_is_a_value_error():
    cap = ops.proc_max_v()
    assert cap == 1 << 19  # a 64 KiB bitmap
    v = cap + 1
    bufs = _Buffers()
    args = (torch.zeros(1, 4, dtype=I32, device=DEV), torch.tensor([2], dtype=I32, device=DEV),
            torch.zeros(1, dtype=I32, device=DEV))
    with pytest.raises(ValueError):
        ops.process_logits(torch.zeros(1, v, device=DEV), *args, 0, v, 1.3, 0, bufs.suppress, bufs.stop, bufs.min_len)
    with pytest.raises(ValueError):  # the binding's own check
        ops.ext().process_logits(torch.zeros(1, v, device=DEV), *args, 0, v, 1.3, ref.inv_penalty(1.3), 0,
                                 bufs.suppress, bufs.stop, bufs.min_len)
    x = torch.randn(1, cap)  # the cap itself: the last bit of the bitmap
    seq = torch.tensor([[0, cap - 1, 5, 5]], dtype=I32)
    _check((x, seq, 4, torch.zeros(1, dtype=I32)), 0, cap, dict(p=2.0, n=1))


# ----------------------------------------------------------------------------------
# 2. decode_update_set
# ----------------------------------------------------------------------------------
@pytest.mark.parametrize("stop", [[5], [2, 5], [0, 1, 2, 3, 4, 5, 6, 7]])
@pytest.mark.parametrize("b", [1, 65, 1025, 2500])
def test_decode_update_set_is_the_transcription(b, stop):
    g = torch.Generator().manual_seed(b)
    nxt = torch.randint(0, 12, (b,), generator=g, dtype=I32)
    fin = (torch.rand(b, generator=g) < 0.4).to(I32)
    seq = torch.randint(10, 99, (b, 8), generator=g, dtype=I32)
    tokens = torch.randint(0, 99, (b, 1), generator=g, dtype=I32)
    pos = torch.randint(0, 4000, (b, 1), generator=g, dtype=I32)
    pad, cur = 9, 3
    t = torch.where(fin != 0, torch.full_like(nxt, pad), nxt)
    hit = torch.tensor([int(x) in stop for x in t.tolist()])
    want_seq = seq.clone()
    want_seq[:, cur] = t
    dev = [x.to(DEV) for x in (nxt, fin, seq, torch.tensor([cur], dtype=I32), tokens, pos, torch.tensor([77], dtype=I32))]
    ops.ext().decode_update_set(*dev, pad, ops.id_buffer(stop, ops.PROC_MAX_STOP, DEV))
    got = [x.cpu() for x in dev]
    assert torch.equal(got[1], ((fin != 0) | hit).to(I32))
    assert torch.equal(got[2], want_seq) and torch.equal(got[4], t.reshape(b, 1)) and torch.equal(got[5], pos + 1)
    assert int(got[3]) == cur + 1 and int(got[6]) == 78 and torch.equal(got[0], nxt)
    if b >= 65:
        assert bool(((fin == 0) & hit).any()) and bool(((fin == 0) & ~hit).any())


# ----------------------------------------------------------------------------------
# 3. the engine on the scripted model
# ----------------------------------------------------------------------------------
_MODEL = []


def _model():
    if not _MODEL:
        cfg = li.config()
        params = meta_state_dict_to_params(li.state_dict(li.SAMPLE_LEVELS), cfg.num_hidden_layers)
        _MODEL.append(LLaMAForCausalLM(cfg, device=DEV, _do_init=False).load_params(params))
    return _MODEL[0]


_WANT = {}


def _expected(name, b, variant=0):
    """The host loop's tokens, computed once per scenario (lp.expected asserts the scenario's conditions)."""
    key = (name, b, variant)
    if key not in _WANT:
        _WANT[key] = lp.expected(lp.scenario(*key))
    return lp.scenario(*key), _WANT[key]


def _run(eng, sc):
    return eng.run(sc.toks, sc.mask, lp.generation_config(sc)).cpu().to(I32)


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("name", lp.GREEDY_SCENARIOS + ("sampled",))
def test_engine_is_the_host_loop(name, b, use_graph):
    sc, want = _expected(name, b)
    eng = DecodeEngine(_model(), b, sc.max_length, use_graph=use_graph)
    assert torch.equal(_run(eng, sc), want)
    assert (eng._graph is not None) == use_graph
    assert eng._logits_mode() == ("argmax" if name == "stop_set" else "last")


@pytest.mark.parametrize("name", lp.GREEDY_SCENARIOS + ("sampled",))
def test_one_engine_two_runs(name):
    """The second run has another penalty / n-gram size / stop list of the same length / minimum-length word /
    suppressed ids, a shorter prompt and other history starts under the same (B, max_length). lp.two_runs asserts on
    the host loop that run 2's tokens change if any of run 1's values that the scenario names in lp.STALE is kept (the
    by-value penalty and n, the device words hist_start, min_len, stop, suppress): a stale one cannot pass."""
    first, want1, second, want2 = lp.two_runs(name)
    eng = DecodeEngine(_model(), 3, first.max_length, use_graph=True)
    assert torch.equal(_run(eng, first), want1)
    assert torch.equal(_run(eng, second), want2)
    assert eng._graph is not None


def _decode_graph_kernels(model, gc):
    eng = DecodeEngine(model, 2, 24, use_graph=True)
    eng.gc = gc
    eng.prefill(torch.randint(3, li.V, (2, 8), generator=torch.Generator().manual_seed(2), dtype=I32), None)
    eng._decode_step()
    eng.keep_graph = True
    eng._ensure_graph()
    return eng._logits_mode(), graph_kernels(eng._graph)


def test_defaults_keep_the_fused_argmax_and_the_graph(monkeypatch):
    """Default options: the fused lm_head argmax, and the same captured step before and after a processor-enabled run
    on another engine, which itself has exactly one launch more than the unfused greedy step (logits + argmax)."""
    model = _model()
    plain = GenerationConfig(max_length=24, pad_token_id=0, eos_token_id=-1)
    mode0, n0 = _decode_graph_kernels(model, plain)
    mode1, n1 = _decode_graph_kernels(model, GenerationConfig(max_length=24, pad_token_id=0, eos_token_id=-1,
                                                             repetition_penalty=1.1, no_repeat_ngram_size=3,
                                                             min_new_tokens=8))
    mode2, n2 = _decode_graph_kernels(model, plain)
    mode3, n3 = _decode_graph_kernels(model, GenerationConfig(max_length=24, pad_token_id=0, eos_token_id=[5, 6]))
    print(f"decode graph kernel nodes: defaults {n0}, processors {n1}, defaults again {n2}, stop list {n3}")
    assert (mode0, mode1, mode2, mode3) == ("argmax", "last", "argmax", "argmax")
    assert n0 > 0 and n2 == n0 and n3 == n0
    monkeypatch.setattr(eng_mod, "FUSED_GREEDY", False)
    mode4, n4 = _decode_graph_kernels(model, plain)
    print(f"unfused greedy step: {n4}")
    assert mode4 == "last" and n1 == n4 + 1


# ----------------------------------------------------------------------------------
# 4. the bounds-checked build
# ----------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import json, sys, torch
sys.path.insert(0, "tests")
import logits_proc_inputs as lp
from jax_llama_amd import ops
from jax_llama_amd.ops import reference as ref
e = ops.ext()
res = {"debug": bool(e.DEBUG_BOUNDS)}
dev, i32 = "cuda", torch.int32
ops.bounds_error(reset=True)
sup, stop, ml = ops.id_buffer([], 64, dev), ops.id_buffer([], 8, dev), torch.zeros(1, dtype=i32, device=dev)
def run(case, cur_len):
    x, seq, _, start = case
    got = ops.process_logits(x.to(dev), seq.to(dev), torch.tensor([cur_len], dtype=i32, device=dev), start.to(dev), 0,
                             x.shape[1], 1.3, 2, sup, stop, ml).cpu()
    want = ref.process_logits(x.clone(), seq, cur_len, start, 0, ref.LogitsProcessors(1.3, 2, vocab=x.shape[1]))
    return bool(torch.equal(got, want)), ops.bounds_error(reset=True)
clean = lp.kernel_case(2, 300, 6, seed=1)       # short history: no out-of-range id is planted
res["clean"] = run(clean, clean[2])
bad = lp.kernel_case(2, 300, 100, seed=1)       # ids vocab + 5 and -3 in the history: skipped and recorded
res["token"] = run(bad, bad[2])
res["seq"] = run(clean, clean[1].shape[1] + 4)  # cur_len past the buffer: clamped to L and recorded
print("RESULT " + json.dumps(res))
"""


@pytest.mark.skipif(not glob.glob(os.path.join(ROOT, "jax_llama_amd", "_C_dbg*.so")),
                    reason="debug build absent (python build.py --debug-bounds)")
def test_debug_build_records_out_of_range_history():
    """The child process loads the bounds-checked build: out-of-range history ids and a cur_len past the buffer are
    skipped / clamped exactly as in release (the result is the reference's) and recorded."""
    env = dict(os.environ, JLA_DEBUG_BOUNDS="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["debug"]
    assert res["clean"] == [True, 0]
    assert res["token"] == [True, 1 << 0]
    assert res["seq"] == [True, 1 << 2]
