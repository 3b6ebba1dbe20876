"""Generation engine: prefill + hipGraph-replayed decode steps.

Semantics follow HF ``FlaxGenerationMixin.generate`` (transformers<5), which the reference
inherits (``generation.py:28-41`` builds the ``GenerationConfig``):

  * ``sequences = full((B, max_length), pad)``; the prompt occupies ``[:, :S]``;
  * the prefill is the first loop-body call, then the decode loop runs while
    ``cur_len < max_length`` and not every row has produced ``eos``;
  * a finished row emits ``pad``; ``is_sent_finished |= next == eos``;
  * greedy = ``argmax`` (first max); sampling = temperature -> top-k (default 50) -> top-p ->
    categorical;
  * logits processors (repetition penalty, no-repeat n-gram, suppressed ids, minimum length) run on the logits
    before either, and ``eos`` may be a set of up to 8 ids (the README's "Logits processors" section);
  * positions: ``cumsum(mask) - 1`` for the prompt, then ``last + 1`` per step
    (``model.py:758, 771``).

MI355X execution model (replaces XLA's compiled ``lax.while_loop``):
  * the whole decode step (embedding, all layers, lm_head, sampler, state update) reads its
    inputs — token ids, positions, the cache slot, ``cur_len`` and the finished flags — from
    device buffers and writes the next state back, so it is captured ONCE into a hipGraph
    (``torch.cuda.CUDAGraph`` is hipGraph on ROCm) and replayed per token with no host
    work besides the launch;
  * the host polls the finished flags only every ``check_every`` steps (rows that finished
    earlier keep emitting ``pad``, so polling late never changes the output).

``num_beams > 1``: HF Flax ``_beam_search`` on a ``BeamEngine`` (below), the same execution model over ``B * K`` rows.
"""
from __future__ import annotations

import dataclasses
import os
from collections import OrderedDict
from dataclasses import dataclass
from typing import Optional

import torch

from .. import ops
from ..models.kv_cache import kv_row_bytes
from ..ops import reference as ref

_NEG_INF = float("-inf")


@dataclass
class GenerationConfig:
    """Subset of HF ``GenerationConfig`` used by the reference (``generation.py:32-40``)."""

    max_length: Optional[int] = None
    max_new_tokens: Optional[int] = None
    do_sample: bool = False
    temperature: float = 1.0
    top_k: int = 50  # HF default; the reference never overrides it
    top_p: float = 1.0
    num_beams: int = 1
    pad_token_id: Optional[int] = None
    eos_token_id: object = None  # one id, or a list of 1 .. 8 ids (the stop set)
    seed: int = 0
    # logits processors (the README's "Logits processors" section; ops/reference.py process_logits)
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    min_length: int = 0
    min_new_tokens: int = 0
    suppress_tokens: Optional[list] = None
    bad_words_ids: Optional[list] = None  # single-token entries only: they join suppress_tokens
    # beam search (num_beams > 1; BeamEngine)
    length_penalty: float = 1.0
    early_stopping: object = False  # False, True or "never"
    num_return_sequences: int = 1


# prompt tokens per prefill forward (DecodeEngine._prefill_rows): larger batches run their prefill in row chunks
PREFILL_TOKENS = int(os.environ.get("JLA_PREFILL_TOKENS", str(1 << 18)))

# greedy decoding takes the argmax inside the lm_head GEMM epilogue (JLA_FUSED_ARGMAX=0: logits + argmax)
FUSED_GREEDY = os.environ.get("JLA_FUSED_ARGMAX", "1") != "0"


def _fused_greedy() -> bool:
    return FUSED_GREEDY


@dataclass
class GenerateOutput:
    sequences: torch.Tensor
    scores: Optional[torch.Tensor] = None  # beam search: fp32 [B * num_return_sequences], the hypotheses' scores


# --------------------------------------------------------------------------------------
# Logits processors and stop sets
# --------------------------------------------------------------------------------------
def stop_ids(gc: GenerationConfig) -> list:
    """The stop set of ``gc.eos_token_id`` (one id or a list); an id below 0 stands for "none"."""
    eos = gc.eos_token_id
    ids = list(eos) if isinstance(eos, (list, tuple)) else ([] if eos is None else [eos])
    return [int(t) for t in ids if int(t) >= 0]


def suppressed_ids(gc: GenerationConfig) -> list:
    """``suppress_tokens`` plus the single-token entries of ``bad_words_ids``, without duplicates."""
    ids = [int(t) for t in (gc.suppress_tokens or [])]
    for word in gc.bad_words_ids or []:
        word = [word] if isinstance(word, int) else list(word)
        if len(word) != 1:
            raise NotImplementedError("bad_words_ids: only single-token entries are supported")
        ids.append(int(word[0]))
    return list(dict.fromkeys(ids))


def processors_active(gc: GenerationConfig) -> bool:
    """Whether a decode step runs ``ops.process_logits`` (a stop list alone does not: it only changes the update)."""
    return (float(gc.repetition_penalty) != 1.0 or gc.no_repeat_ngram_size > 0 or bool(suppressed_ids(gc))
            or ((gc.min_length > 0 or gc.min_new_tokens > 0) and bool(stop_ids(gc))))


def validate_processors(gc: GenerationConfig, vocab: int) -> None:
    """ValueError for settings outside the definition (``generate`` and ``DecodeEngine.run`` both call it)."""
    p = gc.repetition_penalty
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not p > 0:
        raise ValueError(f"repetition_penalty must be a number > 0, got {p!r}")
    for name in ("no_repeat_ngram_size", "min_length", "min_new_tokens"):
        val = getattr(gc, name)
        if isinstance(val, bool) or not isinstance(val, int) or val < 0:
            raise ValueError(f"{name} must be an int >= 0, got {val!r}")
    eos = gc.eos_token_id
    if isinstance(eos, (list, tuple)):
        if not 1 <= len(eos) <= ops.PROC_MAX_STOP:
            raise ValueError(f"eos_token_id: a list of 1 to {ops.PROC_MAX_STOP} ids, got {len(eos)}")
        bad = [t for t in eos if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < vocab]
        if bad:
            raise ValueError(f"eos_token_id: ids outside the vocabulary [0, {vocab}): {bad}")
    sup = suppressed_ids(gc)
    if len(sup) > ops.PROC_MAX_SUPPRESS:
        raise ValueError(f"suppress_tokens (with bad_words_ids): at most {ops.PROC_MAX_SUPPRESS} ids, got {len(sup)}")
    bad = [t for t in sup if not 0 <= t < vocab]
    if bad:
        raise ValueError(f"suppress_tokens: ids outside the vocabulary [0, {vocab}): {bad}")
    if gc.num_beams != 1 and (processors_active(gc) or isinstance(eos, (list, tuple)) or gc.min_length > 0
                              or gc.min_new_tokens > 0):
        raise ValueError("beam search (num_beams > 1) takes no logits processors and no stop list")


# --------------------------------------------------------------------------------------
# Sampling
# --------------------------------------------------------------------------------------
def _greedy(model, logits_local) -> torch.Tensor:
    """``logits_local``: this rank's ``[B, V/tp]`` logits, or its already reduced ``(idx, val)``
    (``forward_tokens(logits_mode="argmax")``: argmax fused into the lm_head GEMM). Under TP the
    per-rank ``(max, argmax)`` pairs are reduced by one custom gather kernel (``comm.argmax``)."""
    if isinstance(logits_local, tuple):
        (idx, val), v_local = logits_local, model.vocab_local
    else:
        (idx, val), v_local = ops.argmax(logits_local), logits_local.shape[1]
    return model.comm.argmax(val, idx, v_local)


def _sample(model, logits_local: torch.Tensor, gc: GenerationConfig, gen: Optional[torch.Generator],
            step: Optional[torch.Tensor] = None):
    """temperature -> top-k -> top-p -> categorical (Gumbel-max), exact under vocab sharding.

    top_k in [1, 64] (HF default 50): the on-device sampler (ops.topk_sample: radix-select top-k
    kernels + Philox Gumbel-max keyed by (seed, step)), graph-capturable and identical on CPU.
    Otherwise (top_k = 0 / > 64): torch sort path."""
    comm = model.comm
    v_local = logits_local.shape[1]
    k = min(gc.top_k or 0, v_local * comm.size)
    if step is not None and 1 <= k <= ops.SAMPLER_MAX_K and gc.temperature and gc.temperature > 0:
        if logits_local.device.type == "cpu" or ops.ext().topk_chunks(v_local) * min(k, v_local) <= 4096:
            return ops.topk_sample(logits_local.float().contiguous(), k, gc.temperature, gc.top_p,
                                   gc.seed, step, comm if comm.size > 1 else None)
    x = logits_local.float()
    if gc.temperature is not None and gc.temperature != 1.0:
        x = x / gc.temperature
    if gc.top_k:
        k = min(gc.top_k, x.shape[1])
        vals, idx = torch.topk(x, k, dim=-1)
        idx = (idx + comm.rank * x.shape[1]).to(torch.int32)
        if comm.size > 1:
            gv, gi = comm.gather_topk(vals.contiguous(), idx.contiguous())
            vals, sel = torch.topk(gv, k, dim=-1)
            idx = gi.gather(1, sel)
    else:
        full = model.gather_logits(x)
        vals, idx = torch.sort(full, dim=-1, descending=True)
    if gc.top_p is not None and gc.top_p < 1.0:
        # vals are sorted descending (topk returns sorted)
        probs = torch.softmax(vals, -1)
        cum = probs.cumsum(-1)
        keep = torch.roll(cum < gc.top_p, 1, dims=-1)
        keep[:, 0] = True
        vals = torch.where(keep, vals, torch.full_like(vals, _NEG_INF))
    u = torch.rand(vals.shape, device=vals.device, generator=gen, dtype=torch.float32)
    gumbel = -torch.log(-torch.log(u.clamp_min(1e-20)).clamp_min(1e-20))
    choice = (vals + gumbel).argmax(-1)
    return idx.gather(1, choice[:, None]).squeeze(1).to(torch.int32)


# --------------------------------------------------------------------------------------
class DecodeEngine:
    """Owns the KV cache and the device-resident decode state for one (B, max_length)."""

    def __init__(self, model, batch_size: int, max_length: int, use_graph: Optional[bool] = None,
                 check_every: int = 16):
        self.model = model
        self.b = batch_size
        self.max_length = max_length
        dev = model.device
        self.device = dev
        if use_graph is None:
            use_graph = dev.type == "cuda" and os.environ.get("JLA_NO_GRAPH", "0") != "1"
        self.use_graph = use_graph
        self.check_every = check_every
        self.cache = model.init_cache(batch_size, max_length)
        i32 = dict(dtype=torch.int32, device=dev)
        self.tokens = torch.zeros(batch_size, 1, **i32)
        self.positions = torch.zeros(batch_size, 1, **i32)
        self.kv_start = torch.zeros(batch_size, **i32)
        self.finished = torch.zeros(batch_size, **i32)
        self.cur_len = torch.zeros(1, **i32)
        self.sequences = torch.zeros(batch_size, max_length, **i32)
        self.key_mask: Optional[torch.Tensor] = None
        self._key_mask_buf: Optional[torch.Tensor] = None  # a holed mask lives here: the graph records its address
        self._graph = None
        self._graph_key = None
        self.keep_graph = False  # keep the captured graph's topology (runtime/benchmark.py counts its kernel nodes)
        self._gen: Optional[torch.Generator] = None
        self.gc: Optional[GenerationConfig] = None
        # logits processors and the stop set: what changes from call to call lives in these fixed buffers, which the
        # captured step reads (filled by prefill; unused id slots hold -1)
        self.hist_start = torch.zeros(batch_size, **i32)  # first attended prompt column (S: none): history start
        self.stop_ids = torch.full((ops.PROC_MAX_STOP,), -1, **i32)
        self.suppress_ids = torch.full((ops.PROC_MAX_SUPPRESS,), -1, **i32)
        self.min_len = torch.zeros(1, **i32)  # max(min_length, S + min_new_tokens)
        self._processors = False
        self._stop_set = False

    # ---------------------------------------------------------------------------------
    def _next_token(self, logits_local):
        if self._processors:  # processors -> temperature -> top-k -> top-p, as in HF
            comm, gc = self.model.comm, self.gc
            logits_local = logits_local.float().contiguous()
            v_local = logits_local.shape[1]
            ops.process_logits(logits_local, self.sequences, self.cur_len, self.hist_start, comm.rank * v_local,
                               v_local * comm.size, gc.repetition_penalty, gc.no_repeat_ngram_size,
                               self.suppress_ids, self.stop_ids, self.min_len)
        if self.gc.do_sample:
            return _sample(self.model, logits_local, self.gc, self._gen, self.cur_len)
        return _greedy(self.model, logits_local)

    def _update(self, nxt: torch.Tensor):
        """Device-side HF loop-body bookkeeping (pad for finished rows, eos tracking,
        sequences write, position/slot/cur_len advance)."""
        if self.device.type == "cuda":
            if self._stop_set:  # eos_token_id is a list: the ids come from the stop buffer
                ops.ext().decode_update_set(nxt, self.finished, self.sequences, self.cur_len, self.tokens,
                                            self.positions, self.cache.index_t, int(self.gc.pad_token_id),
                                            self.stop_ids)
                return
            ops.ext().decode_update(nxt, self.finished, self.sequences, self.cur_len, self.tokens,
                                    self.positions, self.cache.index_t, int(self.gc.pad_token_id),
                                    int(self.gc.eos_token_id))
            return
        fin = self.finished.bool()
        nxt = torch.where(fin, torch.full_like(nxt, self.gc.pad_token_id), nxt)
        if self._stop_set:
            hit = (nxt[:, None] == self.stop_ids[None, :]).any(1)
        else:
            hit = nxt == self.gc.eos_token_id
        self.finished.copy_((fin | hit).to(torch.int32))
        cl = int(self.cur_len.item())
        if cl < self.max_length:
            self.sequences[:, cl] = nxt
        self.tokens[:, 0] = nxt
        self.positions.add_(1)
        self.cache.index_t.add_(1)
        self.cur_len.add_(1)

    def _logits_mode(self) -> str:
        return "argmax" if _fused_greedy() and not self.gc.do_sample and not self._processors else "last"

    def _decode_step(self):
        logits, *_ = self.model.forward_tokens(self.tokens, self.positions, self.cache, self.cache.index_t,
                                               self.kv_start, self.key_mask, logits_mode=self._logits_mode())
        self._update(self._next_token(logits))

    # ---------------------------------------------------------------------------------
    def prefill(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor]):
        model, dev = self.model, self.device
        ids = input_ids.to(dev, torch.int32)
        b, s = ids.shape
        assert b == self.b and s < self.max_length
        if attention_mask is None:
            mask = torch.ones(b, s, dtype=torch.int32)
        else:
            mask = attention_mask.to("cpu", torch.int32)
        positions = (mask.cumsum(-1) - 1).to(torch.int32)
        ext_mask = torch.ones(b, self.max_length, dtype=torch.int32)
        ext_mask[:, :s] = mask
        from ..models.llama import mask_to_kv_start
        kv_start, key_mask = mask_to_kv_start(ext_mask, dev)
        self.kv_start.copy_(kv_start)
        if key_mask is not None:
            if self._key_mask_buf is None:
                self._key_mask_buf = torch.empty_like(key_mask)
            self._key_mask_buf.copy_(key_mask)
            key_mask = self._key_mask_buf
        self.key_mask = key_mask
        self.cache.reset()
        self.sequences.fill_(self.gc.pad_token_id)
        self.sequences[:, :s] = ids
        self.finished.zero_()
        self._set_processors(mask, s)
        pos_dev = positions.to(dev)
        logits = self._prefill_rows(ids, pos_dev)
        self.cache.advance(s)
        # state for the loop body: cur_len = S (also the sampler's Philox step), token/pos of the
        # last prompt position
        self.cur_len.fill_(s)
        nxt = self._next_token(logits)
        self.positions.copy_(pos_dev[:, -1:])
        # _update writes sequences[:, S], advances pos (+1), slot (+1 -> S+1 ... ) and cur_len.
        # The prefill already advanced the slot by S; undo the update's +1 on the slot.
        self.cache.index_t.sub_(1)
        self._update(nxt)
        self.cache.index = s  # host mirror (decode steps track the slot on the device)
        return s + 1

    def _set_processors(self, mask: torch.Tensor, s: int):
        """This call's processor state, into the buffers the captured step reads: each row's history start (its first
        attended prompt column: left padding is not history, a later hole is), the stop and suppress ids and the
        minimum-length word."""
        gc = self.gc
        self._processors = processors_active(gc)
        self._stop_set = isinstance(gc.eos_token_id, (list, tuple))
        if not (self._processors or self._stop_set):
            return
        first = torch.where(mask.bool().any(1), mask.ne(0).to(torch.int32).argmax(1), torch.full((mask.shape[0],), s))
        self.hist_start.copy_(first.to(torch.int32))
        self.stop_ids.copy_(ops.id_buffer(stop_ids(gc), ops.PROC_MAX_STOP, "cpu"))
        self.suppress_ids.copy_(ops.id_buffer(suppressed_ids(gc), ops.PROC_MAX_SUPPRESS, "cpu"))
        self.min_len.fill_(max(int(gc.min_length), s + int(gc.min_new_tokens)))

    def _prefill_rows(self, ids: torch.Tensor, pos_dev: torch.Tensor):
        """The prompt forward, in row chunks of at most PREFILL_TOKENS tokens: every kernel then sees at most the
        token count the GEMMs already saturate the chip with (M = 262144: 2048 rows x 128), whatever the batch, and no
        activation index of a larger batch can pass 2^31 elements. One chunk up to that size (the common case)."""
        b, s = ids.shape
        rows = max(1, PREFILL_TOKENS // max(1, s))
        mode = self._logits_mode()
        if b <= rows:
            logits, *_ = self.model.forward_tokens(ids, pos_dev, self.cache, 0, self.kv_start, self.key_mask,
                                                   logits_mode=mode)
            return logits
        parts = []
        for b0 in range(0, b, rows):
            b1 = min(b, b0 + rows)
            km = self.key_mask[b0:b1] if self.key_mask is not None else None
            lg, *_ = self.model.forward_tokens(ids[b0:b1], pos_dev[b0:b1], self.cache.rows(b0, b1), 0,
                                               self.kv_start[b0:b1], km, logits_mode=mode)
            parts.append(lg)
        if isinstance(parts[0], tuple):  # greedy: (idx, val) per chunk
            return tuple(torch.cat([p[i] for p in parts]) for i in range(len(parts[0])))
        return torch.cat(parts)

    def prefill_only(self, input_ids, attention_mask, gc: GenerationConfig) -> int:
        """Prefill + first token only (time-to-first-token measurement)."""
        self.gc = gc
        return self.prefill(input_ids, attention_mask)

    def _graph_state(self):
        # the graph records buffer addresses (the scratch workspaces of ops.workspace; the state buffers and a holed key
        # mask are this engine's own, fixed ones), the sampling mode, and the scalars its launches take by value:
        # pad and eos (decode_update) and the sampler's settings (topk_merge). A call with other values captures again
        # (so does every new seed of a sampling caller: the seed is a launch argument, not a device word).
        # With processors or a stop list the key grows by their by-value arguments: the penalty (and with it 1 / p)
        # and the n-gram size. The ids, the minimum length and the history starts are read from this engine's buffers.
        gc = self.gc
        sampler = (gc.top_k, gc.temperature, gc.top_p, int(gc.seed)) if gc.do_sample else None
        key = (gc.do_sample, self.key_mask is not None, ops.workspace.generation, _fused_greedy(),
               ops.ARGMAX_FUSED_MIN_M, ops.SKINNY_ARGMAX, ops.QKV_ATTN, self.model.comm.reduce_dtype,
               int(gc.pad_token_id), None if self._stop_set else int(gc.eos_token_id), sampler)
        if self._processors or self._stop_set:
            proc = (float(gc.repetition_penalty), int(gc.no_repeat_ngram_size)) if self._processors else None
            key += (self._stop_set, proc)
        return key

    def _ensure_graph(self):
        if self._graph is not None and self._graph_key == self._graph_state():
            return
        for _ in range(3):
            key = self._graph_state()
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph(keep_graph=self.keep_graph)
            # Capture records kernels without executing them; state buffers are static.
            with torch.cuda.graph(g):
                self._decode_step()
            self._graph, self._graph_key = g, key
            if self._graph_state() == key:  # no workspace grew while capturing
                return
        raise RuntimeError("decode graph capture keeps reallocating workspaces")

    def _poll(self) -> bool:
        """Host poll (every ``check_every`` steps): True once every row has finished. Also raises if a
        custom TP collective gave up waiting for a peer."""
        done = bool(self.finished.all().item())
        self._check()
        return done

    def _check(self):
        """Device-side failure words: a custom TP collective that gave up on a peer (comm.check), an in-launch wait
        that timed out (ops.check_inlaunch: the fused qkv + attention launch), out-of-range indices (debug build)."""
        self.model.comm.check()
        if self.device.type == "cuda":
            ops.check_inlaunch()
        ops.check_bounds()  # bounds-checked debug build only (JLA_DEBUG_BOUNDS=1): out-of-range device indices

    def run(self, input_ids, attention_mask, gc: GenerationConfig) -> torch.Tensor:
        validate_processors(gc, self.model.vocab_local * self.model.comm.size)
        self.gc = gc
        rng_saved = None
        if gc.do_sample:
            self._gen = torch.Generator(device=self.device)
            self._gen.manual_seed(int(gc.seed))
            if self.use_graph:
                # The on-device sampler (ops.topk_sample, top_k <= 64) draws from its own Philox stream keyed by
                # (seed, step) and touches no torch RNG. The torch fallback (top_k = 0 or > 64) under graph capture
                # needs the device's default generator (graph-safe philox offsets): seed it for this call and give
                # the caller's RNG state back afterwards.
                self._gen = None
                if self.device.type == "cuda":
                    rng_saved = torch.cuda.get_rng_state(self.device)
                    torch.cuda.manual_seed(int(gc.seed))
        try:
            return self._run(input_ids, attention_mask)
        except Exception:
            # a failed step (a peer or in-launch timeout, an error mid-decode) can leave non-finite rows in this
            # engine's cache beyond where the next prompt writes; the kernels mask keys past the valid length by
            # probability 0, and 0 x NaN is NaN: zero the cache so the next call starts as from a fresh engine
            self.cache.zero_()
            raise
        finally:
            if rng_saved is not None:
                torch.cuda.set_rng_state(rng_saved, self.device)

    def _run(self, input_ids, attention_mask) -> torch.Tensor:
        cur = self.prefill(input_ids, attention_mask)
        steps_left = self.max_length - cur
        done = steps_left <= 0
        first = True
        step = 0
        while not done:
            if self.use_graph and not first:
                self._ensure_graph()
                self._graph.replay()
            else:
                self._decode_step()  # first step eager: warms up workspaces before capture
                first = False
            step += 1
            steps_left -= 1
            if steps_left <= 0:
                break
            if step % self.check_every == 0 and self._poll():
                break
        self._check()
        return self.sequences


class BeamEngine(DecodeEngine):
    """Beam search (``num_beams = K > 1``) over ``B * K`` cache rows, row ``b*K + j`` = beam j of prompt b. The
    definition is HF Flax ``_beam_search`` as written out in the README's "Beam search" section and in
    ``ops/reference.py`` (``beam_step`` / ``beam_continue``); scores are multiplied by ``1 / t ** length_penalty``
    (one fp32 table, ``ref.beam_inv_pen``) where HF divides by the power: at most one rounding apart.

    All beams of a search have the same length, so the one device slot counter stays. A decode step is the forward,
    ``topk_candidates(2K)``, the rows' log-sum-exp, ``beam_alive`` + ``beam_step`` (the selection and the whole state
    update, on the device) and ``kv_beam_reorder`` (every beam's cache rows follow its parent): fixed-shape, captured
    once and replayed. Once the loop condition fails (``alive == 0``) a replayed step changes nothing, so the host
    polls ``alive`` only every ``check_every`` steps."""

    def __init__(self, model, batch_size: int, num_beams: int, max_length: int, use_graph: Optional[bool] = None,
                 check_every: int = 16):
        if model.comm.size > 1:
            raise NotImplementedError("beam search under tensor parallelism (vocab-parallel logits) is not supported")
        if not 2 <= num_beams <= ops.BEAM_MAX:
            raise ValueError(f"num_beams must be in [2, {ops.BEAM_MAX}], got {num_beams}")
        super().__init__(model, batch_size * num_beams, max_length, use_graph, check_every)
        self.nb, self.k = batch_size, num_beams
        dev = self.device
        self.running_seq = self.sequences.view(batch_size, num_beams, max_length)
        self.seq = torch.zeros_like(self.running_seq)
        self.running_score = torch.zeros(batch_size, num_beams, dtype=torch.float32, device=dev)
        self.score = torch.zeros_like(self.running_score)
        self.is_finished = self.finished.view(batch_size, num_beams)
        self.alive = torch.ones(1, dtype=torch.int32, device=dev)
        self.beam_idx = torch.zeros(batch_size * num_beams, dtype=torch.int32, device=dev)
        self.inv_pen = torch.ones(max_length + 1, dtype=torch.float32, device=dev)
        self.prompt_len = 0
        self.reorder = ops.kv_beam_reorder  # (cache, beam_idx, K), in place
        self.beam_idx_log: Optional[list] = None  # eager runs: a list here receives every step's beam_idx (CPU copy)

    def _beam_select(self, logits: torch.Tensor):
        gc, k = self.gc, self.k
        logits = logits.float().contiguous()
        cand_v, cand_i = ops.topk_candidates(logits, 2 * k)
        lse = ops.row_lse(logits)
        ops.beam_alive(self.running_score, self.score, self.is_finished, self.inv_pen, self.cur_len, self.alive,
                       self.max_length, self.prompt_len, gc.early_stopping, float(gc.length_penalty))
        ops.beam_step(cand_v.contiguous(), cand_i.to(torch.int32).contiguous(), lse, self.running_seq, self.seq,
                      self.running_score, self.score, self.is_finished, self.inv_pen, self.cur_len, self.cache.index_t,
                      self.tokens, self.positions, self.alive, self.beam_idx, self.prompt_len,
                      int(gc.eos_token_id), gc.early_stopping)
        self.reorder(self.cache, self.beam_idx, k)
        if self.beam_idx_log is not None and not self.use_graph:
            self.beam_idx_log.append(self.beam_idx.cpu().clone())

    def _decode_step(self):
        logits, *_ = self.model.forward_tokens(self.tokens, self.positions, self.cache, self.cache.index_t,
                                               self.kv_start, self.key_mask, logits_mode="last")
        self._beam_select(logits)

    def prefill(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor]):
        """The B prompts run once into a temporary B-row cache of length S, which is then broadcast into the ``B*K``-row
        cache; the first beam step runs on the prefill logits replicated K times (the ``[0, -1e7, ...]`` initial
        running scores make that equal to a K-fold prefill)."""
        from ..models.llama import mask_to_kv_start
        model, dev, gc, k = self.model, self.device, self.gc, self.k
        ids = input_ids.to(dev, torch.int32)
        b, s = ids.shape
        assert b == self.nb and s < self.max_length
        if 2 * k > model.vocab_local:
            raise ValueError(f"num_beams {k} needs a vocabulary of at least {2 * k} entries")
        mask = torch.ones(b, s, dtype=torch.int32) if attention_mask is None else attention_mask.to("cpu", torch.int32)
        pos_dev = (mask.cumsum(-1) - 1).to(torch.int32).to(dev)
        # the prompts, once
        tmp = model.init_cache(b, s)
        kv_start_b, key_mask_b = mask_to_kv_start(mask, dev)
        rows = max(1, PREFILL_TOKENS // max(1, s))
        parts = []
        for b0 in range(0, b, rows):
            b1 = min(b, b0 + rows)
            km = key_mask_b[b0:b1] if key_mask_b is not None else None
            lg, *_ = model.forward_tokens(ids[b0:b1], pos_dev[b0:b1], tmp.rows(b0, b1), 0, kv_start_b[b0:b1], km,
                                          logits_mode="last")
            parts.append(lg)
        logits = parts[0] if len(parts) == 1 else torch.cat(parts)
        # ... broadcast to the K beams of each prompt
        self.cache.reset()
        for dst, src in zip(ops.kv_beam_tensors(self.cache), ops.kv_beam_tensors(tmp)):
            dst.unflatten(1, (b, k))[:, :, :, :, :s].copy_(src.unsqueeze(2))
        del tmp
        self.cache.advance(s)
        ext_mask = torch.ones(b, self.max_length, dtype=torch.int32)
        ext_mask[:, :s] = mask
        kv_start, key_mask = mask_to_kv_start(ext_mask.repeat_interleave(k, 0), dev)
        self.kv_start.copy_(kv_start)
        if key_mask is not None:
            if self._key_mask_buf is None:
                self._key_mask_buf = torch.empty_like(key_mask)
            self._key_mask_buf.copy_(key_mask)
            key_mask = self._key_mask_buf
        self.key_mask = key_mask
        # the search state
        self.prompt_len = s
        self.inv_pen.copy_(ref.beam_inv_pen(self.max_length, float(gc.length_penalty)))
        self.running_seq.fill_(gc.pad_token_id)
        self.running_seq[:, :, :s] = ids[:, None]
        self.seq.copy_(self.running_seq)
        self.running_score.fill_(ref.BEAM_NEG)
        self.running_score[:, 0] = 0.0
        self.score.fill_(ref.BEAM_NEG)
        self.is_finished.zero_()
        self.alive.fill_(1)
        self.cur_len.fill_(s)
        self.positions.copy_(pos_dev[:, -1:].repeat_interleave(k, 0))
        # beam_step advances the slot; the prefill already counted the S prompt slots
        self.cache.index_t.sub_(1)
        self._beam_select(logits.repeat_interleave(k, 0))
        self.cache.index = s
        return s + 1

    def _graph_state(self):
        # by-value launch arguments of the captured step: K, S, eos, early_stopping and whether length_penalty > 0 with
        # "never" (beam_alive); pad and length_penalty are listed although the step reads them from device buffers
        gc = self.gc
        return (self.k, self.prompt_len, float(gc.length_penalty), gc.early_stopping, int(gc.pad_token_id),
                int(gc.eos_token_id), self.cache.kv_format, self.key_mask is not None, ops.workspace.generation,
                ops.QKV_ATTN, self.model.comm.reduce_dtype)

    def _poll(self) -> bool:
        done = not bool(self.alive.item())  # the last step found the loop condition false and changed nothing
        self._check()
        return done

    def _run(self, input_ids, attention_mask):
        super()._run(input_ids, attention_mask)
        any_fin = self.is_finished.bool().any(1)
        seqs = torch.where(any_fin[:, None, None], self.seq, self.running_seq)
        scores = torch.where(any_fin[:, None], self.score, self.running_score)
        n = self.gc.num_return_sequences
        return seqs[:, :n].reshape(-1, self.max_length).clone(), scores[:, :n].reshape(-1).clone()


_ENGINES: "OrderedDict" = OrderedDict()


def _engine_budget(model) -> int:
    """Bytes of KV cache the engine cache may keep alive (``JLA_ENGINE_CACHE_GB`` or 40 % of the device)."""
    env = os.environ.get("JLA_ENGINE_CACHE_GB")
    if env:
        return int(float(env) * (1 << 30))
    if model.device.type == "cuda":
        return int(0.4 * torch.cuda.get_device_properties(model.device).total_memory)
    return 8 << 30


def drop_engines(model) -> int:
    """Forget every cached engine of ``model`` (``quantize_weights_`` calls it: an engine's captured decode graph holds
    the addresses of the weights it was captured on). Returns how many were dropped."""
    keys = [k for k in _ENGINES if k[0] == id(model)]
    for k in keys:
        del _ENGINES[k]
    return len(keys)


def get_engine(model, batch_size: int, max_length: int, num_beams: int = 1) -> DecodeEngine:
    """Per-(model, B, max_length, num_beams) engines (each owns a KV cache and a captured decode graph), kept in
    LRU order and bounded by the bytes of their KV caches. The model's KV-cache format is part of the key: an engine
    owns a cache of one format. ``num_beams > 1``: a BeamEngine over ``B * num_beams`` cache rows."""
    fmt = getattr(model, "kv_cache_format", "bf16")
    key = (id(model), batch_size, max_length, fmt, num_beams)
    eng = _ENGINES.get(key)
    if eng is not None:
        _ENGINES.move_to_end(key)
        return eng
    need = (model.config.num_hidden_layers * 2 * batch_size * num_beams * model.n_kv_heads * max_length *
            kv_row_bytes(fmt, model.head_dim))
    budget = _engine_budget(model)
    held = sum(e.cache.nbytes() for e in _ENGINES.values())
    while _ENGINES and held + need > budget:
        _, old = _ENGINES.popitem(last=False)
        held -= old.cache.nbytes()
        del old
    eng = (DecodeEngine(model, batch_size, max_length) if num_beams == 1
           else BeamEngine(model, batch_size, num_beams, max_length))
    _ENGINES[key] = eng
    return eng


def generate(model, input_ids, attention_mask=None, generation_config: Optional[GenerationConfig] = None,
             prng_key=None, **kwargs) -> GenerateOutput:
    # never mutate the caller's config (HF semantics: generate works on a copy)
    gc = dataclasses.replace(generation_config) if generation_config is not None else GenerationConfig()
    for k, v in kwargs.items():
        if hasattr(gc, k):
            setattr(gc, k, v)
    beams = gc.num_beams != 1
    if beams:
        if not isinstance(gc.num_beams, int) or not 2 <= gc.num_beams <= ops.BEAM_MAX:
            raise ValueError(f"num_beams must be 1 (no beam search) or in [2, {ops.BEAM_MAX}], got {gc.num_beams!r}")
        if gc.do_sample:
            raise ValueError("beam search does not sample: num_beams > 1 needs do_sample=False")
        if not 1 <= gc.num_return_sequences <= gc.num_beams:
            raise ValueError(f"num_return_sequences must be in [1, num_beams], got {gc.num_return_sequences}")
        ref.beam_early_code(gc.early_stopping)  # ValueError for anything but True / False / "never"
        if model.comm.size > 1:
            raise NotImplementedError("beam search under tensor parallelism (vocab-parallel logits) is not supported")
    ids = input_ids if torch.is_tensor(input_ids) else torch.as_tensor(input_ids)
    b, s = ids.shape
    if gc.max_length is None:
        gc.max_length = s + (gc.max_new_tokens if gc.max_new_tokens is not None else 20)
    if gc.pad_token_id is None:
        gc.pad_token_id = model.config.pad_token_id if model.config.pad_token_id >= 0 else 0
    if gc.eos_token_id is None:
        gc.eos_token_id = model.config.eos_token_id
    if isinstance(gc.eos_token_id, (list, tuple)):
        gc.eos_token_id = list(gc.eos_token_id)
    validate_processors(gc, model.config.vocab_size)
    if prng_key is not None:
        gc.seed = int(prng_key) if not torch.is_tensor(prng_key) else int(prng_key.reshape(-1)[0])
    if s >= gc.max_length:
        out = ids.to(model.device, torch.int32)[:, : gc.max_length]
        if beams:  # nothing to generate: every hypothesis is its prompt, with score 0
            n = gc.num_return_sequences
            return GenerateOutput(sequences=out.repeat_interleave(n, 0),
                                  scores=torch.zeros(b * n, dtype=torch.float32, device=model.device))
        return GenerateOutput(sequences=out)
    eng = get_engine(model, b, gc.max_length, gc.num_beams)
    res = eng.run(ids, attention_mask if attention_mask is None or torch.is_tensor(attention_mask)
                  else torch.as_tensor(attention_mask), gc)
    if beams:
        return GenerateOutput(sequences=res[0], scores=res[1])
    return GenerateOutput(sequences=res.clone())
