"""``LLaMA`` text generator — same API and post-processing as the reference
(``/root/reference/jax_llama/generation.py:15-79``):

  * ``generate(tokens, attention_mask, max_gen_len, temperature=0.8, top_p=0.95)`` builds a
    generation config with ``do_sample = temperature != 0``, ``max_length = S + max_gen_len``,
    ``pad = eos = tokenizer.eos_id`` and the HF default top-k of 50 (``:28-41``);
  * ``generate_from_str(prompts, ...)`` encodes with BOS, **left-pads with eos_id**, uses
    ``mask = tokens != eos_id`` and decodes each row from its first BOS, cut to
    ``len(prompt) + max_gen_len`` and at the first EOS — the prompt is included (``:47-79``).

Differences by design: no debug prints; the decode loop runs on the hipGraph engine; with
tensor parallelism every rank calls these methods (SPMD) and rank-0's tokenizer output is
what is returned everywhere (token ids are identical on all ranks by construction).
"""
from __future__ import annotations

from typing import Any, List, Optional, Tuple, Union

import torch

from .parallel.partition import P, Mesh, gather_dp, with_named_sharding_constraint
from .runtime.engine import GenerationConfig


class LLaMA:
    def __init__(self, params: Optional[Any], model, tokenizer, mesh: Optional[Mesh] = None):
        self.params = params
        self.model = model
        self.tokenizer = tokenizer
        self.mesh = mesh

    def generate(self, tokens, attention_mask, max_gen_len: int, temperature: float = 0.8,
                 top_p: float = 0.95, seed: int = 0, num_beams: int = 1, length_penalty: float = 1.0,
                 early_stopping=False, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
                 min_new_tokens: int = 0, stop_token_ids=None) -> torch.Tensor:
        """``num_beams > 1``: beam search (``runtime/engine.py`` BeamEngine); it does not sample, so ``temperature``
        must then be 0. Returns each prompt's best hypothesis.

        ``repetition_penalty`` / ``no_repeat_ngram_size`` / ``min_new_tokens``: the logits processors of the README's
        "Logits processors" section. ``stop_token_ids`` (1 to 8 ids, e.g. the Llama-3 tokenizer's ``stop_tokens``): a
        row stops on any of them; without it the stop set is ``tokenizer.eos_id`` alone, as before."""
        if num_beams != 1 and temperature != 0.0:
            raise ValueError("beam search does not sample: num_beams > 1 needs temperature=0")
        tokens = torch.as_tensor(tokens, dtype=torch.int32) if not torch.is_tensor(tokens) else tokens
        attention_mask = (torch.as_tensor(attention_mask, dtype=torch.int32)
                          if not torch.is_tensor(attention_mask) else attention_mask)
        tokens = with_named_sharding_constraint(tokens, self.mesh, P("dp", None))
        attention_mask = with_named_sharding_constraint(attention_mask, self.mesh, P("dp", None))
        gc = GenerationConfig(
            num_beams=num_beams,
            length_penalty=length_penalty,
            early_stopping=early_stopping,
            do_sample=temperature != 0.0,
            max_length=max_gen_len + tokens.shape[1],
            pad_token_id=self.tokenizer.eos_id,
            eos_token_id=self.tokenizer.eos_id if stop_token_ids is None else sorted(int(t) for t in stop_token_ids),
            repetition_penalty=repetition_penalty,
            no_repeat_ngram_size=no_repeat_ngram_size,
            min_new_tokens=min_new_tokens,
            temperature=temperature,
            top_p=top_p,
            seed=seed,
        )
        out = self.model.generate(tokens, attention_mask=attention_mask, generation_config=gc)
        # the reference's output constraint P("dp", None) keeps the batch split across dp replicas;
        # here every replica gets the whole batch back (all-gather over the dp group when there is one)
        return gather_dp(out.sequences, self.mesh)

    def loglikelihood(self, pairs: List[Tuple[str, str]]) -> List[Tuple[float, bool]]:
        """``(log p(continuation | context), continuation is what greedy decoding would produce)`` per
        ``(context, continuation)`` pair -- the evaluation-harness request behind multiple-choice tasks. The context is
        encoded with BOS, the continuation without; rows are left-padded and carry an explicit length mask (no token
        id stands for padding). One ``model.score`` call; with a mesh every replica scores every pair. A pair longer
        than ``max_sequence_length``, the context the model was trained for, is an error here (``score`` itself, like
        ``generate``, goes as far as the RoPE table)."""
        tok = self.tokenizer
        enc = [(tok.encode(c, bos=True, eos=False), tok.encode(x, bos=False, eos=False)) for c, x in pairs]
        if not enc:
            return []
        longest = max(len(c) + len(x) for c, x in enc)
        limit = self.model.config.max_sequence_length
        if longest > limit:
            raise ValueError(f"loglikelihood: a pair of {longest} tokens exceeds max_sequence_length ({limit})")
        width = max(longest, 2)  # (score needs two positions; a lone BOS row is padded)
        tokens = torch.zeros(len(enc), width, dtype=torch.int32)
        mask = torch.zeros(len(enc), width, dtype=torch.int32)
        for i, (c, x) in enumerate(enc):
            row = c + x
            tokens[i, width - len(row):] = torch.tensor(row, dtype=torch.int32)
            mask[i, width - len(row):] = 1
        out = self.model.score(tokens, attention_mask=mask)
        lp, greedy = out.token_logprobs.double().cpu(), out.is_greedy.cpu()
        res = []
        for i, (c, x) in enumerate(enc):
            n = len(x)  # the continuation's tokens are the row's last n: entries width-1-n .. width-2
            res.append((float(lp[i, width - 1 - n:].sum()) if n else 0.0,
                        bool(greedy[i, width - 1 - n:].all()) if n else True))
        return res

    def generate_from_str(self, prompts: List[str], max_gen_len: int, temperature: float = 0.8,
                          top_p: float = 0.95, seed: int = 0, num_beams: int = 1, length_penalty: float = 1.0,
                          early_stopping=False, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0,
                          min_new_tokens: int = 0, stop_token_ids=None) -> List[str]:
        """``stop_token_ids``: each completion is cut at the first of any of them (default: at ``eos_id``)."""
        tok = self.tokenizer
        prompt_tokens = [tok.encode(x, bos=True, eos=False) for x in prompts]
        max_prompt = max(len(t) for t in prompt_tokens)
        tokens = torch.full((len(prompts), max_prompt), tok.eos_id, dtype=torch.int32)
        for i, t in enumerate(prompt_tokens):
            tokens[i, max_prompt - len(t):] = torch.tensor(t, dtype=torch.int32)  # left pad
        attention_mask = (tokens != tok.eos_id).to(torch.int32)
        out_tokens = self.generate(tokens, attention_mask, max_gen_len, temperature, top_p, seed, num_beams,
                                   length_penalty, early_stopping, repetition_penalty, no_repeat_ngram_size,
                                   min_new_tokens, stop_token_ids)
        stops = {tok.eos_id} if stop_token_ids is None else {int(t) for t in stop_token_ids}
        # rows of this dp replica only when the outputs could not be gathered (no process group)
        row0 = 0 if out_tokens.shape[0] == len(prompts) else self.mesh.dp_rank * out_tokens.shape[0]
        decoded = []
        for i, t in enumerate(out_tokens.tolist()):
            t = t[t.index(tok.bos_id):]
            t = t[: len(prompt_tokens[row0 + i]) + max_gen_len]
            # a stop list is looked for in the completion only (a chat prompt holds end-of-turn tokens of its own)
            first = 0 if stop_token_ids is None else len(prompt_tokens[row0 + i])
            cut = [j for j in range(first, len(t)) if t[j] in stops]
            if cut:
                t = t[: cut[0]]
            decoded.append(tok.decode(t))
        return decoded
