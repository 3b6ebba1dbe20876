"""The plan resolver of decode attention (csrc/kernels/attn_plan.h, asked through ``attn_decode_plan_check``): which
shape is served, which of the five kernels (v2 .. v6) runs it with what geometry, how many key splits, whether the
launch may write the packed output copy, and the workspace it is given.

Host calls only (milliseconds); marked gpu because ``_C`` links the HIP runtime.

Every expectation below was derived by reading csrc/kernels/attn_decode.hip, attn_decode_mma.hip and
``ops.attention_packs`` as they stood before the resolver existed, not by running the new function: once as literal
plans at the smallest shapes on each side of every threshold (``RULES``), and once as ``_parent_choice``, a line-by-line
transcription of the ``use_v*`` predicates, ``attn_decode_splits`` / ``attn_decode_packs``, the launcher (its ``-3``
checks, the in-launcher v4 condition, the ladders' template arguments) and Python's ``bsz > 32`` line, compared over a
grid of shapes under every knob state the tests and tools set.

One difference is intended, and asserted as a set: rep 8, at least 2048 (row, kv head) pairs, at most 32 rows and a key
mask. There the parent's ``attention_packs`` said yes and the launch with the packed copy then failed with ``-3``
(``PACKS_THEN_REFUSED``); the plan knows the mask, reports no packed copy and runs v2."""
from __future__ import annotations

import itertools

import pytest

from jax_llama_amd import ops

pytestmark = pytest.mark.gpu
F, T = False, True
DH = 128
BAD = (-1, "", 0, F, 0, 0, 0, 0, 0)
PACKS_THEN_REFUSED = "packs, then -3"


def _form(e, b, h, hkv, dh, t_cap, masked):
    """(rc, kernel, nsplit, packs, kpg, ring, fold, wpp, split_len) of the plan; BAD whatever else a refusal carries."""
    rc, why, kernel, nsplit, packs, _ws, _tickets, _rep, kpg, ring, fold, wpp, split_len = e.attn_decode_plan_check(
        b, h, hkv, dh, t_cap, masked)
    if rc != 0:
        assert rc == -1 and why, (rc, why)  # a refusal names its rule
        return BAD
    return (rc, kernel, nsplit, bool(packs), kpg, ring, fold, wpp, split_len)


def _apply(target, calls):
    for name, args in calls:
        getattr(target, name)(*args)


V6_OFF = [("attn_set_v6", (0,))]
V6_ALL = [("attn_set_v6", (2,))]
V2_FORCED = [("attn_set_impl", (2, -1)), ("attn_set_v5_max_pairs", (0,)), ("attn_set_v3_max_pairs", (0,))]

# (the rule, knob calls, (B, H, Hkv, Dh, t_cap, masked), (rc, kernel, nsplit, packs, kpg, ring, fold, wpp, split_len))
RULES = [
    # --- what is served at all
    ("Dh 64", [], (1, 8, 2, 64, 384, F), BAD),
    ("H not a multiple of Hkv", [], (1, 5, 2, DH, 384, F), BAD),
    ("rep 3", [], (1, 6, 2, DH, 384, F), BAD),
    ("rep 3 at a large batch (the parent fell out of the v4 and v2 ladders)", [], (512, 24, 8, DH, 384, F), BAD),
    ("rep 32", [], (1, 64, 2, DH, 384, F), BAD),
    ("rep 32 even with v6 forced", V6_ALL, (1, 64, 2, DH, 384, F), BAD),
    # --- v6 by shape: rep >= 8, 8 <= pairs < 2048; 2 waves per pair
    ("rep 8, 7 pairs: below v6, v5 with KPG 2 (32-key splits), fold 4 below 16 pairs", [],
     (7, 8, 1, DH, 384, F), (0, "v5", 12, T, 2, 0, 4, 0, 0)),
    ("rep 8, 8 pairs: v6", [], (8, 8, 1, DH, 384, F), (0, "v6", 1, T, 0, 0, 0, 2, 0)),
    ("rep 16, 8 pairs: v6", [], (4, 32, 2, DH, 384, F), (0, "v6", 1, T, 0, 0, 0, 2, 0)),
    ("rep 4, 8 pairs: not v6", [], (8, 4, 1, DH, 384, F), (0, "v5", 6, T, 4, 0, 4, 0, 0)),
    ("rep 8, 2047 pairs: v6", [], (23, 712, 89, DH, 384, F), (0, "v6", 1, T, 0, 0, 0, 2, 0)),
    ("rep 8, 2048 pairs: the mid-batch rule, v4 (KPG 2, 4 slots), packs at B <= 64", [],
     (32, 512, 64, DH, 384, F), (0, "v4", 1, T, 2, 4, 0, 0, 0)),
    ("... with a key mask: v2 (KPG 2, 4 slots), one split, no packed copy (the parent: packs, then -3)", [],
     (32, 512, 64, DH, 384, T), (0, "v2", 1, F, 2, 4, 0, 0, 384)),
    ("v6 forced: every supported rep", V6_ALL, (1, 2, 2, DH, 384, F), (0, "v6", 1, T, 0, 0, 0, 2, 0)),
    ("v6 forced, 4095 pairs: 2 waves per pair", V6_ALL, (21, 1560, 195, DH, 64, F), (0, "v6", 1, T, 0, 0, 0, 2, 0)),
    ("v6 forced, 4096 pairs: 1", V6_ALL, (32, 1024, 128, DH, 64, F), (0, "v6", 1, T, 0, 0, 0, 1, 0)),
    ("... unless pinned", V6_ALL + [("attn_set_v6_wpp", (8,))], (32, 1024, 128, DH, 64, F),
     (0, "v6", 1, T, 0, 0, 0, 8, 0)),
    ("a pin that is no power of two <= 8 is none", V6_ALL + [("attn_set_v6_wpp", (3,))], (1, 2, 2, DH, 384, F),
     (0, "v6", 1, T, 0, 0, 0, 2, 0)),
    # --- v5: pairs <= 64 (256 at rep >= 8); KPG 8 / 8 / 4 / 2 / 1; splits of 16 x KPG keys; fold 4 / 12 at 15 / 16
    ("rep 1: 128-key splits", [], (1, 2, 2, DH, 129, F), (0, "v5", 2, T, 8, 0, 4, 0, 0)),
    ("rep 2: 128-key splits", [], (1, 4, 2, DH, 128, F), (0, "v5", 1, T, 8, 0, 4, 0, 0)),
    ("rep 4, 15 pairs: fold 4", [], (15, 4, 1, DH, 384, F), (0, "v5", 6, T, 4, 0, 4, 0, 0)),
    ("rep 4, 16 pairs: fold 12", [], (16, 4, 1, DH, 384, F), (0, "v5", 6, T, 4, 0, 12, 0, 0)),
    ("... pinned to 4", [("attn_set_v5_fold", (4,))], (16, 4, 1, DH, 384, F), (0, "v5", 6, T, 4, 0, 4, 0, 0)),
    ("... a pin other than 4 / 12 is none", [("attn_set_v5_fold", (8,))], (16, 4, 1, DH, 384, F),
     (0, "v5", 6, T, 4, 0, 12, 0, 0)),
    ("rep 4, 64 pairs: v5, before the mid-batch rule is asked", [], (64, 4, 1, DH, 384, F),
     (0, "v5", 6, T, 4, 0, 12, 0, 0)),
    ("rep 4, 65 pairs: v3, x2 chunks (KPG 4) up to 128 pairs", [], (13, 20, 5, DH, 384, F),
     (0, "v3", 1, T, 4, 0, 0, 0, 0)),
    ("rep 8 without v6, 256 pairs: v5 (4 x 64)", V6_OFF, (32, 64, 8, DH, 384, F), (0, "v5", 12, T, 2, 0, 12, 0, 0)),
    ("rep 8 without v6, 257 pairs: v3, KPG 1", V6_OFF, (1, 2056, 257, DH, 384, F), (0, "v3", 1, T, 1, 0, 0, 0, 0)),
    ("rep 16 without v6, 256 pairs: v5, 16-key splits", V6_OFF, (32, 128, 8, DH, 384, F),
     (0, "v5", 24, T, 1, 0, 12, 0, 0)),
    ("rep 16 without v6, 257 pairs: v2 (KPG 1, 4 slots), 8 splits wanted, 6 of >= 64 keys fit", V6_OFF,
     (1, 4112, 257, DH, 384, F), (0, "v2", 6, F, 1, 4, 0, 0, 64)),
    ("v5 off", [("attn_set_v5_max_pairs", (0,))], (1, 8, 2, DH, 384, F), (0, "v3", 1, T, 4, 0, 0, 0, 0)),
    ("v5 up to 4096 pairs: ahead of v3 and of the mid-batch rule", [("attn_set_v5_max_pairs", (4096,))],
     (512, 32, 8, DH, 384, F), (0, "v5", 6, T, 4, 0, 12, 0, 0)),
    ("attn_set_v5_max_pairs(-1): the default", [("attn_set_v5_max_pairs", (4096,)), ("attn_set_v5_max_pairs", (-1,))],
     (13, 20, 5, DH, 384, F), (0, "v3", 1, T, 4, 0, 0, 0, 0)),
    # --- v3: rep <= 8, outside the v2 / v4 range, pairs <= 4096; KPG min(min(8, 16 / rep), (8 / rep) x mult)
    ("rep 1: KPG 8 whatever the multiplier", [("attn_set_v3_kpg", (1,))], (13, 5, 5, DH, 384, F),
     (0, "v3", 1, T, 8, 0, 0, 0, 0)),
    ("rep 2, 128 pairs: x2, KPG 8", [], (32, 8, 4, DH, 384, F), (0, "v3", 1, T, 8, 0, 0, 0, 0)),
    ("rep 2, 129 pairs: x1, KPG 4", [], (3, 86, 43, DH, 384, F), (0, "v3", 1, T, 4, 0, 0, 0, 0)),
    ("rep 4, 128 pairs: KPG 4", [], (32, 16, 4, DH, 384, F), (0, "v3", 1, T, 4, 0, 0, 0, 0)),
    ("rep 4, 129 pairs: KPG 2", [], (3, 172, 43, DH, 384, F), (0, "v3", 1, T, 2, 0, 0, 0, 0)),
    ("... x4 pinned: capped at rep x KPG = 16", [("attn_set_v3_kpg", (4,))], (3, 172, 43, DH, 384, F),
     (0, "v3", 1, T, 4, 0, 0, 0, 0)),
    ("rep 8 without v6, 128 pairs: KPG 2", V6_OFF + [("attn_set_v5_max_pairs", (0,))], (32, 32, 4, DH, 384, F),
     (0, "v3", 1, T, 2, 0, 0, 0, 0)),
    ("rep 8 without v6, 129 pairs: KPG 1", V6_OFF + [("attn_set_v5_max_pairs", (0,))], (3, 344, 43, DH, 384, F),
     (0, "v3", 1, T, 1, 0, 0, 0, 0)),
    ("rep 4, 4095 pairs at 21 rows: v3", [], (21, 780, 195, DH, 384, F), (0, "v3", 1, T, 2, 0, 0, 0, 0)),
    ("rep 4, 4096 pairs at 32 rows: the v2 / v4 range; v4 (KPG 4, 3 slots) outside the mid-batch rule never packs", [],
     (32, 512, 128, DH, 384, F), (0, "v4", 1, F, 4, 3, 0, 0, 0)),
    # --- the mid-batch rule: rep <= 4 above 32 rows, rep 8 from 2048 pairs; one split
    ("rep 4, 32 rows: v3", [], (32, 32, 8, DH, 384, F), (0, "v3", 1, T, 2, 0, 0, 0, 0)),
    ("rep 4, 33 rows: v4, packs", [], (33, 32, 8, DH, 384, F), (0, "v4", 1, T, 4, 3, 0, 0, 0)),
    ("... with a key mask: v2 (KPG 8, 2 slots), one split", [], (33, 32, 8, DH, 384, T),
     (0, "v2", 1, F, 8, 2, 0, 0, 384)),
    ("rep 1, 64 rows: v4 packs", [], (64, 8, 8, DH, 384, F), (0, "v4", 1, T, 4, 3, 0, 0, 0)),
    ("rep 1, 65 rows: not above the decode GEMV's rows", [], (65, 8, 8, DH, 384, F), (0, "v4", 1, F, 4, 3, 0, 0, 0)),
    ("rep 8, 2080 pairs at 65 rows", [], (65, 256, 32, DH, 384, F), (0, "v4", 1, F, 2, 4, 0, 0, 0)),
    ("impl 4: no v4, so no mid-batch rule either: v3 at 33 rows", [("attn_set_impl", (4, 0))], (33, 32, 8, DH, 384, F),
     (0, "v3", 1, T, 2, 0, 0, 0, 0)),
    ("a moved v2 threshold switches the mid-batch rule off", [("attn_set_impl", (2, -8192))], (33, 32, 8, DH, 384, F),
     (0, "v3", 1, T, 2, 0, 0, 0, 0)),
    # --- the conservative mask rule: with a key mask no packed copy above 32 rows, whichever kernel
    ("v6, 32 rows, masked: packs", [], (32, 64, 8, DH, 384, T), (0, "v6", 1, T, 0, 0, 0, 2, 0)),
    ("v6, 33 rows, masked: no packed copy", [], (33, 64, 8, DH, 384, T), (0, "v6", 1, F, 0, 0, 0, 2, 0)),
    ("v3 (rep 8 from 2048 pairs is far), 33 rows at rep 4 with v4 off, masked", [("attn_set_impl", (4, 0))],
     (33, 32, 8, DH, 384, T), (0, "v3", 1, F, 2, 0, 0, 0, 0)),
    ("v5 up to 4096 pairs, 33 rows, masked", [("attn_set_v5_max_pairs", (4096,))], (33, 32, 8, DH, 384, T),
     (0, "v5", 6, F, 4, 0, 12, 0, 0)),
    # --- v2's splits: ceil(waves target / pairs), at least 64 keys each once t_cap > 64; split_len rounded up to 32
    ("rep 16 without v6, 300 pairs, t_cap 64: one split", V6_OFF, (300, 16, 1, DH, 64, F),
     (0, "v2", 1, F, 1, 4, 0, 0, 64)),
    ("... t_cap 65: two of ceil(33 / 32) x 32 keys", V6_OFF, (300, 16, 1, DH, 65, F), (0, "v2", 2, F, 1, 4, 0, 0, 64)),
    ("... t_cap 1030: 7 wanted", V6_OFF, (300, 16, 1, DH, 1030, F), (0, "v2", 7, F, 1, 4, 0, 0, 160)),
    ("... waves target 300: one split", V6_OFF + [("attn_set_impl", (2, 300))], (300, 16, 1, DH, 1030, F),
     (0, "v2", 1, F, 1, 4, 0, 0, 1056)),
    ("v2 forced at 6 pairs, t_cap 300: 5 splits of 64", V2_FORCED, (3, 8, 2, DH, 300, F),
     (0, "v2", 5, F, 8, 2, 0, 0, 64)),
    ("... t_cap 40, no mask: one split, so the v4 ring", V2_FORCED, (3, 8, 2, DH, 40, F),
     (0, "v4", 1, F, 4, 3, 0, 0, 0)),
    ("... t_cap 40, masked: v2", V2_FORCED, (3, 8, 2, DH, 40, T), (0, "v2", 1, F, 8, 2, 0, 0, 64)),
    ("... rep 16, t_cap 40: v4 has no rep 16", V2_FORCED + V6_OFF, (3, 32, 2, DH, 40, F),
     (0, "v2", 1, F, 1, 4, 0, 0, 64)),
    ("v3 and v5 off, waves target 1: v4 below the v2 threshold too", [("attn_set_impl", (2, 1)),
     ("attn_set_v5_max_pairs", (0,)), ("attn_set_v3_max_pairs", (0,))], (3, 8, 2, DH, 300, F),
     (0, "v4", 1, F, 4, 3, 0, 0, 0)),
    # --- v2's ring at rep <= 4: (KPG 8, 2 slots) below 16384 pairs, (KPG 4, 2 slots) from there and under impl 4
    ("rep 4, 16383 pairs, masked", [], (16383, 4, 1, DH, 64, T), (0, "v2", 1, F, 8, 2, 0, 0, 64)),
    ("rep 4, 16384 pairs, masked", [], (16384, 4, 1, DH, 64, T), (0, "v2", 1, F, 4, 2, 0, 0, 64)),
    ("impl 4 at 512 rows: v2 with the KPG 4 ring", [("attn_set_impl", (4, 0))], (512, 32, 8, DH, 384, F),
     (0, "v2", 1, F, 4, 2, 0, 0, 384)),
    ("rep 8 at 512 rows, masked: (KPG 2, 4 slots)", [], (512, 64, 8, DH, 384, T), (0, "v2", 1, F, 2, 4, 0, 0, 384)),
    ("rep 16 at 512 rows: v2, no v4 form", [], (512, 128, 8, DH, 384, F), (0, "v2", 1, F, 1, 4, 0, 0, 384)),
    ("the headline: Llama-3-8B at 2048 rows", [], (2048, 32, 8, DH, 384, F), (0, "v4", 1, F, 4, 3, 0, 0, 0)),
]


@pytest.mark.parametrize("what,calls,shape,want", RULES, ids=[r[0] for r in RULES])
def test_rule(what, calls, shape, want):
    e = ops.ext()
    e.attn_reset_knobs()
    try:
        _apply(e, calls)
        assert _form(e, *shape) == want, what
    finally:
        e.attn_reset_knobs()


def test_workspace_and_tickets():
    """One size per (shape, splits), whichever kernel runs: room for v5's partials, the largest layout ([m, l, 0, 0,
    o[128]] per head and split; v2's is [m, l, o[128]]), and one ticket per (row, kv head) pair -- what
    ``ops.attention`` allocated before the resolver existed (the bindings checked v2's smaller layout)."""
    e = ops.ext()
    e.attn_reset_knobs()
    try:
        ws = lambda *shape: e.attn_decode_plan_check(*shape)[5:7]  # noqa: E731
        assert ws(3, 8, 2, DH, 384, F) == (3 * 8 * 6 * 132, 6)  # v5, rep 4: 6 splits of 64 keys
        assert ws(13, 20, 5, DH, 384, F) == (13 * 20 * 132, 65)  # v3
        assert ws(8, 8, 1, DH, 384, F) == (8 * 8 * 132, 8)  # v6
        assert ws(2048, 32, 8, DH, 384, F) == (2048 * 32 * 132, 16384)  # v4
        assert ws(512, 64, 8, DH, 384, T) == (512 * 64 * 132, 4096)  # v2, one split
        _apply(e, V2_FORCED)
        assert ws(3, 8, 2, DH, 300, T) == (3 * 8 * 5 * 132, 6)  # v2, 5 splits
    finally:
        e.attn_reset_knobs()


def test_older_queries_ask_the_plan():
    """``attn_decode_splits`` / ``attn_decode_packs`` (no key mask) are the plan's ``nsplit`` / ``packs``."""
    e = ops.ext()
    e.attn_reset_knobs()
    try:
        for calls in ([], V6_OFF, V2_FORCED):
            _apply(e, calls)
            for b, hkv, rep, t_cap in itertools.product((1, 16, 33, 64, 65, 512), (1, 8, 64), (1, 4, 8, 16), (64, 384)):
                _, _, _, nsplit, packs, *_ = e.attn_decode_plan_check(b, hkv * rep, hkv, DH, t_cap, F)
                assert (e.attn_decode_splits(b, hkv, t_cap, rep), bool(e.attn_decode_packs(b, hkv, rep))) == \
                    (nsplit, bool(packs))
            e.attn_reset_knobs()
    finally:
        e.attn_reset_knobs()


# ======================================================================================
# the parent, transcribed
# ======================================================================================
class _ParentKnobs:
    """The file-scope knobs of the parent's attn_decode.hip / attn_decode_mma.hip and their setters, line by line."""

    def __init__(self):
        self.v5_fold, self.v5_max_pairs = 0, 64
        self.waves_target, self.v2_min_pairs, self.v4 = 2048, 4096, True
        self.kpg_small, self.geo_auto = 8, True
        self.v3_max_pairs, self.v3_kpg_mult = 4096, 0
        self.v6, self.v6_wpp = 1, 0

    def attn_set_v5_fold(self, n):
        self.v5_fold = n if n in (4, 12) else 0

    def attn_set_v5_max_pairs(self, n):
        self.v5_max_pairs = 64 if n < 0 else n

    def attn_set_impl(self, impl, waves_target=0):
        self.kpg_small = 4 if impl == 4 else 8
        self.geo_auto = impl != 4
        self.v4 = impl != 4
        if waves_target > 0:
            self.waves_target = waves_target
        self.v2_min_pairs = -waves_target if waves_target < 0 else 4096

    def attn_set_v3_max_pairs(self, n):
        self.v3_max_pairs = n

    def attn_set_v3_kpg(self, mult):
        self.v3_kpg_mult = 4 if mult >= 4 else (2 if mult >= 2 else (1 if mult == 1 else 0))

    def attn_set_v6(self, mode):
        self.v6 = 0 if mode < 0 else (2 if mode > 2 else mode)

    def attn_set_v6_wpp(self, wpp):
        self.v6_wpp = wpp if wpp in (1, 2, 4, 8) else 0


def _kpg5(rep):
    return 1 if rep >= 16 else (2 if rep == 8 else (4 if rep == 4 else 8))


def _kpg_v2(g, rep, pairs):
    if rep <= 4:
        return 4 if (g.geo_auto and pairs >= 16384) else g.kpg_small
    return 2 if rep == 8 else 1


def _v4_midbatch(g, B, Hkv, rep):
    return g.v4 and g.v2_min_pairs == 4096 and rep <= 8 and ((rep <= 4 and B > 32) or (rep == 8 and B * Hkv >= 2048))


def _use_v2(g, B, Hkv, rep):
    return B * Hkv >= g.v2_min_pairs or _v4_midbatch(g, B, Hkv, rep)


def _use_v3(g, B, Hkv, rep):
    return rep <= 8 and not _use_v2(g, B, Hkv, rep) and B * Hkv <= g.v3_max_pairs


def _use_v5(g, B, Hkv, rep):
    pairs = B * Hkv
    return rep <= 16 and (rep & (rep - 1)) == 0 and (pairs <= g.v5_max_pairs or
                                                      (rep >= 8 and pairs <= 4 * g.v5_max_pairs))


def _use_v6(g, B, Hkv, rep):
    if g.v6 == 0 or rep > 16 or (rep & (rep - 1)):
        return False
    if g.v6 == 2:
        return True
    return rep >= 8 and B * Hkv >= 8 and B * Hkv < 2048


def _attn_decode_packs(g, B, Hkv, rep):
    return (_use_v6(g, B, Hkv, rep) or _use_v5(g, B, Hkv, rep) or _use_v3(g, B, Hkv, rep) or
            (B <= 64 and _v4_midbatch(g, B, Hkv, rep)))


def _attn_decode_splits(g, B, Hkv, T, rep):
    if _use_v6(g, B, Hkv, rep):
        return 1
    if _use_v5(g, B, Hkv, rep):
        return (T + 16 * _kpg5(rep) - 1) // (16 * _kpg5(rep))
    if _use_v3(g, B, Hkv, rep):
        return 1
    if _v4_midbatch(g, B, Hkv, rep):
        return 1
    pairs = B * Hkv
    max_split = (T + 63) // 64 if T > 64 else 1
    ns = (g.waves_target + pairs - 1) // pairs
    return 1 if ns < 1 else (max_split if ns > max_split else ns)


def _attn_decode(g, B, H, Hkv, Dh, t_cap, nsplit, masked, out_pack):
    """The parent's launcher: its return code, or (kernel, kpg, ring, fold, wpp, split_len) of the instance it
    launches."""
    if out_pack and not _attn_decode_packs(g, B, Hkv, H // Hkv):
        return -3
    if out_pack and masked and not _use_v6(g, B, Hkv, H // Hkv) and not _use_v5(g, B, Hkv, H // Hkv) and \
            not _use_v3(g, B, Hkv, H // Hkv):
        return -3
    if Dh != 128 or H % Hkv:
        return -1
    rep = H // Hkv
    pairs = B * Hkv
    if _attn_decode_splits(g, B, Hkv, t_cap, rep) != nsplit:
        return -2
    if _use_v6(g, B, Hkv, rep):  # attn_decode_v6: every (rep, wpp) of {1, 2, 4, 8, 16} x {1, 2, 4, 8} has an instance
        wpp = g.v6_wpp if g.v6_wpp else (1 if pairs >= 4096 else 2)
        return ("v6", 0, 0, 0, wpp, 0) if rep in (1, 2, 4, 8, 16) and wpp in (1, 2, 4, 8) else -1
    if _use_v5(g, B, Hkv, rep):
        fold = 4 if (g.v5_fold == 4 or (g.v5_fold == 0 and pairs < 16)) else 12
        ladder = {1: 8, 2: 8, 4: 4, 8: 2, 16: 1}
        return ("v5", ladder[rep], 0, fold, 0, 0) if rep in ladder else -1
    if _use_v3(g, B, Hkv, rep):
        mult = g.v3_kpg_mult if g.v3_kpg_mult else (2 if pairs <= 128 else 1)
        kpg3 = min(min(8, 16 // rep), (8 // rep) * mult)
        return ("v3", kpg3, 0, 0, 0, 0) if (rep, kpg3) in ((1, 8), (2, 4), (2, 8), (4, 2), (4, 4), (8, 1), (8, 2)) \
            else -1
    if g.v4 and nsplit == 1 and not masked and rep <= 8:
        ladder = {1: (4, 3), 2: (4, 3), 4: (4, 3), 8: (2, 4)}
        if rep in ladder:
            return ("v4", ladder[rep][0], ladder[rep][1], 0, 0, 0)
    split_len = (t_cap + nsplit - 1) // nsplit
    split_len = (split_len + 31) // 32 * 32
    k8 = _kpg_v2(g, rep, pairs) == 8
    if rep in (1, 2, 4):
        return ("v2", 8 if k8 else 4, 2, 0, 0, split_len)
    if rep == 8:
        return ("v2", 2, 4, 0, 0, split_len)
    if rep == 16:
        return ("v2", 1, 4, 0, 0, split_len)
    return -1


def _parent_choice(g, B, H, Hkv, Dh, t_cap, masked):
    """What the parent did for one decode step as the model drives it: ``ops.attention_packs`` decides whether the
    packed copy is asked for, ``ops.attention`` asks ``attn_decode_splits`` and launches."""
    rep = H // Hkv
    packs = False if (masked and B > 32) else bool(_attn_decode_packs(g, B, Hkv, rep))  # ops.attention_packs
    nsplit = _attn_decode_splits(g, B, Hkv, t_cap, rep)
    r = _attn_decode(g, B, H, Hkv, Dh, t_cap, nsplit, masked, packs)
    if r == -3:
        return PACKS_THEN_REFUSED
    if r == -1:
        return BAD
    assert r != -2
    kernel, kpg, ring, fold, wpp, split_len = r
    return (0, kernel, nsplit, packs, kpg, ring, fold, wpp, split_len)


def test_parent_transcription_on_the_rules():
    """The transcription agrees with the literal rows (both were read off the parent), but for the intended change."""
    for what, calls, shape, want in RULES:
        g = _ParentKnobs()
        _apply(g, calls)
        got = _parent_choice(g, *shape)
        if "the parent: packs, then -3" in what:
            assert got == PACKS_THEN_REFUSED, what
        else:
            assert got == want, what


# every knob state the tests and tools/bench_attn_decode.py set
_IMPL = "attn_set_impl"
_V3MAX, _V3KPG = "attn_set_v3_max_pairs", "attn_set_v3_kpg"
_V5MAX, _V5FOLD = "attn_set_v5_max_pairs", "attn_set_v5_fold"
_V6, _V6WPP = "attn_set_v6", "attn_set_v6_wpp"
KNOB_STATES = {
    "default": [],
    "impl4": [(_IMPL, (4, 0))],
    "impl2_min1": [(_IMPL, (2, -1))],
    "impl2_waves1": [(_IMPL, (2, 1))],
    "v3_off": [(_V3MAX, (0,))],
    "v5_off": [(_V5MAX, (0,))],
    "v5_4096": [(_V5MAX, (4096,))],
    "v5_4096_fold4": [(_V5MAX, (4096,)), (_V5FOLD, (4,))],
    "v5_4096_fold12": [(_V5MAX, (4096,)), (_V5FOLD, (12,))],
    "v5_off_v3_kpg1": [(_V5MAX, (0,)), (_V3KPG, (1,))],
    "v5_off_v3_kpg2": [(_V5MAX, (0,)), (_V3KPG, (2,))],
    "v5_off_v3_kpg4": [(_V5MAX, (0,)), (_V3KPG, (4,))],
    "v6_off": [(_V6, (0,))],
    "v6_all": [(_V6, (2,))],
    "v6_all_wpp1": [(_V6, (2,)), (_V6WPP, (1,))],
    "v6_all_wpp2": [(_V6, (2,)), (_V6WPP, (2,))],
    "v6_all_wpp4": [(_V6, (2,)), (_V6WPP, (4,))],
    "v6_all_wpp8": [(_V6, (2,)), (_V6WPP, (8,))],
    "v2_forced_impl2": [(_V5MAX, (0,)), (_V3MAX, (0,)), (_IMPL, (2, -1))],
    "v2_forced_impl4": [(_V5MAX, (0,)), (_V3MAX, (0,)), (_IMPL, (4, 0))],
    # tools/bench_attn_decode.py: impl 3 (v3), 5 / 6 (v5, fold 12 / 4), 7 (v4) and 9 (v2) at any pair count
    "bench_v3": [(_V6, (0,)), (_V5MAX, (0,))],
    "bench_v5": [(_V6, (0,)), (_V5MAX, (4096,)), (_V5FOLD, (12,))],
    "bench_v5_first_merge": [(_V6, (0,)), (_V5MAX, (4096,)), (_V5FOLD, (4,))],
    "bench_v4": [(_V6, (0,)), (_IMPL, (2, 1)), (_IMPL, (2, -1)), (_V3MAX, (0,)), (_V5MAX, (0,))],
    "bench_v2": [(_V6, (0,)), (_IMPL, (4, 1)), (_IMPL, (4, -1)), (_V3MAX, (0,)), (_V5MAX, (0,))],
}
GRID_B = (1, 2, 4, 8, 15, 16, 17, 32, 33, 64, 65, 128, 256, 512, 513, 2048, 2049)
GRID_HKV = (1, 2, 8, 64)
GRID_REP = (1, 2, 3, 4, 8, 16, 32)
GRID_T = (1, 64, 65, 129, 384, 1030)
# The intended change, within the grid: rep 8, >= 2048 pairs, <= 32 rows and a key mask is B = 32 at 64 kv heads. It
# shows wherever the mid-batch rule is on (v4 enabled, the v2 threshold at its default) and no kernel asked earlier takes
# the shape: v6 by shape stops below 2048 pairs, v5 at 256 (v5 up to 4096 pairs reaches 16384 at rep 8: no difference).
CHANGED_STATES = {"default", "impl2_waves1", "v3_off", "v5_off", "v5_off_v3_kpg1", "v5_off_v3_kpg2", "v5_off_v3_kpg4",
                  "v6_off", "bench_v3"}


@pytest.mark.parametrize("state", list(KNOB_STATES))
def test_grid_matches_parent(state):
    e = ops.ext()
    e.attn_reset_knobs()
    g = _ParentKnobs()
    diff = {}
    try:
        _apply(e, KNOB_STATES[state])
        _apply(g, KNOB_STATES[state])
        for B, Hkv, rep, t_cap, masked in itertools.product(GRID_B, GRID_HKV, GRID_REP, GRID_T, (F, T)):
            want = _parent_choice(g, B, Hkv * rep, Hkv, DH, t_cap, masked)
            got = _form(e, B, Hkv * rep, Hkv, DH, t_cap, masked)
            if got != want:
                diff[(B, Hkv, rep, t_cap, masked)] = (want, got)
    finally:
        e.attn_reset_knobs()
    allowed = {}
    if state in CHANGED_STATES:
        # the parent: packs, then -3. Now: v2 (KPG 2, 4 slots), one split of t_cap rounded up to 32 keys, no packed copy
        allowed = {(32, 64, 8, t_cap, T): (PACKS_THEN_REFUSED, (0, "v2", 1, F, 2, 4, 0, 0, (t_cap + 31) // 32 * 32))
                   for t_cap in GRID_T}
    assert diff == allowed


# ======================================================================================
# the way back to the defaults
# ======================================================================================
RESET_SHAPES = [(1, 32, 8, DH, 384, F), (8, 8, 1, DH, 384, T), (40, 32, 8, DH, 384, F), (300, 16, 1, DH, 1030, F),
                (3, 8, 2, DH, 300, T), (512, 32, 8, DH, 384, T), (2048, 32, 8, DH, 384, F), (32, 512, 64, DH, 65, T)]
SETTERS = [(_IMPL, (4, 0)), (_IMPL, (2, -1)), (_IMPL, (2, 1)), (_IMPL, (2, 4096)), (_V3MAX, (0,)), (_V3KPG, (4,)),
           (_V5MAX, (0,)), (_V5MAX, (4096,)), (_V5FOLD, (4,)), (_V6, (0,)), (_V6, (2,)), (_V6WPP, (8,))]


def test_reset_knobs():
    """``attn_reset_knobs()`` after every setter, and after all of them, yields the default plans -- the waves target
    included, which ``attn_set_impl(2, 0)`` leaves as it is. Under the default knobs no shape reaches v2 with more
    than one split, so the waves target is read with v6 off: rep 16 at 300 pairs then runs v2."""
    e = ops.ext()

    def plans():
        default = [e.attn_decode_plan_check(*s) for s in RESET_SHAPES]
        e.attn_set_v6(0)
        v2_splits = e.attn_decode_plan_check(300, 16, 1, DH, 1030, F)[2:4]
        e.attn_reset_knobs()
        return default, v2_splits

    e.attn_reset_knobs()
    default = plans()
    assert default[1] == ("v2", 7)  # ceil(2048 / 300)
    try:
        for calls in [[c] for c in SETTERS] + [SETTERS]:
            _apply(e, calls)
            e.attn_reset_knobs()
            assert plans() == default, calls
        e.attn_set_impl(2, 1)
        e.attn_set_impl(2, 0)  # the old "restore": the waves target stays at 1
        e.attn_set_v6(0)
        assert e.attn_decode_plan_check(300, 16, 1, DH, 1030, F)[2:4] == ("v2", 1)
        e.attn_reset_knobs()
        assert plans() == default
    finally:
        e.attn_reset_knobs()
