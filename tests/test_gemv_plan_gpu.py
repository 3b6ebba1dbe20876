"""The plan resolver of the decode GEMV (csrc/kernels/gemv_plan.h, asked through ``gemv_plan_check``): which (variant
id, epilogue mode, activation type and layout, shape) is a legal call, and which form of the kernel runs it.

Host calls only (milliseconds); marked gpu because ``_C`` links the HIP runtime.

Every expected form below was derived by reading csrc/bindings.cpp (``run_skinny``, ``linear_skinny_argmax``,
``linear_tp_residual``) and csrc/kernels/gemv.hip (``linear_skinny``, ``dispatch_mt`` / ``dispatch_nt`` /
``dispatch_nw``, ``launch_skinny``) as they stood before the resolver existed, not by running the new function: once as
literal forms, one case per rule (``RULES``), and once as ``_parent_form``, a line-by-line transcription of those
checks and of the ladder, compared over the whole grid of the smallest shapes that separate the rules. What the parent
refused in any way -- a failed check of the bindings, -1, or -3 from launch_skinny's K-depth check -- is ``BAD``; -3
for buffers that are too small concerns buffers and stays in ``launch_skinny`` and the bindings."""
from __future__ import annotations

import itertools
import json

import pytest
import torch

from jax_llama_amd import ops
from jax_llama_amd.ops import autotune

pytestmark = pytest.mark.gpu
STORE, RESID, SWIGLU, QKV, ARGMAX, TPRESID = 0, 1, 2, 3, 8, 9
F, T = False, True
BAD = (-1, 0, 0, 0, F, F, 0)
NONE = (0, 0, 0, 0, F, F, 0)  # legal, nothing to launch

# (what the parent did, (m, n, k, mode, x_f32, x_packed, variant), (rc, mt, nt, nw, deep, xp, ksplit))
RULES = [
    # --- the empty batch, shapes
    ("empty batch: nothing to run", (0, 64, 64, STORE, F, F, 1), NONE),
    ("empty batch comes before the shape checks", (0, 24, 48, SWIGLU, F, F, 1), NONE),
    ("... but after the bindings' id list", (0, 64, 64, STORE, F, F, 7), BAD),
    ("M = 65", (65, 64, 64, STORE, F, F, 1), BAD),
    ("N % 16", (1, 24, 64, STORE, F, F, 1), BAD),
    ("K % 32", (1, 64, 48, STORE, F, F, 1), BAD),
    ("SwiGLU: N % 32", (1, 48, 64, SWIGLU, F, F, 1), BAD),
    # --- ids
    ("id 0 means 1", (1, 64, 64, STORE, F, F, 0), (0, 1, 1, 4, F, F, 1)),
    ("... also for the fused qkv projection", (17, 64, 64, QKV, T, F, 0), (0, 2, 1, 8, F, F, 1)),
    ("... not in linear_skinny_argmax's list", (1, 64, 64, ARGMAX, F, F, 0), BAD),
    ("... nor in linear_tp_residual", (1, 64, 64, TPRESID, F, F, 0), BAD),
    ("unknown id: a removed form", (1, 64, 64, STORE, F, F, 2), BAD),
    ("unknown id: the tiled GEMM's", (17, 64, 64, RESID, F, F, 7), BAD),
    ("unknown id: past the table", (1, 64, 64, STORE, F, F, 27), BAD),
    # --- m-tiles, and the waves of the default form
    ("M = 16: one m-tile, 4 waves", (16, 64, 64, STORE, F, F, 1), (0, 1, 1, 4, F, F, 1)),
    ("M = 17: two, 8 waves", (17, 64, 64, STORE, F, F, 1), (0, 2, 1, 8, F, F, 1)),
    ("M = 32", (32, 64, 64, RESID, T, F, 1), (0, 2, 1, 8, F, F, 1)),
    ("M = 33: four", (33, 64, 64, STORE, F, F, 1), (0, 4, 1, 8, F, F, 1)),
    ("M = 64", (64, 64, 64, QKV, F, F, 1), (0, 4, 1, 8, F, F, 1)),
    # --- tiles of the default form
    ("SwiGLU: the gate / up pair", (1, 64, 64, SWIGLU, F, F, 1), (0, 1, 2, 4, F, F, 1)),
    ("N / 16 = 2047: one tile", (1, 32752, 64, STORE, F, F, 1), (0, 1, 1, 4, F, F, 1)),
    ("N / 16 = 2048: two", (1, 32768, 64, STORE, F, F, 1), (0, 1, 2, 4, F, F, 1)),
    ("... with the residual, at M > 16", (17, 32768, 64, RESID, F, F, 1), (0, 2, 2, 8, F, F, 1)),
    ("... under the argmax epilogue", (1, 32768, 64, ARGMAX, T, F, 1), (0, 1, 2, 4, F, F, 1)),
    ("... not under QKV", (1, 32768, 64, QKV, F, F, 1), (0, 1, 1, 4, F, F, 1)),
    # --- row-major ids
    ("5: 4 tiles x 4 waves", (17, 64, 64, STORE, F, F, 5), (0, 2, 4, 4, F, F, 1)),
    ("5 at N = 48: silently the default form", (1, 48, 64, STORE, F, F, 5), (0, 1, 1, 4, F, F, 1)),
    ("... at M > 16", (17, 48, 64, RESID, F, F, 5), (0, 2, 1, 8, F, F, 1)),
    ("... the SwiGLU default", (1, 96, 64, SWIGLU, F, F, 5), (0, 1, 2, 4, F, F, 1)),
    ("6: 2 tiles x 4 waves", (17, 48, 64, STORE, T, F, 6), (0, 2, 2, 4, F, F, 1)),
    ("10: 2 x 4 with the doubled ring", (17, 64, 64, STORE, F, F, 10), (0, 2, 2, 4, T, F, 1)),
    ("10 at M = 16: silently the default form", (16, 64, 64, STORE, F, F, 10), (0, 1, 1, 4, F, F, 1)),
    ("10 with fp32 x: silently the default form", (17, 64, 64, STORE, T, F, 10), (0, 2, 1, 8, F, F, 1)),
    ("20: 2 tiles x 8 waves", (1, 64, 64, STORE, T, F, 20), (0, 1, 2, 8, F, F, 1)),
    # --- packed-x ids: exactly with a packed bf16 x
    ("12 without the packed x", (1, 64, 64, STORE, F, F, 12), BAD),
    ("a row-major id with one", (1, 64, 64, STORE, F, T, 1), BAD),
    ("id 0 with one", (1, 64, 64, STORE, F, T, 0), BAD),
    ("12 with fp32 x", (1, 64, 64, STORE, T, T, 12), BAD),
    ("12: 1 tile x 8 waves", (1, 64, 64, STORE, F, T, 12), (0, 1, 1, 8, F, T, 1)),
    ("12 under SwiGLU", (17, 64, 64, SWIGLU, F, T, 12), BAD),
    ("15: 2 x 4, doubled ring, at M <= 16 too", (1, 64, 64, SWIGLU, F, T, 15), (0, 1, 2, 4, T, T, 1)),
    ("21: 2 x 8", (33, 48, 64, RESID, F, T, 21), (0, 4, 2, 8, F, T, 1)),
    ("22: 4 x 4", (17, 64, 64, QKV, F, T, 22), (0, 2, 4, 4, F, T, 1)),
    ("22 at N % 64 != 0: refused", (17, 48, 64, STORE, F, T, 22), BAD),
    # --- split-K ids
    ("16: the default form's waves, K over 2", (1, 64, 64, STORE, F, F, 16), (0, 1, 1, 4, F, F, 2)),
    ("16 under SwiGLU at M > 16: the pair, 8 waves", (17, 64, 64, SWIGLU, F, F, 16), (0, 2, 2, 8, F, F, 2)),
    ("16 with the TP residual", (1, 64, 64, TPRESID, F, F, 16), (0, 1, 1, 4, F, F, 2)),
    ("18: as 16, on packed x", (33, 64, 64, QKV, F, T, 18), (0, 4, 1, 8, F, T, 2)),
    ("26: 4 x 8, K over 4", (17, 64, 128, RESID, F, T, 26), (0, 2, 4, 8, F, T, 4)),
    ("26 at M <= 16", (1, 64, 128, STORE, F, T, 26), (0, 1, 4, 8, F, T, 4)),
    ("26 at N % 64 != 0: refused", (17, 48, 128, STORE, F, T, 26), BAD),
    ("a split id with fp32 x", (1, 64, 64, STORE, T, F, 16), BAD),
    ("... which the empty batch came before", (0, 64, 64, STORE, T, F, 16), NONE),
    ("a split id under argmax", (1, 64, 64, ARGMAX, F, F, 16), BAD),
    ("1024 column groups", (1, 16384, 64, STORE, F, F, 16), (0, 1, 1, 4, F, F, 2)),
    ("1028 column groups", (1, 16448, 64, STORE, F, F, 16), BAD),
    ("... the 4-tile form counts 16-column groups too", (17, 16448, 128, STORE, F, T, 26), BAD),
    ("... even for an empty batch (the bindings' ticket check)", (0, 16448, 64, STORE, F, F, 16), BAD),
    ("16 at K = 32: fewer K steps than splits", (1, 64, 32, STORE, F, F, 16), BAD),
    ("16 at K = 64", (1, 64, 64, STORE, F, F, 16), (0, 1, 1, 4, F, F, 2)),
    ("26 at K = 96", (17, 64, 96, STORE, F, T, 26), BAD),
    # --- the argmax and TP-residual epilogues
    ("argmax: 5", (1, 64, 64, ARGMAX, F, F, 5), (0, 1, 4, 4, F, F, 1)),
    ("argmax: 10", (17, 64, 64, ARGMAX, F, F, 10), (0, 2, 2, 4, T, F, 1)),
    ("argmax: 20 with fp32 x", (64, 64, 64, ARGMAX, T, F, 20), (0, 4, 2, 8, F, F, 1)),
    ("argmax: no packed-x id", (1, 64, 64, ARGMAX, F, T, 12), BAD),
    ("TP residual: bf16 x only", (1, 64, 64, TPRESID, T, F, 1), BAD),
    ("TP residual: M >= 1", (0, 64, 64, TPRESID, F, F, 1), BAD),
    ("TP residual: a packed-x form", (17, 64, 64, TPRESID, F, T, 15), (0, 2, 2, 4, T, T, 1)),
]


@pytest.mark.parametrize("why,args,want", RULES, ids=[f"{i}" for i in range(len(RULES))])
def test_rule(why, args, want):
    assert tuple(ops.ext().gemv_plan_check(*args)) == want, (why, args)


XP_IDS, SPLIT_IDS = (12, 15, 18, 21, 22, 26), (16, 18, 26)


def _parent_form(m, n, k, mode, f32, xp_in, v):
    """What a Python caller reached before the resolver, return statements only, in their order: the checks of the
    binding that owns the mode, then gemv.hip. Launches return the kernel form."""
    # ---- bindings.cpp (every entry point: m <= SKINNY_MAX_M)
    if m > 64:
        return BAD
    if mode == ARGMAX:  # linear_skinny_argmax: no x_packed parameter (a packed x cannot be passed), its own id list
        if xp_in or v not in (1, 5, 6, 10, 20):
            return BAD
    else:
        if mode == TPRESID and (f32 or m < 1 or v in (0, 4, 7)):  # linear_tp_residual, ahead of run_skinny
            return BAD
        if v == 0:  # run_skinny
            v = 1
        xpv = v in XP_IDS
        if xpv != xp_in or (xpv and f32) or (xpv and mode == SWIGLU and v == 12):
            return BAD
        if not (v in (1, 5, 6, 10, 16, 20) or xpv):
            return BAD
        if v in SPLIT_IDS and n // 16 > 1024:  # gemv_split_tickets(n) > 0
            return BAD
    # ---- gemv.hip linear_skinny()
    if m <= 0:
        return NONE
    if m > 64 or n % 16 or k % 32:
        return BAD
    if mode == SWIGLU and n % 32:
        return BAD
    if v in SPLIT_IDS and (f32 or mode == ARGMAX):
        return BAD
    if mode == TPRESID and f32:  # dispatch_tp
        return BAD
    mt = 1 if m <= 16 else (2 if m <= 32 else 4)  # dispatch_mt
    bf16 = not f32

    def launch(nt, nw, deep=F, xp=F, ksplit=1):  # launch_skinny: -3 where a split plan does not fit the shape
        if ksplit > 1 and ((n // 16 + nt - 1) // nt > 1024 or k // 32 < ksplit):
            return BAD
        return (0, mt, nt, nw, deep, xp, ksplit)

    # ---- dispatch_nt
    if v == 5 and n % 64 == 0:
        return launch(4, 4)
    if v == 6:
        return launch(2, 4)
    if mt > 1 and bf16:
        if v == 10:
            return launch(2, 4, deep=T)
    if bf16 and mode != ARGMAX:
        if v == 26:
            if n % 64:
                return BAD
            return launch(4, 8, xp=T, ksplit=4)
        if v in SPLIT_IDS:
            snt, snw = 2 if mode == SWIGLU else 1, 4 if mt == 1 else 8
            if v == 18:
                return launch(snt, snw, xp=T, ksplit=2)
            return launch(snt, snw, ksplit=2)
    if v == 20:
        return launch(2, 8)
    if bf16:
        if v == 21:
            return launch(2, 8, xp=T)
        if v == 22:
            if n % 64:
                return BAD
            return launch(4, 4, xp=T)
    if bf16:
        if v == 15:
            return launch(2, 4, deep=T, xp=T)
        if mode != SWIGLU:
            if v == 12:
                return launch(1, 8, xp=T)
    nw = 4 if mt == 1 else 8  # dispatch_nw
    if mode == SWIGLU:
        return launch(2, nw)
    if mode != QKV and n // 16 >= 2048:
        return launch(2, nw)
    return launch(1, nw)


def test_grid_matches_the_parent_ladder():
    """Every combination of the shapes that separate the rules (M at the m-tile edges and past both ends, N with and
    without whole 32- / 64-column groups, at 1028 column groups and at the default form's two-tile threshold, K around
    the split depths), every mode, fp32 / bf16 x, packed x present or absent, every id from 0 past the table (some
    129000 host calls)."""
    e = ops.ext()
    bad = []
    for args in itertools.product((0, 1, 16, 17, 32, 33, 64, 65), (16, 32, 48, 64, 16448, 32768), (32, 64, 96, 128),
                                  (STORE, RESID, SWIGLU, QKV, ARGMAX, TPRESID), (T, F), (F, T), range(0, 28)):
        got, want = tuple(e.gemv_plan_check(*args)), _parent_form(*args)
        if got != want:
            bad.append((args, got, want))
    assert not bad, (len(bad), bad[:10])


def test_python_copies_equal_the_extension():
    """The one Python copy of the id table (autotune.GEMV_VARIANTS), the split forms' column-group cap and the m-tile
    rule of the packed activation buffers are the extension's."""
    e = ops.ext()
    assert autotune.GEMV_VARIANTS == {int(v): tuple(f) for v, f in e.gemv_variant_table().items()}
    assert autotune.TILED_VARIANT not in autotune.GEMV_VARIANTS and ops.TILED == autotune.TILED_VARIANT
    assert ops.XP_VARIANTS == autotune.XP_CANDIDATES == XP_IDS
    assert ops.SPLIT_VARIANTS == autotune.SPLIT_GEMV == SPLIT_IDS
    assert autotune.ROW_MAJOR_VARIANTS == (1, 5, 6, 10, 20)
    assert autotune.SPLIT_MAX_GROUPS == e.GEMV_SPLIT_MAX_GROUPS
    assert ops.SKINNY_M == e.SKINNY_MAX_M
    for m in range(1, 65):
        assert ops.packed_rows(m) == 16 * e.gemv_plan_check(m, 64, 64, STORE, F, F, 1)[1], m
    # the cap is where the shared workspace stops covering a shape
    cap = autotune.SPLIT_MAX_GROUPS * 16
    assert min(e.skinny_workspace(64, cap)) > 0 and tuple(e.skinny_workspace(64, cap + 16)) == (0, 0)


def _parent_candidates(m, n, mode, dtype, xp_in, pack_out, no_split, tiled_packs):
    """autotune.candidates() and the candidate construction of autotune.choose() as they stood before the resolver."""
    bf16_x = dtype == torch.bfloat16
    c = [1, 6]
    if n % 64 == 0:
        c.insert(1, 5)
    if m > 16:
        c.append(7)
        if bf16_x:
            c.append(10)
    if n // 32 < 512:
        c.append(20)
    if bf16_x and n // 16 <= 1024:
        c.append(16)
    if pack_out:
        c = [v for v in c if v != 7 or tiled_packs]
    if xp_in and bf16_x:
        c += [v for v in XP_IDS if (mode != 2 or v != 12) and
              (v != 18 or n // 16 <= 1024) and (v != 21 or n // 32 < 512) and
              (v != 22 or (n % 64 == 0 and n // 64 >= 64)) and
              (v != 26 or (m > 16 and n % 64 == 0 and n // 64 < 256))]
    if no_split:
        c = [v for v in c if v not in SPLIT_IDS]
    return c


def test_candidate_lists_match_the_parent():
    """Same members in the same order (the order decides ties, and picks are persisted) for every key of the grid."""
    e = ops.ext()
    bad = []
    for key in itertools.product((1, 16, 17, 64), (1280, 4096, 6144, 16448, 28672, 128256), (0, 1, 2),
                                 (torch.bfloat16, torch.float32), (F, T), (F, T), (F, T), (F, T)):
        got, want = autotune.gemv_candidates(e, *key), _parent_candidates(*key)
        if got != want:
            bad.append((key, got, want))
    assert not bad, (len(bad), bad[:10])


def test_shipped_picks_are_candidates():
    """Every gemv@<TUNE_VERSION> key of the packaged table names a variant of that key's candidate list."""
    e = ops.ext()
    with open(autotune.PACKAGED_FILE) as f:
        table = json.load(f)
    prefix = f"gemv@{autotune.TUNE_VERSION}:"
    keys = [key for key in table if key.startswith(prefix)]
    assert keys
    for key in keys:
        m, n, k, mode, dtype, *flags = key[len(prefix):].split(",")
        xp_in, pack_out, no_split, tiled_packs = (f == "True" for f in flags)
        cands = autotune.gemv_candidates(e, int(m), int(n), int(mode), getattr(torch, dtype), xp_in, pack_out, no_split,
                                         tiled_packs, int(k))
        assert table[key] in cands, (key, table[key], cands)
