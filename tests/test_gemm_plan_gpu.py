"""The plan resolver of the tiled GEMM (csrc/kernels/gemm_plan.h, asked through ``gemm_plan_check``): which (tile id,
epilogue mode, fused norm, K split, norm scratch) is a legal plan, and with which return code it fails otherwise.

Host calls only (milliseconds); marked gpu because ``_C`` links the HIP runtime and the CU count comes from the device.

Every expected code below was derived by reading ``gemm()``, ``launch_g2`` / ``launch_g4`` / ``launch_g5`` and
``gemm_argmax()`` of csrc/kernels/gemm.hip as they stood before the resolver existed (the ladder of early returns
-1 / -5 / -6 / -7 and the fall-throughs of the launch ladder), not by running the new function: once as literal codes,
one case per rule (``RULES``), and once as ``_parent_rc``, a line-by-line transcription of that ladder, compared over
the whole grid of the smallest shapes that separate the rules. -3 (workspace too small) concerns buffers and stays in
``gemm()``. ``MODE_ARGMAX`` is ``gemm_argmax()``'s mode (always tile 0, never split): its codes are that function's;
``gemm()`` itself answers -1 to it."""
from __future__ import annotations

import itertools
import json

import pytest

from jax_llama_amd import ops
from jax_llama_amd.ops import autotune

pytestmark = pytest.mark.gpu
STORE, RESID, SWIGLU, QKV, PARTIAL, ARGMAX, TPRESID = 0, 1, 2, 3, 7, 8, 9

# (what the parent did, (m, n, k, mode, rms, ksplit, tile, has_rms_ws[, n_body]), code)
RULES = [
    # --- return codes and their order
    ("empty batch: nothing to run", (0, 192, 256, STORE, False, 1, 0, False), 0),
    ("empty batch comes before the shape checks", (0, 200, 48, STORE, False, 1, 0, False), 0),
    ("tile 17's combination check comes before the empty batch", (0, 192, 96, STORE, False, 1, 17, False), -1),
    ("... norm without the scratch", (0, 192, 256, STORE, True, 1, 17, False), -1),
    ("... and a legal tile 17 call at M = 0 is 0", (0, 192, 256, STORE, True, 1, 17, True), 0),
    ("gemm5 has no empty batch", (0, 192, 256, STORE, False, 1, 11, False), -1),
    ("N % 16", (128, 200, 256, STORE, False, 1, 0, False), -1),
    ("K % 32", (128, 192, 48, STORE, False, 1, 0, False), -1),
    ("SwiGLU: N % 32", (128, 208, 256, SWIGLU, False, 1, 0, False), -1),
    ("norm with the residual epilogue", (128, 192, 256, RESID, True, 1, 0, False), -5),
    ("... -5 comes before -6", (300, 192, 256, RESID, True, 1, 16, False), -5),
    ("... and tile 17's early check does not look at the residual", (300, 192, 256, RESID, True, 1, 17, False), -5),
    ("a caller's mode only (the split launch mode)", (300, 192, 256, PARTIAL, False, 1, 0, False), -1),
    ("... split: the reduce kernel refused it", (300, 192, 256, PARTIAL, False, 2, 0, False), -1),
    ("unknown mode", (300, 192, 256, 5, False, 1, 0, False), -1),
    # --- tile 0 (the kernel shows in the direct-QKV rule: gemm2 128 x 256 has no such epilogue)
    ("tile 0, M <= 128: gemm2 128 x 256", (128, 192, 256, STORE, True, 1, 0, False), 0),
    ("... so no direct QKV", (128, 192, 256, QKV, True, 1, 0, True), -1),
    ("tile 0, M > 128, K % 64 == 0: gemm4", (129, 192, 256, QKV, True, 1, 0, True), 0),
    ("tile 0, M > 128, K % 64 != 0: gemm2 256 x 256 through id 0", (129, 192, 96, QKV, True, 1, 0, True), 0),
    ("tile 0 residual at M >= 4096: persistent gemm4", (4096, 192, 256, RESID, False, 1, 0, False), 0),
    ("every epilogue on tile 0", (300, 448, 256, SWIGLU, True, 1, 0, True), 0),
    # --- gemm4 ids fall through to gemm2 by M where K % 64 != 0 (an id other than 0 / 1: no direct QKV)
    ("tile 7, K % 64 != 0: gemm2 by M", (300, 192, 96, STORE, True, 1, 7, False), 0),
    ("... no direct QKV there", (300, 192, 96, QKV, True, 1, 7, True), -1),
    ("tile 13 likewise", (300, 192, 96, QKV, True, 1, 13, True), -1),
    ("tile 14 likewise", (300, 192, 96, QKV, True, 1, 14, True), -1),
    ("tile 16, K % 64 != 0: gemm2 by M", (300, 192, 96, STORE, False, 1, 16, False), 0),
    ("... the -6 rule still sees the id", (300, 192, 96, STORE, True, 1, 16, False), -6),
    ("tile 17, K % 64 != 0: an error", (300, 192, 96, STORE, False, 1, 17, False), -1),
    ("tile 13 with a K split: plain gemm4", (300, 192, 256, STORE, True, 2, 13, False), 0),
    ("unknown id: gemm2 by M", (300, 192, 256, STORE, True, 1, 5, False), 0),
    ("unknown id beyond the table", (128, 192, 96, SWIGLU, False, 2, 99, False), 0),
    ("... gemm2 256 x 256, but not through id 0 / 1: no direct QKV", (300, 192, 256, QKV, True, 1, 5, True), -1),
    # --- tiles 16 / 17 and the fused norm
    ("tile 16, norm, no scratch", (300, 192, 256, STORE, True, 1, 16, False), -6),
    ("tile 16, norm, K split", (300, 192, 256, STORE, True, 2, 16, True), -6),
    ("tile 16, norm from the scratch", (300, 192, 256, SWIGLU, True, 1, 16, True), 0),
    ("tile 16, split without the norm", (300, 192, 256, STORE, False, 2, 16, False), 0),
    ("tile 17: the same two are -1, from its early check", (300, 192, 256, STORE, True, 1, 17, False), -1),
    ("...", (300, 192, 256, STORE, True, 2, 17, True), -1),
    ("tile 17, norm from the scratch", (300, 192, 256, STORE, True, 1, 17, True), 0),
    ("tile 17: no QKV epilogue without a split", (300, 192, 256, QKV, True, 1, 17, True), -1),
    ("... with one: the reduce kernel's", (300, 192, 256, QKV, False, 2, 17, False), 0),
    ("tile 17: no argmax", (300, 192, 256, ARGMAX, False, 1, 17, False), -1),
    # --- tiles 18 / 19
    ("tail tiles: no QKV", (300, 448, 256, QKV, True, 1, 18, True, 1), -1),
    ("tail tiles: no TP residual", (300, 448, 256, TPRESID, False, 2, 18, False, 1), -1),
    ("tail tiles: no argmax", (300, 448, 256, ARGMAX, False, 1, 19, False, 1), -1),
    ("tail tiles: K % 64", (300, 448, 96, STORE, False, 1, 18, False, 1), -1),
    ("... before the scratch", (300, 448, 96, STORE, True, 1, 18, False, 1), -1),
    ("tail tiles: no K split", (300, 448, 256, STORE, False, 2, 19, False, 1), -1),
    ("tail tiles: norm without the scratch", (300, 448, 256, SWIGLU, True, 1, 18, False, 1), -6),
    ("tail tiles: 2 m-tiles x 448 columns fit one round, nothing offered", (300, 448, 256, STORE, False, 1, 18, False), -7),
    ("... nor with 256-wide body tiles", (300, 448, 256, RESID, False, 1, 19, False), -7),
    ("tail tiles: pinned body 1 x 192 < 448", (300, 448, 256, STORE, True, 1, 18, True, 1), 0),
    ("tail tiles: pinned body 1 x 256 < 448", (300, 448, 256, RESID, False, 1, 19, False, 1), 0),
    ("tail tiles: pinned body 2 x 256 >= 448", (300, 448, 256, STORE, False, 1, 19, False, 2), -7),
    ("tail tiles: pinned body 1 x 192 >= 192", (300, 192, 256, STORE, False, 1, 18, False, 1), -7),
    # --- QKV without a split: the norm and gemm2 256 x 256 (ids 0 / 1), a gemm4 256 x 256 id, or tile 16
    ("direct QKV needs the norm", (300, 192, 256, QKV, False, 1, 1, False), -1),
    ("tile 1 at any M", (128, 192, 256, QKV, True, 1, 1, False), 0),
    ("tile 1, K % 64 != 0", (300, 192, 96, QKV, True, 1, 1, False), 0),
    ("tile 2", (300, 192, 256, QKV, True, 1, 2, True), -1),
    ("tile 3", (300, 192, 256, QKV, True, 1, 3, True), -1),
    ("tile 7", (300, 192, 256, QKV, True, 1, 7, False), 0),
    ("tile 13", (128, 192, 256, QKV, True, 1, 13, True), 0),
    ("tile 14", (300, 192, 256, QKV, True, 1, 14, True), 0),
    ("tile 16 with the scratch", (300, 192, 256, QKV, True, 1, 16, True), 0),
    ("tile 16 without: the norm rule", (300, 192, 256, QKV, True, 1, 16, False), -6),
    ("tile 16, K % 64 != 0", (300, 192, 96, QKV, True, 1, 16, True), -1),
    ("QKV with a split: any gemm2 / gemm4 plan, the reduce kernel's epilogue", (300, 192, 256, QKV, True, 2, 2, False), 0),
    # --- the TP residual lives in the split-K reduce
    ("TP residual needs a split", (300, 192, 256, TPRESID, False, 1, 0, False), -1),
    ("TP residual takes no norm", (300, 192, 256, TPRESID, True, 2, 0, False), -1),
    ("TP residual, split", (300, 192, 256, TPRESID, False, 2, 0, False), 0),
    # --- gemm5: launch_g5's checks; the reduce kernel runs every epilogue, split or not
    ("gemm5: K % 64", (300, 192, 96, STORE, False, 1, 11, False), -1),
    ("gemm5: N % 16", (300, 200, 256, STORE, False, 1, 12, False), -1),
    ("gemm5: SwiGLU N % 32", (300, 208, 256, SWIGLU, False, 1, 11, False), -1),
    ("gemm5: no argmax", (300, 192, 256, ARGMAX, False, 1, 11, False), -1),
    ("gemm5: norm with the residual is -1 here", (300, 192, 256, RESID, True, 1, 12, False), -1),
    ("gemm5: norm with the TP residual", (300, 192, 256, TPRESID, True, 2, 11, False), -1),
    ("gemm5: QKV through the reduce, no split", (300, 192, 256, QKV, True, 1, 11, False), 0),
    ("gemm5: TP residual without a split", (300, 192, 256, TPRESID, False, 1, 12, False), 0),
    ("gemm5: SwiGLU with the norm, split", (128, 448, 256, SWIGLU, True, 2, 12, False), 0),
    # --- gemm_argmax(): tile 0, no split
    ("argmax: gemm4", (129, 192, 256, ARGMAX, True, 1, 0, True), 0),
    ("argmax: gemm2 256 x 256 at any M", (128, 192, 96, ARGMAX, True, 1, 0, False), 0),
    ("argmax: empty batch", (0, 192, 256, ARGMAX, False, 1, 0, False), 0),
    ("argmax: N % 16", (128, 200, 256, ARGMAX, False, 1, 0, False), -1),
    ("argmax through gemm() with a split: the reduce kernel refused it", (300, 192, 256, ARGMAX, False, 2, 0, False), -1),
]


@pytest.mark.parametrize("why,args,want", RULES, ids=[f"{i}" for i in range(len(RULES))])
def test_rule(why, args, want):
    assert ops.ext().gemm_plan_check(*args) == want, (why, args)


def _parent_rc(e, m, n, k, mode, rms, ksplit, tile, ws, n_body=0, g4_default=True):
    """gemm() as it was before the resolver, return statements only, in its order (and gemm_argmax() for the argmax
    mode, which gemm() itself refused). Launches are `return 0`."""
    def tile_cfg():
        return tile if 1 <= tile <= 3 else (2 if m <= 128 else 1)

    def use_g4():
        return k % 64 == 0 and (tile in (7, 13, 14) or (tile == 0 and g4_default and m > 128))

    if tile in (11, 12):
        if mode == ARGMAX or (rms and mode in (RESID, TPRESID)):
            return -1
        if k % 64 or n % 16 or m <= 0:  # launch_g5
            return -1
        if mode == SWIGLU and n % 32:
            return -1
        return 0 if mode in (STORE, RESID, SWIGLU, QKV, TPRESID) else -1  # (launch_reduce's default)
    if tile == 17 and (k % 64 or (mode == QKV and ksplit <= 1) or mode == ARGMAX
                       or (rms and mode != RESID and (ksplit > 1 or not ws))):
        return -1
    if m <= 0:
        return 0
    if n % 16 or k % 32:
        return -1
    if mode == SWIGLU and n % 32:
        return -1
    if rms and mode == RESID:
        return -5
    ks32 = k // 32
    ks = max(1, ksplit)
    kc = (ks32 + ks - 1) // ks
    ks = (ks32 + kc - 1) // kc
    if mode == TPRESID and (ks == 1 or rms):
        return -1
    direct_ok = (tile in (0, 1) and tile_cfg() == 1) or use_g4() or (tile == 16 and k % 64 == 0)
    if mode == QKV and ks == 1 and not (direct_ok and rms):
        return -1
    if tile in (16, 17) and rms and (ks > 1 or not ws):
        return -6
    if tile in (18, 19):
        if k % 64 or ks > 1 or mode not in (STORE, RESID, SWIGLU):
            return -1
        if rms and not ws:
            return -6
        wb = 192 if tile == 18 else 256
        nb = n_body if n_body > 0 else e.gemm_tail_split((m + 255) // 256, n, wb)[0]
        if nb <= 0 or nb * wb >= n:
            return -7
    if mode == ARGMAX:  # gemm_argmax(): tile 0, no split; gemm()'s switch and the reduce kernel both refused the mode
        return 0 if ks == 1 else -1
    return 0 if mode in (STORE, RESID, SWIGLU, QKV, TPRESID) else -1


def test_grid_matches_the_parent_ladder():
    """Every combination of the smallest shapes that separate the rules (M around the 128-row and persistent
    thresholds, K % 64 zero and not, N with and without room for a tail), every mode, split and not, norm on and off,
    scratch present and absent, every tile id of the table and the unknown ones between and past them (some 24000 host calls)."""
    e = ops.ext()
    bad = []
    for m, k, n, mode, ks, rms, ws, tile in itertools.product(
            (0, 128, 129, 300, 4096), (96, 256), (192, 448), (STORE, RESID, SWIGLU, QKV, PARTIAL, ARGMAX, TPRESID),
            (1, 2), (False, True), (False, True), range(0, 21)):
        for nb in ((0, 1) if tile in (18, 19) else (0,)):
            got, want = e.gemm_plan_check(m, n, k, mode, rms, ks, tile, ws, nb), _parent_rc(e, m, n, k, mode, rms, ks, tile, ws, nb)
            if got != want:
                bad.append(((m, n, k, mode, rms, ks, tile, ws, nb), got, want))
    assert not bad, (len(bad), bad[:10])


def test_tail_split_offered_on_the_bench_shape():
    """Tiles 18 / 19 without a pinned body: legal exactly where gemm_tail_split offers a split for the device's CUs
    (Llama-3-8B gate_up at M = 2048: offered on 256 CUs, tests/test_gemm_tail_tiles_gpu.py), -7 otherwise."""
    e = ops.ext()
    for tile, wb in ((18, 192), (19, 256)):
        for n in (28672, 24576, 8192):
            want = 0 if e.gemm_tail_split(8, n, wb)[0] > 0 else -7
            assert e.gemm_plan_check(2048, n, 4096, SWIGLU, True, 1, tile, True) == want, (tile, n)


@pytest.mark.parametrize("m,k", [(128, 256), (300, 256), (300, 96)])
def test_qkv_direct_ok_is_the_resolver(m, k):
    """gemm_qkv_direct_ok(m, t, k) is the resolver's answer for (QKV, norm, no split, scratch present), t in 0..19 --
    except on the gemm5 ids 11 / 12 where K % 64 == 0: that plan is legal too, but its RoPE / KV write runs in the
    reduce kernel (slab workspace), which is not the direct epilogue the name asks about, and was not before."""
    e = ops.ext()
    for t in range(20):
        legal = e.gemm_plan_check(m, 192, k, QKV, True, 1, t, True) == 0
        if t in autotune.G5_TILES and k % 64 == 0:
            assert legal and not e.gemm_qkv_direct_ok(m, t, k), (m, t, k)
        else:
            assert bool(e.gemm_qkv_direct_ok(m, t, k)) == legal, (m, t, k)
    # (as the parent's expression gave them)
    want = {0: m > 128, 1: True, 7: k % 64 == 0, 13: k % 64 == 0, 14: k % 64 == 0, 16: k % 64 == 0}
    assert [bool(e.gemm_qkv_direct_ok(m, t, k)) for t in range(20)] == [want.get(t, False) for t in range(20)]


def test_shipped_picks_are_candidates():
    """Every gemm@<TUNE_VERSION> key of the packaged table: the shipped (split, tile) is one of plan_candidates for
    that key, and every candidate is a legal plan as the tuner runs it."""
    e = ops.ext()
    with open(autotune.PACKAGED_FILE) as f:
        table = json.load(f)
    prefix = f"gemm@{autotune.TUNE_VERSION}:"
    keys = [key for key in table if key.startswith(prefix)]
    assert keys
    for key in keys:
        m, n, k, mode, rms = key[len(prefix):].split(",")
        m, n, k, mode, rms = int(m), int(n), int(k), int(mode), rms == "True"
        cands = autotune.plan_candidates(e, m, n, k, mode, rms)
        assert tuple(table[key]) in cands, (key, table[key], cands)
        assert len(set(cands)) == len(cands), key
        fused = rms and mode != 1
        for c, tm in cands:
            assert e.gemm_plan_check(m, n, k, mode, fused, c, tm, c == 1 and fused) == 0, (key, c, tm)
