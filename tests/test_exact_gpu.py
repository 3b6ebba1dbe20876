"""Exact-answer tests of the HIP kernels on the inputs of tests/exact_inputs.py (validated against ops/reference.py on
the CPU by tests/test_exact_inputs_cpu.py). Where the other GPU tests allow bf16 tolerance scaled by the global maximum,
these have an answer that is known exactly, so one key dropped, doubled or wrongly admitted at a split / chunk / ring
boundary, one K term or column off, a truncated bf16 store or a wrong RoPE table entry is an integer-sized error:

  A. attention key census  -- q = 0, V = unit vectors of the key's class: ``out * n`` counts the valid keys per class;
  B. attention needle      -- +-1 keys, q = 32 K[j*]: the output is V[j*] bit for bit;
  C. integer GEMM / GEMV   -- every fp32 partial sum exact: the int64 product, round-to-nearest-even bf16 stores with
                              planted ties, quarter-turn RoPE epilogues, power-of-two fused-norm row scales;
  D. attention ladder      -- exact scores that differ by up to 181 nats: the fp64 softmax per output element to a
                              relative bound derived from the number formats (A has equal weights and B a single one:
                              this family guards the weighting -- rescale factors and merge weights between 0 and 1).

Every kernel is forced with the knobs tests/test_kernels_gpu.py uses (restored in ``finally``), and the selection is
asserted through ``attn_decode_plan_check`` / ``gemm_plan_check``."""
from __future__ import annotations

import contextlib
import functools

import pytest
import torch

import exact_inputs as xi
from jax_llama_amd import ops
from jax_llama_amd.models.weights import PackedLinear
from jax_llama_amd.ops import autotune
from jax_llama_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
DH = xi.DH
STORE, RESID, SWIGLU, QKV = ops.MODE_STORE, ops.MODE_RESIDUAL, ops.MODE_SWIGLU, ops.MODE_QKV


# ======================================================================================
# A / B. attention
# ======================================================================================
KPG5 = {1: 8, 2: 8, 4: 4, 8: 2, 16: 1}  # v5 keys per lane group: a split holds 16 x this many keys


def _plan(e, b, hkv, t, rep, masked):
    """(kernel name, splits, packs) of the decode launch under the current knobs (csrc/kernels/attn_plan.h)."""
    rc, why, kernel, nsplit, packs, *_ = e.attn_decode_plan_check(b, hkv * rep, hkv, DH, t, masked)
    assert rc == 0, why
    return kernel, nsplit, packs


@contextlib.contextmanager
def _decode_kernel(kernel, knob, b, hkv, t, rep, masked):
    """Force one decode kernel and assert that the dispatcher's plan selects it. Yields whether the kernel writes the
    packed output copy.

    v2: ``attn_set_impl(2, -1)`` / ``(4, 0)`` alone do not reach v2 at 6 (row, kv head) pairs -- the dispatcher asks
    v5, then v3 first -- so those two are switched off as well; then nothing packs and the keys are cut into >= 2
    splits from T = 65 on (with one split, no mask, rep <= 8 and impl 2 the dispatcher runs the v4 ring instead:
    T = 40)."""
    e = ops.ext()
    try:
        if kernel == "v3":
            e.attn_set_v5_max_pairs(0)
            e.attn_set_v3_kpg(knob)
            assert _plan(e, b, hkv, t, rep, masked) == ("v3", 1, True)
        elif kernel == "v5":
            e.attn_set_v5_max_pairs(4096)
            e.attn_set_v5_fold(knob)
            assert _plan(e, b, hkv, t, rep, masked) == ("v5", -(-t // (16 * KPG5[rep])), True)
        elif kernel == "v6":
            e.attn_set_v6(2)
            e.attn_set_v6_wpp(knob)
            assert _plan(e, b, hkv, t, rep, masked) == ("v6", 1, True)
        elif kernel == "v2":
            e.attn_set_v5_max_pairs(0)
            e.attn_set_v3_max_pairs(0)
            if knob == 2:
                e.attn_set_impl(2, -1)
            else:
                e.attn_set_impl(4, 0)
            name, nsplit, packs = _plan(e, b, hkv, t, rep, masked)
            assert name == ("v4" if knob == 2 and t <= 64 and not masked and rep <= 8 else "v2")
            assert not packs
            assert (nsplit > 1) == (t > 64)
        elif kernel == "v4":
            assert not masked
            assert _plan(e, b, hkv, t, rep, masked) == ("v4", 1, b <= 64)
        else:
            raise AssertionError(kernel)
        yield _plan(e, b, hkv, t, rep, masked)[2]
    finally:
        e.attn_reset_knobs()


def _attend(q, kd, vd, slot0, kvs_d, mask_d, packs):
    """ops.attention on device tensors; where the kernel writes the packed copy, it unpacks to the row-major output."""
    b, s, h, _ = q.shape
    sl = torch.tensor([slot0], dtype=torch.int32, device=DEV)
    packed = ops.packed_empty(b, h * DH, DEV) if packs and s == 1 and b <= 64 else None
    out = ops.attention(q, kd, vd, sl, kvs_d, mask_d, out_packed=packed)
    torch.cuda.synchronize()
    if packed is not None:
        assert torch.equal(ref.unpack_act(packed.cpu(), b), out.cpu())
    return out


def _rand_k(b, hkv, t, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(b, hkv, t, DH, generator=g) * 0.5).to(BF16).to(DEV)


def _small_kv_start(slot):
    return torch.tensor([0, 37, slot + 1], dtype=torch.int32)  # inside a chunk; a row with no valid key


@functools.lru_cache(maxsize=None)
def _census_decode_case(b, hkv, t, slot, masked, kvs_kind):
    """Shared, read-only: (count, n, K, V, kv_start, mask) of one decode census shape (device tensors for the kernel)."""
    if kvs_kind == "small":
        kv_start = _small_kv_start(slot)
    else:  # mid-batch: random left padding, one row with no valid key
        kv_start = torch.randint(0, slot // 2, (b,), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
        kv_start[7] = slot + 1
    mask = xi.edge_mask(b, t, slot, seed=t + slot) if masked else None
    count, n = xi.census_counts(b, hkv, t, slot, 1, kv_start, mask)
    return (count, n, _rand_k(b, hkv, t, t + slot), xi.census_v(b, hkv, t, DEV), kv_start.to(DEV),
            None if mask is None else mask.to(DEV))


DECODE_TS = [(40, 17), (300, 299), (384, 255), (384, 256), (1030, 700), (1030, 1029)]
DECODE_KERNELS = ([("v3", k, r) for k in (1, 2, 4) for r in (1, 2, 4, 8)] +
                  [("v5", f, r) for f in (4, 12) for r in (1, 4, 8, 16)] +
                  [("v6", w, r) for w in (1, 2, 4, 8) for r in (1, 4, 8, 16)] +
                  [("v2", i, r) for i in (2, 4) for r in (1, 4, 8, 16)])
_KID = [f"{k}-{knob}-rep{r}" for k, knob, r in DECODE_KERNELS]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("t,slot", DECODE_TS)
@pytest.mark.parametrize("kernel,knob,rep", DECODE_KERNELS, ids=_KID)
def test_census_decode(kernel, knob, rep, t, slot, masked):
    """Every valid key counted exactly once by every small-batch decode kernel and geometry: slot on and just past a
    32 / 64 / 128 boundary, kv_start = 37 inside a chunk, a row without a valid key, forced mask bytes at chunk edges
    (v3 chunks at kpg x 1 / 2 / 4, v5 splits and both folds, v6's 32-key steps at every waves-per-pair, v2's splits)."""
    b, hkv = 3, 2
    count, n, kd, vd, kvs, mask = _census_decode_case(b, hkv, t, slot, masked, "small")
    q = torch.zeros(b, 1, hkv * rep, DH, dtype=BF16, device=DEV)
    with _decode_kernel(kernel, knob, b, hkv, t, rep, masked) as packs:
        out = _attend(q, kd, vd, slot, kvs, mask, packs)
    msg = xi.census_mismatch(out, count, n, rep)
    assert msg is None, msg


@pytest.mark.parametrize("b,hkv,rep,t,slot", [(40, 2, r, t, s) for r in (1, 2, 4) for t, s in ((300, 299), (520, 260))] +
                         [(256, 8, 8, 300, 299)])
def test_census_decode_v4_midbatch(b, hkv, rep, t, slot):
    """The one-split register-ring stream (v4) on mid-size batches (above 32 rows at rep <= 4; rep 8 from 2048 (row,
    kv head) pairs), no mask, random left padding."""
    count, n, kd, vd, kvs, _ = _census_decode_case(b, hkv, t, slot, False, "mid")
    q = torch.zeros(b, 1, hkv * rep, DH, dtype=BF16, device=DEV)
    with _decode_kernel("v4", 0, b, hkv, t, rep, False) as packs:
        out = _attend(q, kd, vd, slot, kvs, None, packs)
    msg = xi.census_mismatch(out, count, n, rep)
    assert msg is None, msg
    assert int(n[7, 0]) == 0


@pytest.mark.parametrize("spl", [1, 2])
@pytest.mark.parametrize("b,hkv,rep", [(1, 1, 8), (3, 1, 8), (2, 8, 4), (24, 1, 8)])
@pytest.mark.parametrize("t,slot", [(200, 199), (384, 300), (512, 130)])
def test_census_fused_qkv_attention_launch(b, hkv, rep, t, slot, spl):
    """The fused qkv + attention launch (128-key splits) without the norm (rms_eps None): row r of x is the unit
    vector e_r (e_0 for one row), the q and k rows of W are 0 and column r of the v rows is the census row of
    (r, kv head, slot) -- so the launch itself writes the new key's V row, which is then counted exactly once. The K
    row it wrote is 0 and the V row the census row, bit for bit; everything else in the caches is untouched."""
    e = ops.ext()
    k = 1024
    h = hkv * rep
    n = (h + 2 * hkv) * DH
    kv_start = (torch.tensor([0, 37, slot + 1] + [5 * i % 60 for i in range(b)], dtype=torch.int32)[:b]
                if b > 1 else torch.tensor([3], dtype=torch.int32))
    count, nv = xi.census_counts(b, hkv, t, slot, 1, kv_start)
    v_full = xi.census_v(b, hkv, t)
    x = torch.zeros(b, k, dtype=BF16)
    x[torch.arange(b), torch.arange(b)] = 1
    w = torch.zeros(n, k, dtype=BF16)
    w[(h + hkv) * DH:, :b] = v_full[:, :, slot].reshape(b, hkv * DH).t()
    kc0, vc0 = _rand_k(b, hkv, t, 5).cpu(), v_full.clone()
    kc0[:, :, slot] = 7.0   # stale rows at the new key's slot: the launch must overwrite both
    vc0[:, :, slot] = 0.5
    kd, vd = kc0.to(DEV), vc0.to(DEV)
    xd, pw = x.to(DEV), PackedLinear.from_dense(w, DEV)
    table = ref.rope_table(DH, 1024, 500000.0).to(DEV)
    pos = torch.full((b,), slot, dtype=torch.int32, device=DEV)
    sl = torch.tensor([slot], dtype=torch.int32, device=DEV)
    splits = e.qkv_attn_splits(b, b, hkv, rep, t, n, ops._num_cus(xd.device), spl)
    if spl == 2 and splits == 0:
        assert e.qkv_attn_splits(b, b, hkv, rep, t, n, ops._num_cus(xd.device), 1) > 0
        pytest.skip("the split qkv grid does not fit the CUs")
    assert splits == (t + 127) // 128
    packed = ops.packed_empty(b, h * DH, DEV)
    out = ops.linear_qkv_attention(xd, pw, None, table, pos, kd, vd, sl, kv_start.to(DEV), h, hkv, DH, splits,
                                   out_packed=packed, spl=spl)
    torch.cuda.synchronize()
    msg = xi.census_mismatch(out, count, nv, rep)
    assert msg is None, msg
    assert torch.equal(ref.unpack_act(packed.cpu(), b), out.cpu())
    kc0[:, :, slot] = 0
    assert torch.equal(vd.cpu(), v_full) and torch.equal(kd.cpu(), kc0)


PREFILL_IMPLS = [1, 2, 7, 8, 9, 13]
PREFILL_SHAPES = [(7, 0, False), (97, 100, False), (130, 10, False), (512, 0, False), (300, 0, True)]
PREFILL_CASES = [(i, s, s0, mk) for i in PREFILL_IMPLS for s, s0, mk in PREFILL_SHAPES if i != 1 or s <= 130]


@functools.lru_cache(maxsize=None)
def _census_prefill_case(s, slot0, masked):
    b, hkv = 2, 2
    t = slot0 + s + 5
    kv_start = torch.tensor([0, slot0 + s // 3], dtype=torch.int32)
    mask = xi.edge_mask(b, t, slot0 + s - 1, seed=s) if masked else None
    count, n = xi.census_counts(b, hkv, t, slot0, s, kv_start, mask)
    return (count, n, _rand_k(b, hkv, t, s), xi.census_v(b, hkv, t, DEV), kv_start.to(DEV),
            None if mask is None else mask.to(DEV))


@contextlib.contextmanager
def _prefill_impl(impl):
    e = ops.ext()
    try:
        e.attn_prefill_set_impl(impl)
        yield
    finally:
        e.attn_prefill_set_impl(2)


@pytest.mark.parametrize("rep", [1, 4, 8])
@pytest.mark.parametrize("impl,s,slot0,masked", PREFILL_CASES)
def test_census_prefill(impl, rep, s, slot0, masked):
    """Every query of a prefill (its own n and count: the causal diagonal at every position) on every prefill kernel:
    slot0 off the 32-key tile grid, an odd and an even number of query blocks (heavy / light pairing), left padding
    from inside a tile, queries without a valid key, forced mask bytes at tile edges."""
    b, hkv = 2, 2
    count, n, kd, vd, kvs, mask = _census_prefill_case(s, slot0, masked)
    q = torch.zeros(b, s, hkv * rep, DH, dtype=BF16, device=DEV)
    with _prefill_impl(impl):
        out = _attend(q, kd, vd, slot0, kvs, mask, False)
    msg = xi.census_mismatch(out, count, n, rep)
    assert msg is None, msg


# ---- B. needle -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _needle_case(b, hkv, rep, t, slot0, s, masked, kvs_kind):
    if kvs_kind == "small":
        kv_start = _small_kv_start(slot0)
    elif kvs_kind == "mid":
        kv_start = torch.randint(0, slot0 // 2, (b,), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
        kv_start[7] = slot0 + 1
    else:
        kv_start = torch.tensor([0, slot0 + s // 3], dtype=torch.int32)
    mask = xi.edge_mask(b, t, slot0 + s - 1, seed=t + slot0) if masked else None
    q, kc, vc, jstar, want = xi.needle_inputs(b, hkv, rep, t, slot0, s, kv_start, mask, seed=t + s + rep)
    # (the CPU tests show the reference's weights exactly one-hot under this condition)
    assert xi.needle_max_cross(kc) <= xi.NEEDLE_MAX_CROSS
    return q.to(DEV), kc.to(DEV), vc.to(DEV), kv_start.to(DEV), None if mask is None else mask.to(DEV), jstar, want


def _needle_report(out, want, jstar, rep):
    bad = (out.cpu() != want).reshape(jstar.shape[0], jstar.shape[1], jstar.shape[2], DH).any(-1).nonzero()
    bi, si, hi = [int(v) for v in bad[0]]
    return f"{bad.shape[0]} (b, s, h) rows are not their needle's V row; first b={bi} s={si} h={hi} j*={int(jstar[bi, si, hi])}"


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("t,slot", [(40, 17), (1030, 700)])
@pytest.mark.parametrize("kernel,knob,rep", DECODE_KERNELS, ids=_KID)
def test_needle_decode(kernel, knob, rep, t, slot, masked):
    """The output is the V row of the one key the query selects (first / last valid key, 32- and 128-boundaries +- 1,
    another key per head of a kv group) bit for bit: exact row fetch and head routing."""
    b, hkv = 3, 2
    q, kd, vd, kvs, mask, jstar, want = _needle_case(b, hkv, rep, t, slot, 1, masked, "small")
    with _decode_kernel(kernel, knob, b, hkv, t, rep, masked) as packs:
        out = _attend(q, kd, vd, slot, kvs, mask, packs)
    assert torch.equal(out.cpu(), want), _needle_report(out, want, jstar, rep)


@pytest.mark.parametrize("rep", [1, 2, 4])
def test_needle_decode_v4_midbatch(rep):
    b, hkv, t, slot = 40, 2, 520, 260
    q, kd, vd, kvs, _, jstar, want = _needle_case(b, hkv, rep, t, slot, 1, False, "mid")
    with _decode_kernel("v4", 0, b, hkv, t, rep, False) as packs:
        out = _attend(q, kd, vd, slot, kvs, None, packs)
    assert torch.equal(out.cpu(), want), _needle_report(out, want, jstar, rep)


@pytest.mark.parametrize("rep", [1, 4, 8])
@pytest.mark.parametrize("impl,s,slot0,masked", PREFILL_CASES)
def test_needle_prefill(impl, rep, s, slot0, masked):
    b, hkv = 2, 2
    q, kd, vd, kvs, mask, jstar, want = _needle_case(b, hkv, rep, slot0 + s + 5, slot0, s, masked, "prefill")
    with _prefill_impl(impl):
        out = _attend(q, kd, vd, slot0, kvs, mask, False)
    assert torch.equal(out.cpu(), want), _needle_report(out, want, jstar, rep)


# ---- D. ladder -----------------------------------------------------------------------
MMA, FMA = xi.LADDER_RTOL_MMA, xi.LADDER_RTOL_FMA  # bf16 P on the matrix cores (2u + 2^-12) / fp32 P (u + 2^-12)
DECODE_RTOL = {"v2": FMA, "v3": FMA, "v4": FMA, "v5": FMA, "v6": MMA}


def _ladder_case(b, hkv, rep, t, slot0, s, kv_start, mask):
    """{profile: (q on the device, K on the device, want fp64)} and the device V / kv_start / mask they share."""
    prof = {}
    for profile in xi.LADDER_PROFILES:
        q, kc, levels, gain = xi.ladder_inputs(b, hkv, rep, t, s, profile, seed=t + slot0)
        prof[profile] = (q.to(DEV), kc.to(DEV), xi.ladder_expected(b, hkv, rep, t, slot0, s, kv_start, mask, levels, gain))
    return prof, xi.census_v(b, hkv, t, DEV), kv_start.to(DEV), None if mask is None else mask.to(DEV)


@functools.lru_cache(maxsize=None)
def _ladder_decode_case(b, hkv, rep, t, slot, masked, kvs_kind):
    if kvs_kind == "small":
        kv_start = _small_kv_start(slot)
    else:
        kv_start = torch.randint(0, slot // 2, (b,), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
        kv_start[7] = slot + 1
    return _ladder_case(b, hkv, rep, t, slot, 1, kv_start, xi.edge_mask(b, t, slot, seed=t + slot) if masked else None)


@functools.lru_cache(maxsize=2)  # (the cases run shape by shape: see LADDER_PREFILL_CASES)
def _ladder_prefill_case(rep, s, slot0, masked):
    b, hkv = 2, 2
    t = slot0 + s + 5
    kv_start = torch.tensor([0, slot0 + s // 3], dtype=torch.int32)
    return _ladder_case(b, hkv, rep, t, slot0, s, kv_start, xi.edge_mask(b, t, slot0 + s - 1, seed=s) if masked else None)


def _assert_ladder(tag, results, rep, rtol):
    """``results``: (profile, out, want) of one case. Prints the worst relative error in units of u = 2^-8."""
    worst = {p: xi.ladder_worst_u(out, want) for p, out, want in results}
    print(f"ladder {tag}: worst relative error {max(worst.values()):.3f} u of the bound {rtol / xi.U_BF16:.4f} u", worst)
    for profile, out, want in results:
        msg = xi.ladder_mismatch(out, want, rep, rtol)
        assert msg is None, f"{profile}: {msg}"


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("t,slot", xi.LADDER_DECODE_TS)
@pytest.mark.parametrize("kernel,knob,rep", DECODE_KERNELS, ids=_KID)
def test_ladder_decode(kernel, knob, rep, t, slot, masked):
    """Scores that differ by design (tests/exact_inputs.py, the ladder) through every small-batch decode kernel: the
    running maximum moves in every chunk / split / wave (``ramp``), just over and under v6's lazy threshold of 8 log2
    units (``steps``), both ways inside a tile (``saw``), and sits at +-(170 .. 181) nats (``high``), with gains of both
    signs in the heads of one kv group. Every element within u + 2^-12 of the fp64 softmax for the fp32-P kernels (v2,
    v3, v5) and 2u + 2^-12 for v6 (P rounded to bf16 for the matrix cores); the row without a valid key exactly 0."""
    b, hkv = 3, 2
    prof, vd, kvs, mask = _ladder_decode_case(b, hkv, rep, t, slot, masked, "small")
    results = []
    with _decode_kernel(kernel, knob, b, hkv, t, rep, masked) as packs:
        for profile, (q, kd, want) in prof.items():
            results.append((profile, _attend(q, kd, vd, slot, kvs, mask, packs), want))
    _assert_ladder(f"decode {kernel}", results, rep, DECODE_RTOL[kernel])


@pytest.mark.parametrize("rep", [1, 2, 4])
def test_ladder_decode_v4_midbatch(rep):
    b, t, slot = xi.LADDER_V4
    hkv = 2
    prof, vd, kvs, _ = _ladder_decode_case(b, hkv, rep, t, slot, False, "mid")
    results = []
    with _decode_kernel("v4", 0, b, hkv, t, rep, False) as packs:
        for profile, (q, kd, want) in prof.items():
            results.append((profile, _attend(q, kd, vd, slot, kvs, None, packs), want))
    _assert_ladder("decode v4", results, rep, DECODE_RTOL["v4"])
    assert float(results[0][2][7].abs().max()) == 0  # (row 7 has no valid key)


# shape by shape, so that the cached inputs of a (rep, shape) serve every kernel in turn
LADDER_PREFILL_CASES = [(i, r, s, s0, mk) for s, s0, mk in xi.LADDER_PREFILL_SHAPES for r in (1, 4, 8)
                        for i in PREFILL_IMPLS if i != 1 or s <= 130]


@pytest.mark.parametrize("impl,rep,s,slot0,masked", LADDER_PREFILL_CASES)
def test_ladder_prefill(impl, rep, s, slot0, masked):
    """The ladder through every prefill kernel, every query checked: the gain cycles with the query index, so the
    lanes of one wave need their rescale at different tiles (and the wave-wide ballot of impls 2 / 7 / 8 / 9 / 13 moves
    a lane's maximum on another lane's account). 2u + 2^-12 for every impl: all of them are matrix-core kernels. Impl
    1 too rounds P to bf16 for its P.V MFMA (attn_prefill_kernel: ``pw[..] = f2bf(p[n][i])``, the row sum from the
    fp32 P), the same rounding as the others', so its bound carries that u: measured on an MI355X, impl 1 is
    off by up to 1.78 u and the impls 2 / 7 / 8 / 9 / 13 by up to 1.88 u."""
    prof, vd, kvs, mask = _ladder_prefill_case(rep, s, slot0, masked)
    results = []
    with _prefill_impl(impl):
        for profile, (q, kd, want) in prof.items():
            results.append((profile, _attend(q, kd, vd, slot0, kvs, mask, False), want))
    _assert_ladder(f"prefill impl {impl}", results, rep, MMA)


@pytest.mark.parametrize("spl", [1, 2])
@pytest.mark.parametrize("b,hkv,rep", [(1, 1, 8), (3, 1, 8), (2, 8, 4)])
@pytest.mark.parametrize("t,slot", xi.LADDER_FUSED_TS)
def test_ladder_fused_qkv_attention_launch(b, hkv, rep, t, slot, spl):
    """The fused qkv + attention launch (128-key splits, merged by the last arriver) on the ladder, built like
    test_census_fused_qkv_attention_launch: row r of x is e_r and column r of W holds row r's q | k | v of the new
    slot, so the launch itself produces the ladder query and writes the new key at its level and its census V row. The
    RoPE table is the quarter-turn table with the row of the new position set to the identity (a whole turn), every
    other row a real rotation. 2u + 2^-12 (bf16 P); the caches afterwards hold the ladder keys and the census bit for
    bit."""
    e = ops.ext()
    k = 1024
    h = hkv * rep
    n = (h + 2 * hkv) * DH
    kv_start = (torch.tensor([0, 37, slot + 1] + [5 * i % 60 for i in range(b)], dtype=torch.int32)[:b]
                if b > 1 else torch.tensor([3], dtype=torch.int32))
    v_full = xi.census_v(b, hkv, t)
    table = xi.quarter_table(NPOS)
    table[slot] = torch.tensor([1.0, 0.0])
    table = table.to(DEV)
    pos = torch.full((b,), slot, dtype=torch.int32, device=DEV)
    sl = torch.tensor([slot], dtype=torch.int32, device=DEV)
    xd = torch.zeros(b, k, dtype=BF16)
    xd[torch.arange(b), torch.arange(b)] = 1
    xd = xd.to(DEV)
    splits = e.qkv_attn_splits(b, b, hkv, rep, t, n, ops._num_cus(xd.device), spl)
    if spl == 2 and splits == 0:
        assert e.qkv_attn_splits(b, b, hkv, rep, t, n, ops._num_cus(xd.device), 1) > 0
        pytest.skip("the split qkv grid does not fit the CUs")
    assert splits == (t + 127) // 128
    results = []
    for profile in xi.LADDER_PROFILES:
        q, kc, levels, gain = xi.ladder_inputs(b, hkv, rep, t, 1, profile, seed=t + slot)
        want = xi.ladder_expected(b, hkv, rep, t, slot, 1, kv_start, None, levels, gain)
        w = torch.zeros(n, k, dtype=BF16)
        w[:h * DH, :b] = q.reshape(b, h * DH).t()
        w[h * DH:(h + hkv) * DH, :b] = kc[:, :, slot].reshape(b, hkv * DH).t()
        w[(h + hkv) * DH:, :b] = v_full[:, :, slot].reshape(b, hkv * DH).t()
        kc0, vc0 = kc.clone(), v_full.clone()
        kc0[:, :, slot] = 7.0   # stale rows at the new key's slot: the launch must overwrite both
        vc0[:, :, slot] = 0.5
        kd, vd = kc0.to(DEV), vc0.to(DEV)
        packed = ops.packed_empty(b, h * DH, DEV)
        out = ops.linear_qkv_attention(xd, PackedLinear.from_dense(w, DEV), None, table, pos, kd, vd, sl,
                                       kv_start.to(DEV), h, hkv, DH, splits, out_packed=packed, spl=spl)
        torch.cuda.synchronize()
        assert torch.equal(ref.unpack_act(packed.cpu(), b), out.cpu())
        assert torch.equal(vd.cpu(), v_full) and torch.equal(kd.cpu(), kc), profile
        results.append((profile, out, want))
    _assert_ladder("fused qkv + attention", results, rep, MMA)


# ======================================================================================
# C. integer GEMM / GEMV
# ======================================================================================
@functools.lru_cache(maxsize=None)
def _int_case(m, n, k, amp=2):
    """Shared, read-only: x (bf16, device), packed W, the interleaved gate/up packing of the same W, y = x W^T (int64)."""
    x, w, y = xi.int_gemm_inputs(m, n, k, seed=m + n + k + amp, amp=amp, plant=amp == 2 and k >= 66)
    if amp == 2 and k >= 66:  # (asserted on the host: the data holds |y| > 256 and exact bf16 ties)
        assert int(y.abs().max()) > 256 and bool(xi.bf16_ties(y)[m - 1, :4].all())
    return x.to(BF16).to(DEV), PackedLinear.from_dense(w.to(BF16), DEV), w, y


def _check_store_residual(run, m, n, y, packed_mirror=False):
    """``run(out, mode, accumulate, mirror, mirror_packed)`` launches one linear layer on the shared operands.
    STORE fp32 == y; STORE bf16 == RNE(y); RESIDUAL (accumulate on / off): h exact, mirror == bf16(h) (and the packed
    mirror unpacks to it)."""
    o32 = torch.empty(m, n, dtype=torch.float32, device=DEV)
    run(o32, STORE, True, None, None)
    assert torch.equal(o32.cpu(), y.float()), f"STORE fp32: {int((o32.cpu() != y.float()).sum())} elements differ"
    ob = torch.empty(m, n, dtype=BF16, device=DEV)
    run(ob, STORE, True, None, None)
    assert torch.equal(ob.cpu(), y.float().to(BF16)), "STORE bf16 is not the round-to-nearest-even of the exact sum"
    h0 = xi.int_residual(m, n, m + n)
    for acc in (True, False):
        hg = h0.float().to(DEV)
        mir = torch.full((m, n), 7.0, dtype=BF16, device=DEV)
        mp = ops.packed_empty(m, n, DEV) if packed_mirror else None
        run(hg, RESID, acc, mir, mp)
        want = (h0 + y if acc else y).float()
        assert torch.equal(hg.cpu(), want), f"RESIDUAL accumulate={acc}"
        assert torch.equal(mir.cpu(), want.to(BF16)), f"mirror accumulate={acc}"
        if mp is not None:
            assert torch.equal(ref.unpack_act(mp.cpu(), m), mir.cpu())


def _swiglu_case(m, f, k):
    """x, interleaved gate/up packing, (want, tol) of silu(g) * u for entries in {-1, 0, 1} (|g| stays far below the
    range where the fp32 sigmoid could cost a bf16 ulp)."""
    x = xi.int_matrix(m, k, 1, m + k)
    w1, w3 = xi.int_matrix(f, k, 1, f + k), xi.int_matrix(f, k, 1, f + k + 1)
    g, u = x @ w1.t(), x @ w3.t()
    assert int(g.abs().max()) <= 128
    gp = PackedLinear.from_dense(ref.interleave_gate_up(w1.to(BF16), w3.to(BF16)), DEV)
    return x.to(BF16).to(DEV), gp, xi.swiglu_exact(g, u)


def _assert_swiglu(got, want_tol):
    want, tol = want_tol
    err = (got.cpu().float() - want.float()).abs()
    assert bool((err <= tol).all()), f"SwiGLU: {int((err > tol).sum())} elements beyond one bf16 ulp, max {float(err.max())}"


GEMV_VARIANTS = [1, 5, 6, 10, 20, 16, 12, 15, 18, 21, 22, 26]
# variants 22 / 26 (4 tiles per workgroup) take N % 64 == 0 only: the launcher refuses the other two widths
GEMV_CASES = [(v, n, k) for v in GEMV_VARIANTS for n, k in ((768, 256), (48, 4096), (272, 1056))
              if v not in (22, 26) or n % 64 == 0]


@contextlib.contextmanager
def _gemv_variant(v):
    try:
        ops.GEMV_VARIANT = v
        yield
    finally:
        ops.GEMV_VARIANT = 0


@pytest.mark.parametrize("m", [1, 16, 17, 64])
@pytest.mark.parametrize("variant,n,k", GEMV_CASES)
def test_int_gemv(variant, n, k, m):
    """Every decode GEMV variant (row-major x and packed x, split-K 16 / 18 / 26): each x[m, k] w[n, k] term counted
    once -- one, two and four m-tiles, a ragged K tail (1056 = 33 x 32), 3 and 17 column tiles."""
    xg, pg, _, y = _int_case(m, n, k)
    xp = ref.pack_act(xg.cpu(), ops.packed_rows(m)).to(DEV) if variant in ops.XP_VARIANTS else None

    def run(out, mode, acc, mirror, mp):
        ops._gpu_linear(xg, pg, out, mode, None, acc, mirror, xp, mp)

    with _gemv_variant(variant):
        _check_store_residual(run, m, n, y, packed_mirror=n % 32 == 0)


@pytest.mark.parametrize("m", [1, 16, 17, 64])
@pytest.mark.parametrize("variant", GEMV_VARIANTS)
def test_int_gemv_swiglu(variant, m):
    f, k = 384, 512
    xg, gp, want = _swiglu_case(m, f, k)
    xp = ref.pack_act(xg.cpu(), ops.packed_rows(m)).to(DEV) if variant in ops.XP_VARIANTS else None
    ap = ops.packed_empty(m, f, DEV)
    with _gemv_variant(variant):
        got = ops.linear_swiglu(xg, gp, None, x_packed=xp, out_packed=ap)
    _assert_swiglu(got, want)
    assert torch.equal(ref.unpack_act(ap.cpu(), m), got.cpu())


@pytest.mark.parametrize("m", [40, 200])
def test_int_tiled_splitk(m):
    """The tiled GEMM's split-K partial slabs + reduce epilogue as the op layer plans it (ops.TILED)."""
    n, k = 768, 4096
    e = ops.ext()
    assert e.gemm_ksplit(m, n, k) > 1
    xg, pg, _, y = _int_case(m, n, k)

    def run(out, mode, acc, mirror, mp):
        ops._gpu_linear(xg, pg, out, mode, None, acc, mirror, None, mp)

    saved = autotune.ENABLED
    autotune.ENABLED = False  # the library's own split (gemm_ksplit) at M = 200 too, not a measured plan
    try:
        with _gemv_variant(ops.TILED):
            _check_store_residual(run, m, n, y,
                                  packed_mirror=m <= 64 and ops._tiled_packs(e, m, n, k, xg.device, RESID, None))
            xs, gp, want = _swiglu_case(m, n // 2, k)
            _assert_swiglu(ops.linear_swiglu(xs, gp, None), want)
    finally:
        autotune.ENABLED = saved


# (tile ids, (m, n, k, ksplit[, n_body])): the ragged shapes the tolerance tests of each kernel use
TILE_CASES = (
    [(t, c) for t in (1, 2, 3) for c in ((200, 768, 1024, 1), (300, 1008, 992, 3), (129, 1040, 96, 1))] +
    [(t, c) for t in (7, 13, 14) for c in ((200, 768, 1024, 1), (300, 1008, 1024, 2))] +
    [(16, c) for c in ((300, 1008, 256, 1), (260, 768, 64, 1), (300, 768, 2048, 2))] +
    [(17, c) for c in ((300, 1056, 1024, 1), (256, 512, 192, 1), (300, 768, 2048, 2))] +
    [(t, (m, n, k, ks)) for t in (11, 12) for m, n, k in ((200, 768, 1024), (129, 512, 3584)) for ks in (1, 3)] +
    [(18, (300, 448, 256, 1, 1)), (18, (300, 416, 256, 1, 1)), (19, (300, 640, 256, 1, 1))])


@pytest.mark.parametrize("tile,case", TILE_CASES, ids=[f"tile{t}-" + "x".join(map(str, c)) for t, c in TILE_CASES])
def test_int_gemm_tiles(tile, case):
    """Every tile id of the tiled GEMM (gemm2 1 / 2 / 3, gemm4 7 / 13 / 14, deep weights 16 / 17, gemm5 11 / 12, the
    tail-balanced 18 / 19) without the norm: store fp32 / bf16, residual + mirror (accumulate on and off), SwiGLU.
    ``gemm_plan_check`` decides what runs; a mode it refuses for a shape (SwiGLU at N % 32 != 0) is left out."""
    e = ops.ext()
    m, n, k, ks = case[:4]
    nb = case[4] if len(case) > 4 else 0
    g5 = tile in (11, 12)
    ran = []

    def legal(mode):
        return e.gemm_plan_check(m, n, k, mode, False, ks, tile, False, nb) == 0

    def ws():
        eks = e.gemm5_ksplit(k, ks) if g5 else ks
        return torch.empty(eks * m * (n + 1), dtype=torch.float32, device=DEV) if (g5 or ks > 1) else None

    if legal(STORE) and legal(RESID):
        xg, pg, _, y = _int_case(m, n, k)

        def run(out, mode, acc, mirror, mp):
            e.gemm(xg, pg.weight, n, k, out, mode, acc, mirror, ks, ws(), -1.0, tile, None, None, nb)
            torch.cuda.synchronize()

        _check_store_residual(run, m, n, y)
        ran += ["store", "residual"]
    if legal(SWIGLU):
        xs, gp, want = _swiglu_case(m, n // 2, k)
        o2 = torch.empty(m, n // 2, dtype=BF16, device=DEV)
        e.gemm(xs, gp.weight, n, k, o2, SWIGLU, True, None, ks, ws(), -1.0, tile, None, None, nb)
        torch.cuda.synchronize()
        _assert_swiglu(o2, want)
        ran.append("swiglu")
    print("ran:", ran)
    if not ran:
        pytest.skip("the plan resolver refuses this tile for this shape")


@pytest.mark.parametrize("g4", [0, 1])
@pytest.mark.parametrize("m,n,k", [(256, 1008, 512), (300, 4096, 1024)])
def test_int_gemm_argmax(m, n, k, g4):
    """Index and value of the fused lm_head argmax are the int64 product's first maximum (integer data: many exact
    ties, across lanes, waves and workgroups), on gemm2 and on gemm4."""
    e = ops.ext()
    xg, pg, _, y = _int_case(m, n, k)
    want_v = y.max(-1).values
    first = (y == want_v[:, None]).float().argmax(-1)  # (the first maximum, whatever torch's tie rule)
    assert int((y == want_v[:, None]).sum(-1).max()) > 1
    try:
        e.gemm_set_g4_default(g4)
        ws = torch.empty(e.gemm_argmax_workspace(m, n), dtype=torch.float32, device=DEV)
        idx = torch.empty(m, dtype=torch.int32, device=DEV)
        val = torch.empty(m, dtype=torch.float32, device=DEV)
        e.gemm_argmax(xg, pg.weight, n, k, ws, -1.0, idx, val)
        torch.cuda.synchronize()
    finally:
        e.gemm_set_g4_default(1)
    assert torch.equal(idx.cpu().long(), first) and torch.equal(val.cpu(), want_v.float())


@pytest.mark.parametrize("m", [1, 17, 64])
@pytest.mark.parametrize("variant", [1, 5, 6, 10, 20])
def test_int_skinny_argmax(variant, m):
    e = ops.ext()
    n, k = 2048, 512
    xg, pg, _, y = _int_case(m, n, k)
    want_v = y.max(-1).values
    first = (y == want_v[:, None]).float().argmax(-1)
    part = torch.empty(m * (n // 16) * 2, dtype=torch.float32, device=DEV)
    idx = torch.empty(m, dtype=torch.int32, device=DEV)
    val = torch.empty(m, dtype=torch.float32, device=DEV)
    e.linear_skinny_argmax(xg, pg.weight, n, k, -1.0, variant, part, idx, val)
    torch.cuda.synchronize()
    assert torch.equal(idx.cpu().long(), first) and torch.equal(val.cpu(), want_v.float())


@pytest.mark.parametrize("m,n,k", [(1, 512, 256), (5, 1000, 4096), (130, 257, 96)])
def test_int_linear_f32(m, n, k):
    x, w, y = xi.int_gemm_inputs(m, n, k, seed=m + n, plant=k >= 66 and n >= 4)
    got = ops.linear_f32(x.float().to(DEV), w.float().to(DEV))
    assert torch.equal(got.cpu(), y.float())


# ---- QKV + RoPE epilogues with the quarter-turn table ---------------------------------
NPOS = 1024


def _positions(m, seed):
    """Distinct, non-monotonic positions: a random permutation of the table's rows."""
    return torch.randperm(NPOS, generator=torch.Generator().manual_seed(seed))[:m].to(torch.int32)


def _assert_qkv(got, want):
    for name, a, b in zip(("q", "K cache", "V cache"), got, want):
        assert torch.equal(a.cpu(), b), f"{name}: {int((a.cpu() != b).sum())} elements differ"


def test_rope_kv_write_exact():
    b, s, h, hkv, t, slot0 = 3, 5, 8, 2, 16, 3
    m = b * s
    qkv = xi.int_matrix(m, (h + 2 * hkv) * DH, 100, 1)  # (|v| <= 100: exact in the bf16 qkv buffer)
    pos = _positions(m, 1)
    want = xi.qkv_rope_exact(qkv, pos, NPOS, b, s, h, hkv, t, slot0)
    kg = torch.zeros(b, hkv, t, DH, dtype=BF16, device=DEV)
    vg = torch.zeros_like(kg)
    qg = ops.rope_kv_write(qkv.to(BF16).to(DEV), xi.quarter_table(NPOS).to(DEV), pos.to(DEV), kg, vg, slot0, s, h, hkv, DH)
    _assert_qkv((qg, kg, vg), want)


@pytest.mark.parametrize("m,s", [(1, 1), (16, 1), (6, 3), (60, 20)])
@pytest.mark.parametrize("variant", [1, 6, 16])
def test_qkv_rope_gemv_epilogue_exact(variant, m, s):
    h, hkv, t, k, slot0 = 4, 2, 40, 1024, 7
    b = m // s
    n = (h + 2 * hkv) * DH
    xg, pg, _, y = _int_case(m, n, k)
    pos = _positions(m, m)
    want = xi.qkv_rope_exact(y, pos, NPOS, b, s, h, hkv, t, slot0)
    kg = torch.zeros(b, hkv, t, DH, dtype=BF16, device=DEV)
    vg = torch.zeros_like(kg)
    with _gemv_variant(variant):
        qg = ops.linear_qkv_rope(xg, pg, None, xi.quarter_table(NPOS).to(DEV), pos.to(DEV), kg, vg,
                                 torch.tensor([slot0], dtype=torch.int32, device=DEV), s, h, hkv, DH)
    _assert_qkv((qg, kg, vg), want)


def _gemm_qkv(e, xg, pg, n, k, pos, b, s, h, hkv, t, slot0, ks, eps, tile, rms_ws):
    m = b * s
    kg = torch.zeros(b, hkv, t, DH, dtype=BF16, device=DEV)
    vg = torch.zeros_like(kg)
    qg = torch.empty(m, h, DH, dtype=BF16, device=DEV)
    g5 = tile in (11, 12)
    eks = e.gemm5_ksplit(k, ks) if g5 else ks
    ws = torch.empty(eks * m * (n + 1), dtype=torch.float32, device=DEV) if (g5 or ks > 1) else None
    e.gemm_qkv(xg, pg.weight, n, k, xi.quarter_table(NPOS).to(DEV), pos.to(DEV), kg, vg,
               torch.tensor([slot0], dtype=torch.int32, device=DEV), s, h, hkv, DH, qg, ks, ws, eps, tile, rms_ws)
    torch.cuda.synchronize()
    return qg, kg, vg


@pytest.mark.parametrize("tile,m,s,ks", [(1, 96, 2, 4), (7, 300, 3, 2), (11, 200, 1, 1), (11, 130, 2, 3), (12, 200, 1, 1),
                                         (12, 130, 2, 3)])
def test_qkv_rope_reduce_epilogue_exact(tile, m, s, ks):
    """RoPE + KV-cache write in the split-K reduce kernel (behind gemm2 / gemm4 partial slabs and gemm5's), no norm."""
    e = ops.ext()
    h, hkv, k, slot0 = 8, 2, 2048, 11
    b = m // s
    t = slot0 + s + 3
    n = (h + 2 * hkv) * DH
    assert e.gemm_plan_check(m, n, k, QKV, False, ks, tile, False) == 0
    xg, pg, _, y = _int_case(m, n, k)
    pos = _positions(m, m + tile)
    want = xi.qkv_rope_exact(y, pos, NPOS, b, s, h, hkv, t, slot0)
    _assert_qkv(_gemm_qkv(e, xg, pg, n, k, pos, b, s, h, hkv, t, slot0, ks, -1.0, tile, None), want)


@functools.lru_cache(maxsize=None)
def _pow2_case(m, n, k):
    x, scale = xi.pow2_rows(m, k, m + k)
    w = xi.int_matrix(n, k, 2, n + k)
    return x.to(BF16).to(DEV), PackedLinear.from_dense(w.to(BF16), DEV), x @ w.t(), scale


@pytest.mark.parametrize("tile,m,s", [(1, 300, 3), (1, 256, 1), (7, 300, 3), (7, 256, 1), (16, 300, 3), (16, 256, 1)])
def test_qkv_rope_direct_epilogue_exact(tile, m, s):
    """The GEMM's own RoPE / KV-write epilogue (gemm2 256 x 256, gemm4, 256 x 192 tiles) needs the fused norm: rms_eps
    0.0, K a power of two and rows of +-2^(r % 3), so the row scale is exactly 1, 1/2 or 1/4 (IEEE 1 / sqrt of 1, 4,
    16 in the gemm2 loop; the rms_rowinv statistic for gemm4) -- a statistic applied to a neighbouring row is off by a
    factor of 2. Measured on an MI355X: both the in-loop 1 / sqrt and the precomputed rsqrt return the three scales
    exactly (test_fused_norm_store_exact prints observed / exact = 1.0), so these cases are compared bit for bit too."""
    e = ops.ext()
    h, hkv, k, slot0 = 8, 2, 1024, 11
    b = m // s
    t = slot0 + s + 3
    n = (h + 2 * hkv) * DH
    rw = torch.empty(m, device=DEV) if tile != 1 else None
    assert e.gemm_qkv_direct_ok(m, tile, k) and e.gemm_plan_check(m, n, k, QKV, True, 1, tile, rw is not None) == 0
    xg, pg, y, scale = _pow2_case(m, n, k)
    pos = _positions(m, m + tile)
    want = xi.qkv_rope_exact(y, pos, NPOS, b, s, h, hkv, t, slot0, scale)
    _assert_qkv(_gemm_qkv(e, xg, pg, n, k, pos, b, s, h, hkv, t, slot0, 1, 0.0, tile, rw), want)


@pytest.mark.parametrize("tile", [1, 7])
def test_fused_norm_store_exact(tile):
    """Plain fp32 store with the fused norm and exact power-of-two row scales: tile 1 sums the statistic in its main
    loop, tile 7 reads the one computed ahead of it (rms_ws). Measured on an MI355X: observed / exact scale = 1.0 on
    every row for both, so the comparison is bit for bit."""
    e = ops.ext()
    m, n, k = 300, 768, 1024
    xg, pg, y, scale = _pow2_case(m, n, k)
    rw = torch.empty(m, device=DEV) if tile == 7 else None
    assert e.gemm_plan_check(m, n, k, STORE, True, 1, tile, rw is not None) == 0
    out = torch.empty(m, n, dtype=torch.float32, device=DEV)
    e.gemm(xg, pg.weight, n, k, out, STORE, True, None, 1, None, 0.0, tile, None, rw)
    torch.cuda.synchronize()
    want = (y.double() * scale[:, None]).float()
    ratio = (out.cpu().double() / want.double())[want != 0]
    print("row scale: observed / exact in", float(ratio.min()), float(ratio.max()))
    assert torch.equal(out.cpu(), want), f"{int((out.cpu() != want).sum())} elements differ"
