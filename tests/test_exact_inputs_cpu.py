"""The exact-answer input builders (tests/exact_inputs.py) validated against ``ops/reference.py`` alone: what the GPU
tests (tests/test_exact_gpu.py) assert about the kernels holds for the reference, with the margins the bounds assume."""
from __future__ import annotations

import math

import pytest
import torch

import exact_inputs as xi
from jax_llama_amd.ops import reference as ref

BF16 = torch.bfloat16


def test_census_bound_margins():
    """|bf16(c / n) * n - c| < 0.04 for every n <= 1152 and c <= min(n, 9) (a class of T <= 1152 keys holds at most
    9). A run of n consecutive keys holds c <= ceil(n / 128) of a class; there one dropped key moves its column by
    (n - c) / (n - 1) >= 0.9 and one extra or doubled key by (n - c) / (n + 1) >= 0.5 from n = 3 on (1 / 3 at n = 2;
    the double of an only key changes nothing in any softmax): CENSUS_TOL = 0.25 plus the rounding separates them."""
    n = torch.arange(1, 1153, dtype=torch.float64)[:, None]
    c = torch.arange(0, 10, dtype=torch.float64)[None, :]
    ok = c <= n
    r = (c / n).float().to(BF16).double() * n - c
    assert float(r[ok].abs().max()) < 0.04 < xi.CENSUS_TOL
    run = (c <= torch.ceil(n / 128)) & (n >= 2)
    drop = ((n - c) / (n - 1))[run & (c >= 1)]
    extra = (n - c) / (n + 1)
    assert float(drop.min()) >= 0.9 and float(extra[run & (n >= 3)].min()) >= 0.5
    assert float(extra[run].min()) > xi.CENSUS_TOL + 0.04


@pytest.mark.parametrize("t,slot,masked", [(40, 17, False), (384, 256, True), (1030, 700, False), (1030, 1029, True)])
def test_census_decode_is_the_reference(t, slot, masked):
    b, hkv, rep = 3, 2, 4
    kv_start = torch.tensor([0, 37, slot + 1], dtype=torch.int32)
    mask = xi.edge_mask(b, t, slot, seed=t + slot) if masked else None
    if masked:
        for j in xi.MASK_ZEROS + (slot - 1,):
            assert j >= t or not mask[:, j].any()
        for j in xi.MASK_ONES + (slot,):
            assert j >= t or mask[:, j].all()
    count, n = xi.census_counts(b, hkv, t, slot, 1, kv_start, mask)
    assert int(n[2, 0]) == 0 and int(n[0, 0]) > 0
    kc = torch.randn(b, hkv, t, xi.DH).to(BF16)
    q = torch.zeros(b, 1, hkv * rep, xi.DH, dtype=BF16)
    out = ref.attention(q, kc, xi.census_v(b, hkv, t), slot, kv_start, mask).reshape(b, -1)
    assert xi.census_mismatch(out, count, n, rep) is None
    # the check has teeth: the census of one key fewer / one key more is refused
    c2, n2 = xi.census_counts(b, hkv, t, slot - 1, 1, kv_start, mask)
    assert xi.census_mismatch(out, c2, n2, rep) is not None
    bad = out.clone().float()
    bad[0, 5] = float("nan")
    assert xi.census_mismatch(bad, count, n, rep) is not None


@pytest.mark.parametrize("s,slot0,masked", [(7, 0, False), (97, 100, False), (130, 10, True)])
def test_census_prefill_is_the_reference(s, slot0, masked):
    b, hkv, rep = 2, 2, 2
    t = slot0 + s + 5
    kv_start = torch.tensor([0, slot0 + s // 3], dtype=torch.int32)
    mask = xi.edge_mask(b, t, slot0 + s - 1, seed=s) if masked else None
    count, n = xi.census_counts(b, hkv, t, slot0, s, kv_start, mask)
    kc = torch.randn(b, hkv, t, xi.DH).to(BF16)
    q = torch.zeros(b, s, hkv * rep, xi.DH, dtype=BF16)
    out = ref.attention(q, kc, xi.census_v(b, hkv, t), slot0, kv_start, mask).reshape(b * s, -1)
    assert xi.census_mismatch(out, count, n, rep) is None
    err = out.double().reshape(b, s, hkv, rep, xi.DH) * n.double()[:, :, None, None, None] - count.double()[:, :, :, None]
    assert float(err.abs().max()) < 0.04


@pytest.mark.parametrize("t,slot0,s,masked", [(40, 17, 1, False), (1030, 1029, 1, False), (384, 255, 1, True),
                                              (135, 0, 130, False), (305, 0, 300, True)])
def test_needle_weights_exactly_one_hot(t, slot0, s, masked):
    """The condition the GPU needle tests rest on, met by the reference alone: the fp32 softmax weights are exactly 1
    at the needle and exactly 0 elsewhere, so the output is the needle's V row bit for bit; and the score lead has the
    margin ``NEEDLE_MAX_CROSS`` promises."""
    b, hkv, rep = (3, 2, 4) if s == 1 else (2, 2, 2)
    h = hkv * rep
    kv_start = (torch.tensor([0, 37, slot0 + 1], dtype=torch.int32) if s == 1
                else torch.tensor([0, slot0 + s // 3], dtype=torch.int32))
    mask = xi.edge_mask(b, t, slot0 + s - 1, seed=t) if masked else None
    q, kc, vc, jstar, want = xi.needle_inputs(b, hkv, rep, t, slot0, s, kv_start, mask, seed=t + s)
    assert xi.needle_max_cross(kc) <= xi.NEEDLE_MAX_CROSS and xi.needle_gap(xi.NEEDLE_MAX_CROSS) > 1.5 * 104
    out, p = ref.attention(q, kc, vc, slot0, kv_start, mask, return_weights=True)
    tl = slot0 + s
    onehot = torch.nn.functional.one_hot(jstar.clamp_min(0), tl).float() * (jstar >= 0)[..., None]  # [b, s, h, tl]
    assert torch.equal(p, onehot.permute(0, 2, 1, 3))
    assert torch.equal(out.reshape(b * s, h * xi.DH), want)
    ok = xi.valid_keys(b, t, slot0, s, kv_start, mask)
    assert bool(ok[torch.arange(b)[:, None, None], torch.arange(s)[None, :, None], jstar.clamp_min(0)][jstar >= 0].all())
    if s == 1:  # the edges are among the needles, and the heads of a kv group differ
        js = set(jstar[0, 0].tolist())
        lo, hi = int(ok[0, 0].nonzero()[0]), int(ok[0, 0].nonzero()[-1])
        assert lo in js and hi == slot0 and len(js) == min(h, len(xi.needle_candidates(ok[0, 0])))
        assert int(jstar[2].max()) == -1 and int(want[2].float().abs().max()) == 0
    else:  # every query's diagonal key is some head's needle at the queries where the cycle starts there
        diag = (jstar == (slot0 + torch.arange(s))[None, :, None]).any(-1)
        assert int(diag.sum()) > 0


# ---- the ladder ------------------------------------------------------------------------
def _ladder_shapes():
    """(b, hkv, rep, t, slot0, s, kv_start kind, masked) of every shape and mask the GPU tests run the ladder at
    (one rep each: the reference and the loop below treat every head alike)."""
    out = []
    for t, slot in dict.fromkeys(xi.LADDER_DECODE_TS + xi.LADDER_KV8_SPLIT_TS):
        out += [(3, 2, 4, t, slot, 1, "small", masked) for masked in (False, True)]
    out.append((xi.LADDER_V4[0], 2, 2, xi.LADDER_V4[1], xi.LADDER_V4[2], 1, "mid", False))
    out += [(2, 2, 4, slot0 + s + 5, slot0, s, "prefill", masked) for s, slot0, masked in xi.LADDER_PREFILL_SHAPES]
    out += [(b, hkv, rep, t, slot, 1, "fused", False) for b, hkv, rep in ((1, 1, 8), (3, 1, 8), (2, 8, 4))
            for t, slot in xi.LADDER_FUSED_TS]
    return out


def _ladder_kv_start(kind, b, slot0, s):
    """The kv_start vectors of the GPU tests (test_exact_gpu.py, test_kv8_gpu.py), by kind."""
    if kind == "small":
        return torch.tensor([0, 37, slot0 + 1], dtype=torch.int32)
    if kind == "mid":
        kv_start = torch.randint(0, slot0 // 2, (b,), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
        kv_start[7] = slot0 + 1
        return kv_start
    if kind == "prefill":
        return torch.tensor([0, slot0 + s // 3], dtype=torch.int32)
    return (torch.tensor([0, 37, slot0 + 1] + [5 * i % 60 for i in range(b)], dtype=torch.int32)[:b]
            if b > 1 else torch.tensor([3], dtype=torch.int32))


def _lazy_rescale_loop(q, kc, cls, ok, rescale=True):
    """The lazy-rescale online softmax of the MFMA kernels in plain tensor steps: 32-key tiles, log2 units, the running
    maximum moves only when some head of the query sees a tile maximum more than 8 above its own (the wave-wide
    ballot), P rounded to bf16 for the P.V sum, the row sum l in fp32 from the unrounded P. ``cls`` [b, h, t]: the
    class of each key's unit V row; ``ok`` [b, s, t]. ``rescale`` False leaves l and O as they are when the maximum
    moves -- the bug the family has to catch. Returns bf16 [b, s, h, 128]."""
    b, s, h, _ = q.shape
    t = kc.shape[2]
    rep = h // kc.shape[1]
    scale_log2 = torch.tensor(math.log2(math.e) / math.sqrt(xi.DH), dtype=torch.float32)
    kf = kc.float().repeat_interleave(rep, dim=1)
    dots = torch.einsum("bshd,bhtd->bsht", q.float(), kf)  # exact in fp32
    sc_all = (dots * scale_log2).masked_fill(~ok[:, :, None, :], float("-inf"))
    m = torch.full((b, s, h), float("-inf"))
    l = torch.zeros(b, s, h)
    o = torch.zeros(b, s, h, xi.DH)
    for k0 in range(0, t, 32):
        sc = sc_all[..., k0:k0 + 32]
        tmax = sc.amax(-1)
        trig = (tmax > m + 8.0).any(-1, keepdim=True)
        m_new = torch.where(trig, torch.maximum(m, tmax), m)
        alpha = torch.exp2(m - torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new))
        alpha = torch.where(torch.isnan(alpha), torch.ones_like(alpha), alpha)
        if rescale:
            l = l * alpha
            o = o * alpha[..., None]
        m = m_new
        p = torch.exp2(sc - torch.where(torch.isinf(m), torch.zeros_like(m), m)[..., None])
        l = l + p.sum(-1)
        o.scatter_add_(-1, cls[:, None, :, k0:k0 + 32].expand(b, s, h, -1), p.to(BF16).float())
    out = torch.where(l[..., None] > 0, o / l[..., None].clamp_min(1e-38), torch.zeros_like(o))
    return out.to(BF16)


@pytest.mark.parametrize("b,hkv,rep,t,slot0,s,kind,masked", _ladder_shapes())
def test_ladder_family(b, hkv, rep, t, slot0, s, kind, masked):
    """What the GPU ladder tests rest on, at each of their shapes and masks and for every profile: the scores of the
    bf16 tensors are gain * level / sqrt(128) bit for bit; ``ref.attention`` (fp32) is within u + 2^-12 of the fp64
    softmax per element and exactly 0 where a query has no key; the keys survive the fp8 round trip; a lazy-rescale loop
    with bf16 P is within 2u + 2^-12 -- and the same loop without the rescale of l and O misses that bound by a factor
    of 1000 or more on ``ramp``, ``steps`` and ``saw`` wherever a query's keys span more than one tile.

    One shape cannot reach the factor 1000 whatever a loop does wrong, the unmasked 8001 keys of the t = 8192 cache
    with their 62 keys of every class: ``ramp`` there holds 64 keys per level, so even at gain 16 a whole period of the
    128 classes spans 4.2 log2 units and the smallest class weight is about 1 / 770, while the loop without the rescale
    weighs every stretch between two moves of the maximum alike, near 1 / 128 per class: 5 times the smallest weight,
    600 times the bound at the very most (411 here). ``steps`` repeats every 544 keys, the maximum stops moving inside
    the first period, and the 14 periods that follow are weighed correctly: the error is one period's share, 22 times
    the bound. These two must still miss the bound 10 times over; with the mask (some classes keep few keys) and on
    ``saw`` the factor 1000 holds there too."""
    import kv8_inputs as k8
    h = hkv * rep
    kv_start = _ladder_kv_start(kind, b, slot0, s)
    mask = xi.edge_mask(b, t, slot0 + s - 1, seed=s if kind == "prefill" else t + slot0) if masked else None
    ok = xi.valid_keys(b, t, slot0, s, kv_start, mask)
    tiles = torch.nn.functional.pad(ok, (0, -t % 32)).reshape(b, s, -1, 32).any(-1).sum(-1)  # 32-key tiles per query
    if kind != "fused" or b == 3:
        assert int(ok.sum(-1).min()) == 0  # a query without a valid key is among them
    vc = xi.census_v(b, hkv, t)
    cls = xi._census_class(b, hkv, t).repeat_interleave(rep, dim=1)
    for profile in xi.LADDER_PROFILES:
        q, kc, levels, gain = xi.ladder_inputs(b, hkv, rep, t, s, profile, seed=t + slot0)
        assert set(gain.unique().tolist()) <= set(xi.GAINS) and torch.equal(q.double().abs().amax(-1), gain.abs())
        assert s == 1 or len(gain.unique()) == len(xi.GAINS)
        want = xi.ladder_expected(b, hkv, rep, t, slot0, s, kv_start, mask, levels, gain)
        tot = want.sum(-1)
        assert bool(((tot - 1).abs() < 1e-12)[ok.any(-1)].all()) and bool((tot[~ok.any(-1)] == 0).all())
        # the scores, recomputed from the tensors the kernels read
        sc = torch.einsum("bshd,bhtd->bsht", q.double(), kc.double().repeat_interleave(rep, dim=1)) / math.sqrt(xi.DH)
        assert torch.equal(sc, xi.ladder_scores(levels, gain))
        # the fp32 reference
        out = ref.attention(q, kc, vc, slot0, kv_start, mask)
        msg = xi.ladder_mismatch(out, want, rep, xi.LADDER_RTOL_FMA)
        assert msg is None, (profile, msg)
        assert bool((out.reshape(b, s, -1)[~ok.any(-1)] == 0).all())
        # the fp8 cache holds the same keys
        k8q = k8.quantize_kv(kc)
        assert torch.equal(k8q.dequant(), kc) and torch.equal(k8.quantize_kv(vc).dequant(), vc)
        # sensitivity
        lazy = _lazy_rescale_loop(q, kc, cls, ok)
        msg = xi.ladder_mismatch(lazy, want, rep, xi.LADDER_RTOL_MMA)
        assert msg is None, (profile, msg)
        broken = _lazy_rescale_loop(q, kc, cls, ok, rescale=False)
        worst = float(xi.ladder_excess(broken, want, xi.LADDER_RTOL_MMA).max())
        print(f"{profile}: reference {xi.ladder_worst_u(out, want):.2f} u, lazy loop {xi.ladder_worst_u(lazy, want):.2f} u, "
              f"loop without the rescale {worst:.3g} x the bound")
        if profile != "high" and int(tiles.max()) > 1:
            assert worst >= (10 if t == 8192 and not masked and profile != "saw" else 1000), (profile, worst)


def test_ladder_mismatch_reports():
    b, hkv, rep, t, slot = 3, 2, 4, 384, 256
    kv_start = torch.tensor([0, 37, slot + 1], dtype=torch.int32)
    q, kc, levels, gain = xi.ladder_inputs(b, hkv, rep, t, 1, "steps", seed=1)
    want = xi.ladder_expected(b, hkv, rep, t, slot, 1, kv_start, None, levels, gain)
    good = want.float().to(BF16).reshape(b, -1)
    assert xi.ladder_mismatch(good, want, rep, xi.LADDER_RTOL_FMA) is None and xi.ladder_worst_u(good, want) <= 1.0
    bad = good.clone().float()
    bad[1, 3 * xi.DH: 4 * xi.DH] *= 2  # head 3 of row 1 twice too large: a skipped rescale by one log2 unit
    msg = xi.ladder_mismatch(bad, want, rep, xi.LADDER_RTOL_MMA)
    assert msg is not None and "b=1 s=0 h=3" in msg and "ratio 2" in msg and "2^1.0" in msg
    leak = good.clone()
    leak[2, 5] = 1e-20  # the row without a valid key must be exactly 0
    assert "b=2" in xi.ladder_mismatch(leak, want, rep, xi.LADDER_RTOL_MMA)
    nan = good.clone().float()
    nan[0, 0] = float("nan")
    assert xi.ladder_mismatch(nan, want, rep, xi.LADDER_RTOL_MMA) is not None


@pytest.mark.parametrize("m,n,k", [(1, 768, 256), (17, 48, 4096), (200, 768, 1024), (129, 1040, 96)])
def test_int_gemm_data_has_ties_and_is_exact_in_fp32(m, n, k):
    x, w, y = xi.int_gemm_inputs(m, n, k, seed=m + n + k)
    assert int(x.abs().max()) <= 2 and int(w.abs().max()) <= 2
    assert m == 1 or float((x == 0).float().mean()) > 0.3
    assert y[m - 1, :4].tolist() == [257, 259, -257, -259]
    ties = xi.bf16_ties(y)
    assert bool(ties[m - 1, :4].all()) and int(y.abs().max()) > 256
    # a tie is where round-to-nearest-even and truncation part: RNE of 257 / 259 is 256 / 260
    yb = y.float().to(BF16)
    assert yb[m - 1, :4].tolist() == [256.0, 260.0, -256.0, -260.0]
    assert not bool(xi.bf16_ties(torch.tensor([255, 256, 258, 260, 3, 0, 516, 1026])).any())
    assert bool(xi.bf16_ties(torch.tensor([257, -259, 514, 1028])).all())
    # the reference GEMM (bf16 operands, fp32 accumulation) is the int64 product exactly
    got = ref.linear(x.float(), w.to(BF16), None, torch.float32)
    assert torch.equal(got.long(), y) and torch.equal(got, y.float())
    h = xi.int_residual(m, n, 3)
    assert int((h + y).abs().max()) < 2 ** 24 and int(h.abs().max()) <= 1000


def test_swiglu_exact_is_the_reference_within_one_ulp():
    m, f, k = 17, 64, 512
    x = xi.int_matrix(m, k, 1, 1)
    w1, w3 = xi.int_matrix(f, k, 1, 2), xi.int_matrix(f, k, 1, 3)
    g, u = x @ w1.t(), x @ w3.t()
    assert int(g.abs().max()) < 100
    want, tol = xi.swiglu_exact(g, u)
    got = ref.linear_swiglu(x.float(), ref.interleave_gate_up(w1.to(BF16), w3.to(BF16)), None)
    assert bool(((got.float() - want.float()).abs() <= tol).all())
    assert bool((got[want == 0] == 0).all())


def test_quarter_turn_rope_is_the_reference():
    """ref.linear_qkv_rope / ref.rope_kv_write with the quarter-turn table give the host-integer result exactly, cache
    slots outside [slot0, slot0 + s) untouched; and the table separates positions and pairs."""
    b, s, h, hkv, t, k, npos, slot0 = 3, 2, 4, 2, 9, 256, 64, 3
    m = b * s
    n = (h + 2 * hkv) * xi.DH
    table = xi.quarter_table(npos)
    qt = xi.quarter_turns(npos)
    assert sorted(qt.unique().tolist()) == [0, 1, 2, 3]
    differ = (qt[:, None, :] != qt[None, :, :]).sum(-1) + 64 * torch.eye(npos, dtype=torch.long)
    assert int(differ.min()) >= 30  # a wrong position shows in many pairs
    assert torch.equal(table.pow(2).sum(-1), torch.ones(npos, xi.DH // 2))
    pos = torch.tensor([5, 40, 0, 63, 17, 2], dtype=torch.int32)
    x, w, y = xi.int_gemm_inputs(m, n, k, seed=9)
    q, kc, vc = xi.qkv_rope_exact(y, pos, npos, b, s, h, hkv, t, slot0)
    kr, vr = torch.zeros(b, hkv, t, xi.DH, dtype=BF16), torch.zeros(b, hkv, t, xi.DH, dtype=BF16)
    qr = ref.linear_qkv_rope(x.float(), w.to(BF16), None, table, pos, kr, vr, slot0, s, h, hkv, xi.DH)
    assert torch.equal(qr, q) and torch.equal(kr, kc) and torch.equal(vr, vc)
    assert int(kc[:, :, :slot0].abs().max()) == 0 and int(kc[:, :, slot0 + s:].abs().max()) == 0
    # rope_kv_write on integers small enough for a bf16 qkv
    ys = xi.int_matrix(m, n, 100, 4)
    q2, kc2, vc2 = xi.qkv_rope_exact(ys, pos, npos, b, s, h, hkv, t, slot0)
    kr.zero_(), vr.zero_()
    qr2 = ref.rope_kv_write(ys.to(BF16), table, pos, kr, vr, slot0, s, h, hkv, xi.DH)
    assert torch.equal(qr2, q2) and torch.equal(kr, kc2) and torch.equal(vr, vc2)


def test_pow2_rows_scale_exactly():
    x, scale = xi.pow2_rows(7, 256, 1)
    assert int((x == 0).sum()) == 0
    assert torch.equal(ref.inv_rms(x.float(), 0.0).flatten().double(), scale)
    assert scale.tolist()[:3] == [1.0, 0.5, 0.25]
