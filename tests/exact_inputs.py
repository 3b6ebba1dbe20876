"""Inputs for which the right answer of a kernel is known exactly, so that an indexing error (one key, one K term,
one column, one table entry off) is an integer-sized error instead of one that hides under a bf16 tolerance.

Plain host code (CPU tensors, integer / fp64 arithmetic); ``tests/test_exact_inputs_cpu.py`` validates every builder
against ``ops/reference.py`` and ``tests/test_exact_gpu.py`` runs the HIP kernels on them.

  * attention key census: q = 0 (every valid score is exactly 0, the softmax is uniform) and V rows that are unit
    vectors of the key's residue class mod 128, so ``out * n`` counts the valid keys of every class;
  * attention needle: +-1 keys and q = 32 * K[j*], so the fp32 softmax is exactly one-hot and the output is the V row
    of the needle bit for bit;
  * attention ladder: keys that equal a +-1 vector u on their first n_j dims and q = gain * u, so every score is the
    exact number gain * n_j / sqrt(128) and the scores differ by design (up to 181 nats): the softmax is known in fp64
    and, with the census V, every output element is a sum of non-negative weights checked to a relative bound -- what
    the census (all weights equal) and the needle (a single weight) cannot weigh: the rescale of l and O by factors
    strictly between 0 and 1 as the running maximum moves, the weights of the wave and key-split merges;
  * integer GEMM operands whose every partial sum stays below 2^24 (fp32 accumulation exact in any order), with planted
    bf16 rounding ties, and a RoPE table of quarter turns (every rotated value is +- an input integer).
"""
from __future__ import annotations

import math

import torch

BF16 = torch.bfloat16
DH = 128
CENSUS_TOL = 0.25  # |out * n - count|: bf16 rounding of count / n moves it by < 0.04 (T <= 1152), one key by >= 0.5
MASK_ZEROS = (31, 32, 63, 64, 127, 128)  # key-mask bytes forced to 0 (and slot - 1) ...
MASK_ONES = (0, 33, 65, 129)             # ... and to 1: the edges of 32 / 64 / 128-key chunks


# ----------------------------------------------------------------------------------
# attention: validity rule, census, needle
# ----------------------------------------------------------------------------------
def valid_keys(b: int, t: int, slot0: int, s: int, kv_start: torch.Tensor, key_mask=None) -> torch.Tensor:
    """bool [b, s, t]: query s of row b (cache slot slot0 + s) attends key j iff kv_start[b] <= j <= slot0 + s and
    key_mask[b, j] -- the rule of ``ref.attention``, written out on its own."""
    j = torch.arange(t)[None, None, :]
    qi = (slot0 + torch.arange(s))[None, :, None]
    ok = (j <= qi) & (j >= kv_start.long().reshape(b, 1, 1))
    if key_mask is not None:
        ok = ok & (key_mask[:, None, :t] != 0)
    return ok


def edge_mask(b: int, t: int, slot: int, seed: int = 0, density: float = 0.7) -> torch.Tensor:
    """uint8 [b, t] key mask: random at ``density``, the key at ``slot`` kept, and the bytes at chunk edges forced."""
    g = torch.Generator().manual_seed(seed)
    mask = (torch.rand(b, t, generator=g) < density).to(torch.uint8)
    for j in MASK_ZEROS + (slot - 1,):
        if 0 <= j < t:
            mask[:, j] = 0
    for j in MASK_ONES:
        if j < t:
            mask[:, j] = 1
    mask[:, slot] = 1
    return mask


def census_v(b: int, hkv: int, t: int, device="cpu") -> torch.Tensor:
    """bf16 [b, hkv, t, 128]: V[b, kvh, j] is the unit vector of class (j + 7 kvh + 3 b) % 128, for EVERY j of the
    cache (also past the query's slot and before kv_start: a wrongly admitted key is counted)."""
    return (_census_class(b, hkv, t).to(device)[..., None] == torch.arange(DH, device=device)).to(BF16)


def _census_class(b: int, hkv: int, t: int) -> torch.Tensor:
    j = torch.arange(t)[None, None, :]
    kvh = torch.arange(hkv)[None, :, None]
    row = torch.arange(b)[:, None, None]
    return (j + 7 * kvh + 3 * row) % DH


def census_counts(b: int, hkv: int, t: int, slot0: int, s: int, kv_start: torch.Tensor, key_mask=None):
    """(count int64 [b, s, hkv, 128], n int64 [b, s]): the valid keys of every class, and of all classes."""
    ok = valid_keys(b, t, slot0, s, kv_start, key_mask)
    cls = _census_class(b, hkv, t)[:, None].expand(b, s, hkv, t)
    count = torch.zeros(b, s, hkv, DH, dtype=torch.long)
    count.scatter_add_(-1, cls, ok[:, :, None, :].expand(b, s, hkv, t).long())
    n = ok.sum(-1)
    assert int(count.sum(-1).sub(n[:, :, None]).abs().max()) == 0
    return count, n


def census_mismatch(out: torch.Tensor, count: torch.Tensor, n: torch.Tensor, rep: int):
    """None if ``out`` ([b * s, hkv * rep * 128], the kernel's layout) is the census within CENSUS_TOL per element and
    exactly 0 on rows without a valid key; else a message naming the first bad (b, s, h) and, per non-zero column of
    ``round(out * n) - count``, the key class (index mod 128, shifted by 7 kvh + 3 b) that is off."""
    b, s, hkv, _ = count.shape
    o = out.detach().double().cpu().reshape(b, s, hkv, rep, DH)
    nn = n.double()[:, :, None, None, None]
    err = o * nn - count.double()[:, :, :, None, :]
    bad = ~(err.abs() <= CENSUS_TOL)  # (a NaN is bad)
    bad |= (nn == 0) & (o != 0)
    if not bad.any():
        return None
    bi, si, gi, ri = [int(v) for v in bad.any(-1).nonzero()[0]]
    diff = (o[bi, si, gi, ri] * float(n[bi, si])).round() - count[bi, si, gi].double()
    cols = {int(d): float(diff[d]) for d in diff.nonzero().flatten()[:16]} if torch.isfinite(diff).all() else "non-finite"
    keys = ({(d - 7 * gi - 3 * bi) % DH: v for d, v in cols.items()} if isinstance(cols, dict) else cols)
    return (f"{int(bad.sum())} bad elements; first at b={bi} s={si} h={gi * rep + ri} (n={int(n[bi, si])}, "
            f"max |out*n - count| there {float(err[bi, si, gi, ri].abs().max()):.3f}): "
            f"round(out*n) - count by key index mod 128 = {keys}")


def needle_candidates(ok_row):
    """The needle positions of one query (``ok_row``: t bools): the first two and last two keys of [first valid, last
    valid] and every multiple of 32 (so also of 128) with its two neighbours in between -- those that are valid."""
    ok_row = ok_row.tolist() if torch.is_tensor(ok_row) else ok_row
    if True not in ok_row:
        return []
    lo = ok_row.index(True)
    hi = len(ok_row) - 1 - ok_row[::-1].index(True)
    cand = [lo, lo + 1, hi, hi - 1]
    for m in range(lo // 32 * 32, hi + 2, 32):
        cand += [m - 1, m, m + 1]
    out = []
    for j in cand:
        if lo <= j <= hi and ok_row[j] and j not in out:
            out.append(j)
    return out


def needle_inputs(b: int, hkv: int, rep: int, t: int, slot0: int, s: int, kv_start: torch.Tensor, key_mask=None,
                  seed: int = 0):
    """(q [b, s, h, 128], kc, vc [b, hkv, t, 128] bf16, jstar int64 [b, s, h], want [b * s, h * 128] bf16).
    K is random +-1, V random; q[b, s, h] = 32 * K[b, h // rep, jstar]; jstar cycles over ``needle_candidates`` with a
    stride per head, so the heads of one kv group pick different keys where there are enough. ``want`` is
    V[b, h // rep, jstar] (0 where the query has no valid key: jstar = -1, q = 0)."""
    g = torch.Generator().manual_seed(seed)
    h = hkv * rep
    kc = (torch.randint(0, 2, (b, hkv, t, DH), generator=g) * 2 - 1).to(BF16)
    vc = torch.randn(b, hkv, t, DH, generator=g).to(BF16)
    ok = valid_keys(b, t, slot0, s, kv_start, key_mask)
    jstar = torch.full((b, s, h), -1, dtype=torch.long)
    for bi in range(b):
        rows = ok[bi].tolist()
        for si in range(s):
            cand = needle_candidates(rows[si])
            if not cand:
                continue
            stride = max(1, len(cand) // h)
            for hh in range(h):
                jstar[bi, si, hh] = cand[(hh * stride + 3 * si + bi) % len(cand)]
    found = jstar >= 0
    jj = jstar.clamp_min(0)
    bb = torch.arange(b)[:, None, None].expand(b, s, h)
    gg = (torch.arange(h) // rep)[None, None, :].expand(b, s, h)
    q = (32.0 * kc[bb, gg, jj].float() * found[..., None]).to(BF16)
    want = (vc[bb, gg, jj].float() * found[..., None]).to(BF16).reshape(b * s, h * DH)
    return q, kc, vc, jstar, want


def needle_max_cross(kc: torch.Tensor) -> int:
    """max over (b, kvh) and i != j of |k_i . k_j| (integers)."""
    k = kc.float()
    g = k @ k.transpose(-1, -2)
    eye = torch.eye(g.shape[-1], dtype=torch.bool)
    return int(g.masked_fill(eye, 0).abs().max())


# fp32 exp(-x) is exactly 0 from x = 104 on (2^-150 rounds to 0). A needle score leads every other by
# 32 * (128 - cross) / sqrt(128); cross <= 72 keeps that lead >= 158, half as much again as the underflow needs.
NEEDLE_MAX_CROSS = 72


def needle_gap(cross: int) -> float:
    return 32.0 * (DH - cross) / math.sqrt(DH)


# ----------------------------------------------------------------------------------
# attention ladder: exact scores that differ by design
# ----------------------------------------------------------------------------------
GAINS = (8.0, -8.0, 1.0, -1.0, 16.0, -16.0, 0.25, -2.0)  # powers of two: q = gain * u is exact in bf16
LADDER_PROFILES = ("ramp", "steps", "saw", "high")
U_BF16 = 2.0 ** -8  # bf16's unit roundoff
# Per element |out - want| <= rtol * want + LADDER_FLOOR. Every term of the output sum is non-negative, so a relative
# error per term is at most that relative error of the sum:
#   fp32-FMA kernels (fp32 P):  the bf16 rounding of the output (u) + the fp32 work (score x scale at arguments up to
#                               about 260 log2 units, exp, sums of up to 8192 terms, merges: under 1e-4, so 2^-12);
#   MFMA kernels (bf16 P):      one more u for P rounded to bf16 (the row sum l stays fp32).
# The floor is for weights below 2^-126 of the maximum, which fp32 and bf16 may flush; nothing else fits under it.
LADDER_RTOL_FMA = U_BF16 + 2.0 ** -12
LADDER_RTOL_MMA = 2 * U_BF16 + 2.0 ** -12
LADDER_FLOOR = 1e-30
# the shapes the GPU tests run the ladder at (tests/test_exact_gpu.py, tests/test_kv8_gpu.py, test_kv8_split_gpu.py);
# tests/test_exact_inputs_cpu.py validates the family at every one of them
LADDER_DECODE_TS = ((40, 17), (384, 256), (1030, 1029))
LADDER_V4 = (40, 520, 260)  # b, t, slot of the register-ring stream
LADDER_PREFILL_SHAPES = ((97, 100, False), (130, 10, False), (512, 0, False), (300, 0, True))  # s, slot0, masked
LADDER_FUSED_TS = ((200, 199), (512, 130))
LADDER_KV8_SPLIT_TS = ((40, 17), (300, 299), (1030, 700), (8192, 8000))


def ladder_levels(profile: str, t: int) -> torch.Tensor:
    """int64 [t] in 0..128: the level n_j of key j (the number of leading dims on which the key equals u).
      ramp   j * 128 // (t - 1): the maximum grows in every tile / chunk / split for a positive gain (the newest key
             dominates); for a negative gain the first valid key is a sink and every later split has m far below M;
      steps  8 * ((j // 32) % 17): constant over 32 keys, +8 levels per step, then a drop of 128. At gain 8 a step's
             maximum exceeds the last by 8.16 log2 units (just over the lazy-rescale threshold of 8); at gains -2, 1
             and 0.25 it stays under it for several steps, so p > 1 drifts up to 2^8 before a rescale;
      saw    (37 * j) % 129: large jumps both ways inside a tile;
      high   120 + (5 * j) % 9: with gain +-16 every score sits in +-(170 .. 181) nats."""
    j = torch.arange(t)
    if profile == "ramp":
        return j * 128 // max(t - 1, 1)
    if profile == "steps":
        return 8 * ((j // 32) % 17)
    if profile == "saw":
        return (37 * j) % 129
    if profile == "high":
        return 120 + (5 * j) % 9
    raise ValueError(profile)


def ladder_inputs(b: int, hkv: int, rep: int, t: int, s: int, profile: str, seed: int = 0):
    """(q bf16 [b, s, h, 128], K bf16 [b, hkv, t, 128], levels int64 [t], gain fp64 [b, s, h]).
    u[b, kvh] is a seeded +-1 vector; K[b, kvh, j] = u on dims < levels[j] and 0 elsewhere (entries 0 / +-1: exact in
    bf16 and, at any row scale, in e4m3); q[b, s, h] = gain * u[b, h // rep] with gain = GAINS[(b + s + h + h // rep)
    % 8], so both signs, sharp and flat, meet in the heads of one kv group and in neighbouring queries. q . k =
    gain * levels[j] exactly in fp32, in any summation order; the score is that over sqrt(128). V is ``census_v``."""
    g = torch.Generator().manual_seed(seed)
    h = hkv * rep
    u = (torch.randint(0, 2, (b, hkv, DH), generator=g) * 2 - 1).double()
    levels = ladder_levels(profile, t)
    assert int(levels.min()) >= 0 and int(levels.max()) <= DH
    on = torch.arange(DH)[None, :] < levels[:, None]  # [t, 128]
    kc = (u[:, :, None, :] * on[None, None]).to(BF16)
    hh = torch.arange(h)
    idx = (torch.arange(b)[:, None, None] + torch.arange(s)[None, :, None] + (hh + hh // rep)[None, None, :]) % len(GAINS)
    gain = torch.tensor(GAINS, dtype=torch.float64)[idx]
    q = (gain[..., None] * u[:, hh // rep][:, None]).to(BF16)
    return q, kc, levels, gain


def ladder_scores(levels: torch.Tensor, gain: torch.Tensor) -> torch.Tensor:
    """fp64 [b, s, h, t]: gain * levels / sqrt(128) in natural units (the product is exact)."""
    return gain[..., None] * levels.double() / math.sqrt(DH)


def ladder_expected(b: int, hkv: int, rep: int, t: int, slot0: int, s: int, kv_start: torch.Tensor, key_mask,
                    levels: torch.Tensor, gain: torch.Tensor) -> torch.Tensor:
    """fp64 [b, s, h, 128]: want[b, s, h, cls] = sum of the softmax weights of the valid keys of class cls (the class
    of ``census_v``), the softmax taken in fp64 over the valid keys of ``valid_keys``; 0 for a query without one."""
    h = hkv * rep
    ok = valid_keys(b, t, slot0, s, kv_start, key_mask)[:, :, None, :]  # [b, s, 1, t]
    sc = ladder_scores(levels, gain).masked_fill(~ok, float("-inf"))
    mx = sc.amax(-1, keepdim=True)
    w = torch.exp(sc - torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx)))  # (exp(-inf) = 0 on invalid keys)
    den = w.sum(-1, keepdim=True)
    w = torch.where(den > 0, w / den.clamp_min(1e-300), torch.zeros_like(w))
    cls = _census_class(b, hkv, t).repeat_interleave(rep, dim=1)[:, None].expand(b, s, h, t)
    return torch.zeros(b, s, h, DH, dtype=torch.float64).scatter_add_(-1, cls, w)


def ladder_excess(out: torch.Tensor, want: torch.Tensor, rtol: float) -> torch.Tensor:
    """fp64 [b, s, h, 128]: |out - want| / (rtol * want + LADDER_FLOOR); inf where it is not a number, or where a
    query without a valid key is not exactly 0. ``out``: the kernel's [b * s, h * 128] (or [b, s, h * 128])."""
    o = out.detach().double().cpu().reshape(want.shape)
    ex = (o - want).abs() / (rtol * want + LADDER_FLOOR)
    ex = torch.where(torch.isnan(ex), torch.full_like(ex, float("inf")), ex)
    empty = (want.sum(-1, keepdim=True) == 0) & (o != 0)
    return torch.where(empty, torch.full_like(ex, float("inf")), ex)


def ladder_worst_u(out: torch.Tensor, want: torch.Tensor) -> float:
    """The largest relative error beyond the floor, (|out - want| - LADDER_FLOOR) / want, in units of u (to report)."""
    o = out.detach().double().cpu().reshape(want.shape)
    rel = ((o - want).abs() - LADDER_FLOOR).clamp_min(0)[want > 0] / want[want > 0]
    return float(rel.max()) / U_BF16 if rel.numel() else 0.0


def ladder_mismatch(out: torch.Tensor, want: torch.Tensor, rep: int, rtol: float):
    """None if every element has |out - want| <= rtol * want + LADDER_FLOOR and the queries without a valid key are
    exactly 0; else a message naming the first bad (b, s, h, class), observed and expected there and their ratio -- a
    power of two or e^k points at a rescale that was skipped or applied in the wrong unit."""
    ex = ladder_excess(out, want, rtol)
    bad = ~(ex <= 1.0)
    if not bad.any():
        return None
    o = out.detach().double().cpu().reshape(want.shape)
    bi, si, hi, ci = [int(v) for v in bad.nonzero()[0]]
    got, exp = float(o[bi, si, hi, ci]), float(want[bi, si, hi, ci])
    ratio = got / exp if exp != 0 else float("inf" if got != 0 else "nan")
    logs = (f" (2^{math.log2(ratio):.3f}, e^{math.log(ratio):.3f})" if 0 < ratio < float("inf") else "")
    return (f"{int(bad.sum())} bad elements, worst |err| / bound {float(ex.max()):.3g}; first at b={bi} s={si} h={hi} "
            f"(kv head {hi // rep}) class={ci}: observed {got!r}, expected {exp!r}, ratio {ratio:.6g}{logs}")


# ----------------------------------------------------------------------------------
# integer GEMM operands
# ----------------------------------------------------------------------------------
def int_matrix(rows: int, cols: int, amp: int, seed: int) -> torch.Tensor:
    """int64 [rows, cols], uniform in {-amp .. amp} with every second entry (at random) zeroed."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-amp, amp + 1, (rows, cols), generator=g)
    return v * torch.randint(0, 2, (rows, cols), generator=g)


def int_gemm_inputs(m: int, n: int, k: int, seed: int = 0, amp: int = 2, plant: bool = True):
    """(x int64 [m, k], w int64 [n, k], y int64 [m, n] = x @ w^T). K * amp^2 <= 16384 < 2^24: every partial sum of
    any summation order is an exact fp32 integer. With ``plant`` (amp 2, k >= 66, n >= 4) the last row of x and the
    first four rows of w are set so that y[m - 1, 0:4] = 257, 259, -257, -259: exact bf16 ties (spacing 2 above 256)
    whose round-to-nearest-even results are 256, 260, -256, -260 and whose truncations are 256, 258, ..."""
    assert k * amp * amp <= 16384
    x = int_matrix(m, k, amp, seed * 2 + 1)
    w = int_matrix(n, k, amp, seed * 2 + 2)
    if plant:
        assert amp == 2 and k >= 66 and n >= 4
        x[m - 1, :] = 2
        x[m - 1, 0] = 1
        w[:4, :] = 0
        w[:4, 0] = 1
        w[:4, 1:65] = 2       # 1 + 64 * 4 = 257
        w[1, 65] = w[3, 65] = 1  # + 2 = 259
        w[2:4] = -w[2:4]
    y = x @ w.t()
    return x, w, y


def bf16_ties(y: torch.Tensor) -> torch.Tensor:
    """bool: integers that lie exactly between two bf16 values (8 significant bits): |y| in (2^e, 2^(e+1)), e >= 8,
    with y mod 2^(e-7) == 2^(e-8)."""
    a = y.abs().long()
    e = torch.floor(torch.log2(a.clamp_min(1).double())).long()
    half = torch.where(e >= 8, 2 ** (e - 8).clamp_min(0), torch.zeros_like(a))
    return (e >= 8) & (a % (2 * half).clamp_min(1) == half)


def int_residual(m: int, n: int, seed: int) -> torch.Tensor:
    """int64 [m, n] in [-1000, 1000]."""
    return torch.randint(-1000, 1001, (m, n), generator=torch.Generator().manual_seed(seed))


def swiglu_exact(g: torch.Tensor, u: torch.Tensor):
    """(want bf16, tol fp32) of silu(g) * u for exact integer g, u: computed in fp64 and rounded once. A result may
    differ by one bf16 ulp of ``want`` (2^-7 |want| bounds it) where the fp32 sigmoid lands on the other side of a
    rounding boundary, never more; an exactly representable 0 stays 0. The absolute term 2^-126 |g u| is for g below
    about -87, where sigmoid(g) is under the smallest normal fp32 number and an fp32 kernel may return 0 for it
    (exp(-g) overflows): that moves the product by less than 2^-126 |g u|, some 1e-35 against outputs of order 1."""
    gd, ud = g.double(), u.double()
    want = (gd * torch.sigmoid(gd) * ud).float().to(BF16)
    return want, want.float().abs() * 2.0 ** -7 + (gd * ud).abs().float() * 2.0 ** -126


# ----------------------------------------------------------------------------------
# RoPE by quarter turns
# ----------------------------------------------------------------------------------
def quarter_turns(npos: int, pairs: int = DH // 2) -> torch.Tensor:
    """int64 [npos, pairs] in 0..3: a hash of (position, pair) that is not a sum of a position and a pair term."""
    p = torch.arange(npos)[:, None]
    i = torch.arange(pairs)[None, :]
    m32 = (1 << 32) - 1
    v = (p * pairs + i + 1) * 2654435761 & m32  # (a 32-bit multiply-xorshift hash: any two positions of a 1024-row
    v = (v ^ (v >> 15)) * 2246822519 & m32      #  table differ in 30 or more of the 64 pairs, any two pairs likewise)
    return ((v ^ (v >> 13)) % 4).long()


def quarter_table(npos: int, pairs: int = DH // 2) -> torch.Tensor:
    """fp32 [npos, pairs, 2] (cos, sin) of ``quarter_turns``: (1, 0), (0, 1), (-1, 0), (0, -1)."""
    qt = quarter_turns(npos, pairs)
    cos = torch.tensor([1, 0, -1, 0])[qt]
    sin = torch.tensor([0, 1, 0, -1])[qt]
    return torch.stack([cos, sin], -1).float().contiguous()


def rotate_int(x: torch.Tensor, positions: torch.Tensor, npos: int) -> torch.Tensor:
    """Interleaved-pair RoPE of integer x [M, nh, 128] by the quarter-turn table, in int64."""
    qt = quarter_turns(npos, x.shape[-1] // 2)[positions.long().clamp(0, npos - 1)]  # [M, pairs]
    c = torch.tensor([1, 0, -1, 0])[qt][:, None, :]
    s = torch.tensor([0, 1, 0, -1])[qt][:, None, :]
    xp = x.reshape(*x.shape[:-1], -1, 2)
    xr, xi = xp[..., 0], xp[..., 1]
    return torch.stack([xr * c - xi * s, xr * s + xi * c], -1).reshape(x.shape)


def qkv_rope_exact(y, positions, npos: int, b: int, s: int, h: int, hkv: int, t: int, slot0: int, scale=None):
    """Exact outputs of the fused qkv epilogue for integer (or exactly scaled) projections y [b * s, (h + 2 hkv) * 128]:
    (q bf16 [M, h, 128], K cache, V cache bf16 [b, hkv, t, 128] with every untouched slot 0). ``scale``: an exact
    per-row power of two (fp64 [M]) applied before the one bf16 rounding."""
    m = b * s
    hq, hk = h * DH, hkv * DH
    q = rotate_int(y[:, :hq].reshape(m, h, DH), positions, npos).double()
    k = rotate_int(y[:, hq:hq + hk].reshape(m, hkv, DH), positions, npos).double()
    v = y[:, hq + hk:].reshape(m, hkv, DH).double()
    if scale is not None:
        q, k, v = [a * scale.double()[:, None, None] for a in (q, k, v)]
    kc = torch.zeros(b, hkv, t, DH, dtype=BF16)
    vc = torch.zeros_like(kc)
    kc[:, :, slot0:slot0 + s] = k.float().to(BF16).reshape(b, s, hkv, DH).permute(0, 2, 1, 3)
    vc[:, :, slot0:slot0 + s] = v.float().to(BF16).reshape(b, s, hkv, DH).permute(0, 2, 1, 3)
    return q.float().to(BF16), kc, vc


def pow2_rows(m: int, k: int, seed: int):
    """(x int64 [m, k], scale fp64 [m]): row r holds +-2^(r % 3) and no zero, so mean(x^2) is 1, 4 or 16 and
    rsqrt(mean + 0) is exactly 1, 1/2 or 1/4 -- another power of two per row."""
    g = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, (m, k), generator=g) * 2 - 1
    e = torch.arange(m) % 3
    return sign * (2 ** e)[:, None], 0.5 ** e.double()
