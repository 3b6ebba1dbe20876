// The two merges of the decode-attention kernels whose workgroups hold several waves (attn_decode.hip v3 / v5, kv8.hip
// attn_decode_q8_kernel), once: the waves of a workgroup through LDS, and the key splits of a (row, kv head) pair
// through the workspace. Everything is a running (m, l, o) per query head -- the maximum score, the sum of exp(s - m)
// and the unnormalised P.V -- merged by log-sum-exp; the kernels differ only in the units of m (ExpNat / ExpLog2).
//
// The waves: a lane holds 8 dims (8 li ..) of the keys of its lane group g; wave_sum_groups() adds the 4 groups (they
// share the wave's m), wave_put() writes the wave's (m, l, o[128]) to LDS from the g == 0 lanes, and behind one
// __syncthreads() waves_combine1 / waves_combine4 give a thread the workgroup's (M, den, num) of one head and 1 / 4
// dims. The kernel normalises and writes.
//
// The key splits (Guideline 16 of cdna_hip_programming.md, R1 form with a counter): the workgroups of a pair are the
// splits that hold keys, n_act of them, every one of which computes the same n_act from device state.
//   * split_part_store: a split stores its partial, [m, l, 0, 0, o[128]] per head (ATTN_PART_FLOATS floats, attn_plan.h
//     sizes the workspace with the same constant), with write-through (sc1) 16-B buffer stores: the bytes go to
//     agent-coherent memory, not to a cache only this CU or XCD reads, so there is nothing for a release fence to flush.
//   * split_arrive: every storing wave drains its stores (s_waitcnt vmcnt(0): a write-through store counts as done when
//     it is visible to the agent) BEFORE the workgroup's barrier -- a store still in flight in another wave would not be
//     ordered before thread 0's add by the barrier alone. Then thread 0 adds 1 to the pair's ticket, relaxed, agent
//     scope. Relaxed suffices: the payload was made visible by the drained write-through stores and is read with sc1
//     loads, which bypass the reader's L1 (no stale line to invalidate, so no acquire either); the add only has to be
//     one atomic total order of arrivals, and the barrier that follows it orders the merging workgroup's loads behind
//     it. The workgroup that draws n_act - 1 is the last: every other split's partial is complete. It stores 0 to the
//     ticket -- nobody else touches that ticket again in this launch (all n_act adds have happened), and the next launch
//     on the stream starts after this one ends -- so a ticket zeroed once at allocation serves every call and every
//     graph replay. An LDS flag tells the other waves; the function returns "this workgroup merges".
//   * split_merge: the last arriver folds the partials of splits [s_begin, s_end) in split order (the same bits whoever
//     arrives last) with sc1 loads, FOLD splits' loads in flight per round; a load past the end re-reads the last split
//     and is never folded. It returns (M, den, num) like a wave combine; den = 0 for a row with no valid key.
// No float atomics, nothing waits on another workgroup.
//
// Not served here, on purpose: v2's merge (attn_decode.hip) -- one WAVE is the arriver, its partial is [m, l, o[128]]
// (130 floats) written with scalar write-through stores, and the ticket is per wave, so sharing would change its
// workspace indexing and its code -- and the fused qkv + attention launch (gemv.hip) -- 8 dims per thread, asm loads
// into pinned registers that tools/check_asm_ring.py checks, and the flag in its dynamic LDS.
#pragma once

#include "attn_plan.h"
#include "common.h"

namespace jla {

// The numeric flavour of a kernel's merges, a policy type because the results must not move by a bit. w / wf: the weight
// exp(m - M) of a part with maximum m in a merge with maximum M >= m; for w, m may be -inf (a part without a valid key),
// for wf it is known to be finite. fold_in_place: which of the two spellings of split_merge's fold step the kernel was
// written with (see there).
struct ExpNat {  // v3 / v5: natural-log units, the -inf guards written out
  static constexpr bool fold_in_place = false;
  static JLA_DEV float w(float m, float M) { return m == -INFINITY ? 0.f : __expf(m - M); }
  static JLA_DEV float wf(float m, float M) { return __expf(m - M); }
};
struct ExpLog2 {  // the fp8 kernel: log2 units, v_exp_f32 directly (exp2(-inf) = 0, and M is finite wherever it runs)
  static constexpr bool fold_in_place = true;
  static JLA_DEV float w(float m, float M) { return __builtin_amdgcn_exp2f(m - M); }
  static JLA_DEV float wf(float m, float M) { return __builtin_amdgcn_exp2f(m - M); }
};

// ---- the waves of a workgroup
// l and o summed over the 4 lane groups (lanes li, li + 16, li + 32, li + 48), in every lane. o: the lane's 8 dims in
// either shape the kernels keep them, float[8] or f32x2_t[4]. They are read in place, not through a helper that
// returns the element: __shfl_xor takes its argument as maybe_undef (a freeze at the call), a by-value parameter or
// return is noundef and drops that freeze, and the kernels' main loops then compile to other code (one chunk of loads
// in flight instead of two in the fp8 kernel).
template <class O>
JLA_DEV void wave_sum_groups(float& l, const O& o, float (&of)[8]) {
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float v;
    if constexpr (sizeof(o[0]) == sizeof(float))
      v = o[e];
    else
      v = o[e >> 1][e & 1];
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    of[e] = v;
  }
}

template <int W, int REP>
JLA_DEV void wave_put(float (&sm_m)[W][REP], float (&sm_l)[W][REP], float (&sm_o)[W][REP][ATTN_DH], int w, int h, int g,
                      int li, float m, float l, const float (&of)[8]) {
  if (g == 0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) sm_o[w][h][8 * li + e] = of[e];
    if (li == 0) {
      sm_m[w][h] = m;
      sm_l[w][h] = l;
    }
  }
}

struct Merged1 {
  float M, den, num;
};
struct Merged4 {
  float M, den, num[4];
};

// head h, dim d
template <class EXP, int W, int REP>
JLA_DEV Merged1 waves_combine1(const float (&sm_m)[W][REP], const float (&sm_l)[W][REP],
                               const float (&sm_o)[W][REP][ATTN_DH], int h, int d) {
  Merged1 c{-INFINITY, 0.f, 0.f};
#pragma unroll
  for (int ww = 0; ww < W; ++ww) c.M = fmaxf(c.M, sm_m[ww][h]);
  if (c.M != -INFINITY) {
#pragma unroll
    for (int ww = 0; ww < W; ++ww) {
      const float mw = sm_m[ww][h];
      const float f = EXP::w(mw, c.M);
      c.num += f * sm_o[ww][h][d];
      c.den += f * sm_l[ww][h];
    }
  }
  return c;
}

// head h, dims [d, d + 4)
template <class EXP, int W, int REP>
JLA_DEV Merged4 waves_combine4(const float (&sm_m)[W][REP], const float (&sm_l)[W][REP],
                               const float (&sm_o)[W][REP][ATTN_DH], int h, int d) {
  float M = -INFINITY;
#pragma unroll
  for (int ww = 0; ww < W; ++ww) M = fmaxf(M, sm_m[ww][h]);
  float num[4] = {0.f, 0.f, 0.f, 0.f}, den = 0.f;
  if (M != -INFINITY) {
#pragma unroll
    for (int ww = 0; ww < W; ++ww) {
      const float mw = sm_m[ww][h];
      const float f = EXP::w(mw, M);
      den += f * sm_l[ww][h];
#pragma unroll
      for (int e = 0; e < 4; ++e) num[e] += f * sm_o[ww][h][d + e];
    }
  }
  // (sums kept in locals, not in the struct's members: the compiler then contracts the same multiply-adds as before)
  return Merged4{M, den, {num[0], num[1], num[2], num[3]}};
}

// ---- the key splits of a pair
// the pair's nsplit partials of REP heads each, as a buffer resource (offsets in bytes, out-of-range reads give 0)
template <int REP>
JLA_DEV __amdgpu_buffer_rsrc_t split_parts_rsrc(float* ws, size_t pair, int nsplit) {
  constexpr int PS = REP * ATTN_PART_FLOATS;
  return __builtin_amdgcn_make_buffer_rsrc(ws + pair * nsplit * PS, 0, nsplit * PS * 4, 0x00020000);
}

template <int REP>
JLA_DEV void split_part_store(__amdgpu_buffer_rsrc_t rs, int split, int h, int d, const Merged4& c) {
  constexpr int HS = ATTN_PART_FLOATS, PS = REP * HS;
  const int off = (split * PS + h * HS) * 4;
  __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(c.num[0]), __float_as_uint(c.num[1]),
                                               __float_as_uint(c.num[2]), __float_as_uint(c.num[3])},
                                         rs, off + (4 + d) * 4, 0, 16);
  if (d == 0)
    __builtin_amdgcn_raw_buffer_store_b128(u32x4{__float_as_uint(c.M), __float_as_uint(c.den), 0u, 0u}, rs, off, 0, 16);
}

// Called by the whole workgroup behind its split_part_store()s. flag: an LDS word (int or float) nothing else uses from
// the barrier inside on.
template <class F>
JLA_DEV bool split_arrive(int32_t* tickets, size_t pair, int n_act, F& flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t* tk = tickets + pair;
    const int prev = __hip_atomic_fetch_add(tk, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = prev == n_act - 1;
    if (last) __hip_atomic_store(tk, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // reset for the next call
    flag = last ? F(1) : F(0);
  }
  __syncthreads();
  return flag != F(0);
}

// The partials of splits [s_begin, s_end) folded in split order: (M, den, num) of head h, dims [d, d + 4), unnormalised
// (den = 0 where no split held a valid key); the kernel divides and writes, as after a wave combine.
// The fold step is spelled twice, and EXP::fold_in_place picks: v5 wrote it as a lambda that takes the two loaded
// vectors by value, the fp8 kernel in the loop body on ml[u] / ov[u]. It is the same arithmetic, but the compiler
// contracts a different subset of its multiply-adds into fmas for the two (at FOLD 4: all of them for the lambda, all
// but the second split's for the in-place form), which is other bits in the last place of the fp32 sums. Each kernel
// keeps its spelling until a change that may move its bits picks one.
template <class EXP, int FOLD, int REP>
JLA_DEV Merged4 split_merge(__amdgpu_buffer_rsrc_t rs, int s_begin, int s_end, int h, int d) {
  constexpr int HS = ATTN_PART_FLOATS, PS = REP * HS;
  float Mr = -INFINITY, Lr = 0.f, Or[4] = {0.f, 0.f, 0.f, 0.f};
  auto fold = [&](const u32x4 ml, const u32x4 ov) {
    const float ms = __uint_as_float(ml[0]);
    if (ms == -INFINITY) return;  // (a split whose keys are all masked)
    const float mn = fmaxf(Mr, ms);
    const float a = EXP::w(Mr, mn), f = EXP::wf(ms, mn);
    Lr = Lr * a + f * __uint_as_float(ml[1]);
#pragma unroll
    for (int e = 0; e < 4; ++e) Or[e] = Or[e] * a + f * __uint_as_float(ov[e]);
    Mr = mn;
  };
  // all loads of a round in flight together: one dependent L2 round trip per FOLD splits
  for (int s = s_begin; s < s_end; s += FOLD) {
    u32x4 ml[FOLD], ov[FOLD];
#pragma unroll
    for (int u = 0; u < FOLD; ++u) {
      const int off = (min(s + u, s_end - 1) * PS + h * HS) * 4;
      ml[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 16);
      ov[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, off + (4 + d) * 4, 0, 16);
    }
#pragma unroll
    for (int u = 0; u < FOLD; ++u) {
      if constexpr (EXP::fold_in_place) {
        const float ms = __uint_as_float(ml[u][0]);
        if (s + u >= s_end || ms == -INFINITY) continue;  // (past the end; a split whose keys are all masked)
        const float mn = fmaxf(Mr, ms);
        const float a = EXP::w(Mr, mn), f = EXP::wf(ms, mn);
        Lr = Lr * a + f * __uint_as_float(ml[u][1]);
#pragma unroll
        for (int e = 0; e < 4; ++e) Or[e] = Or[e] * a + f * __uint_as_float(ov[u][e]);
        Mr = mn;
      } else {
        if (s + u < s_end) fold(ml[u], ov[u]);
      }
    }
  }
  return Merged4{Mr, Lr, {Or[0], Or[1], Or[2], Or[3]}};
}

}  // namespace jla
