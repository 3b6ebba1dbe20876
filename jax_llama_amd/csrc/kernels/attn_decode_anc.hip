// Decode attention through a beam-ancestry table (the README's "Beam search" section, ops/reference.py attention_anc):
// the cache never moves. Query row r = b K + j of a beam search reads key slot t from physical row b K + anc[r, t], anc
// uint8 [rows, T]; a value >= K is clamped to K - 1, so no row outside the prompt's group is ever addressed. Everything
// else -- the slot range [kv_start, slot] less the key mask, scale, softmax, GQA, zeros for a row with no valid key --
// is attn_decode's. bf16 cache, Dh = 128, rep 1 / 2 / 4 / 8, no packed copy.
//
// Work split: one 8-wave workgroup per (row, kv head) pair, or -- few pairs with a long context -- one per (pair, key
// split), the splits cutting the pair's valid keys by attn_q8_split_range() (attn_plan.h) as the fp8 kernel's do. A
// chunk is 32 KPG keys: lane group G = 4 w + g of the workgroup (16 lanes = one 256-B row, 8 dims per lane) owns the
// KPG CONSECUTIVE keys c0 + G KPG .. + KPG - 1. That is what the table wants: a group's KPG table bytes are one 2- / 4-
// / 8-byte load per lane and chunk (anc_load), not one per key. A gathered key's K and V rows have no neighbour to
// share a line with anyway -- the next key may live in another beam's row -- so nothing is lost against v3's
// interleaved rows, where one wave load covers 1 KiB of one row.
//
// The table bytes sit on the critical path of every K / V address, so they run one chunk ahead of the rows, which run
// one chunk ahead of the math: at the top of the step for chunk c the wave has chunk c's rows and chunk c + 1's bytes
// (both issued a step ago; the vector-memory counter retires in order, so the one wait covers both), issues chunk
// c + 1's rows from those bytes, then chunk c + 2's bytes, and scores chunk c under them. No address waits on a load
// issued in the same step. Byte r of the word is key r's beam: v_bfe_u32, v_min_u32 and one v_mad_u64_u32 by the row
// stride give the per-lane row base -- integer VALU only.
//
// Math: the fp8 kernel's VALU form on bf16 rows (v_dot2_f32_bf16 scores summed over the 16 lanes by DPP, base-2 online
// softmax per wave, packed fp32 fmas for P.V, no barrier in the loop). The matrix-core form (attn_mma.h) was the other
// candidate; attn_plan.h attn_decode_anc_plan says why this one. A key mask's bytes are fetched the same way as the
// table's (one word per lane group and chunk, with the chunk's rows), so a masked launch has no load-and-wait in its
// scoring either. Both merges -- the 8 waves through LDS, the key
// splits through the workspace with a last arriver -- are attn_merge.h's, in log2 units: no float atomics, nothing
// waits, the same bits on every call.
#include "attn_merge.h"
#include "common.h"
#include "launchers.h"

namespace jla {

constexpr int ANC_DH = ATTN_DH;
constexpr int ANC_WAVES = 8;

// The KPG table bytes of keys [j0, j0 + KPG) of one table row. The row is T >= 8 bytes at any alignment (T need not be
// a multiple of 4), so the load is an unaligned one, and it never passes the row's end: the group that holds the end
// reads the row's last KPG bytes. anc_load only issues the load; anc_word, called where the bytes are used (a step
// later, so the wait for them is the wait for the rows issued before them), shifts that group's word into place: byte r
// in bits [8 r, 8 r + 8), bytes of keys >= T come out 0 (those keys are never valid).
template <int KPG>
struct AncWord {
  typedef uint32_t type;
};
template <>
struct AncWord<8> {
  typedef uint64_t type;
};
template <int KPG>
JLA_DEV typename AncWord<KPG>::type anc_load(const uint8_t* __restrict__ row, int j0, int T) {
  typedef typename AncWord<KPG>::type W;
  const uint8_t* p = row + min(j0, T - KPG);
  if constexpr (KPG == 2) {
    uint16_t x;
    __builtin_memcpy(&x, p, 2);
    return x;
  } else {
    W v;
    __builtin_memcpy(&v, p, sizeof(W));
    return v;
  }
}
template <int KPG>
JLA_DEV typename AncWord<KPG>::type anc_word(typename AncWord<KPG>::type raw, int j0, int T) {
  typedef typename AncWord<KPG>::type W;
  const int sh = max(j0 - (T - KPG), 0);  // > 0 only in the group that holds the row's end
  return sh >= KPG ? W(0) : raw >> (8 * sh);
}

template <int REP, int KPG, bool SPLIT>
__global__ void __launch_bounds__(ANC_WAVES * 64)
    attn_decode_anc_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
                           const uint8_t* __restrict__ anc, int nbeams, const int32_t* __restrict__ slot_ptr,
                           const int32_t* __restrict__ kv_start, const uint8_t* __restrict__ key_mask, int mask_len,
                           bf16_t* __restrict__ out, float* __restrict__ ws, int32_t* __restrict__ tickets, int nsplit,
                           int H, int Hkv, int T, int t_cap, float scale) {
  typedef typename AncWord<KPG>::type W;
  constexpr int CH = ANC_WAVES * 4 * KPG;  // keys per chunk
  __shared__ float sm_m[ANC_WAVES][REP];
  __shared__ float sm_l[ANC_WAVES][REP];  // (SPLIT: sm_l[0][0] also carries "this workgroup merges")
  __shared__ float sm_o[ANC_WAVES][REP][ANC_DH];

  const int split = SPLIT ? blockIdx.x : 0;
  const int kvh = SPLIT ? blockIdx.y : blockIdx.x, b = SPLIT ? blockIdx.z : blockIdx.y;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int g = lane >> 4, li = lane & 15;
  const int slot = slot_ptr[0];
  if (slot >= T && threadIdx.x == 0) JLA_FLAG(JLA_BOUNDS_ATTN_T);  // keys past the cache are never read
  const int lo = max(kv_start[b], 0);
  int hi_key = min(min(slot + 1, t_cap), T);  // keys [lo, hi_key): the pair's valid keys, or this split's share
  int c_begin = lo - (lo % CH);
  int n_act = 1;
  if constexpr (SPLIT) {
    const AttnQ8SplitRange sr = attn_q8_split_range(lo, hi_key, CH, nsplit, split);
    n_act = sr.n_act;
    // a row with no valid key (n_act 0): split 0 alone goes on, streams nothing and writes 0
    if (split >= max(n_act, 1)) return;
    if (n_act > 0) c_begin = sr.c_begin, hi_key = sr.key_end;
  }
  const int h0 = kvh * REP;
  const uint8_t* mrow = key_mask ? key_mask + (size_t)b * mask_len : nullptr;
  const uint8_t* arow = anc + (size_t)b * T;
  // beam 0's row of this row's prompt, this kv head, this lane's 8 dims; beam a's row is a * row_stride further
  const size_t row_stride = (size_t)Hkv * T * ANC_DH;
  const size_t base = ((size_t)(b - b % nbeams) * Hkv + kvh) * T * ANC_DH + 8 * li;
  const bf16_t* kbase = kc + base;
  const bf16_t* vbase = vc + base;
  const uint32_t amax = (uint32_t)(nbeams - 1);
  const int k0 = (4 * w + g) * KPG;  // this lane group's first key within a chunk

  u32x4 qp[REP];  // this lane's 8 dims of each query head, packed bf16 (the v_dot2 operand)
#pragma unroll
  for (int h = 0; h < REP; ++h)
    qp[h] = *reinterpret_cast<const u32x4*>(q + ((size_t)b * H + h0 + h) * ANC_DH + 8 * li);
  float m_h[REP], l_h[REP];
  f32x2_t o[REP][4];  // dims 8 li + 2 i, 8 li + 2 i + 1
#pragma unroll
  for (int h = 0; h < REP; ++h) {
    m_h[h] = -INFINITY;
    l_h[h] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[h][i] = f32x2_t{0.f, 0.f};
  }
  // base-2 softmax: 1 / sqrt(Dh) and log2 e in one factor, v_exp_f32 directly
  const float scale2 = scale * 1.4426950408889634f;

  u32x4 kr[KPG], vr[KPG];
  W mr = 0;  // the key-mask bytes of the same keys: one more such word, loaded with the rows (mask_len >= 8)
  // the rows of the chunk at c0 through its table bytes (a key past hi_key re-reads slot hi_key - 1 of whichever row
  // its byte names: in range, masked)
  auto load_rows = [&](int c0, W raw) {
    const W tb = anc_word<KPG>(raw, c0 + k0, T);
#pragma unroll
    for (int r = 0; r < KPG; ++r) {
      const int j = min(c0 + k0 + r, hi_key - 1);  // (hi_key >= 1 wherever this runs)
      const uint32_t a = min((uint32_t)(tb >> (8 * r)) & 0xffu, amax);
      const size_t off = a * row_stride + (size_t)j * ANC_DH;
      kr[r] = *reinterpret_cast<const u32x4*>(kbase + off);
      vr[r] = *reinterpret_cast<const u32x4*>(vbase + off);
    }
    if (mrow) mr = anc_load<KPG>(mrow, c0 + k0, mask_len);
  };
  W tb = 0;
  if (lo < hi_key) {
    load_rows(c_begin, anc_load<KPG>(arow, c_begin + k0, T));
    if (c_begin + CH < hi_key) tb = anc_load<KPG>(arow, c_begin + CH + k0, T);
  }
  for (int c0 = c_begin; c0 < hi_key && lo < hi_key; c0 += CH) {
    u32x4 kcur[KPG], vcur[KPG];
#pragma unroll
    for (int r = 0; r < KPG; ++r) {
      kcur[r] = kr[r];
      vcur[r] = vr[r];
    }
    const W mcur = mr;
    if (c0 + CH < hi_key) {
      load_rows(c0 + CH, tb);  // next chunk's rows in flight while this one is scored ...
      if (c0 + 2 * CH < hi_key) tb = anc_load<KPG>(arow, c0 + 2 * CH + k0, T);  // ... and the bytes of the one after
    }
    float sc[REP][KPG];
    const W mw = mrow ? anc_word<KPG>(mcur, c0 + k0, mask_len) : ~W(0);  // (keys >= mask_len: byte 0, masked)
#pragma unroll
    for (int r = 0; r < KPG; ++r) {
      const int j = c0 + k0 + r;
      const bool valid = j >= lo && j < hi_key && ((uint32_t)(mw >> (8 * r)) & 0xffu) != 0;
#pragma unroll
      for (int h = 0; h < REP; ++h) {
        const float d = row16_sum(dot8_bf16(qp[h], kcur[r], 0.f));
        sc[h][r] = valid ? d * scale2 : -INFINITY;
      }
    }
    float mref[REP];  // the new running max, 0 while this wave has seen no valid key (every score then is -inf -> p = 0)
#pragma unroll
    for (int h = 0; h < REP; ++h) {
      float mx = sc[h][0];
#pragma unroll
      for (int r = 1; r < KPG; ++r) mx = fmaxf(mx, sc[h][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float mn = fmaxf(m_h[h], mx);
      mref[h] = mn == -INFINITY ? 0.f : mn;
      const float alpha = __builtin_amdgcn_exp2f(m_h[h] - mref[h]);  // m_h = -inf -> 0 (o and l are 0 then)
      m_h[h] = mn;
      l_h[h] *= alpha;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[h][i] *= alpha;
    }
#pragma unroll
    for (int r = 0; r < KPG; ++r) {
      float vf8[8];
      unpack8(vcur[r], vf8);
      const f32x2_t vf[4] = {{vf8[0], vf8[1]}, {vf8[2], vf8[3]}, {vf8[4], vf8[5]}, {vf8[6], vf8[7]}};
#pragma unroll
      for (int h = 0; h < REP; ++h) {
        const float p = __builtin_amdgcn_exp2f(sc[h][r] - mref[h]);  // a masked key: exp2(-inf) = 0
        l_h[h] += p;  // the 16 lanes of a group hold the same p (and the same running sum)
        const f32x2_t pp = {p, p};
#pragma unroll
        for (int i = 0; i < 4; ++i) o[h][i] = __builtin_elementwise_fma(pp, vf[i], o[h][i]);
      }
    }
  }
  // ---- per wave: sum the 4 groups (same max), then the waves through LDS (attn_merge.h)
  float of[REP][8];
#pragma unroll
  for (int h = 0; h < REP; ++h) {
    wave_sum_groups(l_h[h], o[h], of[h]);
    wave_put(sm_m, sm_l, sm_o, w, h, g, li, m_h[h], l_h[h], of[h]);
  }
  __syncthreads();
  if constexpr (SPLIT) {
    if (n_act > 1) {  // (workgroup-uniform; n_act <= 1 writes the output below, with no workspace traffic)
      const size_t pair = (size_t)b * Hkv + kvh;
      const __amdgpu_buffer_rsrc_t rs = split_parts_rsrc<REP>(ws, pair, nsplit);
      // ---- this split's unnormalised (m, l, o) per head: thread -> (head, 4 dims)
      for (int it = threadIdx.x; it < REP * 32; it += ANC_WAVES * 64) {
        const int h = it >> 5, d = 4 * (it & 31);
        split_part_store<REP>(rs, split, h, d, waves_combine4<ExpLog2>(sm_m, sm_l, sm_o, h, d));
      }
      // (the flag in sm_l[0][0]: every read of the wave partials is behind the barrier inside)
      if (!split_arrive(tickets, pair, n_act, sm_l[0][0])) return;
      // ---- last arriver: the active splits [0, n_act) in split order, 4 per load round
      for (int it = threadIdx.x; it < REP * 32; it += ANC_WAVES * 64) {
        const int h = it >> 5, d = 4 * (it & 31);
        const Merged4 c = split_merge<ExpLog2, 4, REP>(rs, 0, n_act, h, d);
        const float Lr = c.den;
        u32x2 pk;
        pk[0] = pack2bf(Lr > 0.f ? c.num[0] / Lr : 0.f, Lr > 0.f ? c.num[1] / Lr : 0.f);
        pk[1] = pack2bf(Lr > 0.f ? c.num[2] / Lr : 0.f, Lr > 0.f ? c.num[3] / Lr : 0.f);
        *reinterpret_cast<u32x2*>(out + ((size_t)b * H + h0 + h) * ANC_DH + d) = pk;
      }
      return;
    }
  }
  for (int i = threadIdx.x; i < REP * ANC_DH; i += ANC_WAVES * 64) {
    const int h = i / ANC_DH, d = i - h * ANC_DH;
    const Merged1 c = waves_combine1<ExpLog2>(sm_m, sm_l, sm_o, h, d);
    out[((size_t)b * H + h0 + h) * ANC_DH + d] = f2bf(c.den > 0.f ? c.num / c.den : 0.f);
  }
}

// Launches what attn_decode_anc_plan() (attn_plan.h) names. ws / tickets: needed (and checked against the plan, -2)
// only where the plan splits the keys. T >= 8 (and a key mask's row >= 8): anc_load reads up to 8 bytes of a row.
int attn_decode_anc(const bf16_t* q, const bf16_t* kc, const bf16_t* vc, const uint8_t* anc, int num_beams,
                    const int32_t* slot, const int32_t* kv_start, const uint8_t* key_mask, int mask_len, bf16_t* out,
                    int B, int H, int Hkv, int Dh, int T, int t_cap, hipStream_t s, float* ws, size_t ws_floats,
                    int32_t* tickets, int n_tickets) {
  if (B <= 0) return 0;
  const AttnAncPlanResult r = attn_decode_anc_plan(attn_knobs(), B, H, Hkv, Dh, t_cap, key_mask != nullptr, num_beams);
  if (r.rc) return r.rc;
  if (t_cap > T || T < 8 || (key_mask && mask_len < 8) || B > 65535 || Hkv > 65535) return -1;
  const AttnAncPlan& p = r.plan;
  const bool split = p.nsplit > 1;
  if (split && (!ws || !tickets || ws_floats < p.ws_floats || n_tickets < p.tickets)) return -2;
  const float scale = 1.f / sqrtf((float)Dh);
  const dim3 grid = split ? dim3(p.nsplit, Hkv, B) : dim3(Hkv, B);
#define JLA_ADANC(R, K, S)                                                                                     \
  if (p.rep == R && p.kpg == K && split == S) {                                                                \
    attn_decode_anc_kernel<R, K, S><<<grid, ANC_WAVES * 64, 0, s>>>(q, kc, vc, anc, num_beams, slot, kv_start, \
                                                                    key_mask, mask_len, out, ws, tickets,      \
                                                                    p.nsplit, H, Hkv, T, t_cap, scale);        \
    JLA_CHECK_LAUNCH();                                                                                        \
    return 0;                                                                                                  \
  }
  JLA_ADANC(1, 8, false) JLA_ADANC(2, 8, false) JLA_ADANC(4, 4, false) JLA_ADANC(8, 2, false)
  JLA_ADANC(1, 8, true) JLA_ADANC(2, 8, true) JLA_ADANC(4, 4, true) JLA_ADANC(8, 2, true)
#undef JLA_ADANC
  return -1;
}

JLA_BOUNDS_ACCESSOR(attn_decode_anc)

}  // namespace jla
