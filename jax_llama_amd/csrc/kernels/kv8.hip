// The FP8 (OCP e4m3fn) KV cache: the quantising RoPE + cache write, the dequantiser the S > 1 attention reads through,
// and the decode attention that streams the fp8 bytes.
//
// A KV row is the 128 values of one (batch row, kv head, slot), of K (post-RoPE) or of V. It is stored as 128 e4m3
// bytes in natural element order plus one fp32 scale 2^e, by the rule of ops/reference.py quantize_fp8_rows: amax =
// m 2^x with m in [0.5, 1) (frexp), e = x - 9 where m <= 0.875 (448 = 0.875 * 2^9) and x - 8 above, clamped to
// [-100, 100], 0 for an all-zero row; q = fp8_rne(row / 2^e). q * 2^e is exact in bf16, and the model with this cache
// is the bf16 model whose K / V rows are replaced by q * 2^e when they are written. 132 bytes per row instead of 256.
// gfx950's FP8 conversions are OCP (e4m3fn), not fnuz.
#include "attn_merge.h"
#include "common.h"
#include "launchers.h"

namespace jla {

constexpr int KV8_DH = ATTN_DH;

// The scale exponent of a row from the fp32 bits of its amax (>= 0), integer operations only. A normal amax has x =
// (biased exponent) - 126 and m <= 0.875 exactly where the 23 mantissa bits are <= 0x600000; an fp32-subnormal amax has
// x < -126, which the clamp maps to -100 like every x below -91.
JLA_DEV int kv8_exponent(uint32_t amax_bits) {
  if (amax_bits == 0) return 0;
  const int x = (int)(amax_bits >> 23) - 126;
  const int e = (amax_bits & 0x7fffffu) <= 0x600000u ? x - 9 : x - 8;
  return e < -100 ? -100 : (e > 100 ? 100 : e);
}
JLA_DEV float kv8_pow2(int e) { return __uint_as_float((uint32_t)(127 + e) << 23); }  // e in [-100, 100]

// 8 floats x 2^-e -> 8 e4m3 bytes, two values per v_cvt_pk_fp8_f32 (round to nearest even). The product is exact; the
// clamp acts only where the exponent was clamped (as the reference's).
JLA_DEV u32x2 kv8_quant8(const float* f, float inv) {
  float s[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = fminf(fmaxf(f[e] * inv, -448.f), 448.f);
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(s[0], s[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(s[2], s[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(s[4], s[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(s[6], s[7], hi, true);
  return u32x2{(uint32_t)lo, (uint32_t)hi};
}

// 8 e4m3 bytes -> the same 8 values as packed bf16 (exact): four v_cvt_scalef32_pk_bf16_fp8 at scale 1.0
JLA_DEV u32x4 kv8_to_bf16(const u32x2 q) {
  u32x4 r;
  r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[0], 1.0f, false));
  r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[0], 1.0f, true));
  r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[1], 1.0f, false));
  r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[1], 1.0f, true));
  return r;
}

// ---------------------------------------------------------------------------------------------
// rope_kv_kernel (rope_kv.hip) with the quantising store: the same launch shape, one 16-byte qkv vector per thread,
// so the 16 lanes of a DPP row own one 128-value head row, 8 values per lane. q heads: rotate, store bf16. k heads:
// rotate, round to bf16 (the value the bf16 cache would hold), amax over the 16 lanes, exponent, x 2^-e, convert,
// 8 bytes per lane = one contiguous 128-B row; lane 0 of the row stores the scale. v heads: the same without the
// rotation. The slot comes from device memory (graph replay). Every lane of a row takes the same branches (the head is
// per row), so the DPP row operations see whole rows.
__global__ void __launch_bounds__(256)
    rope_kv_q8_kernel(const bf16_t* __restrict__ qkv, const float2* __restrict__ table, int table_len,
                      const int32_t* __restrict__ positions, uint8_t* __restrict__ kq, float* __restrict__ ks,
                      uint8_t* __restrict__ vq, float* __restrict__ vs, const int32_t* __restrict__ slot_ptr, int S,
                      int H, int Hkv, int T, bf16_t* __restrict__ q_out) {
  constexpr int Dh = KV8_DH, VPH = Dh >> 3;  // 16 vectors per head
  const int m = blockIdx.x;
  const int b = m / S, s = m - b * S;
  const int nvec = (H + 2 * Hkv) * VPH;
  int pos = positions[m];
  if (pos < 0 || pos >= table_len) JLA_FLAG(JLA_BOUNDS_ROPE_POS);
  pos = pos < 0 ? 0 : (pos >= table_len ? table_len - 1 : pos);
  const int slot = slot_ptr[0] + s;
  const u32x4* row = reinterpret_cast<const u32x4*>(qkv + (size_t)m * (H + 2 * Hkv) * Dh);
  for (int v = threadIdx.x; v < nvec; v += blockDim.x) {
    const int head = v / VPH, li = v - head * VPH, d0 = li * 8;
    u32x4 val = row[v];
    if (head < H + Hkv) {
      float f[8];
      unpack8(val, f);
      const float2* cs = table + (size_t)pos * (Dh >> 1) + (d0 >> 1);
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const float2 t = cs[p];
        const float xr = f[2 * p], xi = f[2 * p + 1];
        f[2 * p] = xr * t.x - xi * t.y;
        f[2 * p + 1] = xr * t.y + xi * t.x;
      }
      val = pack8(f);
    }
    if (head < H) {
      reinterpret_cast<u32x4*>(q_out + ((size_t)m * H + head) * Dh + d0)[0] = val;
      continue;
    }
    float f[8];
    unpack8(val, f);  // the bf16 row values
    uint32_t a = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) a = max(a, __float_as_uint(f[e]) & 0x7fffffffu);
    a = row16_max_u32(a);
    const int ex = kv8_exponent(a);
    const u32x2 pk = kv8_quant8(f, kv8_pow2(-ex));
    if (slot >= 0 && slot < T) {
      const bool is_k = head < H + Hkv;
      const int kh = is_k ? head - H : head - H - Hkv;
      const size_t r = ((size_t)b * Hkv + kh) * T + slot;
      *reinterpret_cast<u32x2*>((is_k ? kq : vq) + r * Dh + d0) = pk;
      if (li == 0) (is_k ? ks : vs)[r] = kv8_pow2(ex);
    } else {
      JLA_FLAG(JLA_BOUNDS_KV_SLOT);
    }
  }
}

int rope_kv_write_q8(const bf16_t* qkv, const float* table, int table_len, const int32_t* positions, uint8_t* kq,
                     float* ks, uint8_t* vq, float* vs, const int32_t* slot, int M, int S, int H, int Hkv, int Dh,
                     int T, bf16_t* q_out, hipStream_t s) {
  if (M <= 0) return 0;
  if (Dh != KV8_DH || S <= 0 || M % S || T <= 0) return -1;
  rope_kv_q8_kernel<<<M, 256, 0, s>>>(qkv, reinterpret_cast<const float2*>(table), table_len, positions, kq, ks, vq,
                                      vs, slot, S, H, Hkv, T, q_out);
  JLA_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Slots [0, n) of every pair of one layer's K (blockIdx.y 0) and V (1) as bf16 rows [pairs, n_out, 128]: one thread per
// 8 values; the conversion is exact and so is the power-of-two multiply. Read by the S > 1 attention (attn_prefill on
// the scratch) and by output_attentions.
__global__ void __launch_bounds__(256)
    kv8_dequant_kernel(const uint8_t* __restrict__ kq, const float* __restrict__ ks, const uint8_t* __restrict__ vq,
                       const float* __restrict__ vs, bf16_t* __restrict__ kout, bf16_t* __restrict__ vout,
                       long long vecs, int T, int n, int n_out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;  // (pair, slot, 16 vectors)
  if (i >= vecs) return;
  const int li = (int)(i & 15);
  const long long rj = i >> 4;
  const long long pair = rj / n;
  const int j = (int)(rj - pair * n);
  const bool is_v = blockIdx.y != 0;
  const size_t r = (size_t)pair * T + j;
  const u32x2 q = *reinterpret_cast<const u32x2*>((is_v ? vq : kq) + r * KV8_DH + 8 * li);
  const float sc = (is_v ? vs : ks)[r];
  float f[8];
  unpack8(kv8_to_bf16(q), f);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] *= sc;
  *reinterpret_cast<u32x4*>((is_v ? vout : kout) + ((size_t)pair * n_out + j) * KV8_DH + 8 * li) = pack8(f);
}

int kv8_dequant(const uint8_t* kq, const float* ks, const uint8_t* vq, const float* vs, bf16_t* kout, bf16_t* vout,
                int pairs, int T, int n, int n_out, hipStream_t s) {
  if (pairs <= 0 || n <= 0) return 0;
  if (n > T || n > n_out) return -1;
  const long long vecs = (long long)pairs * n * 16;
  const long long grid = (vecs + 255) / 256;
  if (grid > 0x7fffffffLL) return -1;
  kv8_dequant_kernel<<<dim3((unsigned)grid, 2), 256, 0, s>>>(kq, ks, vq, vs, kout, vout, vecs, T, n, n_out);
  JLA_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------------------------------------
// Decode attention on the fp8 bytes: one workgroup of WAVES waves per (row, kv head) pair, attn_decode_v3_kernel's
// structure (attn_decode.hip): the valid keys [kv_start, slot] in interleaved 16-lane rows -- row r of lane group g of
// wave w in the chunk at c0 is key c0 + 4 WAVES r + 4 w + g, so one wave load covers 4 consecutive cache rows -- the
// next chunk's loads issued before the current one is scored, a running (max, sum, o) per query head and wave (online
// softmax, no barrier in the loop), one LDS merge of the waves (none at WAVES = 1, the large-batch form: there the
// pairs alone fill the chip). A lane loads 8 bytes of K and 8 of V per key (16 lanes = one 128-B row) and the key's
// two scales, converts K to packed bf16 in registers (exact) for v_dot2, and V to fp32. The K scale multiplies the
// score after the dot, score = (q . k_q) * sk / sqrt(Dh); the V scale multiplies p before the accumulation. kv_start,
// the key mask, t_cap and "rows with no valid key give 0" are v3's. No packed copy.
//
// SPLIT (8 waves only; few pairs with a long context, where one workgroup per pair leaves most CUs idle): the grid is
// (nsplit, Hkv, B) and a workgroup streams the keys attn_q8_split_range() (attn_plan.h) gives its split of the pair's
// valid keys -- the valid range is device state, so the splits cut it, not the cache. Splits without keys exit at once;
// a pair with one active split (early in a generation) writes its output directly. Otherwise the key-split protocol of
// attn_merge.h over the active splits [0, n_act), m in log2 units: no float atomics, nothing waits, the same bits on
// every call.
template <int REP, int KPG, int WAVES, bool SPLIT>
__global__ void __launch_bounds__(WAVES * 64)
    attn_decode_q8_kernel(const bf16_t* __restrict__ q, const uint8_t* __restrict__ kq, const float* __restrict__ ks,
                          const uint8_t* __restrict__ vq, const float* __restrict__ vs,
                          const int32_t* __restrict__ slot_ptr, const int32_t* __restrict__ kv_start,
                          const uint8_t* __restrict__ key_mask, int mask_len, bf16_t* __restrict__ out,
                          float* __restrict__ ws, int32_t* __restrict__ tickets, int nsplit, int H, int Hkv, int T,
                          int t_cap, float scale) {
  static_assert(!SPLIT || WAVES == 8, "key splits: the 8-wave form only");
  constexpr int CH = WAVES * 4 * KPG;  // keys per chunk
  constexpr int MW = WAVES > 1 ? WAVES : 1;
  __shared__ float sm_m[WAVES > 1 ? MW : 1][REP];
  __shared__ float sm_l[WAVES > 1 ? MW : 1][REP];  // (SPLIT: sm_l[0][0] also carries "this workgroup merges")
  __shared__ float sm_o[WAVES > 1 ? MW : 1][WAVES > 1 ? REP : 1][WAVES > 1 ? KV8_DH : 1];

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
  const size_t pair_row = ((size_t)b * Hkv + kvh) * T;
  const uint8_t* kbase = kq + pair_row * KV8_DH + 8 * li;
  const uint8_t* vbase = vq + pair_row * KV8_DH + 8 * li;
  const float* ksb = ks + pair_row;
  const float* vsb = vs + pair_row;

  u32x4 qp[REP];  // this lane's 8 dims of each query head, packed bf16 (the v_dot2 operand)
#pragma unroll
  for (int h = 0; h < REP; ++h)
    qp[h] = *reinterpret_cast<const u32x4*>(q + ((size_t)b * H + h0 + h) * KV8_DH + 8 * li);
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

  u32x2 kr[KPG], vr[KPG];
  float skr[KPG], svr[KPG];
  auto load = [&](int c0) {
#pragma unroll
    for (int r = 0; r < KPG; ++r) {
      const int j = min(max(c0 + 4 * WAVES * r + 4 * w + g, 0), hi_key - 1);  // (hi_key >= 1 wherever this runs)
      kr[r] = *reinterpret_cast<const u32x2*>(kbase + (size_t)j * KV8_DH);
      vr[r] = *reinterpret_cast<const u32x2*>(vbase + (size_t)j * KV8_DH);
      skr[r] = ksb[j];
      svr[r] = vsb[j];
    }
  };
  if (lo < hi_key) load(c_begin);
  for (int c0 = c_begin; c0 < hi_key && lo < hi_key; c0 += CH) {
    u32x2 kcur[KPG], vcur[KPG];
    float skc[KPG], svc[KPG];
#pragma unroll
    for (int r = 0; r < KPG; ++r) {
      kcur[r] = kr[r];
      vcur[r] = vr[r];
      skc[r] = skr[r];
      svc[r] = svr[r];
    }
    if (c0 + CH < hi_key) load(c0 + CH);  // next chunk in flight while this one is scored
    float sc[REP][KPG];
#pragma unroll
    for (int r = 0; r < KPG; ++r) {
      const int j = c0 + 4 * WAVES * r + 4 * w + g;
      bool valid = j >= lo && j < hi_key;
      if (mrow) valid = valid && j < mask_len && mrow[j] != 0;
      const u32x4 kb = kv8_to_bf16(kcur[r]);
      // (q . k_q) * sk / sqrt(Dh), in log2 units: sk is a power of two, so sk * scale2 is exact and the score has the
      // one rounding of the triple product whichever way it is associated
      const float kscale = skc[r] * scale2;
#pragma unroll
      for (int h = 0; h < REP; ++h) {
        const float d = row16_sum(dot8_bf16(qp[h], kb, 0.f));
        sc[h][r] = valid ? d * kscale : -INFINITY;
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
      const f32x2_t vf[4] = {__builtin_amdgcn_cvt_pk_f32_fp8((int)vcur[r][0], false),
                             __builtin_amdgcn_cvt_pk_f32_fp8((int)vcur[r][0], true),
                             __builtin_amdgcn_cvt_pk_f32_fp8((int)vcur[r][1], false),
                             __builtin_amdgcn_cvt_pk_f32_fp8((int)vcur[r][1], true)};
#pragma unroll
      for (int h = 0; h < REP; ++h) {
        const float p = __builtin_amdgcn_exp2f(sc[h][r] - mref[h]);  // a masked key: exp2(-inf) = 0
        l_h[h] += p;  // the 16 lanes of a group hold the same p (and the same running sum)
        const float ps = p * svc[r];  // the V scale on p, before the accumulation
        const f32x2_t pp = {ps, ps};
#pragma unroll
        for (int i = 0; i < 4; ++i) o[h][i] = __builtin_elementwise_fma(pp, vf[i], o[h][i]);
      }
    }
  }
  // ---- per wave: sum the 4 groups (same max)
  float of[REP][8];
#pragma unroll
  for (int h = 0; h < REP; ++h) wave_sum_groups(l_h[h], o[h], of[h]);
  if constexpr (WAVES == 1) {
    if (g == 0) {
#pragma unroll
      for (int h = 0; h < REP; ++h) {
        const float inv = l_h[h] > 0.f ? 1.f / l_h[h] : 0.f;
        float r8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) r8[e] = of[h][e] * inv;
        *reinterpret_cast<u32x4*>(out + ((size_t)b * H + h0 + h) * KV8_DH + 8 * li) = pack8(r8);
      }
    }
  } else {
    // ---- merge the waves through LDS
#pragma unroll
    for (int h = 0; h < REP; ++h) wave_put(sm_m, sm_l, sm_o, w, h, g, li, m_h[h], l_h[h], of[h]);
    __syncthreads();
    if constexpr (SPLIT) {
      if (n_act > 1) {  // (workgroup-uniform; n_act <= 1 writes the output below, with no workspace traffic)
        const size_t pair = (size_t)b * Hkv + kvh;
        const __amdgpu_buffer_rsrc_t rs = split_parts_rsrc<REP>(ws, pair, nsplit);
        // ---- this split's unnormalised (m, l, o) per head: thread -> (head, 4 dims)
        for (int it = threadIdx.x; it < REP * 32; it += WAVES * 64) {
          const int h = it >> 5, d = 4 * (it & 31);
          split_part_store<REP>(rs, split, h, d, waves_combine4<ExpLog2>(sm_m, sm_l, sm_o, h, d));
        }
        // (the flag in sm_l[0][0]: every read of the wave partials is behind the barrier inside)
        if (!split_arrive(tickets, pair, n_act, sm_l[0][0])) return;
        // ---- last arriver: the active splits [0, n_act) in split order, 4 per load round
        for (int it = threadIdx.x; it < REP * 32; it += WAVES * 64) {
          const int h = it >> 5, d = 4 * (it & 31);
          const Merged4 c = split_merge<ExpLog2, 4, REP>(rs, 0, n_act, h, d);
          const float Lr = c.den;
          u32x2 pk;
          pk[0] = pack2bf(Lr > 0.f ? c.num[0] / Lr : 0.f, Lr > 0.f ? c.num[1] / Lr : 0.f);
          pk[1] = pack2bf(Lr > 0.f ? c.num[2] / Lr : 0.f, Lr > 0.f ? c.num[3] / Lr : 0.f);
          *reinterpret_cast<u32x2*>(out + ((size_t)b * H + h0 + h) * KV8_DH + d) = pk;
        }
        return;
      }
    }
    for (int i = threadIdx.x; i < REP * KV8_DH; i += WAVES * 64) {
      const int h = i / KV8_DH, d = i - h * KV8_DH;
      const Merged1 c = waves_combine1<ExpLog2>(sm_m, sm_l, sm_o, h, d);
      out[((size_t)b * H + h0 + h) * KV8_DH + d] = f2bf(c.den > 0.f ? c.num / c.den : 0.f);
    }
  }
}

// Launches what attn_decode_q8_plan() (attn_plan.h) names: one instantiation per (rep, kpg, waves, split or not) the plan
// can give. ws / tickets: needed (and checked against the plan, -2) only where the plan splits the keys.
int attn_decode_q8(const bf16_t* q, const uint8_t* kq, const float* ks, const uint8_t* vq, const float* vs,
                   const int32_t* slot, const int32_t* kv_start, const uint8_t* key_mask, int mask_len, bf16_t* out,
                   int B, int H, int Hkv, int Dh, int T, int t_cap, hipStream_t s, float* ws, size_t ws_floats,
                   int32_t* tickets, int n_tickets) {
  if (B <= 0) return 0;
  const AttnQ8PlanResult r = attn_decode_q8_plan(attn_knobs(), B, H, Hkv, Dh, t_cap, key_mask != nullptr);
  if (r.rc) return r.rc;
  if (t_cap > T || B > 65535) return -1;
  const AttnQ8Plan& p = r.plan;
  const bool split = p.nsplit > 1;
  if (split && Hkv > 65535) return -1;  // (the split grid has the kv heads in y)
  if (split && (!ws || !tickets || ws_floats < p.ws_floats || n_tickets < p.tickets)) return -2;
  const float scale = 1.f / sqrtf((float)Dh);
  const dim3 grid = split ? dim3(p.nsplit, Hkv, B) : dim3(Hkv, B);
#define JLA_ADQ8(R, K, W, S)                                                                                        \
  if (p.rep == R && p.kpg == K && p.waves == W && split == S) {                                                     \
    attn_decode_q8_kernel<R, K, W, S><<<grid, W * 64, 0, s>>>(q, kq, ks, vq, vs, slot, kv_start, key_mask, mask_len, \
                                                              out, ws, tickets, p.nsplit, H, Hkv, T, t_cap, scale); \
    JLA_CHECK_LAUNCH();                                                                                             \
    return 0;                                                                                                       \
  }
  JLA_ADQ8(1, 8, 8, false) JLA_ADQ8(2, 8, 8, false) JLA_ADQ8(4, 4, 8, false) JLA_ADQ8(8, 2, 8, false)
  JLA_ADQ8(1, 8, 1, false) JLA_ADQ8(2, 8, 1, false) JLA_ADQ8(4, 4, 1, false) JLA_ADQ8(8, 2, 1, false)
  JLA_ADQ8(1, 8, 8, true) JLA_ADQ8(2, 8, 8, true) JLA_ADQ8(4, 4, 8, true) JLA_ADQ8(8, 2, 8, true)
#undef JLA_ADQ8
  return -1;
}

JLA_BOUNDS_ACCESSOR(kv8)

}  // namespace jla
