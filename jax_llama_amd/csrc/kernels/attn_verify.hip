// Decode attention for a few queries per row (the verify step of speculative decoding): q [B, S, H, 128] at cache
// slots slot0 .. slot0 + S - 1 against bf16 [B, Hkv, T, 128] caches, 2 <= S, S x REP <= 32, REP = H / Hkv in {1, 2, 4,
// 8}. Reference ops: ops/reference.py attention (the math attn_prefill serves for every other S > 1). attn_prefill
// gives such a launch one workgroup per (row, kv head, 64 query positions) with no key split -- 8 workgroups for
// Llama-3-8B at B = 1 whatever the context -- so this kernel treats the launch as what it is, a decode step with a
// few more columns.
//
// Column map. attn_mma.h's tile is 32 keys x 16 columns of v_mfma_f32_16x16x32_bf16, the columns being the REP heads
// of a (row, kv head) pair. Here column c = s REP + j is head j of the pair at query position s, and NT = 1 or 2
// such tiles (S REP <= 16 or <= 32) ride on one key stream: column c lives in tile c >> 4, lane column c & 15.
// Columns >= S REP are zero queries whose results are never written. Column c sees keys [kv_start[b], slot0 + s]:
// the lower bound is the pair's, the upper bound the column's, so the compare that attn_mma.h makes per step
// against [lo, hi) is here made per lane against [lo, hi_col[tile]). A step that lies wholly inside [lo, slot0 + 1)
// -- every step but the first and the last one or two -- skips the compare.
//
// Reused across tiles. A 32-key step loads its K rows once (attn_mma.h ad6_issue: 8 x 16 B per lane straight into
// VGPRs, the A operand of the score MFMAs) and its V rows once (8 LDS-DMAs into the swizzled [32][128] image, read
// back transposed by ds_read_b64_tr_b16 as the A operand of P.V). The 8 K fragments feed 8 score MFMAs per tile, each
// V^T fragment pair one P.V MFMA per tile: 16 NT MFMAs on 16 vector-memory ops. Q^T fragments (4 per tile), the
// running (m, l) and the 8 O^T accumulators (AGPRs, ad6_mfma_acc) are per tile; the online softmax is attn_mma.h's,
// log2 domain with the lazy rescale, run once per tile.
//
// Work split. One 4-wave workgroup per (row, kv head, key split). The pair's valid keys [kv_start, slot0 + S) are cut
// at 32-key steps by attn_q8_split_range (attn_plan.h: n_act <= nsplit splits get keys, every workgroup of a pair
// computes the same n_act), and the 4 waves of a split interleave its steps (wave w: steps w, w + 4, ...) with no
// barrier in the loop.
//
// Ring and waits. Per wave two slots, each 8 K registers + one 8 KiB V image: v6's loop. Every half-iteration issues
// the step after next into the slot just consumed and waits vmcnt(16), which leaves exactly the newer step's 16 ops in
// flight; a slot's V image is refilled only behind lgkmcnt(0) (its transposed reads are done). Past the wave's last
// step the issue repeats the last step (clamped rows, computed fully masked), so there is no branch around the loads.
//
// Merges. The waves of a split merge (m, l, O) per tile through LDS (attn_merge.h waves_combine4, log2 units); a pair
// with more than one active split publishes that as its partial -- NC = 16 NT columns in the place of attn_merge.h's
// "heads" -- and the last arriver folds the partials in split order and writes: no float atomics, nothing waits, the
// same bits on every call. A column with no valid key writes zeros.
//
// LDS: 4 waves x 2 slots x 8 KiB = 64 KiB of V images; the wave merge reuses it one tile at a time (4 x 16 x 130
// floats = 32.5 KiB), plus one flag word.
#include "attn_merge.h"
#include "attn_mma.h"
#include "common.h"
#include "launchers.h"
#include "ring.h"

namespace jla {

constexpr int AV_WAVES = ATTN_VERIFY_WAVES;

// per-wave state of one column tile
struct AvTile {
  float m, l;
  f32x4 o[8];
};

// scores, online softmax and P.V of the step at key0 for NT column tiles (the step's loads have landed). full: every
// key of the step is valid for every live column (wave-uniform); otherwise key k counts for the lane's column of tile
// t iff valid && lo <= k < hi_col[t].
template <int NT>
JLA_DEV void av_compute(AvTile (&st)[NT], u32x4 (&kr)[8], const u32x4 (&qf)[NT][4], const char* vslot, int key0,
                        bool valid, bool full, int lo, const int (&hi_col)[NT], float scale_log2, int lane) {
  const int c = lane >> 4;
#pragma unroll
  for (int i = 0; i < 8; ++i) pin(kr[i]);
  u32x4 pf[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      s0 = mfma16x16x32(kr[jj], qf[t][jj], s0);
      s1 = mfma16x16x32(kr[4 + jj], qf[t][jj], s1);
    }
    // lane (c, j): s0[r] = score of key key0 + 4c + r, s1[r] = key key0 + 16 + 4c + r, column 16t + j
    float sc[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sc[r] = s0[r] * scale_log2;
      sc[4 + r] = s1[r] * scale_log2;
    }
    if (!full) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int key = key0 + (e < 4 ? 4 * c + e : 16 + 4 * c + e - 4);
        sc[e] = (valid && key >= lo && key < hi_col[t]) ? sc[e] : -INFINITY;
      }
    }
    float tmax = sc[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) tmax = fmaxf(tmax, sc[e]);
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    if (__ballot(tmax > st[t].m + 8.f)) {  // lazy rescale
      const float m_new = fmaxf(st[t].m, tmax);
      const float alpha = __builtin_amdgcn_exp2f(st[t].m - (m_new == -INFINITY ? 0.f : m_new));
      st[t].l *= alpha;
      st[t].m = m_new;
#pragma unroll
      for (int dt = 0; dt < 8; ++dt) {
        f32x4 v = ad6_take(st[t].o[dt]);
        v *= alpha;
        ad6_put(st[t].o[dt], v);
      }
    }
    const float m_use = st[t].m == -INFINITY ? 0.f : st[t].m;
    float p[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      p[e] = __builtin_amdgcn_exp2f(sc[e] - m_use);
      st[t].l += p[e];
    }
    pf[t] = pack8(p);
  }
  // VALU writes of the P operands (and any accumulator write above) -> MFMA read
  if constexpr (NT == 1)
    asm volatile("s_nop 4" : "+v"(pf[0]));
  else
    asm volatile("s_nop 4" : "+v"(pf[0]), "+v"(pf[1]));
  // V^T fragments: lane 4q + pp of group c reads row 4c + q (and 16 + 4c + q), columns 16dt + 4pp .. +3
  const int q4 = (lane & 15) >> 2, pp = lane & 3;
  const int r0 = 4 * c + q4;
#pragma unroll
  for (int dt = 0; dt < 8; ++dt) {
    const int ch = 2 * dt + (pp >> 1);
    const u32x2 a = ad6_tr(vslot, ad6_off(r0, ch) + 8 * (pp & 1));
    const u32x2 bb = ad6_tr(vslot, ad6_off(r0 + 16, ch) + 8 * (pp & 1));
    const u32x4 vt = {a[0], a[1], bb[0], bb[1]};
#pragma unroll
    for (int t = 0; t < NT; ++t) ad6_mfma_acc(st[t].o[dt], vt, pf[t]);
  }
}

template <int REP, int NT>
__global__ void __launch_bounds__(AV_WAVES * 64)
    attn_verify_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ kc, const bf16_t* __restrict__ vc,
                       const int32_t* __restrict__ slot_ptr, const int32_t* __restrict__ kv_start,
                       bf16_t* __restrict__ out, float* __restrict__ ws, int32_t* __restrict__ tickets, int nsplit,
                       int S, int H, int Hkv, int T, int t_cap, float scale_log2) {
  constexpr int NC = 16 * NT;
  extern __shared__ __attribute__((aligned(16))) char ldsv[];
  __shared__ int flag;
  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = lane >> 4, j = lane & 15;
  const int ncols = S * REP;  // live columns (<= NC)

  const int slot = slot_ptr[0];
  if (slot + S > T && threadIdx.x == 0) JLA_FLAG(JLA_BOUNDS_ATTN_T);  // keys past the cache are never read
  const int cap = min(t_cap, T);
  const int lo = max(kv_start[b], 0);
  const int hi = min(slot + S, cap);       // the pair's keys [lo, hi): the last column's
  const int hi_all = min(slot + 1, cap);   // every live column sees [lo, hi_all)
  const AttnQ8SplitRange sr = attn_q8_split_range(lo, hi, AD6_STEP, nsplit, split);
  const int n_act = sr.n_act;
  // a row with no valid key (n_act 0): split 0 alone goes on, streams nothing and writes 0
  if (split >= max(n_act, 1)) return;

  const int h0 = kvh * REP;
  const size_t head_off = ((size_t)b * Hkv + kvh) * (size_t)T * AD6_DH;
  const bf16_t* const kb = kc + head_off;
  const bf16_t* const vb = vc + head_off;

  // Q^T fragments per tile: the lane's column 16t + j is (query position s, head jh); dead columns load the last live
  // one and are zeroed. A wait hipcc sees, ahead of the hand-counted ring.
  u32x4 qf[NT][4];
  int hi_col[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = 16 * t + j, cc = min(col, ncols - 1);
    const int s = cc / REP, jh = cc - s * REP;
    const bf16_t* qrow = q + (((size_t)b * S + s) * H + h0 + jh) * AD6_DH + 8 * c;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) qf[t][jj] = *reinterpret_cast<const u32x4*>(qrow + 32 * jj);
    hi_col[t] = col < ncols ? min(slot + s + 1, cap) : 0;
  }
  ::wait_vmcnt<0>();
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      pin(qf[t][jj]);
      if (16 * t + j >= ncols) qf[t][jj] = u32x4{0u, 0u, 0u, 0u};
    }

  AvTile st[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    st[t].m = -INFINITY;
    st[t].l = 0.f;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) st[t].o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // this wave's steps of the split's keys (n_act 0: none)
  const Ad6Steps steps = ad6_steps<AV_WAVES>(sr.key_begin, sr.key_end, w);
  const int s_begin = steps.first, my_steps = steps.mine;
  char* const slotA = ldsv + w * AD6_WAVE_LDS;
  char* const slotB = slotA + AD6_SLOT_BYTES;
  auto issue = [&](int step, u32x4 (&kr)[8], char* vslot) {
    ad6_issue<false>((s_begin + step) * AD6_STEP, kr, vslot, kb, vb, T, lane);
  };
  auto compute = [&](int step, bool valid, u32x4 (&kr)[8], const char* vslot) {
    const int key0 = (s_begin + step) * AD6_STEP;
    const bool full = valid && key0 >= lo && key0 + AD6_STEP <= hi_all;
    av_compute<NT>(st, kr, qf, vslot, key0, valid, full, lo, hi_col, scale_log2, lane);
  };
  u32x4 ka[8], kb2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) ka[i] = kb2[i] = u32x4{0u, 0u, 0u, 0u};
  const int last = my_steps - 1;
  auto step_of = [&](int i) { return w + min(i, last) * AV_WAVES; };
  if (my_steps > 0) {
    issue(step_of(0), ka, slotA);
    for (int i = 0; i < my_steps; i += 2) {
      issue(step_of(i + 1), kb2, slotB);
      wait_vmcnt<16>();  // step i (slot A) landed; step i + 1 stays in flight
      compute(step_of(i), true, ka, slotA);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // slot A's V reads are done: refill it
      issue(step_of(i + 2), ka, slotA);
      wait_vmcnt<16>();
      compute(step_of(i + 1), i + 1 < my_steps, kb2, slotB);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    wait_vmcnt<0>();  // the last refill of slot A: drained before the LDS is reused or the wave ends
  }

  // ---- per wave: the accumulators out of the AGPRs, the row sums over the 4 lane groups (they share the max). Lane
  // (c, j) then holds O[column 16t + j][dims 16dt + 4c + r] in st[t].o[dt][r].
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) st[t].o[dt] = ad6_take(st[t].o[dt]);
    st[t].l += __shfl_xor(st[t].l, 16, 64);
    st[t].l += __shfl_xor(st[t].l, 32, 64);
  }

  // ---- the waves through LDS, one tile at a time (the V images are free once every wave is past its loop)
  auto& sm_o = *reinterpret_cast<float (*)[AV_WAVES][16][ATTN_DH]>(ldsv);
  auto& sm_m = *reinterpret_cast<float (*)[AV_WAVES][16]>(ldsv + sizeof(sm_o));
  auto& sm_l = *reinterpret_cast<float (*)[AV_WAVES][16]>(ldsv + sizeof(sm_o) + sizeof(sm_m));
  const bool parts = n_act > 1;  // (workgroup-uniform; n_act <= 1 writes the output here, with no workspace traffic)
  const size_t pair = (size_t)b * Hkv + kvh;
  const __amdgpu_buffer_rsrc_t rs = split_parts_rsrc<NC>(ws, parts ? pair : 0, parts ? nsplit : 0);
  // column col's 4 dims from d on, normalised, to out row b S + s, head h0 + jh
  auto write4 = [&](int col, int d, const Merged4& m4) {
    if (col >= ncols) return;
    const int s = col / REP, jh = col - s * REP;
    const float inv = m4.den > 0.f ? 1.f / m4.den : 0.f;
    const u32x2 pk = {pack2bf(m4.num[0] * inv, m4.num[1] * inv), pack2bf(m4.num[2] * inv, m4.num[3] * inv)};
    *reinterpret_cast<u32x2*>(out + (((size_t)b * S + s) * H + h0 + jh) * AD6_DH + d) = pk;
  };
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    __syncthreads();
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) *reinterpret_cast<f32x4*>(&sm_o[w][j][16 * dt + 4 * c]) = st[t].o[dt];
    if (c == 0) {
      sm_m[w][j] = st[t].m;
      sm_l[w][j] = st[t].l;
    }
    __syncthreads();
    for (int it = threadIdx.x; it < 16 * 32; it += AV_WAVES * 64) {
      const int col16 = it >> 5, d = 4 * (it & 31);
      const Merged4 m4 = waves_combine4<ExpLog2>(sm_m, sm_l, sm_o, col16, d);
      if (parts)
        split_part_store<NC>(rs, split, 16 * t + col16, d, m4);
      else
        write4(16 * t + col16, d, m4);
    }
  }
  if (!parts) return;
  // ---- the key splits: the last arriver folds the active splits [0, n_act) in split order, 4 per load round
  if (!split_arrive(tickets, pair, n_act, flag)) return;
  for (int it = threadIdx.x; it < NC * 32; it += AV_WAVES * 64) {
    const int col = it >> 5, d = 4 * (it & 31);
    write4(col, d, split_merge<ExpLog2, 4, NC>(rs, 0, n_act, col, d));
  }
}

// Launches what attn_verify_plan() (attn_plan.h) names. ws / tickets: needed (and checked against the plan, -2) only
// where the plan splits the keys.
int attn_verify(const bf16_t* q, const bf16_t* kc, const bf16_t* vc, const int32_t* slot, const int32_t* kv_start,
                bf16_t* out, int B, int S, int H, int Hkv, int Dh, int T, int t_cap, hipStream_t s, float* ws,
                size_t ws_floats, int32_t* tickets, int n_tickets) {
  if (B <= 0) return 0;
  const AttnVerifyPlanResult r = attn_verify_plan(attn_knobs(), B, S, H, Hkv, Dh, t_cap, false, false, false);
  if (r.rc) return r.rc;
  if (t_cap > T || B > 65535 || Hkv > 65535) return -1;
  const AttnVerifyPlan& p = r.plan;
  if (p.nsplit > 1 && (!ws || !tickets || ws_floats < p.ws_floats || n_tickets < p.tickets)) return -2;
  const float scale_log2 = 1.4426950408889634f / sqrtf((float)Dh);
  const dim3 grid(p.nsplit, Hkv, B);
#define JLA_AV(R, N)                                                                                             \
  if (p.rep == R && p.tiles == N) {                                                                              \
    attn_verify_kernel<R, N><<<grid, AV_WAVES * 64, AV_WAVES * AD6_WAVE_LDS, s>>>(                               \
        q, kc, vc, slot, kv_start, out, ws, tickets, p.nsplit, S, H, Hkv, T, t_cap, scale_log2);                 \
    JLA_CHECK_LAUNCH();                                                                                          \
    return 0;                                                                                                    \
  }
  JLA_AV(1, 1) JLA_AV(2, 1) JLA_AV(4, 1) JLA_AV(8, 1)
  JLA_AV(1, 2) JLA_AV(2, 2) JLA_AV(4, 2) JLA_AV(8, 2)
#undef JLA_AV
  return -1;
}

JLA_BOUNDS_ACCESSOR(attn_verify)

}  // namespace jla
