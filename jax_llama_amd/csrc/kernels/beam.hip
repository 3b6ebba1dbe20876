// Beam search on the device (HF Flax _beam_search semantics; the definition is the README's "Beam search" section and
// ops/reference.py beam_step / beam_continue / kv_beam_reorder, which these kernels match bit for bit).
//
// beam_alive:  the loop condition, evaluated from the state before a step into one device word.
// beam_step:   one workgroup (one wave) per batch item: ranks the K x 2K candidates by counting, writes the next
//   running beams, merges the finished pool, permutes running_seq / seq in place (a lane owns whole columns and loads
//   every source before it stores), and writes beam_idx, the next input tokens, positions + 1, cur_len + 1, slot + 1.
//   With alive == 0 it writes the identity beam_idx and nothing else.
// kv_beam_reorder: every beam's KV rows follow its parent, in place, for the slots below the device slot counter.
//
// Score arithmetic is single fp32 adds and multiplies (contraction off: an fma would round differently from the CPU).
#include "common.h"
#include "launchers.h"

namespace jla {

namespace {
constexpr float BEAM_NEG = -1.0e7f;
constexpr int BEAM_MAX_K = 8;
}  // namespace

__global__ void __launch_bounds__(64)
    beam_alive_kernel(const float* __restrict__ running_score, const float* __restrict__ score,
                      const int32_t* __restrict__ is_finished, const float* __restrict__ inv_pen,
                      const int32_t* __restrict__ cur_len, int32_t* __restrict__ alive, int B, int K, int L, int S,
                      int early, int never_full) {
#pragma clang fp contract(off)
  const int c = cur_len[0];
  int all_fin = 1, improve = 0;
  int d = never_full ? L - S : c - S;
  d = d < 0 ? 0 : (d > L ? L : d);
  const float pen = inv_pen[d];
  for (int b = threadIdx.x; b < B; b += 64) {
    int any = 0;
    float worst = INFINITY;
    for (int j = 0; j < K; ++j) {
      const int f = is_finished[b * K + j] != 0;
      any |= f;
      all_fin &= f;
      worst = fminf(worst, score[b * K + j]);
    }
    const float best_running = __fmul_rn(running_score[b * K], pen);
    const float worst_finished = any ? worst : BEAM_NEG;
    improve |= best_running > worst_finished;
  }
  all_fin = __all(all_fin);
  improve = __any(improve);
  if (threadIdx.x == 0) alive[0] = (c < L && !(early == 1 && all_fin) && (c == S || improve)) ? 1 : 0;
}

// LDS state of one batch item's step
struct BeamShared {
  float lp[2 * BEAM_MAX_K * BEAM_MAX_K];
  float top_lp[2 * BEAM_MAX_K];
  float run_lp[2 * BEAM_MAX_K];
  int32_t top_tok[2 * BEAM_MAX_K];
  int32_t top_par[2 * BEAM_MAX_K];
  float m_score[3 * BEAM_MAX_K];
  int32_t m_fin[3 * BEAM_MAX_K];
  int32_t run_src[BEAM_MAX_K];  // next running beam j' <- candidate rank
  int32_t fin_src[BEAM_MAX_K];  // next finished slot <- merged entry (< K: an old slot, else candidate rank + K)
  int32_t old_fin_all;
};

__global__ void __launch_bounds__(64)
    beam_step_kernel(const float* __restrict__ cand_v, const int32_t* __restrict__ cand_i,
                     const float* __restrict__ lse, int32_t* running_seq, int32_t* seq, float* running_score,
                     float* score, int32_t* is_finished, const float* __restrict__ inv_pen, int32_t* cur_len,
                     int32_t* slot, int32_t* tokens, int32_t* positions, const int32_t* __restrict__ alive,
                     int32_t* __restrict__ beam_idx, int B, int K, int L, int S, int eos, int early) {
#pragma clang fp contract(off)
  __shared__ BeamShared sh;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int K2 = 2 * K, NC = K * K2;
  const int c = cur_len[0];
  // c outside [S, L) can only come from a caller that steps past the buffer: treated like alive == 0
  const bool live = alive[0] != 0 && c >= S && c < L;
  if (alive[0] != 0 && !live) JLA_FLAG(JLA_BOUNDS_SEQ);
  if (!live) {
    if (tid < K) beam_idx[b * K + tid] = tid;
    return;
  }
  // 1-3: candidate log-probs
  for (int i = tid; i < NC; i += 64) {
    const int j = i / K2;
    sh.lp[i] = __fadd_rn(running_score[b * K + j], __fsub_rn(cand_v[(size_t)b * NC + i], lse[b * K + j]));
  }
  // every index the later phases read is in range even where NaN scores leave a rank unassigned
  if (tid < 2 * BEAM_MAX_K) {
    sh.top_lp[tid] = BEAM_NEG;
    sh.top_tok[tid] = 0;
    sh.top_par[tid] = 0;
  }
  if (tid < BEAM_MAX_K) {
    sh.run_src[tid] = 0;
    sh.fin_src[tid] = 0;
  }
  if (tid == 0) {
    int af = 1;
    for (int j = 0; j < K; ++j) af &= is_finished[b * K + j] != 0;
    sh.old_fin_all = af;
  }
  __syncthreads();
  // 4: best 2K of the K x 2K by (lp desc, flat index asc)
  for (int i = tid; i < NC; i += 64) {
    const float x = sh.lp[i];
    int rank = 0;
    for (int o = 0; o < NC; ++o) {
      const float y = sh.lp[o];
      rank += (y > x || (y == x && o < i)) ? 1 : 0;
    }
    if (rank < K2) {
      sh.top_lp[rank] = x;
      sh.top_tok[rank] = cand_i[(size_t)b * NC + i];
      sh.top_par[rank] = i / K2;
    }
  }
  __syncthreads();
  // 5 + 7: running and finished-pool scores of the 2K candidates; the old pool goes first in the merge
  const float pen = inv_pen[c + 1 - S];
  if (tid < K2) {
    const float x = sh.top_lp[tid];
    const bool just = sh.top_tok[tid] == eos;
    sh.run_lp[tid] = just ? __fadd_rn(BEAM_NEG, x) : x;
    const float f = __fmul_rn(x, pen);
    const bool add = !just || (sh.old_fin_all && early == 1);
    sh.m_score[K + tid] = add ? __fadd_rn(f, BEAM_NEG) : f;
    sh.m_fin[K + tid] = just ? 1 : 0;
  } else if (tid < K2 + K) {
    const int j = tid - K2;
    sh.m_score[j] = score[b * K + j];
    sh.m_fin[j] = is_finished[b * K + j] != 0 ? 1 : 0;
  }
  __syncthreads();
  // 6: next running beams = best K by run_lp (ties: lower candidate rank); 7: best K of the 3K merged entries
  if (tid < K2) {
    const float x = sh.run_lp[tid];
    int rank = 0;
    for (int o = 0; o < K2; ++o) {
      const float y = sh.run_lp[o];
      rank += (y > x || (y == x && o < tid)) ? 1 : 0;
    }
    if (rank < K) sh.run_src[rank] = tid;
  } else if (tid < K2 + 3 * K) {
    const int e = tid - K2;
    const float x = sh.m_score[e];
    int rank = 0;
    for (int o = 0; o < 3 * K; ++o) {
      const float y = sh.m_score[o];
      rank += (y > x || (y == x && o < e)) ? 1 : 0;
    }
    if (rank < K) sh.fin_src[rank] = e;
  }
  __syncthreads();
  // sequences, in place: a lane owns columns; every load of a column comes before its stores
  int32_t* rs = running_seq + (size_t)b * K * L;
  int32_t* fs = seq + (size_t)b * K * L;
  for (int col = tid; col < L; col += 64) {  // whole rows, as the definition has it (past c they hold pad)
    int32_t nr[BEAM_MAX_K], nf[BEAM_MAX_K];
#pragma unroll
    for (int j = 0; j < BEAM_MAX_K; ++j) {
      if (j < K) {
        const int r = sh.run_src[j];
        nr[j] = col == c ? sh.top_tok[r] : rs[(size_t)sh.top_par[r] * L + col];
        const int e = sh.fin_src[j];
        if (e < K)
          nf[j] = fs[(size_t)e * L + col];
        else
          nf[j] = col == c ? sh.top_tok[e - K] : rs[(size_t)sh.top_par[e - K] * L + col];
      }
    }
#pragma unroll
    for (int j = 0; j < BEAM_MAX_K; ++j) {
      if (j < K) {
        rs[(size_t)j * L + col] = nr[j];
        fs[(size_t)j * L + col] = nf[j];
      }
    }
  }
  if (tid < K) {
    const int r = sh.run_src[tid];
    running_score[b * K + tid] = sh.run_lp[r];
    beam_idx[b * K + tid] = sh.top_par[r];
    tokens[b * K + tid] = sh.top_tok[r];
    positions[b * K + tid] += 1;
    const int e = sh.fin_src[tid];
    score[b * K + tid] = sh.m_score[e];
    is_finished[b * K + tid] = sh.m_fin[e];
  }
}

// cur_len and the slot advance in a launch of their own: every workgroup of beam_step reads cur_len
__global__ void beam_advance_kernel(const int32_t* __restrict__ alive, int32_t* cur_len, int32_t* slot, int L, int S) {
  const int c = cur_len[0];
  if (threadIdx.x == 0 && alive[0] != 0 && c >= S && c < L) {
    cur_len[0] = c + 1;
    slot[0] += 1;
  }
}

int beam_alive(const float* running_score, const float* score, const int32_t* is_finished, const float* inv_pen,
               const int32_t* cur_len, int32_t* alive, int B, int K, int L, int S, int early, int never_full,
               hipStream_t s) {
  if (B <= 0 || K < 2 || K > BEAM_MAX_K || S < 1 || S > L) return -1;
  beam_alive_kernel<<<1, 64, 0, s>>>(running_score, score, is_finished, inv_pen, cur_len, alive, B, K, L, S, early,
                                     never_full);
  JLA_CHECK_LAUNCH();
  return 0;
}

int beam_step(const float* cand_v, const int32_t* cand_i, const float* lse, int32_t* running_seq, int32_t* seq,
              float* running_score, float* score, int32_t* is_finished, const float* inv_pen, int32_t* cur_len,
              int32_t* slot, int32_t* tokens, int32_t* positions, const int32_t* alive, int32_t* beam_idx, int B,
              int K, int L, int S, int eos, int early, hipStream_t s) {
  if (B <= 0 || K < 2 || K > BEAM_MAX_K || S < 1 || S > L) return -1;
  beam_step_kernel<<<B, 64, 0, s>>>(cand_v, cand_i, lse, running_seq, seq, running_score, score, is_finished, inv_pen,
                                    cur_len, slot, tokens, positions, alive, beam_idx, B, K, L, S, eos, early);
  JLA_CHECK_LAUNCH();
  beam_advance_kernel<<<1, 64, 0, s>>>(alive, cur_len, slot, L, S);
  JLA_CHECK_LAUNCH();
  return 0;
}

// ---- KV-cache beam reorder ---------------------------------------------------------------------------------------
// One cache tensor [layers, B*K rows, heads, T slots, RB bytes]: per (layer, row, head) a contiguous run of T * RB
// bytes, cut into units of sizeof(U) bytes (16, or 4 where the run is no multiple of 16). A thread owns unit u of a
// (layer, group, head) across the group's K beams: K loads from the permuted sources, then the stores of the rows
// that changed parent. No other thread touches those addresses, so a rotation or a swap inside a group is safe. Units
// below ceil(count * RB / sizeof(U)) move: the last one may carry slots >= count of the same (layer, head) along.
template <int K, typename U>
__global__ void __launch_bounds__(256)
    kv_beam_reorder_kernel(U* base, const int32_t* __restrict__ beam_idx, const int32_t* __restrict__ slot, int heads,
                           int T, int RB, int groups) {
  const int g = blockIdx.y % groups, layer = blockIdx.y / groups, head = blockIdx.z;
  int p[K];
  bool ident = true;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    int v = beam_idx[g * K + j];
    if (v < 0 || v >= K) {
      JLA_FLAG(JLA_BOUNDS_BEAM);
      v = v < 0 ? 0 : K - 1;
    }
    p[j] = v;
    ident = ident && v == j;
  }
  if (ident) return;
  int count = slot[0];
  if (count < 0 || count > T) {
    JLA_FLAG(JLA_BOUNDS_KV_SLOT);
    count = count < 0 ? 0 : T;
  }
  const size_t run = (size_t)T * RB / sizeof(U);  // units per (layer, row, head)
  const size_t n = ((size_t)count * RB + sizeof(U) - 1) / sizeof(U);
  U* grp = base + (((size_t)layer * groups + g) * K * heads + head) * run;
  const size_t row = (size_t)heads * run;
  for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < n; u += (size_t)gridDim.x * 256) {
    U v[K];
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = __builtin_nontemporal_load(grp + p[j] * row + u);
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (p[j] != j) grp[j * row + u] = v[j];
  }
}

template <typename U>
static int kv_beam_reorder_launch(void* base, const int32_t* beam_idx, const int32_t* slot, int layers, int groups,
                                  int K, int heads, int T, int RB, hipStream_t s) {
  const size_t run = (size_t)T * RB / sizeof(U);
  const long long lgh = (long long)layers * groups * heads;
  long long gx = (long long)((run + 255) / 256);
  const long long cap = (8192 + lgh - 1) / lgh;  // about 8192 workgroups in all; the threads stride over the run
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  const dim3 grid((unsigned)gx, (unsigned)(layers * groups), (unsigned)heads);
  U* p = (U*)base;
  switch (K) {
#define JLA_BEAM_CASE(KK)                                                                                    \
  case KK:                                                                                                   \
    kv_beam_reorder_kernel<KK, U><<<grid, 256, 0, s>>>(p, beam_idx, slot, heads, T, RB, groups);             \
    break;
    JLA_BEAM_CASE(2)
    JLA_BEAM_CASE(3)
    JLA_BEAM_CASE(4)
    JLA_BEAM_CASE(5)
    JLA_BEAM_CASE(6)
    JLA_BEAM_CASE(7)
    JLA_BEAM_CASE(8)
#undef JLA_BEAM_CASE
    default:
      return -1;
  }
  JLA_CHECK_LAUNCH();
  return 0;
}

int kv_beam_reorder(void* base, const int32_t* beam_idx, const int32_t* slot, int layers, int groups, int K,
                    int heads, int T, int RB, hipStream_t s) {
  if (layers <= 0 || groups <= 0 || heads <= 0 || T <= 0 || RB <= 0 || RB % 4 || K < 2 || K > BEAM_MAX_K) return -1;
  if ((long long)layers * groups > 65535 || heads > 65535) return -2;
  if (((size_t)T * RB) % 16 == 0 && ((uintptr_t)base) % 16 == 0)
    return kv_beam_reorder_launch<u32x4>(base, beam_idx, slot, layers, groups, K, heads, T, RB, s);
  return kv_beam_reorder_launch<uint32_t>(base, beam_idx, slot, layers, groups, K, heads, T, RB, s);
}

JLA_BOUNDS_ACCESSOR(beam)

}  // namespace jla
