// Logits processors of the decode loop, between "logits" and "token" (the definition is the README's "Logits
// processors" section and ops/reference.py process_logits, which process_logits_kernel matches bit for bit).
//
// process_logits: one workgroup per row, in place on this rank's fp32 logits [B, V]. The work is a scatter over the
//   row's token history H = sequences[b, hist_start[b] : cur_len], never a sweep over V:
//     1. repetition penalty: an LDS bitmap of V bits; threads stride over H and atomicOr their token's bit, and the
//        thread that finds it clear owns the token (each distinct token is scaled once, whichever duplicate wins);
//     2. after a barrier, the masks, which all store -inf and commute: the no-repeat n-gram ban (threads stride over
//        the start i of every earlier n-gram and compare its first n - 1 tokens with the history's last n - 1), the
//        suppress list, and the stop ids while cur_len is below the minimum-length word.
//   Everything that changes between calls without a new capture is read from device words (cur_len, hist_start, the
//   minimum length, the suppress and stop ids); p, 1/p and n are launch arguments. Plain vector stores only.
// decode_update_set: decode_update (sample.hip) with the stop ids read from a device int32[8] (unused entries -1).
#include "common.h"
#include "launchers.h"

namespace jla {

namespace {
constexpr int PROC_THREADS = 256;
constexpr int PROC_MAX_V = 1 << 19;  // bitmap bits: 64 KiB of LDS, what a launch gets without opting in to more
constexpr int PROC_SUPPRESS = 64;
constexpr int PROC_STOP = 8;
}  // namespace

__global__ void __launch_bounds__(PROC_THREADS)
    process_logits_kernel(float* __restrict__ logits, int V, const int32_t* __restrict__ sequences, int L,
                          const int32_t* __restrict__ cur_len, const int32_t* __restrict__ hist_start, int col_offset,
                          int vocab, float p, float inv_p, int n, const int32_t* __restrict__ suppress,
                          const int32_t* __restrict__ stop, const int32_t* __restrict__ min_len) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) uint32_t seen[];  // V bits
  const int b = blockIdx.x, tid = threadIdx.x;
  float* x = logits + (size_t)b * V;
  const int c = cur_len[0];
  int cl = c, hs = hist_start[b];
  if (cl < 0 || cl > L) {
    JLA_FLAG(JLA_BOUNDS_SEQ);
    cl = cl < 0 ? 0 : L;
  }
  hs = hs < 0 ? 0 : (hs > cl ? cl : hs);
  const int32_t* h = sequences + (size_t)b * L + hs;
  const int len = cl - hs;
  if (p != 1.0f) {
    const int words = (V + 31) >> 5;
    for (int w = tid; w < words; w += PROC_THREADS) seen[w] = 0u;
    __syncthreads();
    for (int i = tid; i < len; i += PROC_THREADS) {
      const int t = h[i];
      if (t < 0 || t >= vocab) {
        JLA_FLAG(JLA_BOUNDS_TOKEN);
        continue;
      }
      const int col = t - col_offset;
      if (col < 0 || col >= V) continue;  // another rank's shard
      const uint32_t bit = 1u << (col & 31);
      if ((atomicOr(&seen[col >> 5], bit) & bit) == 0u) {
        const float l = x[col];
        x[col] = l > 0.f ? __fmul_rn(l, inv_p) : __fmul_rn(l, p);
      }
    }
  }
  __syncthreads();  // the masks overwrite penalised logits: every penalty store comes first
  if (n >= 1 && len >= n) {
    const int32_t* suf = h + (len - n + 1);  // the history's last n - 1 tokens
    for (int i = tid; i + n <= len; i += PROC_THREADS) {
      bool same = true;
      for (int j = 0; j < n - 1 && same; ++j) same = h[i + j] == suf[j];
      if (!same) continue;
      const int t = h[i + n - 1];
      if (t < 0 || t >= vocab) {
        JLA_FLAG(JLA_BOUNDS_TOKEN);
        continue;
      }
      const int col = t - col_offset;
      if (col >= 0 && col < V) x[col] = -INFINITY;
    }
  }
  if (tid < PROC_SUPPRESS) {
    const int col = suppress[tid] - col_offset;
    if (suppress[tid] >= 0 && col >= 0 && col < V) x[col] = -INFINITY;
  } else if (tid < PROC_SUPPRESS + PROC_STOP) {
    const int t = stop[tid - PROC_SUPPRESS], col = t - col_offset;
    if (c < min_len[0] && t >= 0 && col >= 0 && col < V) x[col] = -INFINITY;
  }
}

int process_logits(float* logits, int B, int V, const int32_t* sequences, int L, const int32_t* cur_len,
                   const int32_t* hist_start, int col_offset, int vocab, float p, float inv_p, int n,
                   const int32_t* suppress, const int32_t* stop, const int32_t* min_len, hipStream_t s) {
  if (B <= 0) return 0;
  if (V <= 0 || V > PROC_MAX_V || L <= 0 || n < 0 || col_offset < 0 || vocab < V || !(p > 0.f)) return -1;
  const size_t lds = (size_t)((V + 31) >> 5) * sizeof(uint32_t);
  process_logits_kernel<<<B, PROC_THREADS, lds, s>>>(logits, V, sequences, L, cur_len, hist_start, col_offset, vocab,
                                                     p, inv_p, n, suppress, stop, min_len);
  JLA_CHECK_LAUNCH();
  return 0;
}

int process_logits_max_v() { return PROC_MAX_V; }

__global__ void decode_update_set_kernel(const int32_t* __restrict__ nxt, int32_t* __restrict__ finished,
                                         int32_t* __restrict__ sequences, int32_t* __restrict__ cur_len,
                                         int32_t* __restrict__ tokens, int32_t* __restrict__ positions,
                                         int32_t* __restrict__ slot, int B, int L, int pad,
                                         const int32_t* __restrict__ stop) {
  const int cl = cur_len[0];
  int32_t st[PROC_STOP];
#pragma unroll
  for (int j = 0; j < PROC_STOP; ++j) st[j] = stop[j];
  for (int b = threadIdx.x; b < B; b += blockDim.x) {  // one workgroup: any batch size
    int t = nxt[b];
    const int fin = finished[b];
    if (fin) t = pad;
    bool hit = false;
#pragma unroll
    for (int j = 0; j < PROC_STOP; ++j) hit = hit || t == st[j];
    finished[b] = (fin || hit) ? 1 : 0;
    if (cl < L)
      sequences[(size_t)b * L + cl] = t;
    else
      JLA_FLAG(JLA_BOUNDS_SEQ);
    tokens[b] = t;
    positions[b] += 1;
  }
  __syncthreads();  // every thread has read cur_len before it advances
  if (threadIdx.x == 0) {
    cur_len[0] = cl + 1;
    slot[0] += 1;
  }
}

int decode_update_set(const int32_t* nxt, int32_t* finished, int32_t* sequences, int32_t* cur_len, int32_t* tokens,
                      int32_t* positions, int32_t* slot, int B, int L, int pad, const int32_t* stop, hipStream_t s) {
  if (B <= 0) return -1;
  decode_update_set_kernel<<<1, min(1024, ((B + 63) / 64) * 64), 0, s>>>(nxt, finished, sequences, cur_len, tokens,
                                                                         positions, slot, B, L, pad, stop);
  JLA_CHECK_LAUNCH();
  return 0;
}

JLA_BOUNDS_ACCESSOR(logits_proc)

}  // namespace jla
