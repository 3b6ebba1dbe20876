// Token selection and decode-loop bookkeeping (replaces HF FlaxGenerationMixin's loop body that the
// reference inherits: generation.py:28-41 -> _greedy_search / _sample).
//
// argmax: first index of the row maximum (jnp.argmax semantics), also returns the max value so a
//   vocab-parallel (TP) caller can pick the global winner from one (value, index) pair per rank.
// decode_update: finished rows emit pad, is_sent_finished |= (token == eos), sequences[:, cur_len]
//   = token, positions += 1, cache slot += 1, cur_len += 1 -- all on the device so the whole decode
//   step (model + sampler + state) replays from one hipGraph without host round trips.
#include "common.h"
#include "launchers.h"

namespace jla {

__global__ void __launch_bounds__(1024)
    argmax_kernel(const float* __restrict__ logits, int V, int32_t* __restrict__ idx, float* __restrict__ val) {
  __shared__ float sv[16];
  __shared__ int si[16];
  const int row = blockIdx.x;
  const float* x = logits + (size_t)row * V;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = threadIdx.x; i < V; i += blockDim.x) {
    const float v = x[i];
    if (v > bv) {  // strictly greater: keeps the first index within a thread's stride
      bv = v;
      bi = i;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    sv[wid] = bv;
    si[wid] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
    for (int w = 1; w < nw; ++w)
      if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) {
        bv = sv[w];
        bi = si[w];
      }
    idx[row] = bi == 0x7fffffff ? 0 : bi;
    val[row] = bv;
  }
}

int argmax(const float* logits, int B, int V, int32_t* idx, float* val, hipStream_t s) {
  if (B <= 0) return 0;
  argmax_kernel<<<B, 1024, 0, s>>>(logits, V, idx, val);
  JLA_CHECK_LAUNCH();
  return 0;
}

// Scoring from stored fp32 logits (the unfused form of gemm_logprob, gemm.hip): one workgroup per row; tgt = the logit
// at column targets[row] - col_offset (0 where that is outside [0, V): an ignored label, another rank's shard), mx =
// the row maximum, se = sum exp(logit - mx). Two passes over the row (the second one reads it from the caches), fixed
// reduction order.
__global__ void __launch_bounds__(1024)
    logprob_rows_kernel(const float* __restrict__ logits, int V, const int32_t* __restrict__ targets, int col_offset,
                        float* __restrict__ tgt, float* __restrict__ mx, float* __restrict__ se) {
  __shared__ float sm[16];
  __shared__ float ssum[16];
  constexpr float LOG2E = 1.4426950408889634f;
  const int row = blockIdx.x;
  const float* x = logits + (size_t)row * V;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  float m = -INFINITY;
  for (int i = threadIdx.x; i < V; i += blockDim.x) m = fmaxf(m, x[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if (lane == 0) sm[wid] = m;
  __syncthreads();
  m = sm[0];
  for (int w = 1; w < nw; ++w) m = fmaxf(m, sm[w]);
  float s = 0.f;
  if (m != -INFINITY) {  // (never inf - inf)
    for (int i = threadIdx.x; i < V; i += blockDim.x) s += __builtin_amdgcn_exp2f((x[i] - m) * LOG2E);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) ssum[wid] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < nw; ++w) s += ssum[w];
    const int col = targets[row] - col_offset;
    tgt[row] = col >= 0 && col < V ? x[col] : 0.f;
    mx[row] = m;
    se[row] = s;
  }
}

int logprob_rows(const float* logits, int B, int V, const int32_t* targets, int col_offset, float* tgt, float* mx,
                 float* se, hipStream_t s) {
  if (B <= 0) return 0;
  if (V <= 0) return -1;
  logprob_rows_kernel<<<B, 1024, 0, s>>>(logits, V, targets, col_offset, tgt, mx, se);
  JLA_CHECK_LAUNCH();
  return 0;
}

__global__ void decode_update_kernel(const int32_t* __restrict__ nxt, int32_t* __restrict__ finished,
                                     int32_t* __restrict__ sequences, int32_t* __restrict__ cur_len,
                                     int32_t* __restrict__ tokens, int32_t* __restrict__ positions,
                                     int32_t* __restrict__ slot, int B, int L, int pad, int eos) {
  const int cl = cur_len[0];
  for (int b = threadIdx.x; b < B; b += blockDim.x) {  // one workgroup: any batch size
    int t = nxt[b];
    const int fin = finished[b];
    if (fin) t = pad;
    finished[b] = (fin || t == eos) ? 1 : 0;
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

int decode_update(const int32_t* nxt, int32_t* finished, int32_t* sequences, int32_t* cur_len, int32_t* tokens,
                  int32_t* positions, int32_t* slot, int B, int L, int pad, int eos, hipStream_t s) {
  if (B <= 0) return -1;
  decode_update_kernel<<<1, min(1024, ((B + 63) / 64) * 64), 0, s>>>(nxt, finished, sequences, cur_len, tokens, positions, slot,
                                                          B, L, pad, eos);
  JLA_CHECK_LAUNCH();
  return 0;
}

JLA_BOUNDS_ACCESSOR(sample)

}  // namespace jla
