// The two state kernels of prompt-lookup speculative decoding (runtime/engine.py LookupEngine; the definitions are
// ops/reference.py prompt_lookup / spec_accept, which these match exactly). Both read only device state -- the
// sequences, cur_len, the history starts, the stop set -- so one captured step serves every call.
//
// prompt_lookup: one wave per row. HF's PromptLookupCandidateGenerator rule with a fixed draft count: for n =
//   max_ngram .. 1 the earliest p in [hist_start, cur_len - n) whose n tokens equal the row's last n (p < cur_len - n,
//   so at least one token follows the match); the k tokens after it are the drafts, a shorter continuation and a row
//   without a match fill with the row's last token. The lanes test 64 consecutive p at a time; the first lane of the
//   first chunk with a hit is the earliest match.
// spec_accept: one wave, row r = lane (B <= 64). a_r = the leading drafts that equal the verify step's greedy tokens;
//   the whole batch advances by n = 1 + min a_r over unfinished rows (k if none is left), clamped to max_length -
//   cur_len: the project keeps ONE slot counter. Every row appends tgt[r, 0 .. n - 1] (pad after a stop id, as
//   decode_update_set does for one token), then tokens[:, 0], the positions of all k + 1 columns, cur_len and the slot
//   counter move by n. n = 0 (the buffer is full) changes nothing, so a replay past the end is safe.
#include "common.h"
#include "launchers.h"

namespace jla {

namespace {
constexpr int SPEC_STOP = 8;       // ops.PROC_MAX_STOP
constexpr int SPEC_MAX_ROWS = 64;  // one wave of rows
}  // namespace

__global__ void __launch_bounds__(64)
    prompt_lookup_kernel(const int32_t* __restrict__ sequences, const int32_t* __restrict__ cur_len,
                         const int32_t* __restrict__ hist_start, int32_t* __restrict__ tokens, int L, int k,
                         int max_ngram) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int cl = cur_len[0];
  if (cl < 1 || cl > L) {
    JLA_FLAG(JLA_BOUNDS_SEQ);
    cl = cl < 1 ? 1 : L;
  }
  const int32_t* row = sequences + (size_t)b * L;
  const int hs = min(max(hist_start[b], 0), cl);
  const int32_t last = row[cl - 1];
  int found = -1, fn = 0;
  for (int n = max_ngram; n >= 1 && found < 0; --n) {
    const int end = cl - n;  // p in [hs, end)
    for (int p0 = hs; p0 < end; p0 += 64) {  // (wave-uniform bounds)
      const int p = p0 + lane;
      bool ok = p < end;
      for (int i = 0; ok && i < n; ++i) ok = row[p + i] == row[end + i];
      const unsigned long long hits = __ballot(ok);
      if (hits) {
        found = p0 + __builtin_ctzll(hits);
        fn = n;
        break;
      }
    }
  }
  if (lane < k) {
    const int src = found + fn + lane;
    tokens[(size_t)b * (k + 1) + 1 + lane] = (found >= 0 && src < cl) ? row[src] : last;
  }
}

__global__ void __launch_bounds__(64)
    spec_accept_kernel(const int32_t* __restrict__ tgt, int32_t* __restrict__ finished, int32_t* __restrict__ sequences,
                       int32_t* __restrict__ cur_len, int32_t* __restrict__ tokens, int32_t* __restrict__ positions,
                       int32_t* __restrict__ slot, int B, int L, int k, int pad, const int32_t* __restrict__ stop) {
  const int r = threadIdx.x, S = k + 1;
  const int cl = cur_len[0];
  int32_t st[SPEC_STOP];
#pragma unroll
  for (int j = 0; j < SPEC_STOP; ++j) st[j] = stop[j];
  const bool row = r < B;
  int fin = row ? (finished[r] != 0) : 1;
  int a = k;  // finished rows and the lanes past B do not bound the advance
  if (!fin) {
    a = 0;
    while (a < k && tokens[r * S + 1 + a] == tgt[r * S + a]) ++a;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = min(a, __shfl_xor(a, o, 64));
  const int n = max(min(1 + a, L - cl), 0);
  if (row && n > 0) {
    int32_t t = pad;
    for (int i = 0; i < n; ++i) {
      t = fin ? pad : tgt[r * S + i];
      bool hit = false;
#pragma unroll
      for (int j = 0; j < SPEC_STOP; ++j) hit = hit || t == st[j];
      fin = (fin || hit) ? 1 : 0;
      sequences[(size_t)r * L + cl + i] = t;
    }
    finished[r] = fin;
    tokens[r * S] = t;
    const int p0 = positions[r * S] + n;
    for (int s = 0; s < S; ++s) positions[r * S + s] = p0 + s;
  }
  __syncthreads();  // every thread has read cur_len before it advances
  if (r == 0) {
    cur_len[0] = cl + n;
    slot[0] += n;
  }
}

int prompt_lookup(const int32_t* sequences, const int32_t* cur_len, const int32_t* hist_start, int32_t* tokens, int B,
                  int L, int k, int max_ngram, hipStream_t s) {
  if (B <= 0 || B > 65535 || L < 1 || k < 1 || k > 63 || max_ngram < 1) return -1;
  prompt_lookup_kernel<<<B, 64, 0, s>>>(sequences, cur_len, hist_start, tokens, L, k, max_ngram);
  JLA_CHECK_LAUNCH();
  return 0;
}

int spec_accept(const int32_t* tgt, int32_t* finished, int32_t* sequences, int32_t* cur_len, int32_t* tokens,
                int32_t* positions, int32_t* slot, int B, int L, int k, int pad, const int32_t* stop, hipStream_t s) {
  if (B <= 0 || B > SPEC_MAX_ROWS || L < 1 || k < 1) return -1;
  spec_accept_kernel<<<1, 64, 0, s>>>(tgt, finished, sequences, cur_len, tokens, positions, slot, B, L, k, pad, stop);
  JLA_CHECK_LAUNCH();
  return 0;
}

JLA_BOUNDS_ACCESSOR(spec)

}  // namespace jla
