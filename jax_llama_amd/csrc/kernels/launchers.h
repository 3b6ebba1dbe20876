// Host launchers of the gfx950 kernels (pure HIP translation units; no torch headers).
// Every launcher returns 0 on success, <0 on a shape/argument error, >0 for a hipError_t.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "attn_plan.h"
#include "gemm_plan.h"
#include "gemv_plan.h"

namespace jla {
typedef uint16_t bf16_t;

int embedding(const int32_t* ids, const bf16_t* table, float* out, bf16_t* mirror, int M, int D, int V,
              hipStream_t s);
int rms_scale(const float* x, bf16_t* out, int M, int D, float eps, hipStream_t s);
int rms_scale_bf16(const bf16_t* x, bf16_t* out, int M, int D, float eps, hipStream_t s);
int rms_rowinv(const bf16_t* x, float* inv, int M, int D, float eps, hipStream_t s);  // inv[M] = 1/sqrt(mean(x^2)+eps)
int residual_add(float* h, const void* p, int p_bf16, bf16_t* hb, long long n, hipStream_t s);
int prefetch(const void* p, long long nbytes, int grid, unsigned* sink, hipStream_t s);
int stream_probe(const void* p, long long nbytes, int grid, unsigned* sink, hipStream_t s);  // bytes read: per-wave contiguous ranges
int gemm_f32(const float* x, const float* w, float* y, int M, int N, int K, hipStream_t s);
int rmsnorm(const float* x, const float* w, float* out, int M, int D, float eps, hipStream_t s);

// Epilogue arguments of the fused qkv projection (MODE_QKV): RoPE + KV-cache write.
struct QKVArgs {
  const float2* table;        // [table_len, Dh/2] (cos, sin)
  int table_len;
  union {
    const int32_t* positions;   // [M]
    const int32_t* lp_targets;  // MODE_LOGPROB: [M] global target columns (outside this shard / negative: ignored)
  };
  bf16_t* kc;                 // [B, Hkv, T, Dh] (this layer)
  bf16_t* vc;
  const int32_t* slot;        // device int32[1]: cache slot of sequence position 0
  int S, H, Hkv, Dh, T;       // tokens per sequence in this call, heads, kv heads, head dim, cache len
  bf16_t* q;                  // [M, H, Dh] rotated queries
  bf16_t* res_bf16;           // MODE_RESIDUAL: optional bf16 mirror of the updated residual (next A operand)
  bf16_t* pack;               // optional packed-layout copy (common.h pack_off) of the bf16 output: RESIDUAL -> the
                              // mirror, SWIGLU -> the activation (GEMV only; the next projection's packed-x input)
  const void* tp;             // MODE_TPRESID: the TP group's CarDevice (car.h) the partials are all-reduced through
  union {
    float* sk_ws;             // split-K GEMV variants (gemv.hip, 16 / 18 / 26): per-(group, split) partial slabs
    float* lp_tgt;            // MODE_LOGPROB: [M] the logit at the target column (zeroed by the launcher; written by the
  };                          //   one lane that holds it)
  int32_t* sk_tk;             //   and per-group tickets (zero-initialised once, reset by each group's last arriver)
  union {
    int sk_ws_floats;         //   slab buffer size (buffer-descriptor range)
    int lp_col_offset;        // MODE_LOGPROB: global column of this weight shard's column 0 (vocab-parallel TP)
  };
};
// The lp_* names of MODE_LOGPROB (gemm_logprob: no RoPE, no split) share the storage of fields that mode never uses: a
// larger struct changes the kernel-argument block, and with it the register allocation, of every kernel that takes one.

// MODE_TPRESID: granule bytes each workgroup of the fused row-parallel GEMV owns in every (parity, source rank) slot
constexpr int CAR_WG_COUNTERS = 4096;  // per-workgroup call counters of the fused GEMV (workgroups per launch)
constexpr long long TPRES_REGION = 64 * 64 * 4;  // up to 64 rows x 64 columns x 2 bf16 per 8-byte granule

// fused small-batch qkv projection + decode attention (gemv.hip qkv_attn_kernel): one launch; splits from
// qkv_attn_splits (0 = not applicable: run the two kernels); ws >= pairs * splits * rep * 132 floats, tickets >= pairs,
// sync >= qkv_attn_sync_ints() int32 (zeroed once, self-resetting). With o_w, the same launch also runs the o projection into the residual
// (o_mode MODE_RESIDUAL: h += out @ Wo^T + qo->res_bf16 / qo->pack mirrors; MODE_TPRESID: the TP granule exchange of
// qo->tp first); o_groups = qkv_attn_o_groups(...) (0: the o projection cannot be fused at this shape).
int qkv_attn_o_groups(int M, int rep, int N, int K);
size_t qkv_attn_sync_ints();
void qkv_attn_set_o_nt(int nt);  // o tiles per fused-o workgroup (1 / 2; tools, A/B)
int qkv_attn_splits(int M, int B, int Hkv, int rep, int t_cap, int N, int cus, int spl = 1, int o_groups = 0);
int qkv_attn_occupancy(int M, int rep, int spl = 1, int o_groups = 0);  // resident workgroups per CU it counts on
void qkv_attn_set_stamps(unsigned long long* p);  // tools: [grid][8] phase timestamps per workgroup (nullptr: off)
void qkv_attn_set_diag(int d);  // tests only: 1 = the qkv workgroups never publish (forces the timeout path)
int linear_qkv_attn(const bf16_t* x, const void* W, int M, int N, int K, float rms_eps, const QKVArgs& qa, bool xp,
                    bf16_t* out, bf16_t* out_pack, const int32_t* kv_start, float* ws, int32_t* tickets, int32_t* sync,
                    int t_cap, int splits, int spl, hipStream_t s,  // spl 2: K of the qkv GEMV over 2 (qa.sk_ws/sk_tk)
                    const void* o_w = nullptr, float* o_h = nullptr, int o_n = 0, int o_k = 0, int o_mode = 0,
                    const QKVArgs* qo = nullptr);
// Decode GEMV (gemv.hip): y = epilogue(x[M, K] @ W[N, K]^T), M <= 64, on the form the variant id names (gemv_plan.h:
// the variant table, and gemv_plan(), every rule of a legal call; -1 is its code). x is the packed copy for a packed-x
// id. -3: a split form's slabs (qkv->sk_ws / sk_tk, gemv_split_workspace_floats / gemv_split_tickets) are too small.
int linear_skinny(const void* x, int x_is_f32, const void* W, void* out, int M, int N, int K, int mode,
                  float rms_eps, int accumulate, int out_f32, const QKVArgs* qkv, int variant, hipStream_t s);
// FP8 (OCP e4m3fn) weight-only linears (gemv.hip): W8 is the weight in 16 x 64 blocks [N / 16][K / 64][64 lanes][16
// bytes], scale fp32 [N] one power of two per output row (W_deq = q * scale, exact in bf16).
// dequant_fp8: out = W_deq in the bf16 fragment-packed layout [N / 16][K / 32][64][8] (N % 16 == 0, K % 64 == 0).
// linear_skinny_w8: the decode GEMV on the fp8 bytes, y = epilogue(x @ W_deq^T), for the calls gemv_w8_plan()
// (gemv_plan.h) accepts; -1 is its code. qkv as linear_skinny (MODE_QKV's arguments, res_bf16 / pack mirrors).
int dequant_fp8(const void* W8, const float* scale, void* out, int N, int K, hipStream_t s);
int linear_skinny_w8(const void* x, int x_is_f32, const void* W8, const float* scale, void* out, int M, int N, int K,
                     int mode, float rms_eps, int accumulate, int out_f32, const QKVArgs* qkv, hipStream_t s);
// MXFP4 weight-only linears (gemv.hip): W4 is the e2m1 codes in 16 x 128 blocks [N / 16][K / 128][64 lanes][16 bytes]
// (two codes per byte, the lower k in the low nibble), S4 the e8m0 scale bytes [N / 16][K / 128][16 rows][4 k-steps]
// (W_deq = value(code) * 2^(byte - 127), exact in bf16). N % 16 == 0, K % 128 == 0.
// dequant_fp4: out = W_deq in the bf16 fragment-packed layout [N / 16][K / 32][64][8].
// linear_skinny_w4: the decode GEMV on the codes, y = epilogue(x @ W_deq^T), for the calls gemv_w4_plan() (gemv_plan.h)
// accepts; -1 is its code. qkv as linear_skinny.
int dequant_fp4(const void* W4, const void* S4, void* out, int N, int K, hipStream_t s);
int linear_skinny_w4(const void* x, int x_is_f32, const void* W4, const void* S4, void* out, int M, int N, int K,
                     int mode, float rms_eps, int accumulate, int out_f32, const QKVArgs* qkv, hipStream_t s);
int clock_probe(int iters, int grid, unsigned long long* out, hipStream_t s);  // [cycles, 100 MHz ticks]
// Tiled MFMA GEMM (gemm.hip): y = epilogue(x[M, K] @ W[N, K]^T) on the kernel the tile id names (gemm_plan.h: the
// tile table, and gemm_plan(), every rule of a legal call; the return codes -1 / -5 / -6 / -7 are its). ksplit > 1
// splits K over workgroups into fp32 partial slabs (ws >= ksplit * M * N floats, + ksplit * M under the fused norm;
// gemm5: for any split, gemm5_ksplit(K, ksplit) slabs; -3: too small) that gemm_reduce_kernel sums in fixed order before
// it runs the epilogue. gemm_ksplit / gemm_workspace_floats: the library's split heuristic and its workspace.
// rms_eps >= 0: x is the UNscaled activation and each output row is scaled by rsqrt(mean(x^2) + eps) (fused RMSNorm;
// not for MODE_RESIDUAL). rms_ws (>= M floats): a gemm4 plan without a K split computes the row statistic ahead of the
// GEMM into it (rms_rowinv) instead of inside its main loop; null: in-loop statistic.
// n_body (tail-balanced tiles): > 0 pins the body n-tile count, 0 takes gemm_tail_split(m-tiles, N, width, CUs).
// MODE_TPRESID: the row-parallel projection's split-K reduce with the TP all-reduce and residual add in its epilogue
// (out = h, mirror = hb, qkv->tp = the group's CarDevice; split plans only).
int gemm(const bf16_t* x, const void* W, void* out, int M, int N, int K, int mode, int accumulate, int out_f32,
         bf16_t* mirror, const QKVArgs* qkv, float* ws, size_t ws_floats, int ksplit, hipStream_t s,
         float rms_eps = -1.f, int tile = 0, float* rms_ws = nullptr, size_t rms_ws_floats = 0, int n_body = 0);
// gemm_plan()'s return code for this call on the current device (MODE_ARGMAX: as gemm_argmax() runs it)
int gemm_plan_check(int M, int N, int K, int mode, int rms, int ksplit, int tile, int has_rms_ws, int n_body);
int gemm_ksplit(int M, int N, int K);
size_t gemm_workspace_floats(int M, int N, int K);
int gemm_tp_groups(int M, int N);  // workgroups (= fused-exchange regions and call counters) of the MODE_TPRESID reduce
int gemm_qkv_direct_ok(int M, int tile, int K);  // qkv without a K split: the direct RoPE / KV-write GEMM epilogue applies
int gemm_num_cus();                // CUs of the current device (gemm_plan's `cus`)
void gemm_set_g4_default(int on);  // gemm_plan's `g4_default`: tile 0 runs gemm4 where it applies (on by default)
void gemm_set_g4_group(int gm);    // tools: m-tiles per group of gemm4's launch order (0: the default, 4)
void gemm5_set_diag(int d);        // tools only: gemm5 / gemm4 store ablations (wrong results)
// greedy lm_head: GEMM + first-max argmax epilogue (ws >= gemm_argmax_workspace_floats(M, N) floats)
int gemm_argmax(const bf16_t* x, const void* W, float* ws, size_t ws_floats, int M, int N, int K, float rms_eps,
                int32_t* idx, float* val, hipStream_t s, float* rms_ws = nullptr, size_t rms_ws_floats = 0);
size_t gemm_argmax_workspace_floats(int M, int N);
// first max per row over [M][P] (value, index) float2 partials
int argmax_partials(const float* part, int P, int M, int32_t* idx, float* val, hipStream_t s);
// scoring lm_head: GEMM + log-sum-exp epilogue. Per row of this weight shard: tgt = the logit at column
// targets[row] - col_offset (0 where that is outside [0, N)), mx = the row maximum, se = sum exp(logit - mx); the fp32
// logits are never written. ws >= gemm_logprob_workspace_floats(M, N) floats. -1 where gemm_plan() has no MODE_LOGPROB
// plan for the shape (the caller then runs the GEMM and logprob_rows).
int gemm_logprob(const bf16_t* x, const void* W, float* ws, size_t ws_floats, int M, int N, int K, float rms_eps,
                 const int32_t* targets, int col_offset, float* tgt, float* mx, float* se, hipStream_t s,
                 float* rms_ws = nullptr, size_t rms_ws_floats = 0);
size_t gemm_logprob_workspace_floats(int M, int N);

int rope_kv_write(const bf16_t* qkv, const float* table, int table_len, const int32_t* positions, bf16_t* kc,
                  bf16_t* vc, const int32_t* slot, int M, int S, int H, int Hkv, int Dh, int T, bf16_t* q_out,
                  hipStream_t s);

// decode attention: the process-wide knobs attn_decode() resolves its plan with (attn_plan.h AttnKnobs), the setters
// tests and tools move them with, and the way back to the defaults
const AttnKnobs& attn_knobs();
void attn_reset_knobs();
void attn_set_impl(int impl, int waves_target);  // impl 4: v2's (KPG 4, 2 slots) ring, no v4; waves_target: see there
void attn_set_v3_max_pairs(int n);
void attn_set_v3_kpg(int mult);
void attn_set_v5_max_pairs(int n);  // < 0: the default
void attn_set_v5_fold(int n);
void attn_set_v6(int mode);
void attn_set_v6_wpp(int wpp);
void attn_set_q8_waves(int waves);  // the fp8 KV cache's kernel: 1 / 8 waves per pair pinned; 0: by shape
void attn_set_q8_splits(int n);     // ... its key splits per pair: 0 by shape, 1 never, n > 1 pinned (the plan clamps it)
void attn_set_diag(int d);     // tools only: 1 = v2 / v4 stream K/V without the math (wrong results)
void attn_set_v6_diag(int d);  // tools only: v6 ablations (1 no compute, 2 no K loads, 4 no V DMAs; wrong results)
// bounds-checked debug build: per-translation-unit error words (JLA_BOUNDS_* bits; 0 in release builds)
unsigned jla_bounds_norm_embed(int reset);
unsigned jla_bounds_rope_kv(int reset);
unsigned jla_bounds_sample(int reset);
unsigned jla_bounds_gemm(int reset);
unsigned jla_bounds_gemv(int reset);
unsigned jla_bounds_attn_decode(int reset);
unsigned jla_bounds_attn_prefill(int reset);
// The launch attn_decode_plan() (attn_plan.h) resolves for (knobs, shape, key mask): nsplit must be the plan's, ws and
// tickets hold the plan's ws_floats / tickets (tickets zero-initialised once, self-resetting), out_pack only where the
// plan packs. Returns the plan's rc where it refuses; -2 / -3 for a wrong nsplit / an out_pack the plan does not write.
int attn_decode(const bf16_t* q, const bf16_t* kc, const bf16_t* vc, const int32_t* slot, const int32_t* kv_start,
                const uint8_t* key_mask, int mask_len, bf16_t* out, float* ws, int32_t* tickets, int B, int H,
                int Hkv, int Dh, int T, int t_cap, int nsplit, hipStream_t s, bf16_t* out_pack = nullptr);
// decode attention on the matrix cores (attn_decode_mma.hip) at the plan's waves per pair; launched by attn_decode
int attn_decode_v6(const bf16_t* q, const bf16_t* kc, const bf16_t* vc, const int32_t* slot, const int32_t* kv_start,
                   const uint8_t* key_mask, int mask_len, bf16_t* out, int B, int H, int Hkv, int T, int t_cap,
                   int wpp, hipStream_t s, bf16_t* out_pack);
// ---- the FP8 (e4m3) KV cache (kv8.hip): per layer q bytes uint8 [B, Hkv, T, 128] (natural element order) and one
// power-of-two fp32 scale per (row, kv head, slot) [B, Hkv, T], for K (post-RoPE) and for V
unsigned jla_bounds_kv8(int reset);
// rope_kv_write with the quantising store: q rotated to q_out as there; each k / v head row quantised by the rule of
// ops/reference.py quantize_fp8_rows from its bf16 value. Dh == 128.
int rope_kv_write_q8(const bf16_t* qkv, const float* table, int table_len, const int32_t* positions, uint8_t* kq,
                     float* ks, uint8_t* vq, float* vs, const int32_t* slot, int M, int S, int H, int Hkv, int Dh,
                     int T, bf16_t* q_out, hipStream_t s);
// slots [0, n) of every (row, kv head) pair -> bf16 kout / vout [pairs, n_out, 128] (n <= n_out; rows past n untouched)
int kv8_dequant(const uint8_t* kq, const float* ks, const uint8_t* vq, const float* vs, bf16_t* kout, bf16_t* vout,
                int pairs, int T, int n, int n_out, hipStream_t s);
// decode attention on the fp8 bytes, launched as attn_decode_q8_plan() (attn_plan.h) says; returns the plan's rc where
// it refuses. Where the plan splits the keys (nsplit > 1) ws / tickets hold the plan's ws_floats / tickets (tickets
// zero-initialised once, self-resetting), -2 if they do not; an unsplit launch ignores them.
int attn_decode_q8(const bf16_t* q, const uint8_t* kq, const float* ks, const uint8_t* vq, const float* vs,
                   const int32_t* slot, const int32_t* kv_start, const uint8_t* key_mask, int mask_len, bf16_t* out,
                   int B, int H, int Hkv, int Dh, int T, int t_cap, hipStream_t s, float* ws = nullptr,
                   size_t ws_floats = 0, int32_t* tickets = nullptr, int n_tickets = 0);
void attn_prefill_set_impl(int impl);  // 2 = GQA-shared MFMA 32x32 flash kernel (default), 1 = v1
int attn_prefill(const bf16_t* q, const bf16_t* kc, const bf16_t* vc, const int32_t* slot, const int32_t* kv_start,
                 const uint8_t* key_mask, int mask_len, bf16_t* out, int B, int S, int H, int Hkv, int Dh, int T,
                 hipStream_t s);

int argmax(const float* logits, int B, int V, int32_t* idx, float* val, hipStream_t s);
// the (tgt, mx, se) triple of gemm_logprob from stored fp32 logits [B, V]
int logprob_rows(const float* logits, int B, int V, const int32_t* targets, int col_offset, float* tgt, float* mx,
                 float* se, hipStream_t s);
// top-k / top-p sampler (topk_sample.hip): cv/ci [B, topk_chunks(V) * K] candidates
int topk_chunks(int V);
int topk_chunk(const float* logits, int B, int V, int K, int idx_offset, float* cv, int32_t* ci, hipStream_t s);
int topk_merge(const float* cv, const int32_t* ci, int B, int C, int K, int mode, float* out_v, int32_t* out_i,
               int32_t* nxt, float temperature, float top_p, uint64_t seed, const int32_t* step, hipStream_t s);
// custom xGMI collectives over IPC-mapped uncached buffers (allreduce.hip)
size_t car_buffer_bytes(long long max_bytes, int world);
int car_alloc(long long max_bytes, int world, void** buf, void** sig, hipIpcMemHandle_t* hbuf, hipIpcMemHandle_t* hsig);
void car_free(void* buf, void* sig);
int car_init(int rank, int world, long long max_bytes, void* own_buf, void* own_sig, const hipIpcMemHandle_t* hbufs,
             const hipIpcMemHandle_t* hsigs, double timeout_s, void** state);
// op 0: out = sum over ranks of in (bf16/fp32); op 1: h (fp32) += sum, hb (bf16) = h. two_shot: reduce-scatter +
// all-gather instead of every rank reading every peer's copy
int car_reduce(void* state, int op, const void* in, void* out, float* h, bf16_t* hb, long long nbytes, int is_bf16,
               int two_shot, hipStream_t s,
               bf16_t* hb_pack = nullptr, int pack_cols = 0);
// all-gather of (fp32, int32 + idx_offset) pairs: mode 0 = first max over ranks per pair, mode 1 = [n/k][world*k]
int car_pairs(void* state, int mode, const float* a, const int32_t* b, int idx_offset, long long n, int k,
              float* out_a, int32_t* out_b, hipStream_t s);
void car_set_gran_max(long long n);  // granule one-shot up to n payload bytes per rank (0: flag protocol only)
int car_error(void* state);
const void* car_device(void* state);      // the device-side CarDevice (car.h) of an instance (MODE_TPRESID)
long long car_max_bytes(void* state);
int car_world(void* state);
int car_set_grid(void* state, int grid);  // collective blocks per launch (0: the maximum; same on every rank, before first use)
void car_destroy(void* state);
int decode_update(const int32_t* nxt, int32_t* finished, int32_t* sequences, int32_t* cur_len, int32_t* tokens,
                  int32_t* positions, int32_t* slot, int B, int L, int pad, int eos, hipStream_t s);
// logits processors (logits_proc.hip), in place on fp32 logits [B, V] (V <= process_logits_max_v()): repetition
// penalty p (inv_p = fp32(1 / p)), no-repeat n-gram size n (0: off), suppress int32[64] and stop int32[8] (unused
// entries -1; the stop ids are banned while cur_len[0] < min_len[0]) over the history sequences[b, hist_start[b] :
// cur_len[0]]; vocab = the whole vocabulary, of which this rank holds columns [col_offset, col_offset + V).
// decode_update_set: decode_update with a device stop set int32[8]
unsigned jla_bounds_logits_proc(int reset);
int process_logits_max_v();
int process_logits(float* logits, int B, int V, const int32_t* sequences, int L, const int32_t* cur_len,
                   const int32_t* hist_start, int col_offset, int vocab, float p, float inv_p, int n,
                   const int32_t* suppress, const int32_t* stop, const int32_t* min_len, hipStream_t s);
int decode_update_set(const int32_t* nxt, int32_t* finished, int32_t* sequences, int32_t* cur_len, int32_t* tokens,
                      int32_t* positions, int32_t* slot, int B, int L, int pad, const int32_t* stop, hipStream_t s);
// beam search (beam.hip): the loop condition into alive[0]; one step of B items x K beams (alive[0] == 0: identity
// beam_idx, nothing else changes); every beam's cache rows follow its parent (one cache tensor [layers, groups * K,
// heads, T, RB bytes], slots below slot[0])
unsigned jla_bounds_beam(int reset);
int beam_alive(const float* running_score, const float* score, const int32_t* is_finished, const float* inv_pen,
               const int32_t* cur_len, int32_t* alive, int B, int K, int L, int S, int early, int never_full,
               hipStream_t s);
int beam_step(const float* cand_v, const int32_t* cand_i, const float* lse, int32_t* running_seq, int32_t* seq,
              float* running_score, float* score, int32_t* is_finished, const float* inv_pen, int32_t* cur_len,
              int32_t* slot, int32_t* tokens, int32_t* positions, const int32_t* alive, int32_t* beam_idx, int B,
              int K, int L, int S, int eos, int early, hipStream_t s);
int kv_beam_reorder(void* base, const int32_t* beam_idx, const int32_t* slot, int layers, int groups, int K,
                    int heads, int T, int RB, hipStream_t s);
// CU placement (placement.hip): CU-masked streams and a census of where a launch's workgroups run
int cu_census(uint32_t* out, int blocks, hipStream_t s);
int cu_mask_stream_create(const uint32_t* mask, int words, hipStream_t* out);
int cu_mask_stream_get(hipStream_t s, uint32_t* mask, int words);
int stream_destroy(hipStream_t s);
int graph_kernel_nodes(hipGraph_t g);  // kernel nodes of a captured graph (< 0: error)

}  // namespace jla
