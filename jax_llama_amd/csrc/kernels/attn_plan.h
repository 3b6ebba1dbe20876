// The plan of one decode-attention launch (attn_decode.hip / attn_decode_mma.hip: one query position per sequence):
// every rule that decides whether a shape is served, which of the five kernels runs it and with what geometry lives in
// attn_decode_plan() below, in one order. Plain C++ (no HIP headers): the launcher, the bindings (attn_decode_plan_check),
// ops.attention / ops.attention_packs and the tests all ask this one function.
#pragma once

#include <cstddef>

#include "gemv_plan.h"  // SKINNY_MAX_M: the decode GEMV's rows, up to which the o projection reads a packed copy

namespace jla {

constexpr int ATTN_DH = 128;               // the only head dim the kernels are built for
constexpr int ATTN_PART_FLOATS = ATTN_DH + 4;  // a key split's partial per head, [m, l, 0, 0, o[128]] (attn_merge.h)
constexpr int ATTN_V2_MIN_PAIRS = 4096;    // v2 / v4 stream whole (row, kv head) pairs from here (B = 512 at 8 kv heads)
constexpr int ATTN_MASK_PACK_MAX_B = 32;   // with a key mask, no packed copy above this many rows (the last rule below)

// Every tunable of the dispatch, defaults written once. One process-wide instance (attn_decode.hip: the attn_set_*
// setters write it, attn_reset_knobs() restores this state). The *_diag ablation switches are not here: they are
// tool-only, give wrong results and are not part of a plan.
struct AttnKnobs {
  int v6_mode = 1;          // 0 off, 1 where it wins (by shape), 2 every decode shape it supports (A/B, tests)
  int v6_wpp = 0;           // v6 waves per (row, kv head) pair pinned to 1 / 2 / 4 / 8 (A/B); 0 = by pairs
  int v5_max_pairs = 64;    // v5 up to this many pairs, 4 x that at rep >= 8 (0: off)
  int v5_fold = 0;          // v5 splits the last arriver merges per load round pinned to 4 / 12 (A/B); 0 = by pairs
  int v3_max_pairs = 4096;  // v3 up to this many pairs (0: off): up to the v2 threshold
  int v3_kpg_mult = 0;      // v3 key rows per lane group per chunk = (8 / rep) x 1 / 2 / 4 (A/B); 0 = by pairs
  int v2_min_pairs = ATTN_V2_MIN_PAIRS;  // v2 / v4 from this many pairs (attn_set_impl(.., -n): down to n, A/B)
  int waves_target = 2048;  // v2 splits the keys until pairs x splits reaches this many waves
  bool v4 = true;           // the register-ring stream (v4); impl 4 turns it off (v2 everywhere v4 would run)
  bool v2_kpg4 = false;     // impl 4: v2's (KPG 4, 2 slots) ring at rep <= 4 for every size, not only from 16384 pairs
  int q8_waves = 0;         // the fp8 KV cache's kernel (attn_decode_q8_plan): waves per pair pinned to 1 / 8; 0 = by shape
  int q8_splits = 0;        // ... its key splits per pair: 0 = by shape, 1 = never, n > 1 pinned (clamped to the chunks of t_cap)
};

enum AttnKernel { ATTN_V2 = 2, ATTN_V3, ATTN_V4, ATTN_V5, ATTN_V6 };
inline const char* attn_kernel_name(AttnKernel k) {
  static const char* const names[] = {"v2", "v3", "v4", "v5", "v6"};
  return names[k - ATTN_V2];
}

struct AttnPlan {
  AttnKernel kernel;
  int rep;         // query heads per kv head
  int kpg;         // v2 / v3 / v4 / v5: key rows per lane group per chunk (0 for v6)
  int ring;        // v4: register-ring slots U; v2: LDS-ring slots NS (0 elsewhere)
  int fold;        // v5: splits merged per load round, 4 or 12 (0 elsewhere)
  int wpp;         // v6: waves per pair (0 elsewhere)
  int nsplit;      // key splits per pair (the launch's nsplit argument must equal it)
  int split_len;   // v2: keys per split, a multiple of 32 (0 elsewhere)
  bool packs;      // this launch may also write the packed copy the o projection's packed-x GEMV reads
  size_t ws_floats;  // the workspace the launch is given holds at least this many floats ...
  int tickets;       // ... and this many zero-initialised int32 tickets (self-resetting); see the last rule
};
struct AttnPlanResult {
  int rc;           // 0 legal; -1 not (-2 / -3, a wrong nsplit / a packed copy the plan does not write: attn_decode's)
  const char* why;  // the rule that refused the call
  AttnPlan plan;
};

// One kernel per regime, asked in this order; pairs = B x Hkv (row, kv head) pairs, rep = H / Hkv:
//   v6  matrix-core scores / P.V, one workgroup per pair, no workspace (attn_decode_mma.hip)
//   v5  keys split over 4-wave workgroups, last arriver merges -- the latency-bound B = 1..8 steps
//   v3  one 8-wave workgroup per pair, no cross-workgroup merge -- mid batches
//   v4  one wave per pair, register ring, one split, no key mask -- large batches (the B = 2048 headline)
//   v2  one wave per (pair, key split), LDS ring, optional key mask -- large batches with a padding mask, and every
//       other shape (rep 16 mid batches, long contexts at few pairs once v3 / v5 are off)
// masked: the launch gets a key mask. t_cap: the key slots the launch covers.
inline AttnPlanResult attn_decode_plan(const AttnKnobs& k, int B, int H, int Hkv, int Dh, int t_cap, bool masked) {
  const auto fail = [](const char* why) { return AttnPlanResult{-1, why, AttnPlan{}}; };
  if (Dh != ATTN_DH) return fail("head dim: Dh == 128");
  if (H < 1 || Hkv < 1 || H % Hkv) return fail("GQA: H a positive multiple of Hkv");
  const int rep = H / Hkv, pairs = B * Hkv;
  if (rep > 16 || (rep & (rep - 1))) return fail("query heads per kv head: 1, 2, 4, 8 or 16");
  AttnPlan p{};
  p.rep = rep, p.nsplit = 1;
  if (B <= 0) return {0, "", p};  // nothing to launch

  // ---- v6. By shape (graph-timed with cold K/V, profiles/r5_attn_decode_v6_ab.jsonl): at rep >= 8 from 8 up to (not
  // including) 2048 pairs -- Llama-3-70B at MP 8, B = 32 / 256: 12.9 / 28.8 -> 10.2 / 14.1 us; MP 1, B = 32: 39.0 ->
  // 18.7 -- the VALU kernels there are compute-bound on the 8 q heads of a pair; v4 keeps rep 8 from 2048 pairs (MP 1,
  // B = 256: 80 vs 94 us) and every rep <= 4 shape (v4 / v3 / v5 stream those faster).
  if (k.v6_mode == 2 || (k.v6_mode == 1 && rep >= 8 && pairs >= 8 && pairs < 2048)) {
    p.kernel = ATTN_V6;
    // enough workgroups to cover the CUs, fewer waves (less merge) for many pairs: 2 waves were best or tied from 1 to
    // 256 pairs (r5_attn_decode_v6_ab.jsonl)
    p.wpp = k.v6_wpp ? k.v6_wpp : (pairs >= 4096 ? 1 : 2);
    p.packs = true;
  }
  // ---- v5, ahead of v3 (tools/bench_attn_decode.py, profiles/r3_attn_decode_v5_vs_v3.jsonl: at rep 8 -- Llama-3-70B
  // at MP 8 -- v3 is compute-bound on one CU per pair, so v5 wins 1.5-2x up to 32 pairs and further; at rep 4 --
  // Llama-3-8B -- the two tie at 64 pairs and v3 wins at 128). One split is one 16 x KPG-key workgroup.
  else if (pairs <= k.v5_max_pairs || (rep >= 8 && pairs <= 4 * k.v5_max_pairs)) {
    p.kernel = ATTN_V5;
    p.kpg = rep >= 16 ? 1 : (rep == 8 ? 2 : (rep == 4 ? 4 : 8));
    p.nsplit = (t_cap + 16 * p.kpg - 1) / (16 * p.kpg);
    // all of a round's partial loads in flight together: 12 from 16 pairs on (70B MP 8 B = 32 T = 384: 13.9 -> 12.8
    // us) and 4 below (B = 1: 8.8 vs 9.4 us; profiles/r3_attn_decode_v5_fold_ab.jsonl)
    p.fold = k.v5_fold ? k.v5_fold : (pairs < 16 ? 4 : 12);
    p.packs = true;
  } else {
    // ---- the v2 / v4 range: from v2_min_pairs up, or the mid-batch rule. The one-split register-ring stream (v4)
    // also serves batches below the v2 threshold: at rep <= 4 above 32 rows, at rep 8 from 2048 pairs. Graph-timed
    // with cold K/V (profiles/r3_attn_decode_v4_midbatch.jsonl): Llama-3-8B B = 128 / 256 (T 384) 71.9 / 129 us (v3)
    // -> 57.9 / 70.5; Llama-3-70B B = 256 (T 256 / 384) 158 / 206 -> 87 / 125; v3 stays ahead at rep 8 below 2048
    // pairs. Off while attn_set_impl moves the v2 threshold (A/B runs compare v2 / v4 with v3 there).
    const bool midbatch = k.v4 && k.v2_min_pairs == ATTN_V2_MIN_PAIRS &&
                          ((rep <= 4 && B > 32) || (rep == 8 && pairs >= 2048));
    // ---- v3: faster than the split kernels at B = 1..256 (8 kv heads)
    if (rep <= 8 && !(pairs >= k.v2_min_pairs || midbatch) && pairs <= k.v3_max_pairs) {
      p.kernel = ATTN_V3;
      // key rows per lane group per chunk = base (rep x KPG = 8) x mult, at most 8 rows and rep x KPG <= 16 (no
      // spills): fewer, larger chunks = fewer dependent load round trips on the latency-bound small-batch path. By
      // size: x2 up to 128 pairs (B <= 16 at 8 kv heads: B = 1 T = 384 12.4 -> 11.0 us, B = 8 12.8 -> 11.3, B = 1
      // T = 1024 25.2 -> 22.1), x1 above (B = 32 / 64 slightly faster at x1; profiles/r2_attn_decode_v3_kpg_ab.jsonl)
      const int mult = k.v3_kpg_mult ? k.v3_kpg_mult : (pairs <= 128 ? 2 : 1);
      const int cap = 16 / rep < 8 ? 16 / rep : 8;
      p.kpg = (8 / rep) * mult < cap ? (8 / rep) * mult : cap;
      p.packs = true;
    } else {
      // splits only when the pairs alone cannot fill the chip (few pairs / long context): enough for waves_target
      // waves, at least 64 keys each; the mid-batch rule means one split
      if (!midbatch) {
        const int max_split = t_cap > 64 ? (t_cap + 63) / 64 : 1;
        const int ns = (k.waves_target + pairs - 1) / pairs;
        p.nsplit = ns < 1 ? 1 : (ns > max_split ? max_split : ns);
      }
      // ---- v4: 5-12 % faster than v2 at B = 512-2048 (profiles/r2_attn_decode_v4_vs_v2.jsonl). It has no split
      // merge and no mask path.
      if (k.v4 && p.nsplit == 1 && !masked && rep <= 8) {
        p.kernel = ATTN_V4;
        // rep 8 (Llama-3-70B): twice the q / o registers of rep 4, so 8-key chunks, 3 in flight (16-key chunks x 3
        // slots at rep 8 fail the ring check: the compiler reuses in-flight ring registers)
        p.kpg = rep == 8 ? 2 : 4, p.ring = rep == 8 ? 4 : 3;
        // v3 stays ahead at B <= 64, where the o projection is a GEMV: there v4 runs only under the mid-batch rule,
        // and writes the packed copy that GEMV reads
        p.packs = midbatch && B <= SKINNY_MAX_M;
      } else {
        // ---- v2: everything else. The ring by size at rep <= 4: from 16384 pairs (B >= 2048 at 8 kv heads) the
        // 17-KiB (KPG 4, 2 slots) ring -- 9 waves per CU instead of 4 -- streams 5.4-5.8 TB/s against 4.0-5.6 for
        // (KPG 8, 2 slots), which stays best at B = 1024 (profiles/r2_attn_decode_b2048_geometry.jsonl)
        p.kernel = ATTN_V2;
        p.kpg = rep <= 4 ? ((k.v2_kpg4 || pairs >= 16384) ? 4 : 8) : (rep == 8 ? 2 : 1);
        p.ring = rep <= 4 ? 2 : 4;
        p.split_len = ((t_cap + p.nsplit - 1) / p.nsplit + 31) / 32 * 32;
        p.packs = false;
      }
    }
  }
  // ---- the conservative mask rule: with a key mask, no packed copy above 32 rows, whichever kernel runs. v6 / v5 /
  // v3 could write it there; the rule predates them and stays because removing it would change which GEMV form the o
  // projection runs at those shapes.
  if (masked && B > ATTN_MASK_PACK_MAX_B) p.packs = false;
  // ---- the buffers: one size per (shape, splits), whichever kernel runs. v5 publishes [m, l, 0, 0, o[128]] per head
  // and split, the largest layout (v2: [m, l, o[128]], and only with more than one split; v3 / v4 / v6 publish
  // nothing), and one ticket per pair. It is what the callers always allocated: sizing each kernel exactly (nothing for
  // v4 at the headline shape) moves every later allocation, and measured 0.3 % slower on the headline in two sessions
  // (profiles/attn_plan_resolver_headline.jsonl).
  p.ws_floats = (size_t)B * H * p.nsplit * ATTN_PART_FLOATS;
  p.tickets = pairs;
  return {0, "", p};
}

// ---- the FP8 (e4m3) KV cache (kv8.hip): one kernel template, attn_decode_q8_kernel, straight on the fp8 bytes: one
// workgroup per (row, kv head) pair, or -- few pairs with a long context -- one per (pair, key split) with a
// last-arriver merge; no packed copy. Every rule of that launch:
constexpr int ATTN_Q8_ONE_WAVE_MIN_PAIRS = 2048;  // one wave per pair from here (B = 256 at 8 kv heads); see the rule
constexpr int ATTN_Q8_SPLIT_WGS = 256;            // key splits until pairs x splits reaches this many workgroups ...
constexpr int ATTN_Q8_SPLIT_MIN_CHUNKS = 4;       // ... of at least this many chunks of t_cap each; see the rule
constexpr int ATTN_Q8_MAX_SPLITS = 64;            // what a pinned count is cut to (the merge is one workgroup's)
struct AttnQ8Plan {
  int rep;     // query heads per kv head
  int waves;   // waves per pair: 8 (v3's structure) or 1 (large batches, as v4 serves them for bf16)
  int kpg;     // key rows per lane group per chunk
  int nsplit;  // key splits per pair (1: the unsplit launch, no workspace); only with 8 waves
  size_t ws_floats;  // nsplit > 1: the launch is given this many floats, [m, l, 0, 0, o[128]] per head and split ...
  int tickets;       // ... and this many zero-initialised int32 tickets, one per pair (self-resetting); 0 / 0 unsplit
};
struct AttnQ8PlanResult {
  int rc;           // 0 legal; -1 not
  const char* why;  // the rule that refused the call
  AttnQ8Plan plan;
};

#if defined(__HIPCC__)
#define JLA_PLAN_HD __host__ __device__
#else
#define JLA_PLAN_HD
#endif
// The keys of one split of the 8-wave kernel. The valid keys [lo, hi) of a pair are device state (kv_start, the slot),
// so the splits cut them, not the cache: the chunks (ch = 32 kpg keys, aligned to multiples of ch as the unsplit
// stream's are) from the one that holds lo to the one that holds hi - 1 are dealt out per = ceil(chunks / nsplit) at a
// time, split s takes chunks [s per, min((s + 1) per, chunks)), and n_act = ceil(chunks / per) <= nsplit splits get
// any. A split with s >= n_act has no keys; lo >= hi gives n_act = 0. Called by the kernel (every workgroup of a pair
// computes the same n_act: it is what the ticket counts to) and, through attn_q8_split_ranges, by the tests.
struct AttnQ8SplitRange {
  int n_act;      // the splits of this pair that hold keys
  int c_begin;    // the first chunk's first key, a multiple of ch (<= key_begin)
  int key_begin;  // the split's keys [key_begin, key_end), within [lo, hi); empty for s >= n_act
  int key_end;
};
JLA_PLAN_HD inline AttnQ8SplitRange attn_q8_split_range(int lo, int hi, int ch, int nsplit, int s) {
  AttnQ8SplitRange r{0, 0, 0, 0};
  if (lo < 0) lo = 0;
  if (lo >= hi || ch < 1 || nsplit < 1) return r;
  const int first = lo - lo % ch;
  const int chunks = (hi - first + ch - 1) / ch;
  const int per = (chunks + nsplit - 1) / nsplit;
  r.n_act = (chunks + per - 1) / per;
  if (s < 0 || s >= r.n_act) return r;
  const int c0 = s * per, c1 = (s + 1) * per < chunks ? (s + 1) * per : chunks;
  r.c_begin = first + c0 * ch;
  r.key_begin = r.c_begin > lo ? r.c_begin : lo;
  r.key_end = hi - first > c1 * ch ? first + c1 * ch : hi;  // (no first + c1 ch past hi: no overflow near INT_MAX)
  return r;
}

inline AttnQ8PlanResult attn_decode_q8_plan(const AttnKnobs& k, int B, int H, int Hkv, int Dh, int t_cap, bool masked) {
  const auto fail = [](const char* why) { return AttnQ8PlanResult{-1, why, AttnQ8Plan{}}; };
  (void)masked;  // no rule depends on it (both wave forms and the split form take a key mask)
  if (Dh != ATTN_DH) return fail("head dim: Dh == 128");
  if (H < 1 || Hkv < 1 || H % Hkv) return fail("GQA: H a positive multiple of Hkv");
  const int rep = H / Hkv, pairs = B * Hkv;
  if (rep > 8 || (rep & (rep - 1))) return fail("fp8 KV cache: query heads per kv head 1, 2, 4 or 8");
  if (k.q8_splits > 1 && k.q8_waves == 1) return fail("fp8 KV cache: key splits (q8_splits > 1) only with 8 waves per pair");
  AttnQ8Plan p{};
  p.rep = rep, p.nsplit = 1;
  // One wave per pair from 2048 pairs, 8 waves below. The rule started as the bf16 plan's v3 / v4 boundary (1 wave where
  // rep <= 4 && B > 32, or from 4096 pairs) and moved on these records (profiles/kv8_attn_decode_ab.jsonl; graph-timed,
  // cold K / V, medians of 7 rounds, us at 8 waves / 1 wave), T = 384 unless noted:
  //   rep 4 (Llama-3-8B, 8 kv heads)  B = 64: 27.1 / 34.4   B = 128: 49.4 / 51.1   B = 256: 87.7 / 82.3
  //                                   B = 512: 160 / 151    B = 2048: 581 / 414    B = 4096: 1142 / 805
  //                                   B = 64 at T = 8192: 318 / 659
  //   rep 8 (Llama-3-70B, 8 kv heads) B = 32: 19.7 / 65.6   B = 256: 143.5 / 102.6
  // so 512 and 1024 pairs (where the old rule ran 1 wave at rep 4) stay with 8 waves, and rep 8 at 2048 pairs (where it
  // ran 8) takes 1. Few pairs with a long context want the 8 waves all the more, and key splits (below).
  p.waves = k.q8_waves ? k.q8_waves : (pairs >= ATTN_Q8_ONE_WAVE_MIN_PAIRS ? 1 : 8);
  // 16 scores per query-head set and lane group at most (rep x KPG <= 16, the v3 bound: no spills), 8 rows at most
  p.kpg = rep <= 2 ? 8 : 16 / rep;
  // ---- key splits, 8 waves only (the 1-wave form is for pairs that fill the chip on their own). An unsplit pair
  // streams on one CU, so below one workgroup per CU the launch takes the time of one pair's whole context. By shape:
  // enough splits for ATTN_Q8_SPLIT_WGS workgroups, each at least ATTN_Q8_SPLIT_MIN_CHUNKS chunks of t_cap so that a
  // split's stream outlasts the merge it causes. Both constants on these records (profiles/kv8_attn_decode_split_ab.jsonl;
  // graph-timed, cold K / V, medians of 7 rounds, us; "u" unsplit, then pinned counts, "*" the rule's), cache full:
  //   rep 4 (Llama-3-8B, 8 kv heads), T = 8192
  //     B = 1:  u 121.8   2: 66.7   4: 36.9   8: 22.8   16*: 18.4   32: 20.5     (bf16 plan: 40.3)
  //     B = 4:  u 126.9   2: 72.3   4: 41.6   8*: 34.0   16: 39.4   32: 50.1     (84.6)
  //     B = 16: u 128.3   2*: 107.3   4: 107.2   8: 118.9   16: 123.0            (161.8)
  //     B = 64: u 290.2   2: 302.4   4: 318.2                                    (568.4)  512 pairs: unsplit
  //   T = 32768   B = 1: u 476.5   8: 73.3   16: 43.6   32*: 38.5   B = 4: u 477.8   4: 132.5   8*: 108.3   16: 110.3
  //               B = 16: u 484.6   2*: 284.6   4: 289.4           B = 64: u 1062   2: 1076
  //   T = 384     B = 1: u 10.1   2: 10.8   3: 8.8   B = 4: u 10.4   2: 11.4   3: 9.7 (the rounds overlap)
  //               B = 16: u 11.3   2: 13.1   3: 16.9   B = 64: u 28.3   2: 41.0          -> under 4 chunks: unsplit
  //   rep 8 (Llama-3-70B, 8 kv heads), T = 8192   B = 1: u 250.5   8: 40.9   16: 28.3   32*: 26.0   (125.7)
  //                                               B = 8: u 252.1   2: 132.8   4*: 76.2   8: 86.6    (292.8)
  // and with the slot at T / 8 of a T = 8192 cache (the splits cut the valid keys): rep 4 B = 1 u 19.0 -> 10.5,
  // B = 4 20.8 -> 13.5, B = 16 20.7 -> 18.9; rep 8 B = 1 37.3 -> 15.5, B = 8 38.0 -> 21.2. So one workgroup per CU is
  // the count to aim for (twice that is up to 16 % slower, half of it 13-74 %), splits shorter than 4 chunks lose to
  // their merge (T = 8192 B = 1: 32 splits of 2 chunks 20.5 against 16 of 4 18.4), and from 256 pairs no count wins.
  // A pinned q8_waves alone keeps the unsplit launch (that knob A/Bs the two wave forms). A pinned count is cut so that
  // no split is emptier than one chunk at t_cap.
  if (p.waves == 8 && B > 0 && k.q8_splits != 1 && (k.q8_splits > 1 || k.q8_waves == 0)) {
    const int ch = 32 * p.kpg;
    int ns, most;
    if (k.q8_splits > 1) {
      ns = k.q8_splits < ATTN_Q8_MAX_SPLITS ? k.q8_splits : ATTN_Q8_MAX_SPLITS;
      most = (t_cap + ch - 1) / ch;
    } else {
      ns = (ATTN_Q8_SPLIT_WGS + pairs - 1) / pairs;
      most = t_cap / (ATTN_Q8_SPLIT_MIN_CHUNKS * ch);
    }
    p.nsplit = ns > most ? (most < 1 ? 1 : most) : ns;
  }
  if (p.nsplit > 1) {
    p.ws_floats = (size_t)B * H * p.nsplit * ATTN_PART_FLOATS;
    p.tickets = pairs;
  }
  return {0, "", p};
}

}  // namespace jla
