// The plan of one tiled-GEMM call (gemm.hip): every rule that decides whether (tile id, epilogue mode, fused norm,
// K split, norm scratch) is legal and which kernel runs it lives in gemm_plan() below, in one order. Plain C++ (no HIP
// headers): the launchers, the bindings and the Python tuner (through gemm_plan_check) all ask this one function.
#pragma once

// Linear epilogue modes (mirrors ops/__init__.py)
#define MODE_STORE 0
#define MODE_RESIDUAL 1
#define MODE_SWIGLU 2
#define MODE_QKV 3
#define MODE_PARTIAL 7  // launch mode of a K split (not a caller's mode): fp32 partial tile to the workspace
#define MODE_ARGMAX 8   // gemm_argmax() only
#define MODE_TPRESID 9  // row-parallel partial -> granule all-reduce over the TP group -> residual (gemv.hip)
#define MODE_LOGPROB 10 // gemm_logprob() only: per-row (max, sum of exponentials) partials + the logit at a target column

namespace jla {

// Tile ids (the `tile` argument of gemm(); any other id runs gemm2 by M, as 0 does where gemm4 does not apply):
//   id  kernel                   workgroup tile      notes
//    0  by shape                 --                  gemm4 (as 7) where K % 64 == 0, M > 128 and the gemm4 default is
//                                                    on -- persistent (as 13) for the residual epilogue at M >= 4096
//                                                    without a K split; else gemm2 2 (M <= 128) / 1
//    1  gemm2                    256 x 256           8 waves (two ping-pong rows) of 128 x 64, full-line x staging
//    2  gemm2                    128 x 256           4 waves of 128 x 64
//    3  gemm2                    128 x 128           8 waves of 64 x 32; 64 KiB of LDS: two workgroups share a CU
//    7  gemm4                    256 x 256           4 waves of 128 x 128 (gemm4w.h); K % 64 == 0
//   11  gemm5                    128|256 x 256       weight-streaming split-K (gemm5ws.h), 4 n-tiles per wave; the
//   12  gemm5                    128|256 x 128       reduce kernel runs every epilogue, even without a split (2 n-tiles)
//   13  gemm4 persistent         256 x 256           one workgroup per CU walks the tiles; plain gemm4 under a K split
//   14  gemm4, deep weights      256 x 256           the weight operand three K-tiles deep (160 KiB of LDS)
//   16  gemm4, deep weights      256 x 192           the fused norm only precomputed (scratch, no K split)
//   17  gemm4, deep weights      256 x 128           as 16; no QKV epilogue without a split; K % 64 != 0 is an error
//   18  gemm4 tail-balanced      256 x 192 + 128     whole rounds of body tiles, then the rest in 128-wide tail tiles
//   19  gemm4 tail-balanced      256 x 256 + 128     (gemm4t_kernel): store / residual / SwiGLU, never split
// Tiles 7 / 13 / 14 / 16 with K % 64 != 0 run gemm2 by M.
constexpr int G2_256_TILE = 1, G2_128_TILE = 2, G2_128N_TILE = 3;
constexpr int G4_TILE = 7, G5_TILE = 11, G5N_TILE = 12, G4P_TILE = 13, G4D_TILE = 14;
constexpr int G4N6D_TILE = 16, G4ND_TILE = 17, G4T6_TILE = 18, G4T8_TILE = 19;

enum GemmFamily {
  GEMM_NONE = 0,       // M <= 0: nothing to launch
  GEMM2_256x256 = 1,   // gemm2 tile configs 1 / 2 / 3
  GEMM2_128x256 = 2,
  GEMM2_128x128 = 3,
  GEMM4,
  GEMM4_PERSISTENT,
  GEMM4_TAIL,
  GEMM5,
};
enum GemmNorm { NORM_NONE = 0, NORM_INLOOP = 1, NORM_PRECOMPUTED = 2 };  // (= gemm4's RMSM template argument)

struct GemmPlan {
  GemmFamily family;
  int nj;        // gemm4: 32-column n-steps of the tile (8 / 6 / 4; tail-balanced: of the body); gemm5: n-tiles per wave
  bool deep;     // gemm4: the weights three K-tiles deep
  int ksplit;    // effective K split (1: none)
  int kc;        // K-tiles per split (gemm2: 32 deep; gemm4 / gemm5: 64 deep)
  GemmNorm norm; // fused RMSNorm: in the main loop (split: per-split partial sums) / from the scratch, ahead of the GEMM
  int n_body;    // tail-balanced: body n-tiles
  bool reduce;   // the epilogue runs in gemm_reduce_kernel over partial slabs, not in the tile kernel
};
struct GemmPlanResult {
  int rc;  // 0 legal; -1 shape / combination; -5 norm with the residual; -6 norm needs the scratch; -7 no tail split
  GemmPlan plan;
};

inline int gemm5_ksplit(int K, int ksplit) {  // gemm5: the effective split count over 64-deep K-stages
  const int KS64 = K >> 6;
  if (ksplit < 1) ksplit = 1;
  const int kc = (KS64 + ksplit - 1) / ksplit;
  return (KS64 + kc - 1) / kc;
}

inline int gemm_tail_width(int tile) { return tile == G4T6_TILE ? 192 : (tile == G4T8_TILE ? 256 : 0); }

// The body n-tile count of the tail-balanced plan for tiles_m m-tiles x N columns, body tiles `width` (192 / 256)
// columns wide, on `cus` CUs; the tail is the remaining columns in 128-wide tiles. Minimises the modelled time
// rounds x tile width, ceil(tm * n_body / cus) * width + ceil(tm * n_tail / cus) * 128 * (1 + 1/16): the narrow tile
// moves 1.5x / 2x the operand bytes per MFMA of the 192 / 256 one, which the 1/16 stands for. Ties go to regions that
// are multiples of 8 workgroups (the XCD count), then to the wider body. 0: no split beats the uniform `width` grid
// (N already fills whole rounds, or the tail would cost a round of its own for nothing).
inline int gemm_tail_split(int tiles_m, int N, int width, int cus) {
  if (tiles_m <= 0 || N <= 0 || cus <= 0 || (width != 192 && width != 256)) return 0;
  auto rounds = [&](long long wgs) { return (wgs + cus - 1) / cus; };
  auto tail_tiles = [&](int nb) { return (N - nb * width + 127) / 128; };
  auto aligned = [&](int nb) { return (tiles_m * nb) % 8 == 0 && (tiles_m * tail_tiles(nb)) % 8 == 0; };
  long long best = rounds((long long)tiles_m * ((N + width - 1) / width)) * width * 16;  // the uniform grid
  int best_nb = 0;
  for (int nb = (N - 1) / width; nb >= 1; --nb) {
    const long long cost =
        rounds((long long)tiles_m * nb) * width * 16 + rounds((long long)tiles_m * tail_tiles(nb)) * 128 * 17;
    if (cost < best || (best_nb != 0 && cost == best && aligned(nb) && !aligned(best_nb))) {
      best = cost;
      best_nb = nb;
    }
  }
  return best_nb;
}

// rms: the caller asks for the fused RMSNorm (rms_eps >= 0); ksplit: the requested split (<= 1: none); has_rms_ws: a
// scratch of >= M floats for the precomputed row statistic; n_body: tail-balanced body n-tiles (<= 0: the modelled
// split); cus: CUs of the device; g4_default: gemm4 is tile 0's kernel where it applies.
inline GemmPlanResult gemm_plan(int M, int N, int K, int mode, bool rms, int ksplit, int tile, bool has_rms_ws,
                                int n_body, int cus, bool g4_default) {
  GemmPlan p{};
  const auto fail = [](int rc) { return GemmPlanResult{rc, GemmPlan{}}; };
  const bool k64 = (K & 63) == 0;
  const bool caller_mode = mode == MODE_STORE || mode == MODE_RESIDUAL || mode == MODE_SWIGLU || mode == MODE_QKV ||
                           mode == MODE_TPRESID;

  // ---- gemm5: partial slabs for any split, every epilogue in the reduce kernel
  if (tile == G5_TILE || tile == G5N_TILE) {
    if (mode == MODE_ARGMAX || mode == MODE_LOGPROB || (rms && (mode == MODE_RESIDUAL || mode == MODE_TPRESID)))
      return fail(-1);
    if (K <= 0 || !k64 || (N & 15) || M <= 0) return fail(-1);
    if (mode == MODE_SWIGLU && (N & 31)) return fail(-1);
    if (!caller_mode) return fail(-1);
    p.family = GEMM5;
    p.nj = tile == G5_TILE ? 4 : 2;
    p.ksplit = gemm5_ksplit(K, ksplit);
    p.kc = ((K >> 6) + p.ksplit - 1) / p.ksplit;
    p.norm = rms ? NORM_INLOOP : NORM_NONE;
    p.reduce = true;
    return {0, p};
  }

  // ---- shape and mode rules of every other tile, in this order
  // (the 256 x 128 tile's combination check comes before the empty batch: illegal is -1 even at M = 0; it sees the
  // requested split, not the effective one)
  if (tile == G4ND_TILE &&
      (!k64 || (mode == MODE_QKV && ksplit <= 1) || mode == MODE_ARGMAX || mode == MODE_LOGPROB ||
       (rms && mode != MODE_RESIDUAL && (ksplit > 1 || !has_rms_ws))))
    return fail(-1);
  if (M <= 0) return {0, p};
  if (K <= 0 || (N & 15) || (K & 31)) return fail(-1);
  if (mode == MODE_SWIGLU && (N & 31)) return fail(-1);
  if (rms && mode == MODE_RESIDUAL) return fail(-5);  // the caller pre-scales x instead
  const int KS = K >> 5;
  p.kc = (KS + (ksplit < 1 ? 1 : ksplit) - 1) / (ksplit < 1 ? 1 : ksplit);
  p.ksplit = (KS + p.kc - 1) / p.kc;
  const bool split = p.ksplit > 1;
  if (mode == MODE_TPRESID && (!split || rms)) return fail(-1);  // the exchange lives in the split-K reduce
  const int lmode = split ? MODE_PARTIAL : mode;                 // what the tile kernel runs
  p.reduce = split;

  // ---- the kernel family of the tile id
  const bool tail = tile == G4T6_TILE || tile == G4T8_TILE;
  if (tail) {
    p.family = GEMM4_TAIL;
    p.nj = tile == G4T6_TILE ? 6 : 8;
  } else if (tile == G4ND_TILE) {
    p.family = GEMM4, p.nj = 4, p.deep = true;
  } else if (tile == G4N6D_TILE && k64 && lmode != MODE_ARGMAX && lmode != MODE_LOGPROB) {
    p.family = GEMM4, p.nj = 6, p.deep = true;
  } else if (k64 && (tile == G4_TILE || tile == G4P_TILE || tile == G4D_TILE || (tile == 0 && g4_default && M > 128))) {
    // persistent: asked for (13), or the residual epilogue at prefill sizes (o / down at M = 32768 3.5 / 2.4 % faster:
    // the CUs' fp32 read-modify-write bursts desynchronise; the store / SwiGLU / QKV epilogues lose 1.5-3.6 % that
    // way, profiles/r5_gemm4_persistent_ab.jsonl); never under a K split or with the argmax / log-prob epilogues
    const bool persist = tile == G4P_TILE || (lmode == MODE_RESIDUAL && tile == 0 && M >= 4096);
    p.family = persist && !split && lmode != MODE_ARGMAX && lmode != MODE_LOGPROB ? GEMM4_PERSISTENT : GEMM4;
    p.nj = 8, p.deep = tile == G4D_TILE;
  } else if (mode == MODE_ARGMAX) {  // gemm2 has the argmax epilogue on the 256 x 256 tile only
    p.family = GEMM2_256x256;
  } else {  // gemm2: the id's config, else by M
    p.family = tile >= G2_256_TILE && tile <= G2_128N_TILE ? (GemmFamily)tile
                                                           : (M <= 128 ? GEMM2_128x256 : GEMM2_256x256);
  }
  const bool g4 = p.family == GEMM4 || p.family == GEMM4_PERSISTENT || p.family == GEMM4_TAIL;
  if (g4) p.kc = ((K >> 6) + p.ksplit - 1) / p.ksplit;  // 64-deep K-tiles; splits past the end run none (zero slabs)

  // ---- rules of the family
  // qkv without a K split: the RoPE / KV-write epilogue in the tile kernel needs the fused norm and gemm2's
  // 256 x 256 tile (ids 0 / 1 only), gemm4's 256 x 256 tile or the 256 x 192 one
  if (mode == MODE_QKV && !split &&
      !(rms && ((p.family == GEMM2_256x256 && (tile == 0 || tile == G2_256_TILE)) || p.family == GEMM4 ||
                p.family == GEMM4_PERSISTENT)))
    return fail(-1);
  // the 256 x 128 / 192 tiles (whichever kernel the id resolved to) take the fused norm only as the precomputed
  // statistic, so not under a K split
  if ((tile == G4ND_TILE || tile == G4N6D_TILE) && rms && (split || !has_rms_ws)) return fail(-6);
  if (tail) {
    if (!k64 || split || (mode != MODE_STORE && mode != MODE_RESIDUAL && mode != MODE_SWIGLU)) return fail(-1);
    if (rms && !has_rms_ws) return fail(-6);
    const int wb = gemm_tail_width(tile);
    p.n_body = n_body > 0 ? n_body : gemm_tail_split((M + 255) / 256, N, wb, cus);
    if (p.n_body <= 0 || (long long)p.n_body * wb >= N) return fail(-7);  // no split beats the uniform grid
  }
  if (mode == MODE_ARGMAX || mode == MODE_LOGPROB ? split : !caller_mode) return fail(-1);
  // the log-prob epilogue exists on gemm4's 256 x 256 tile only (so K % 64 == 0; gemm2 has none)
  if (mode == MODE_LOGPROB && !(p.family == GEMM4 && p.nj == 8)) return fail(-1);

  // ---- the fused norm: gemm4 without a split reads the precomputed statistic where the scratch is there (the narrow
  // and tail-balanced tiles: always, see above); every other plan sums it in the main loop
  if (rms) p.norm = g4 && !split && has_rms_ws ? NORM_PRECOMPUTED : NORM_INLOOP;
  return {0, p};
}

}  // namespace jla
