// The plan of one decode-GEMV call (gemv.hip linear_skinny, M <= 64): every rule that decides whether (variant id,
// epilogue mode, activation type and layout, shape) is legal and which form of linear_skinny_kernel runs it lives in
// gemv_plan() below, in one order. Plain C++ (no HIP headers): the launcher, the bindings and the Python tuner (through
// gemv_plan_check) all ask this one function.
#pragma once

#include <cstddef>

#include "gemm_plan.h"  // the epilogue modes

#define SKINNY_MAX_M 64

namespace jla {

// Variant ids (the `variant` argument of linear_skinny(); ids of removed forms are not reused,
// profiles/r4_variant_pruning.md). A workgroup is `tiles` consecutive 16-column n-tiles x `waves` waves over the whole
// K; at M > 16 every form runs 2 (M <= 32) or 4 m-tiles per weight fragment.
//   id  x       tiles x waves  notes
//    0  --      --             = 1 (not with the argmax / TP-residual epilogues: their callers name a form)
//    1  row     1|2 x 4|8      the default form: tiles and waves by the rule below
//    5  row     4 x 4          x re-reads / 4; at N % 64 != 0 the default form
//    6  row     2 x 4          x re-reads / 2
//   10  row     2 x 4          doubled register ring (bytes in flight); at M <= 16 or with fp32 x the default form
//   12  packed  1 x 8          no SwiGLU (the pair needs 2 tiles)
//   15  packed  2 x 4          doubled register ring; the SwiGLU form of 12
//   16  row     1|2 x 4|8      K over 2 workgroups per column group (tensor-parallel shards); the pair under SwiGLU
//   18  packed  1|2 x 4|8      as 16
//   20  row     2 x 8          wide projections with few column groups (w1|w3 shards)
//   21  packed  2 x 8          as 20
//   22  packed  4 x 4          N % 64 == 0
//   26  packed  4 x 8          K over 4 workgroups (narrow, deep projections at M = 17..64: w2); N % 64 == 0
// The default form: 2 tiles for SwiGLU (the gate / up pair in one workgroup) or, outside QKV, at N / 16 >= 2048
// (lm_head, w1|w3: half the x re-reads), else 1; 4 waves at M <= 16 (measured best there on every Llama-3-8B
// projection), 8 above. "packed": x is the packed copy (common.h pack_off, padded to 16 x the m-tiles rows), bf16
// only. The split forms (16 / 18 / 26) read bf16 x and have no argmax epilogue; the last arriver of a column group
// sums the splits (slabs and tickets below) and runs the epilogue.
struct GemvVariant {
  int id;
  bool xp, split;
};
constexpr GemvVariant GEMV_VARIANTS[] = {
    {1, false, false},  {5, false, false}, {6, false, false}, {10, false, false}, {12, true, false}, {15, true, false},
    {16, false, true},  {18, true, true},  {20, false, false}, {21, true, false}, {22, true, false}, {26, true, true},
};
inline const GemvVariant* gemv_variant(int id) {
  for (const GemvVariant& v : GEMV_VARIANTS)
    if (v.id == id) return &v;
  return nullptr;
}

constexpr int GEMV_SPLIT_MAX_GROUPS = 1024;  // column groups (N / 16) a split form's tickets cover
constexpr int GEMV_MAX_KSPLIT = 4;           // (variant 26)
inline int gemv_m_tiles(int M) { return M <= 16 ? 1 : (M <= 32 ? 2 : 4); }

// slab floats / tickets of the split forms for this shape, whatever the id (0 when N has too many column groups for
// them): launch_skinny needs groups x splits x (m-tiles x tiles x 256 accumulators + m-tiles x 16 row sums)
inline size_t gemv_split_workspace_floats(int M, int N) {
  const int groups = N >> 4;  // upper bound: 1 tile per column group
  if (groups > GEMV_SPLIT_MAX_GROUPS || M < 1 || M > SKINNY_MAX_M) return 0;
  const int mt = gemv_m_tiles(M);
  return (size_t)groups * GEMV_MAX_KSPLIT * (mt * 256 + mt * 16);
}
inline int gemv_split_tickets(int N) { return (N >> 4) > GEMV_SPLIT_MAX_GROUPS ? 0 : (N >> 4); }

struct GemvPlan {
  int mt, nt, nw;         // m-tiles (0: nothing to launch), n-tiles and waves per workgroup
  bool deep, xp, split;   // doubled register ring / packed x / K over `ksplit` workgroups per column group
  int ksplit;
};
struct GemvPlanResult {
  int rc;           // 0 legal; -1 not (-3, workspace or tickets too small, concerns buffers: launch_skinny's)
  const char* why;  // the rule that refused the call
  GemvPlan plan;
};

// x_f32: fp32 activations (else bf16); x_packed: the caller passes the packed copy of x.
inline GemvPlanResult gemv_plan(int M, int N, int K, int mode, bool x_f32, bool x_packed, int variant) {
  const auto fail = [](const char* why) { return GemvPlanResult{-1, why, GemvPlan{}}; };
  if (mode != MODE_STORE && mode != MODE_RESIDUAL && mode != MODE_SWIGLU && mode != MODE_QKV && mode != MODE_ARGMAX &&
      mode != MODE_TPRESID)
    return fail("not an epilogue of the decode GEMV");

  // ---- rules of the id (they come before the empty batch: an illegal id is an error even at M = 0)
  if (variant == 0 && mode != MODE_ARGMAX && mode != MODE_TPRESID) variant = 1;
  const GemvVariant* v = gemv_variant(variant);
  if (!v) return fail("unknown decode GEMV variant");
  if (v->xp != x_packed) return fail("packed-x variants need the packed x, the others must not get one");
  if (v->xp && x_f32) return fail("packed-x variants read bf16 activations");
  if (variant == 12 && mode == MODE_SWIGLU) return fail("no one-tile packed-x form under SwiGLU (15 is its form)");
  if (mode == MODE_ARGMAX && (v->xp || v->split)) return fail("the argmax epilogue: row-major x, no K split");
  if (mode == MODE_TPRESID && (x_f32 || M < 1)) return fail("the TP-residual epilogue: bf16 x, M >= 1");
  if (v->split && (N >> 4) > GEMV_SPLIT_MAX_GROUPS) return fail("too many column groups (N / 16 > 1024) for a K split");

  // ---- shape
  if (M <= 0) return {0, "", GemvPlan{}};
  if (M > SKINNY_MAX_M || (N & 15) || (K & 31)) return fail("shape: M <= 64, N % 16 == 0, K % 32 == 0");
  if (mode == MODE_SWIGLU && (N & 31)) return fail("SwiGLU: N % 32 == 0");
  if (v->split && x_f32) return fail("split-K variants read bf16 activations");

  // ---- the form: the default one, then what the id changes
  GemvPlan p{};
  p.mt = gemv_m_tiles(M);
  p.nt = mode == MODE_SWIGLU || (mode != MODE_QKV && (N >> 4) >= 2048) ? 2 : 1;
  p.nw = p.mt == 1 ? 4 : 8;
  p.xp = v->xp, p.split = v->split, p.ksplit = 1;
  const bool n64 = (N & 63) == 0;
  switch (variant) {
    case 5:
      if (n64) p.nt = 4, p.nw = 4;
      break;
    case 6: p.nt = 2, p.nw = 4; break;
    case 10:
      if (p.mt > 1 && !x_f32) p.nt = 2, p.nw = 4, p.deep = true;
      break;
    case 12: p.nt = 1, p.nw = 8; break;
    case 15: p.nt = 2, p.nw = 4, p.deep = true; break;
    case 16:
    case 18: p.nt = mode == MODE_SWIGLU ? 2 : 1, p.ksplit = 2; break;
    case 20:
    case 21: p.nt = 2, p.nw = 8; break;
    case 22:
    case 26:
      if (!n64) return fail("the four-tile packed-x forms: N % 64 == 0");
      p.nt = 4, p.nw = variant == 22 ? 4 : 8, p.ksplit = variant == 22 ? 1 : 4;
      break;
    default: break;  // 1
  }
  if (p.split && (K >> 5) < p.ksplit) return fail("fewer 32-deep K steps than K splits");
  return {0, "", p};
}

// The plan of one FP8-weight decode-GEMV call (gemv.hip linear_skinny_w8: e4m3 weights in 16 x 64 blocks, one fp32
// power-of-two scale per output row). One form per (m-tiles, epilogue): the tiles and waves of the default form above,
// row-major bf16 x, no K split. Whatever this refuses runs on the bf16 kernels over the dequantised weight.
inline GemvPlanResult gemv_w8_plan(int M, int N, int K, int mode, bool x_f32) {
  const auto fail = [](const char* why) { return GemvPlanResult{-1, why, GemvPlan{}}; };
  if (mode != MODE_STORE && mode != MODE_RESIDUAL && mode != MODE_SWIGLU && mode != MODE_QKV)
    return fail("the FP8-weight GEMV: store, residual, SwiGLU and qkv epilogues only");
  if (x_f32) return fail("the FP8-weight GEMV reads bf16 activations");
  if (M <= 0) return {0, "", GemvPlan{}};
  if (M > SKINNY_MAX_M || (N & 15) || (K & 63)) return fail("shape: M <= 64, N % 16 == 0, K % 64 == 0");
  if (mode == MODE_SWIGLU && (N & 31)) return fail("SwiGLU: N % 32 == 0");
  GemvPlan p{};
  p.mt = gemv_m_tiles(M);
  p.nt = mode == MODE_SWIGLU || (mode != MODE_QKV && (N >> 4) >= 2048) ? 2 : 1;
  p.nw = p.mt == 1 ? 4 : 8;
  p.ksplit = 1;
  return {0, "", p};
}

// The plan of one MXFP4-weight decode-GEMV call (gemv.hip linear_skinny_w4: e2m1 codes in 16 x 128 blocks, one e8m0
// scale byte per output row and 32 consecutive K elements). The twin of gemv_w8_plan(): one form per (m-tiles,
// epilogue), the tiles and waves of the default form, row-major bf16 x, no K split; K in whole 128-deep blocks (one
// 16-byte lane load holds four k-steps). Whatever this refuses runs on the bf16 kernels over the dequantised weight.
inline GemvPlanResult gemv_w4_plan(int M, int N, int K, int mode, bool x_f32) {
  const auto fail = [](const char* why) { return GemvPlanResult{-1, why, GemvPlan{}}; };
  if (mode != MODE_STORE && mode != MODE_RESIDUAL && mode != MODE_SWIGLU && mode != MODE_QKV)
    return fail("the MXFP4-weight GEMV: store, residual, SwiGLU and qkv epilogues only");
  if (x_f32) return fail("the MXFP4-weight GEMV reads bf16 activations");
  if (M <= 0) return {0, "", GemvPlan{}};
  if (M > SKINNY_MAX_M || (N & 15) || (K & 127)) return fail("shape: M <= 64, N % 16 == 0, K % 128 == 0");
  if (mode == MODE_SWIGLU && (N & 31)) return fail("SwiGLU: N % 32 == 0");
  GemvPlan p{};
  p.mt = gemv_m_tiles(M);
  p.nt = mode == MODE_SWIGLU || (mode != MODE_QKV && (N >> 4) >= 2048) ? 2 : 1;
  p.nw = p.mt == 1 ? 4 : 8;
  p.ksplit = 1;
  return {0, "", p};
}

}  // namespace jla
