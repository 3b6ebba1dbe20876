// gemm5q: gemm5's weight-streaming workgroup (gemm5ws.h) on the quantised weight bytes -- FP8 e4m3 with one power-of-two
// scale per row, MXFP4 (e2m1 codes + e8m0 block scales) -- for decode batches above the GEMVs' 64 rows. The dequant
// path writes W_deq to a bf16 workspace on every call and then streams it again; here the quantised bytes go from HBM
// into the register ring and are converted to the bf16 MFMA fragment between the wait for a stage and its MFMAs. Each
// converted fragment feeds MT = 8 / 16 MFMAs (the GEMVs: 1-4), so the conversions cost ~1 / 2 VALU op per MFMA.
//
// Everything but the weight side is gemm5's and is kept as it is there: the tile (16 MT rows x 64 NTW columns, wave w:
// n-tiles 4 NTW tn + NTW w + j), the XCD-aware workgroup remap, x by LDS-DMA into the swizzled stage image (four
// slots), one barrier per 64-deep K-stage, the C^T accumulators and the float4 slab stores, the fused-norm statistic
// from the staged x, clamped n-tiles and rows, stages past the end contributing zero. The MFMA order over K is the
// same and the converted fragment is W_deq's bits (the scale is the conversion's operand, nothing multiplies the
// accumulators), so the [split][M][N] slabs (+ [split][M] sums of squares) carry the bits gemm5 writes on the
// dequantised copy, and gemm_reduce_kernel runs every epilogue behind it unchanged.
//
// A ring slot (the lane's registers of one stage, per n-tile):
//   FP8    one u32x4 -- the lane's 16 bytes of the 16 x 64 block [N/16][K/64][64][16]: bytes 0-7 the B fragment of
//          k-step 0 of the stage, 8-15 of k-step 1 (gemm5: two u32x4). One non-temporal 16-byte load. The lane's row
//          16 nt + (lane & 15) is fixed, so its scale is loaded once per n-tile ahead of the main loop.
//   MXFP4  one u32x2 + one dword -- a 16 x 128 block [N/16][K/128][64][16] spans two stages; stage s takes dwords
//          2 (s & 1), +1 of the lane's 16 bytes (one 8-byte load) and the block's scale dword [N/16][K/128][16][4], of
//          which it uses bytes 2 (s & 1), +1. Indexed by the parity of the absolute stage: a K split may start
//          mid-block.
// Past-the-end stages load the zero fragment (FP8 byte 0 / e2m1 code 0 convert to 0 at any scale).
#pragma once
#include "common.h"
#include "gemm4w.h"
#include "gemm_plan.h"
#include "ring.h"
#include "wq_cvt.h"

namespace jla {

// gemm5's depth (G5Q_A / G5Q_SLOTS of gemm5ws.h): K-stages in flight beyond the one being computed; x stage slots in LDS
// = weight ring slots. Four 32 KiB x slots are the LDS limit at 256 rows.
constexpr int G5Q_A = 3;
constexpr int G5Q_SLOTS = G5Q_A + 1;
static __device__ u32x4 g5q_zero_frag[64];  // 1 KiB of zeros: the weight bytes of stages past the end

template <int FMT>
struct G5qSlot;
template <>
struct G5qSlot<WQ_FP8> {
  u32x4 q;
  static constexpr int LOADS = 1;
};
template <>
struct G5qSlot<WQ_MXFP4> {
  u32x2 q;
  unsigned s;
  static constexpr int LOADS = 2;
};

// S: FP8 the fp32 row scales [N]; MXFP4 the packed e8m0 scale dwords [N/16][K/128][16]
template <int FMT, int MT, int NTW>
__global__ void __launch_bounds__(256, 1)
    gemm5q_partial_kernel(const bf16_t* __restrict__ x, const u32x4* __restrict__ Wq, const void* __restrict__ S,
                          float* __restrict__ ws, int M, int N, int K, int kc, int tiles_m, int tiles_n,
                          float* __restrict__ ssq) {
  static_assert(FMT == WQ_FP8 || FMT == WQ_MXFP4, "weight format");
  static_assert(MT == 8 || MT == 16, "rows per workgroup: 128 or 256");
  static_assert(NTW == 2 || NTW == 4, "n-tiles per wave");
  constexpr bool F8 = FMT == WQ_FP8;
  using Slot = G5qSlot<FMT>;
  constexpr int ROWS = 16 * MT;
  constexpr int XS_U4 = ROWS * 8;              // one x stage: ROWS x 128 B
  constexpr int XP = ROWS / 8 / 4;             // x DMA pieces (8 rows x 128 B) per wave per stage
  constexpr int OPS = XP + NTW * Slot::LOADS;  // vector-memory ops per wave per stage: x pieces + weight (+ scale) loads
  __shared__ u32x4 lds[G5Q_SLOTS * XS_U4];

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // XCD-aware bijective remap (gemm5's): consecutive ids share an XCD; the workgroups of one (split, m-tile) are
  // consecutive
  const int nwg = gridDim.x, orig = blockIdx.x;
  const int xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
  const int tn = wgid % tiles_n, rest = wgid / tiles_n;
  const int tm = rest % tiles_m, split = rest / tiles_m;
  const int KS64 = K >> 6;
  const int s0 = split * kc;
  const int NS = min(KS64, s0 + kc) - s0;  // <= 0: a split past the end (writes zero slabs)
  const int NTT = N >> 4;
  const int m0 = tm * ROWS;
  const int nt0 = (tn * 4 + w) * NTW;

  f32x4 acc[NTW][MT];
#pragma unroll
  for (int j = 0; j < NTW; ++j)
#pragma unroll
    for (int i = 0; i < MT; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float ss[MT / 4];
#pragma unroll
  for (int q = 0; q < MT / 4; ++q) ss[q] = 0.f;

  if (NS > 0) {
    // FP8: the lane's 16 bytes of stage s0 + u of n-tile nt0 + j at wp[j] + 1024 u. MXFP4: its 8 bytes at
    // wp[j] + 1024 ((s0 + u) >> 1) + 8 ((s0 + u) & 1), the scale dword at sp[j] + 64 ((s0 + u) >> 1). Clamped n-tiles
    // re-read the last
    const char* wp[NTW];
    [[maybe_unused]] const char* sp[NTW];
    [[maybe_unused]] float rs[NTW];  // FP8: the scale of the lane's row of n-tile j
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      const int nt = min(nt0 + j, NTT - 1);
      if constexpr (F8) {
        wp[j] = reinterpret_cast<const char*>(Wq + ((size_t)nt * KS64 + s0) * 64 + lane);
        rs[j] = static_cast<const float*>(S)[nt * 16 + (lane & 15)];
      } else {
        wp[j] = reinterpret_cast<const char*>(Wq + (size_t)nt * (KS64 >> 1) * 64 + lane);
        sp[j] = reinterpret_cast<const char*>(static_cast<const unsigned*>(S) + (size_t)nt * (KS64 >> 1) * 16 +
                                              (lane & 15));
      }
    }
    // (the compiler's own wait for the scale loads lands here, ahead of the hand-counted ring, not inside its loop)
    if constexpr (F8) {
#pragma unroll
      for (int j = 0; j < NTW; ++j) asm volatile("" : "+v"(rs[j]));
    }
    // x DMA: piece P = w + 4 i (rows 8P .. 8P + 7), lane L -> row 8P + L / 8, cell L % 8 <- k-chunk cell ^ swz(row)
    const char* const xbase = reinterpret_cast<const char*>(x + (size_t)s0 * 64);
    unsigned xoff[XP];
#pragma unroll
    for (int i = 0; i < XP; ++i) {
      const int P = w + 4 * i;
      const int row = min(m0 + 8 * P + (lane >> 3), M - 1);
      const int chunk = (lane & 7) ^ (4 * (P & 1) + (lane >> 4));
      xoff[i] = (unsigned)row * (unsigned)K * 2u + 16u * (unsigned)chunk;
    }
    Slot r0[NTW], r1[NTW], r2[NTW], r3[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      if constexpr (F8) {
        r0[j].q = r1[j].q = r2[j].q = r3[j].q = u32x4{0u, 0u, 0u, 0u};
      } else {
        r0[j].q = r1[j].q = r2[j].q = r3[j].q = u32x2{0u, 0u};
        r0[j].s = r1[j].s = r2[j].s = r3[j].s = 0u;
      }
    }

    // stage u into x slot `slot` / ring slot wr. Past the end (the ring is unrolled by 4 and never branches around
    // its loads) x re-loads the last stage and the weights load zeros, so the extra MFMAs add 0 (the MXFP4 scale
    // re-loads the last stage's: code 0 converts to 0 at any scale byte)
    const char* const zf = reinterpret_cast<const char*>(g5q_zero_frag + lane);
    auto issue = [&](int u, Slot (&wr)[NTW], int slot) {
      const bool live = u < NS;
      const int uc = min(u, NS - 1);
      u32x4* const xs = lds + slot * XS_U4;
#pragma unroll
      for (int i = 0; i < XP; ++i) glds16_asm(xbase + (size_t)uc * 128 + xoff[i], xs + (w + 4 * i) * 64);
      if constexpr (F8) {
#pragma unroll
        for (int j = 0; j < NTW; ++j) asm_load_nt<true>(wr[j].q, live ? wp[j] + (size_t)uc * 1024 : zf);
      } else {
        const int sa = s0 + uc;  // the absolute stage: block sa >> 1, half sa & 1
#pragma unroll
        for (int j = 0; j < NTW; ++j)
          asm_load_nt<true>(wr[j].q, live ? wp[j] + (size_t)(sa >> 1) * 1024 + 8 * (sa & 1) : zf);
#pragma unroll
        for (int j = 0; j < NTW; ++j) asm_load_b32<true>(wr[j].s, sp[j] + (size_t)(sa >> 1) * 64);
      }
    };
    // x fragment of m-tile i, k-step half h of a stage: row 16 i + (lane & 15), k-chunk 4h + (lane >> 4)
    const int xrow = (lane & 15) * 8;
    const int xc0 = (lane >> 4) ^ ((lane >> 1) & 7), xc1 = (4 + (lane >> 4)) ^ ((lane >> 1) & 7);
    // the bf16 fragment of k-step h of the stage in ring slot r; sh: the MXFP4 stage's first scale byte in the dword
    auto convert = [&](const Slot& r, int j, int h, int sh) -> u32x4 {
      if constexpr (F8)
        return fp8x8_to_bf16(r.q[2 * h], r.q[2 * h + 1], rs[j]);
      else
        return fp4x8_to_bf16(r.q[h], (r.s >> (sh + 8 * h)) & 0xffu);
    };
    auto compute = [&](Slot (&wr)[NTW], int slot, int u) {
      const bool live = u < NS;
#pragma unroll
      for (int j = 0; j < NTW; ++j) {
        pin(wr[j].q);
        if constexpr (!F8) pin(wr[j].s);
      }
      const int sh = 16 * ((s0 + min(u, NS - 1)) & 1);
      // the converted fragments of this stage (the only ones live): k-step 0 ahead of the MFMAs, k-step 1 one n-tile
      // per m-tile step under k-step 0's MFMAs (each pinned where it is issued, so it cannot sink to its first use)
      u32x4 cv[2][NTW];
#pragma unroll
      for (int j = 0; j < NTW; ++j) {
        cv[0][j] = convert(wr[j], j, 0, sh);
        pin(cv[0][j]);
      }
      const u32x4* const xs = lds + slot * XS_U4;
      // x fragment e = (h, i) of the stage, read two fragments ahead of its MFMAs (as gemm5)
      auto xfrag = [&](int e) { return xs[xrow + (e % MT) * 128 + (e < MT ? xc0 : xc1)]; };
      u32x4 xq[4];
      xq[0] = xfrag(0);
      xq[1] = xfrag(1);
#pragma unroll
      for (int e = 0; e < 2 * MT; ++e) {
        if (e + 2 < 2 * MT) xq[(e + 2) % 4] = xfrag(e + 2);
        const int h = e / MT, i = e % MT;
        if (e < NTW) {
          cv[1][e] = convert(wr[e], e, 1, sh);
          pin(cv[1][e]);
        }
#pragma unroll
        for (int j = 0; j < NTW; ++j) g4_mfma(acc[j][i], cv[h][j], xq[e % 4]);
      }
      if (ssq != nullptr && live) {  // wave-uniform: this wave's rows of the fused-norm statistic
#pragma unroll
        for (int q = 0; q < MT / 4; ++q) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const u32x4 f = xs[xrow + (w + 4 * q) * 128 + (h ? xc1 : xc0)];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float lo = __uint_as_float(f[e] << 16), hi = __uint_as_float(f[e] & 0xffff0000u);
              ss[q] = fmaf(lo, lo, ss[q]);
              ss[q] = fmaf(hi, hi, ss[q]);
            }
          }
        }
      }
    };
    // one stage: wait for its loads (this wave's), barrier (every wave's x landed; every wave done with the slot the
    // next issue overwrites), refill that slot with stage u + G5Q_A, convert and compute stage u
    auto stage = [&](int u, Slot (&cur)[NTW], int cslot, Slot (&nxt)[NTW], int nslot) {
      // stages u + 1 .. u + G5Q_A - 1 may stay in flight: OPS = XP x pieces + NTW weight loads (+ NTW scale loads,
      // MXFP4) each -- MT 16: 8 + 4 (+ 4) / 8 + 2 (+ 2); MT 8: 4 + 4 (+ 4) / 4 + 2 (+ 2); at most 32 <= vmcnt's 63
      wait_vmcnt<(G5Q_A - 1) * OPS>();
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      issue(u + G5Q_A, nxt, nslot);
      compute(cur, cslot, u);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    issue(0, r0, 0);
    issue(1, r1, 1);
    issue(2, r2, 2);
    static_assert(G5Q_A == 3, "the ring below is unrolled for 3 stages in flight");
    for (int u = 0; u < NS; u += 4) {
      stage(u, r0, 0, r3, 3);
      stage(u + 1, r1, 1, r0, 0);
      stage(u + 2, r2, 2, r1, 1);
      stage(u + 3, r3, 3, r2, 2);
    }
    // drain the ring (the clamped tail loads) before anything reuses its registers or the LDS
    wait_vmcnt<0>();
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      pin(r0[j].q);
      pin(r1[j].q);
      pin(r2[j].q);
      pin(r3[j].q);
      if constexpr (!F8) {
        pin(r0[j].s);
        pin(r1[j].s);
        pin(r2[j].s);
        pin(r3[j].s);
      }
    }
  }
  g4_acc_fence();
  // fp32 partial slab [split][M][N]: lane (c, q) of acc[j][i] -> row m0 + 16 i + c, columns 16 (nt0 + j) + 4q .. +3
  const int c = lane & 15, q4 = lane >> 4;
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int row = m0 + 16 * i + c;
#pragma unroll
    for (int j = 0; j < NTW; ++j) {
      const f32x4 v = g4_take(acc[j][i]);
      const int col = 16 * (nt0 + j) + 4 * q4;
      if (row < M && nt0 + j < NTT) *reinterpret_cast<f32x4*>(ws + ((size_t)split * M + row) * N + col) = v;
    }
  }
  if (ssq != nullptr && tn == 0) {
#pragma unroll
    for (int q = 0; q < MT / 4; ++q) {
      float v = ss[q];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      const int row = m0 + 16 * (w + 4 * q) + c;
      if (q4 == 0 && row < M) ssq[(size_t)split * M + row] = v;
    }
  }
}

}  // namespace jla
