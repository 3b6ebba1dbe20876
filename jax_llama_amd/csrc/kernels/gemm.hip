// Linear layer for M > 32 rows (prefill, and large-batch decode): y = epilogue(x[M, K] @ W[N, K]^T),
// bf16 MFMA. x arrives RMS-scaled in bf16 (rms_scale) when a norm precedes the projection.
//
// Tiling (CDNA4): 128 x 128 output tile per 256-thread workgroup, 4 waves in 2 x 2, each wave a
// 64 x 64 sub-tile = 4 x 4 v_mfma_f32_16x16x32_bf16 accumulators. K advances 64 per stage. Both
// operands are staged into LDS in the MFMA *fragment* layout (16 rows x 32 k = 64 lanes x 16 B),
// so every LDS fragment read is a lane-linear ds_read_b128 (bank-conflict free) and the packed
// weights are copied verbatim (each 1 KiB fragment is already contiguous in HBM). Double-buffered
// LDS; the next stage's global loads are issued before the current stage's MFMAs and written to
// LDS after them (issue-early / write-late), one barrier per stage.
//
// Decode at batch 64..512 has too few 128x128 tiles to fill 256 CUs, so K can be split over
// gridDim.z workgroups: each writes an fp32 partial tile, and gemm_reduce_kernel sums the splits in
// fixed order (deterministic) and runs the epilogue: store bf16/fp32, residual add (+ bf16 mirror),
// SiLU(gate)*up over the interleaved [w1;w3] tiles, or RoPE + KV-cache write for the fused qkv
// projection (reference ops: model.py:210/294/338/736, :58-92, :169-199, :392/:398).
#include <type_traits>

#include "car.h"
#include "common.h"
#include "gemm4w.h"
#include "gemm5ws.h"
#include "gemm_plan.h"
#include "launchers.h"
#include "ring.h"

namespace jla {

// ---------------------------------------------------------------------------------------------
// gemm2: BM x 256 tile (BM = 128 * WM), 4 * WM waves as WM(M) x 4(N), each wave a 128 x 64 sub-tile
// (8 x 4 accumulators of 16x16, 128 fp32 registers). K advances 32 per LDS tile; 4 LDS tile buffers
// filled by LDS-DMA (global_load_lds_dwordx4, no VGPR staging) run 3 tiles ahead of the MFMAs: at
// the top of each K-tile a wave waits (counted vmcnt, never 0 in steady state) only for ITS part of
// the tile it is about to read, then one raw s_barrier publishes every wave's part and retires the
// reads of the buffer being refilled next (WAR). Both operands are stored fragment-shaped in LDS
// (1 KiB = 16 rows x 32 k, lane-linear), so every ds_read_b128 is conflict-free: the packed weights
// are copied verbatim, x is gathered by per-lane source addresses (16 rows x 64 B per wave-load).
// Workgroups are remapped so consecutive tiles share an XCD (its own L2), M-grouped by 8.
constexpr int G2_BN = 256, G2_NBUF = 4, G2_GROUP_M = 8;
#ifdef JLA_GEMM_STAMPS
// diagnostic build only (tools/debug/gemm_stamps.hip): per-wave cycles of the ping-pong phases
__device__ unsigned long long g_gemm_stamps[8192 * 8 * 6];
#endif

// tile index (in the M-grouped launch order) -> (m tile, n tile)
JLA_DEV void g2_tile_coords(int pid, int tiles_m, int tiles_n, int& tm, int& tn) {
  const int in_group = G2_GROUP_M * tiles_n;
  const int first_m = (pid / in_group) * G2_GROUP_M;
  const int gsz = min(tiles_m - first_m, G2_GROUP_M);
  tm = first_m + (pid % in_group) % gsz;
  tn = (pid % in_group) / gsz;
}

// RMS (fused RMSNorm, reference model.py:28-48 with the gain folded into W): the A operand is the
// UNscaled bf16 activation; the waves square-sum the A fragments they already read from LDS (wave wc
// takes m-tiles 2wc, 2wc+1 of its row block, 8 v_dot2 per K-tile) and the epilogue scales each output
// row by rsqrt(mean(x^2) + eps). Split-K: each split stores its partial sums ([split][M] after the
// fp32 slabs) and the reduce kernel finishes the statistic. No rms_scale launch, no scaled copy of x.
// FA (full-line A; 256 x 256 ping-pong only): x is staged in 8-row x 128-B pieces that cover a PAIR of
// K-tiles (lane l of a piece loads row l>>3, 16-B chunk (l&7) ^ swz(row)), instead of 16-row x 64-B
// fragment-shaped loads: half the cache lines per LDS-DMA instruction, so half the TA work for x
// (cdna_hip_programming.md §5 "x through LDS in full 128-B lines"). The LDS image [row][8 chunks] is
// XOR-swizzled (swz = (row & 15) >> 1) so the A-fragment ds_read_b128s stay conflict-free under the
// gfx950 b128 lane groups. x pairs live in a 3-slot ring (96 KiB), weights in the usual 4-slot K-tile
// ring (64 KiB); pair p is issued in two halves with K-tiles 2p-4 and 2p-3 (4 LDS-DMA per wave per
// K-tile, as before), so the vmcnt accounting stays "everything issued two K-tiles back has landed".
template <int MODE, int WM, bool LATE_WAIT = false, bool RMS = false, int MT = 8, int NTW = 4, bool FA = false,
          int FAM = 0>
__global__ void __launch_bounds__(256 * WM)
    gemm2_kernel(const bf16_t* __restrict__ x, const u32x4* __restrict__ W, void* __restrict__ out, int M, int N,
                 int K, int accumulate, int out_f32, bf16_t* __restrict__ mirror, int kc, int tiles_m, int tiles_n,
                 float rms_eps, float* __restrict__ ssq_ws, QKVArgs qa) {
  // wave tile: MT m-tiles x NTW n-tiles of 16x16 (128 x 64 by default; 64 x 32 for the 128 x 128 tile)
  constexpr int NW = 4 * WM, BM = 16 * MT * WM, BN = 64 * NTW;
  constexpr int RPW = MT / 4;  // RMS: m-tiles whose row statistics each wave accumulates
  constexpr int AF = BM / 16, BF = BN / 16, FR = AF + BF;  // fragments per K-tile
  constexpr int G = FR / NW;                                   // LDS-DMA loads per wave per K-tile
  static_assert(FR % NW == 0, "fragment split");
  constexpr int DIST = G2_NBUF - 1;
  constexpr int A_SLOTS = 3, A_PIECES = BM / 8, A_RING = FA ? A_SLOTS * A_PIECES * 64 : 0;
  static_assert(!FA || (WM == 2 && MT == 8 && NTW == 4 && G2_NBUF == 4 && BF == 2 * NW),
                "FA: 256 x 256 ping-pong, 2 weight fragments per wave per K-tile");
  __shared__ u32x4 lds[FA ? A_RING + G2_NBUF * BF * 64 : G2_NBUF * FR * 64];
  u32x4* const bring = lds + A_RING;  // FA: the weight ring follows the x ring

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wr = w >> 2, wc = w & 3;

  // XCD-aware bijective remap, then (split, M-grouped tile) order
  const int nwg = gridDim.x, orig = blockIdx.x;
  const int xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
  const int tiles = tiles_m * tiles_n;
  const int split = wgid / tiles;
  const int pid = wgid - split * tiles;
  int tm, tn;
  g2_tile_coords(pid, tiles_m, tiles_n, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;

  const int KS = K >> 5, NTT = N >> 4;
  const int ks0 = split * kc;
  const int KT = min(KS, ks0 + kc) - ks0;  // K-tiles (32 deep) of this split

  // per-wave LDS-DMA sources: fragment f = w + NW*j (A fragments first, then B)
  const char* src[G];
  int step[G];
#pragma unroll
  for (int j = 0; j < G; ++j) {
    const int f = w + NW * j;
    if (f < AF) {
      const int row = min(m0 + 16 * f + (lane & 15), M - 1);
      src[j] = reinterpret_cast<const char*>(x + (size_t)row * K + (size_t)ks0 * 32 + 8 * (lane >> 4));
      step[j] = 64;
    } else {
      const int nt = min((n0 >> 4) + (f - AF), NTT - 1);
      src[j] = reinterpret_cast<const char*>(W + ((size_t)nt * KS + ks0) * 64 + lane);
      step[j] = 1024;
    }
  }
  auto issue = [&](int t) {
    u32x4* buf = lds + (t % G2_NBUF) * FR * 64;
#pragma unroll
    for (int j = 0; j < G; ++j) glds16(src[j] + (size_t)t * step[j], buf + (w + NW * j) * 64);
  };
  // FA sources, saddr form: one wave-uniform 64-bit base per operand (advanced by scalar adds) plus a
  // 32-bit per-lane byte offset within the tile (< 15 MB for every Llama shape). x piece 16h + wu + 8j
  // of a K-tile pair (h = issue half, a compile-time constant at every call), weight fragments wu + 8j.
  const int wu = __builtin_amdgcn_readfirstlane(w);
  const char* const baseA = reinterpret_cast<const char*>(x + (size_t)m0 * K + (size_t)ks0 * 32);
  const char* const baseB = reinterpret_cast<const char*>(W + ((size_t)(n0 >> 4) * KS + ks0) * 64);
  unsigned offA[2][2], offAt[2][2], offB[2];
  if constexpr (FA) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int P = 16 * h + wu + 8 * j;
        const int row = min(m0 + 8 * P + (lane >> 3), M - 1) - m0;
        const int c = (lane & 7) ^ ((P & 1) * 4 + (lane >> 4));  // the chunk stored at cell lane & 7
        offA[h][j] = (unsigned)row * (unsigned)K * 2u + 16u * (unsigned)c;
        // a pair whose second K-tile is past this split's range: re-read the first K-tile into the
        // unused cells (never past the end of a row)
        offAt[h][j] = offA[h][j] - (c >= 4 ? 64u : 0u);
      }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int nt = min((n0 >> 4) + wu + NW * j, NTT - 1) - (n0 >> 4);
      offB[j] = (unsigned)nt * (unsigned)KS * 1024u + 16u * (unsigned)lane;
    }
  }
  auto issueA1 = [&](int p, auto HC, int j) {  // x pair p (K-tiles 2p, 2p+1), half HC of its pieces
    constexpr int h = decltype(HC)::value;
    glds16(baseA + (size_t)p * 128 + (2 * p + 1 >= KT ? offAt[h][j] : offA[h][j]),
           lds + (p % A_SLOTS) * A_PIECES * 64 + (16 * h + wu + 8 * j) * 64);
  };
  auto issueA = [&](int p, auto HC) {
#pragma unroll
    for (int j = 0; j < 2; ++j) issueA1(p, HC, j);
  };
  auto issueB1 = [&](int t, int j) {
    glds16(baseB + (size_t)t * 1024 + offB[j], bring + (t % G2_NBUF) * BF * 64 + (wu + NW * j) * 64);
  };
  auto issueB = [&](int t) {
#pragma unroll
    for (int j = 0; j < 2; ++j) issueB1(t, j);
  };

  f32x4 acc[MT][NTW];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NTW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float ss0 = 0.f, ss1 = 0.f;  // RMS: partial sums of squares of m-tiles RPW*wc (+1) (row lane & 15)
  // The two fragments are re-read from LDS (2 extra ds_read_b128): selecting them out of a[] by the
  // runtime wc makes hipcc move the fragment array to scratch.
  auto sumsq = [&](const u32x4* buf) {
    if constexpr (RMS) {
      const u32x4 f0 = buf[(wr * MT + RPW * wc) * 64 + lane];
      ss0 = dot8_bf16(f0, f0, ss0);
      if constexpr (RPW == 2) {
        const u32x4 f1 = buf[(wr * MT + RPW * wc + 1) * 64 + lane];
        ss1 = dot8_bf16(f1, f1, ss1);
      }
    }
  };

  if constexpr (FA) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
      if (2 * p < KT) {
        issueA(p, std::integral_constant<int, 0>{});
        issueA(p, std::integral_constant<int, 1>{});
      }
#pragma unroll
    for (int t = 0; t < DIST; ++t)
      if (t < KT) issueB(t);
  } else {
#pragma unroll
    for (int t = 0; t < DIST; ++t)
      if (t < KT) issue(t);
  }

  if constexpr (WM == 2) {
    // Ping-pong: wave rows 0 and 1 (one wave of each per SIMD) run one barrier apart, so while
    // one group issues its LDS-DMA + ds_reads (L phase) the other keeps the SIMD's MFMA pipe busy
    // (M phase). Phase p of a wave: L_p = [issue tile p+3; wait own part of tile p+1; ds_read tile p;
    // lgkmcnt(0)] -> barrier -> M_p (32 MFMAs) -> barrier. Group 0's L_p sits between barrier
    // instances 2p and 2p+1, group 1's between 2p+1 and 2p+2, hence:
    //  RAW: every wave retires its part of tile t in L_{t-1}, before instance 2t; group 0 reads t
    //       after instance 2t, group 1 after 2t+1.
    //  WAR: tile t+3 refills tile t-1's slot in L_t; every wave's reads of t-1 completed
    //       (lgkmcnt(0)) in L_{t-1}, before instance 2t.
    // Both groups call 2*KT + 2 barriers (the stagger and the closing one are balanced).
    if (KT > 0) {
      wait_vmcnt<0>();  // tile 0 (and the rest of the prologue) landed; simple, once per WG
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (wr == 1) __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#ifdef JLA_GEMM_STAMPS
    unsigned long long st_l = 0, st_b1 = 0, st_m = 0, st_b2 = 0, st_iss = 0, st_lds = 0, t0, t1;
#define JLA_STAMP(v)                                                                     \
  __builtin_amdgcn_sched_barrier(0);                                                     \
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory");              \
  __builtin_amdgcn_sched_barrier(0);
#else
#define JLA_STAMP(v)
#endif
    if constexpr (FA) {
      // FA main loop, unrolled by K-tile pairs so each step's x issue half (and its LDS read chunk) is a
      // compile-time constant. Same phase/barrier structure as the loop below.
      // vmcnt: every load of K-tile t+1 (its weights and both halves of its x pair) was issued at K-tile
      // t-2 or earlier (or in the drained prologue); this wave's issues of K-tiles t-1 and t may stay in
      // flight: 2 weight + 2 x loads per K-tile while there is something left to issue.
      // FAM (0..4): that many of a K-tile's 4 loads (weights first, then x) are issued from its M phase,
      // spread between the MFMAs, instead of at the head of its L phase (the stamps put the L phase --
      // issue + reads + wait -- above the M phase); at the wait of K-tile t only the L-phase part of
      // K-tile t's loads has been issued.
      constexpr int MB = FAM < 2 ? FAM : 2, MA = FAM - MB;  // moved weight / x loads
      auto fa_cnt = [&](int s, bool l_only) {
        return s < 0 ? 0
                     : (s + DIST < KT ? (l_only ? 2 - MB : 2) : 0) +
                           (2 * ((s >> 1) + 2) < KT ? (l_only ? 2 - MA : 2) : 0);
      };
      auto fa_step = [&](int t, auto HC) {
        constexpr int h = decltype(HC)::value;  // == t & 1
#ifdef JLA_GEMM_STAMPS
        unsigned long long t0, t1;
        JLA_STAMP(t0)
#endif
        const bool more_b = t + DIST < KT, more_a = 2 * ((t >> 1) + 2) < KT;
        if (more_b) {
#pragma unroll
          for (int j = 0; j < 2 - MB; ++j) issueB1(t + DIST, j);
        }
        if (more_a) {
#pragma unroll
          for (int j = 0; j < 2 - MA; ++j) issueA1((t >> 1) + 2, HC, j);
        }
#ifdef JLA_GEMM_STAMPS
        JLA_STAMP(t1) st_iss += t1 - t0; t0 = t1;
#endif
        // row r of the tile, chunk c of its 64-deep pair sits at u32x4 r * 8 + (c ^ ((r & 15) >> 1))
        const u32x4* abuf = lds + ((t >> 1) % A_SLOTS) * A_PIECES * 64;
        const u32x4* bbuf = bring + (t % G2_NBUF) * BF * 64;
        const int ab = (wr * MT * 16 + (lane & 15)) * 8 + ((4 * h + (lane >> 4)) ^ ((lane >> 1) & 7));
        u32x4 a[MT], b[NTW];
#pragma unroll
        for (int j = 0; j < NTW; ++j) b[j] = bbuf[(wc * NTW + j) * 64 + lane];
#pragma unroll
        for (int i = 0; i < MT; ++i) a[i] = abuf[ab + i * 128];
        if constexpr (RMS) {
          const u32x4 f0 = abuf[ab + RPW * wc * 128];
          ss0 = dot8_bf16(f0, f0, ss0);
          if constexpr (RPW == 2) {
            const u32x4 f1 = abuf[ab + (RPW * wc + 1) * 128];
            ss1 = dot8_bf16(f1, f1, ss1);
          }
        }
#ifdef JLA_GEMM_STAMPS
        JLA_STAMP(t1) st_lds += t1 - t0; t0 = t1;
#endif
        if (t >= 1 && t + 4 < KT) {  // steady state: K-tiles t-1 and t issued 2 + 2 loads (t: its L part)
          wait_vmcnt<8 - FAM>();
        } else {
          const int n = fa_cnt(t - 1, false) + fa_cnt(t, true);
          if (n >= 8)
            wait_vmcnt<8>();
          else if (n == 7)
            wait_vmcnt<7>();
          else if (n == 6)
            wait_vmcnt<6>();
          else if (n == 5)
            wait_vmcnt<5>();
          else if (n == 4)
            wait_vmcnt<4>();
          else if (n == 3)
            wait_vmcnt<3>();
          else if (n == 2)
            wait_vmcnt<2>();
          else if (n == 1)
            wait_vmcnt<1>();
          else
            wait_vmcnt<0>();
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#ifdef JLA_GEMM_STAMPS
        JLA_STAMP(t1) st_l += t1 - t0; t0 = t1;
#endif
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
#ifdef JLA_GEMM_STAMPS
        JLA_STAMP(t1) st_b1 += t1 - t0; t0 = t1;
#endif
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < MT; ++i) {
#pragma unroll
          for (int j = 0; j < NTW; ++j) acc[i][j] = mfma16x16x32(a[i], b[j], acc[i][j]);
          // moved load m (0..FAM-1) goes after m-tile (2m + 1) * MT / (2 FAM): weights j = 2-MB.., then x
#pragma unroll
          for (int m = 0; m < FAM; ++m) {
            if (i == (2 * m + 1) * MT / (2 * FAM)) {
              if (m < MB) {
                if (more_b) {
                  __builtin_amdgcn_sched_barrier(0);
                  issueB1(t + DIST, 2 - MB + m);
                  __builtin_amdgcn_sched_barrier(0);
                }
              } else if (more_a) {
                __builtin_amdgcn_sched_barrier(0);
                issueA1((t >> 1) + 2, HC, 2 - MA + (m - MB));
                __builtin_amdgcn_sched_barrier(0);
              }
            }
          }
        }
        __builtin_amdgcn_s_setprio(0);
        asm volatile("" ::: "memory");
#ifdef JLA_GEMM_STAMPS
        JLA_STAMP(t1) st_m += t1 - t0; t0 = t1;
#endif
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
#ifdef JLA_GEMM_STAMPS
        JLA_STAMP(t1) st_b2 += t1 - t0;
#endif
      };
      for (int t = 0; t < KT; t += 2) {
        fa_step(t, std::integral_constant<int, 0>{});
        if (t + 1 < KT) fa_step(t + 1, std::integral_constant<int, 1>{});
      }
    } else
    for (int t = 0; t < KT; ++t) {
      JLA_STAMP(t0)
      if (t + DIST < KT) issue(t + DIST);
      const int after = min(KT - 1, t + DIST) - (t + 1);  // tiles issued after t+1
      auto wait_next = [&]() {
        if (after >= 3)
          wait_vmcnt<3 * G>();
        else if (after == 2)
          wait_vmcnt<2 * G>();
        else if (after == 1)
          wait_vmcnt<G>();
        else
          wait_vmcnt<0>();
      };
      if constexpr (!LATE_WAIT) wait_next();
#ifdef JLA_GEMM_STAMPS
      JLA_STAMP(t1) st_iss += t1 - t0; t0 = t1;
#endif
      const u32x4* buf = lds + (t % G2_NBUF) * FR * 64;
      u32x4 a[MT], b[NTW];
#pragma unroll
      for (int j = 0; j < NTW; ++j) b[j] = buf[(AF + wc * NTW + j) * 64 + lane];
#pragma unroll
      for (int i = 0; i < MT; ++i) a[i] = buf[(wr * MT + i) * 64 + lane];
      sumsq(buf);
#ifdef JLA_GEMM_STAMPS
      JLA_STAMP(t1) st_lds += t1 - t0; t0 = t1;
#endif
      // LATE_WAIT: tile t+1 only has to land before this phase's barrier, not before tile t's reads
      if constexpr (LATE_WAIT) wait_next();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#ifdef JLA_GEMM_STAMPS
      JLA_STAMP(t1) st_l += t1 - t0; t0 = t1;
#endif
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
#ifdef JLA_GEMM_STAMPS
      JLA_STAMP(t1) st_b1 += t1 - t0; t0 = t1;
#endif
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NTW; ++j) acc[i][j] = mfma16x16x32(a[i], b[j], acc[i][j]);
      __builtin_amdgcn_s_setprio(0);
      asm volatile("" ::: "memory");
#ifdef JLA_GEMM_STAMPS
      JLA_STAMP(t1) st_m += t1 - t0; t0 = t1;
#endif
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
#ifdef JLA_GEMM_STAMPS
      JLA_STAMP(t1) st_b2 += t1 - t0;
#endif
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();
#ifdef JLA_GEMM_STAMPS
    if (lane == 0 && MODE == MODE_STORE) {
      unsigned long long* d = g_gemm_stamps + ((size_t)blockIdx.x * NW + w) * 6;
      d[0] = st_l;
      d[1] = st_b1;
      d[2] = st_m;
      d[3] = st_b2;
      d[4] = st_iss;
      d[5] = st_lds;
    }
#endif
  } else
  for (int t = 0; t < KT; ++t) {
    const int ahead = min(KT - 1 - t, DIST - 1);  // tiles issued after t
    if (ahead >= 3)
      wait_vmcnt<3 * G>();
    else if (ahead == 2)
      wait_vmcnt<2 * G>();
    else if (ahead == 1)
      wait_vmcnt<G>();
    else
      wait_vmcnt<0>();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + DIST < KT) issue(t + DIST);  // refills the buffer read at t-1 (retired by the barrier)
    const u32x4* buf = lds + (t % G2_NBUF) * FR * 64;
    u32x4 a[MT], b[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j) b[j] = buf[(AF + wc * NTW + j) * 64 + lane];
#pragma unroll
    for (int i = 0; i < MT; ++i) a[i] = buf[(wr * MT + i) * 64 + lane];
    sumsq(buf);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NTW; ++j) acc[i][j] = mfma16x16x32(a[i], b[j], acc[i][j]);
  }

  if constexpr (RMS) {
    // complete each row's sum over the 4 lanes that hold its k-chunks (lane >> 4)
    ss0 += __shfl_xor(ss0, 16, 64);
    ss0 += __shfl_xor(ss0, 32, 64);
    ss1 += __shfl_xor(ss1, 16, 64);
    ss1 += __shfl_xor(ss1, 32, 64);
  }
  if constexpr (RMS) {
    const int rA = m0 + (wr * MT + RPW * wc) * 16 + (lane & 15), rB = rA + 16;
    if constexpr (MODE == MODE_PARTIAL) {
      if (lane < 16) {
        if (rA < M) ssq_ws[(size_t)split * M + rA] = ss0;
        if (RPW == 2 && rB < M) ssq_ws[(size_t)split * M + rB] = ss1;
      }
    } else {
      // publish the row statistics through LDS (the tile buffers are free once every wave is past
      // its last ds_read), then scale every accumulator row
      float* rs = reinterpret_cast<float*>(lds);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __syncthreads();
      if (lane < 16) {
        // (t / K exactly as gemm_reduce_kernel: split and unsplit plans agree bit for bit)
        const float fk = (float)K;
        rs[(wr * MT + RPW * wc) * 16 + lane] = 1.f / sqrtf(ss0 / fk + rms_eps);
        if constexpr (RPW == 2) rs[(wr * MT + RPW * wc + 1) * 16 + lane] = 1.f / sqrtf(ss1 / fk + rms_eps);
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float sc = rs[(wr * MT + i) * 16 + 4 * (lane >> 4) + r];
#pragma unroll
          for (int j = 0; j < NTW; ++j) acc[i][j][r] *= sc;
        }
    }
  }

  const int c = lane & 15;
  if constexpr (MODE == MODE_SWIGLU) {
    const int F = N >> 1;
    bf16_t* o = static_cast<bf16_t*>(out);
#pragma unroll
    for (int j = 0; j < NTW; j += 2) {
      const int gtile = (n0 >> 4) + wc * NTW + j;  // even: gate tile, gtile + 1: its up tile
      if (gtile >= NTT) continue;
      const int col = (gtile >> 1) * 16 + c;
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = m0 + (wr * MT + i) * 16 + 4 * (lane >> 4) + r;
          if (row < M) o[(size_t)row * F + col] = f2bf(silu(acc[i][j][r]) * acc[i][j + 1][r]);
        }
    }
  } else if constexpr (MODE == MODE_ARGMAX) {
    // greedy lm_head: the logits never leave the registers. Per row, the first maximum over this
    // wave's 64 columns (lane: its 4 columns in ascending order, strict >; then the 16 lanes of the
    // row, ties to the smaller index) -> one (value, index) partial at [row][n0 / 64 + wc] of `out`;
    // argmax_partials_kernel finishes the row (same result as argmax over the stored fp32 logits).
    float2* o = static_cast<float2*>(out);
    const int P = tiles_n * (BN / (16 * NTW)), slot = (n0 >> 6) + wc;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
          const int tile = (n0 >> 4) + wc * NTW + j;
          const float v = acc[i][j][r];
          if (tile < NTT && v > bv) {
            bv = v;
            bi = tile * 16 + c;
          }
        }
#pragma unroll
        for (int sh = 1; sh < 16; sh <<= 1) {
          const float ov = __shfl_xor(bv, sh, 64);
          const int oi = __shfl_xor(bi, sh, 64);
          if (ov > bv || (ov == bv && oi < bi)) {
            bv = ov;
            bi = oi;
          }
        }
        const int row = m0 + (wr * MT + i) * 16 + 4 * (lane >> 4) + r;
        if (c == 0 && row < M) o[(size_t)row * P + slot] = make_float2(bv, __int_as_float(bi));
      }
  } else if constexpr (MODE == MODE_QKV) {
    // fused qkv projection without a K split (decode B = 2048, prefill): the (norm-scaled) accumulators are staged
    // through LDS one wave row (128 x 256 fp32) at a time, then every thread takes 4 consecutive columns of a row --
    // two RoPE pairs -- rotates the q / k heads and writes q, or the k / v cache row at slot[0] + (position in the
    // sequence), 8 bytes per store; replaces the bf16 store + rope_kv_kernel round trip (same arithmetic as
    // gemm_reduce_kernel<MODE_QKV>; reference model.py:58-92, :169-199)
    static_assert(WM == 2 && MT == 8 && NTW == 4, "QKV epilogue: 256 x 256 tiles");
    float* ep = reinterpret_cast<float*>(lds);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();  // every wave is past its last read of the tile buffers
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      if (wr == half) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NTW; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = i * 16 + 4 * (lane >> 4) + r;
              const int col = ((wc * NTW + j) * 16 + c) ^ (((row >> 2) & 3) << 4);
              ep[row * BN + col] = acc[i][j][r];
            }
      }
      __syncthreads();
#pragma unroll 2
      for (int qq = 0; qq < 16; ++qq) {
        const int e = threadIdx.x + 512 * qq;
        const int row = e >> 6, c4 = (e & 63) * 4;
        const int grow = m0 + half * 128 + row, gcol = n0 + c4;
        const float4 v = *reinterpret_cast<const float4*>(ep + row * BN + (c4 ^ (((row >> 2) & 3) << 4)));
        if (grow >= M || gcol >= N) continue;
        float v0 = v.x, v1 = v.y, v2 = v.z, v3 = v.w;
        const int head = gcol / qa.Dh, d0 = gcol - head * qa.Dh;
        const int b = grow / qa.S, sq = grow - b * qa.S;
        if (head < qa.H + qa.Hkv) {
          int pos = qa.positions[grow];
          if (pos < 0 || pos >= qa.table_len) JLA_FLAG(JLA_BOUNDS_ROPE_POS);
          pos = pos < 0 ? 0 : (pos >= qa.table_len ? qa.table_len - 1 : pos);
          const float4 cs = *reinterpret_cast<const float4*>(qa.table + (size_t)pos * (qa.Dh >> 1) + (d0 >> 1));
          const float r0 = v0 * cs.x - v1 * cs.y, r1 = v0 * cs.y + v1 * cs.x;
          const float r2 = v2 * cs.z - v3 * cs.w, r3 = v2 * cs.w + v3 * cs.z;
          v0 = r0;
          v1 = r1;
          v2 = r2;
          v3 = r3;
        }
        const uint2 packed = make_uint2(pack2bf(v0, v1), pack2bf(v2, v3));
        if (head < qa.H) {
          *reinterpret_cast<uint2*>(qa.q + ((size_t)grow * qa.H + head) * qa.Dh + d0) = packed;
        } else {
          const int cslot = qa.slot[0] + sq;
          if (cslot < qa.T) {
            const bool is_k = head < qa.H + qa.Hkv;
            const int kh = is_k ? head - qa.H : head - qa.H - qa.Hkv;
            bf16_t* cache = is_k ? qa.kc : qa.vc;
            *reinterpret_cast<uint2*>(cache + (((size_t)b * qa.Hkv + kh) * qa.T + cslot) * qa.Dh + d0) = packed;
          } else {
            JLA_FLAG(JLA_BOUNDS_KV_SLOT);
          }
        }
      }
      __syncthreads();  // the half-tile is consumed before the other wave row overwrites it
    }
  } else {
    // rows outer, n-tiles inner: a row's adjacent 64-byte pieces back to back (as gemm4's fp32 epilogue; 2-4 % on the
    // split qkv / gate_up slabs and the residual o, profiles/r6_g2_epilogue_order_ab.jsonl); residual: the m-tile's h
    // values loaded before any is used (one round trip per m-tile, not per value)
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      float hv[4][NTW];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < NTW; ++j) hv[r][j] = 0.f;
      if constexpr (MODE == MODE_RESIDUAL) {
        if (accumulate) {  // (unconditional loads at clamped addresses: no per-load branch and join wait)
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < NTW; ++j) {
              const int tile = min((n0 >> 4) + wc * NTW + j, NTT - 1);
              const int row = min(m0 + (wr * MT + i) * 16 + 4 * (lane >> 4) + r, M - 1);
              hv[r][j] = static_cast<const float*>(out)[(size_t)row * N + tile * 16 + c];
            }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < NTW; ++j) {
          const int tile = (n0 >> 4) + wc * NTW + j;
          const int row = m0 + (wr * MT + i) * 16 + 4 * (lane >> 4) + r;
          if (tile >= NTT || row >= M) continue;
          const size_t idx = (size_t)row * N + tile * 16 + c;
          const float v = acc[i][j][r];
          if constexpr (MODE == MODE_PARTIAL) {
            static_cast<float*>(out)[(size_t)split * M * N + idx] = v;
          } else if constexpr (MODE == MODE_RESIDUAL) {
            const float nv = hv[r][j] + v;
            static_cast<float*>(out)[idx] = nv;
            if (mirror) mirror[idx] = f2bf(nv);
          } else if (out_f32) {
            static_cast<float*>(out)[idx] = v;
          } else {
            static_cast<bf16_t*>(out)[idx] = f2bf(v);
          }
        }
    }
  }
}


// ---------------------------------------------------------------------------------------------
// gemm4: the 4-wave 256 x 256 main loop of gemm4w.h (one wave per SIMD, 128 x 128 per wave, 64-deep K-tiles)
// with every epilogue of gemm2. The accumulators are C^T fragments: lane (c = lane & 15, q = lane >> 4) holds,
// per (n-tile j, m-tile i) of its wave block, output row m0 + wr*128 + 16i + c at the 4 consecutive columns
// n0 + wc*128 + 16j + 4q + 0..3 -- so SwiGLU gate/up pairs (adjacent n-tiles), RoPE pairs (adjacent columns) and
// the fp32 residual (one float4) are all in-lane, and every store is 8 or 16 bytes. Split-K: MODE_PARTIAL slabs
// [split][M][N] (+ the fused-RMS partial sums [split][M]) summed by gemm_reduce_kernel, as gemm2's.
// RMSM (fused RMSNorm statistic): 0 none; 1 summed inside the main loop from the x fragments (split-K partial
// slabs: per-split sums to ssq_ws); 2 read from rms_inv[M], computed ahead of the GEMM by rms_rowinv_kernel.
// The epilogue of one gemm4 output tile (every mode; see gemm4_kernel), shared by the data-parallel, persistent and
// tail-balanced launches. acc: this wave's finished C^T accumulators; ss: the in-loop RMS partial sums (RMSM 1).
struct G4Epi {
  void* out;
  int M, N, K, accumulate, out_f32;
  bf16_t* mirror;
  int tiles_n;
  float rms_eps;
  float* ssq_ws;
  const float* rms_inv;
};
template <int MODE, int RMSM, typename Acc, int NJ = 8>
JLA_DEV void g4_epilogue(Acc& acc, float* ss, u32x4* lds, int wu, int lane, int m0, int n0, int split,
                         const G4Epi& ep, const QKVArgs& qa) {
  constexpr bool RMS = RMSM == 1;
  static_assert(NJ == 8 || (RMSM != 1 && MODE != MODE_ARGMAX && MODE != MODE_LOGPROB),
                "the 256 x 128 / 192 tiles: precomputed norm statistic; no argmax / log-prob epilogue");
  constexpr int WN = 16 * NJ;  // output columns of a wave block
  constexpr int PJ = NJ == 6 ? 8 : NJ;  // staged row width in n-tiles (a power of two; NJ = 6 leaves the rest unused)
  const int wr = wu >> 1, wc = wu & 1;
  void* const out = ep.out;
  const int M = ep.M, N = ep.N, K = ep.K, accumulate = ep.accumulate, out_f32 = ep.out_f32;
  bf16_t* const mirror = ep.mirror;
  const int tiles_n = ep.tiles_n;
  const float rms_eps = ep.rms_eps;
  float* const ssq_ws = ep.ssq_ws;
  const float* const rms_inv = ep.rms_inv;
  (void)K, (void)tiles_n, (void)rms_eps, (void)ssq_ws, (void)rms_inv, (void)split, (void)accumulate, (void)out_f32,
      (void)mirror, (void)wc;
  const int c = lane & 15, q = lane >> 4, NTT = N >> 4;
  const int rbase = m0 + wr * 128 + c;  // + 16 i: this lane's output row in m-tile i
  float sc[8];                           // RMS: per m-tile row scale
  if constexpr (RMSM == 2) {
#pragma unroll
    for (int i = 0; i < 8; ++i) sc[i] = rms_inv[min(rbase + 16 * i, M - 1)];
  }
  if constexpr (RMS) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // complete each row's sum over the 4 lanes holding its k-chunks
      ss[i] += __shfl_xor(ss[i], 16, 64);
      ss[i] += __shfl_xor(ss[i], 32, 64);
    }
    if constexpr (MODE == MODE_PARTIAL) {
      if (q == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = m0 + wr * 128 + (4 * wc + i) * 16 + c;
          if (row < M) ssq_ws[(size_t)split * M + row] = ss[i];
        }
      }
    } else {
      float* rs = reinterpret_cast<float*>(lds + 8192);  // beside the 128 KiB staging space
      __syncthreads();  // every wave is past its last fragment read
      if (q == 0) {
        const float fk = (float)K;  // (t / K exactly as gemm_reduce_kernel and gemm2)
#pragma unroll
        for (int i = 0; i < 4; ++i) rs[wr * 128 + (4 * wc + i) * 16 + c] = 1.f / sqrtf(ss[i] / fk + rms_eps);
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 8; ++i) sc[i] = rs[wr * 128 + 16 * i + c];
    }
  }
  // one accumulator tile at a time, scaled by its row's norm: g4_take keeps hipcc from copying all 256 AGPRs to
  // VGPRs at once (which spilled)
  auto tile_val = [&](int j, int i) -> f32x4 {
    f32x4 v = g4_take(acc[j][i]);
    if constexpr (RMSM != 0 && MODE != MODE_PARTIAL) v *= sc[i];
    return v;
  };

  // bf16 outputs go through the wave's 32 KiB of LDS (g4_stage_put / g4_stage_rows); every wave must be past its
  // last fragment read first (the RMS path above already synchronised)
  char* const wl = reinterpret_cast<char*>(lds) + wu * 32768;
  constexpr bool STAGED = MODE == MODE_SWIGLU || MODE == MODE_QKV || MODE == MODE_STORE;
  if constexpr (STAGED && !(RMS && MODE != MODE_PARTIAL)) __syncthreads();
  const int mrow0 = m0 + wr * 128;  // first output row of the wave block
  if constexpr (MODE == MODE_SWIGLU) {
    // gate tile j (even) and up tile j + 1 -> 16 activation columns; the wave block's 64 columns = 128-byte rows
    const int F = N >> 1;
    bf16_t* o = static_cast<bf16_t*>(out);
#pragma unroll
    for (int j = 0; j < NJ; j += 2) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const f32x4 gv = tile_val(j, i), uv = tile_val(j + 1, i);
        const u32x2 p = {pack2bf(silu(gv[0]) * uv[0], silu(gv[1]) * uv[1]),
                         pack2bf(silu(gv[2]) * uv[2], silu(gv[3]) * uv[3])};
        g4_stage_put<16 * PJ>(wl, 16 * i + c, 16 * j + 8 * q, p);
      }
    }
    const int fcol0 = ((n0 >> 4) + wc * NJ) * 8;  // first activation column of the wave block
    g4_stage_rows<16 * PJ>(wl, lane, [&](int r, int ch, u32x4 v) {
      const int row = mrow0 + r, col = fcol0 + 8 * ch;
      if (row < M && col < F && ch < NJ) *reinterpret_cast<u32x4*>(o + (size_t)row * F + col) = v;
    });
  } else if constexpr (MODE == MODE_ARGMAX) {
    // per row: the first maximum over this wave's 128 columns -> one (value, index) partial at
    // [row][n0 / 128 + wc] (P = 2 tiles_n slots per row); argmax_partials_kernel finishes the row
    float2* o = static_cast<float2*>(out);
    const int P = tiles_n * 2, slot = (n0 >> 7) + wc;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float bv = -INFINITY;
      int bi = 0x7fffffff;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int tile = (n0 >> 4) + wc * 8 + j;
        const f32x4 tv = tile_val(j, i);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = tv[r];
          if (tile < NTT && v > bv) {  // ascending columns in-lane, strict >: the first max
            bv = v;
            bi = tile * 16 + 4 * q + r;
          }
        }
      }
#pragma unroll
      for (int sh = 16; sh < 64; sh <<= 1) {
        const float ov = __shfl_xor(bv, sh, 64);
        const int oi = __shfl_xor(bi, sh, 64);
        if (ov > bv || (ov == bv && oi < bi)) {
          bv = ov;
          bi = oi;
        }
      }
      const int row = rbase + 16 * i;
      if (q == 0 && row < M) o[(size_t)row * P + slot] = make_float2(bv, __int_as_float(bi));
    }
  } else if constexpr (MODE == MODE_LOGPROB) {
    // per row over this wave's 128 columns: m = the maximum and s = sum exp(v - m) of the valid ones -> one (m, s)
    // partial at [row][n0 / 128 + wc] (the argmax partials' layout; lse_partials_kernel finishes the row), and the
    // logit at the row's target column, stored by the one lane of the grid that holds it. A wave block with no valid
    // column writes (-inf, 0), the identity of every merge. Two passes over the accumulators (the maximum, then the
    // sum against it), in a fixed order and without atomics: the same bits on every call.
    float2* o = static_cast<float2*>(out);
    const int P = tiles_n * 2, slot = (n0 >> 7) + wc, tile0 = (n0 >> 4) + wc * 8;
    const int32_t* const targets = qa.lp_targets;
    float* const tgt = qa.lp_tgt;
    const int col_offset = qa.lp_col_offset;
    // the targets of this lane's 8 rows, loaded as one batch -> the n-tile of this wave block (0..7) in which this
    // lane holds the target column, or -1 (another lane's, another wave's, an ignored label, another rank's shard)
    int tg[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) tg[i] = targets[min(rbase + 16 * i, M - 1)];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int col = tg[i] - col_offset;
      const bool mine = col >= 0 && col < N && ((col >> 2) & 3) == q && (unsigned)((col >> 4) - tile0) < 8u;
      tg[i] = mine ? (((col >> 4) - tile0) << 2 | (col & 3)) : -1;
    }
    constexpr float LOG2E = 1.4426950408889634f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float m = -INFINITY, tv_t = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const f32x4 tv = tile_val(j, i);
        if (tile0 + j < NTT) m = fmaxf(fmaxf(m, fmaxf(tv[0], tv[1])), fmaxf(tv[2], tv[3]));
        if ((tg[i] >> 2) == j) {  // (-1 >> 2 = -1: never)
          const int r = tg[i] & 3;
          tv_t = r == 0 ? tv[0] : (r == 1 ? tv[1] : (r == 2 ? tv[2] : tv[3]));
        }
      }
      m = fmaxf(m, __shfl_xor(m, 16, 64));
      m = fmaxf(m, __shfl_xor(m, 32, 64));
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const f32x4 tv = tile_val(j, i);
        if (tile0 + j < NTT) {  // (a valid column makes m finite: no inf - inf)
#pragma unroll
          for (int r = 0; r < 4; ++r) s += __builtin_amdgcn_exp2f((tv[r] - m) * LOG2E);
        }
      }
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      const int row = rbase + 16 * i;
      if (row < M) {
        if (q == 0) o[(size_t)row * P + slot] = make_float2(m, s);
        if (tg[i] >= 0) tgt[row] = tv_t;
      }
    }
  } else if constexpr (MODE == MODE_QKV) {
    // RoPE on the two (even, odd) pairs of the lane's 4 columns in fp32, then staged: 16-byte pieces of a row go to
    // q or to the k / v cache row at slot[0] + (position in the sequence); same arithmetic as gemm2's /
    // gemm_reduce_kernel's QKV epilogue (reference model.py:58-92, :169-199)
    // the positions of this lane's 8 rows, then per n-tile the 8 rows' RoPE factors, each batch loaded before any
    // value is used (loaded where used, behind the staged stores, they went one memory round trip at a time)
    int posr[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) posr[i] = qa.positions[min(rbase + 16 * i, M - 1)];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (posr[i] < 0 || posr[i] >= qa.table_len) JLA_FLAG(JLA_BOUNDS_ROPE_POS);
      posr[i] = posr[i] < 0 ? 0 : (posr[i] >= qa.table_len ? qa.table_len - 1 : posr[i]);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int gcol = n0 + wc * WN + 16 * j + 4 * q;
      const int head = gcol / qa.Dh, d0 = gcol - head * qa.Dh;
      float4 cs[8];  // (loaded for every head; used for q and k)
#pragma unroll
      for (int i = 0; i < 8; ++i)
        cs[i] = *reinterpret_cast<const float4*>(qa.table + (size_t)posr[i] * (qa.Dh >> 1) + (d0 >> 1));
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const f32x4 tv = tile_val(j, i);
        float v0 = tv[0], v1 = tv[1], v2 = tv[2], v3 = tv[3];
        if (head < qa.H + qa.Hkv) {
          const float r0 = v0 * cs[i].x - v1 * cs[i].y, r1 = v0 * cs[i].y + v1 * cs[i].x;
          const float r2 = v2 * cs[i].z - v3 * cs[i].w, r3 = v2 * cs[i].w + v3 * cs[i].z;
          v0 = r0;
          v1 = r1;
          v2 = r2;
          v3 = r3;
        }
        g4_stage_put<256>(wl, 16 * i + c, 32 * j + 8 * q, u32x2{pack2bf(v0, v1), pack2bf(v2, v3)});
      }
    }
    g4_stage_rows<256>(wl, lane, [&](int r, int ch, u32x4 v) {
      const int grow = mrow0 + r, gcol = n0 + wc * WN + 8 * ch;
      if (grow >= M || gcol >= N || 8 * ch >= WN) return;
      const int head = gcol / qa.Dh, d0 = gcol - head * qa.Dh;
      if (head < qa.H) {
        *reinterpret_cast<u32x4*>(qa.q + ((size_t)grow * qa.H + head) * qa.Dh + d0) = v;
      } else {
        const int b = grow / qa.S, sq = grow - b * qa.S;
        const int cslot = qa.slot[0] + sq;
        if (cslot < qa.T) {
          const bool is_k = head < qa.H + qa.Hkv;
          const int kh = is_k ? head - qa.H : head - qa.H - qa.Hkv;
          bf16_t* cache = is_k ? qa.kc : qa.vc;
          *reinterpret_cast<u32x4*>(cache + (((size_t)b * qa.Hkv + kh) * qa.T + cslot) * qa.Dh + d0) = v;
        } else {
          JLA_FLAG(JLA_BOUNDS_KV_SLOT);
        }
      }
    });
  } else if constexpr (MODE == MODE_STORE) {
    if (out_f32) {  // fp32 logits (16-byte pieces, direct)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int tile = (n0 >> 4) + wc * NJ + j;
        if (tile >= NTT) continue;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int row = rbase + 16 * i;
          const f32x4 v = tile_val(j, i);
          if (row < M) *reinterpret_cast<f32x4*>(static_cast<float*>(out) + (size_t)row * N + tile * 16 + 4 * q) = v;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const f32x4 v = tile_val(j, i);
          g4_stage_put<32 * PJ>(wl, 16 * i + c, 32 * j + 8 * q, u32x2{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])});
        }
      bf16_t* o = static_cast<bf16_t*>(out);
      g4_stage_rows<32 * PJ>(wl, lane, [&](int r, int ch, u32x4 v) {
        const int row = mrow0 + r, col = n0 + wc * WN + 8 * ch;
        if (row < M && col < N && 8 * ch < WN) *reinterpret_cast<u32x4*>(o + (size_t)row * N + col) = v;
      });
    }
  } else {  // PARTIAL / RESIDUAL: fp32, one 16-byte piece per lane per tile
    // rows outer, tiles inner: consecutive instructions take the two 64-byte halves of each 128-byte line of h (and the
    // adjacent 32-byte pieces of the mirror's line) back to back -- 4-7 % faster than tiles outer on the o projection,
    // 1.5-3.5 % on down, M = 4096 and 32768 (profiles/r6_g4_epilogue_order_ab.jsonl)
    // residual: a row's h pieces of every tile are loaded before any is used -- with the stores in between (which may
    // alias h as far as hipcc knows) the loads were issued one at a time, a full memory round trip per 16-byte piece
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = rbase + 16 * i;
      f32x4 hv[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) hv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (MODE == MODE_RESIDUAL) {
        if (accumulate) {  // (unconditional loads at clamped addresses: a per-load branch made hipcc wait at each join)
          const float* hrow = static_cast<const float*>(out) + (size_t)min(row, M - 1) * N + 4 * q;
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            hv[j] = *reinterpret_cast<const f32x4*>(hrow + min((n0 >> 4) + wc * NJ + j, NTT - 1) * 16);
        }
      }
      // every result of the row first, then the stores (a store between two uses made hipcc wait for the store too)
#pragma unroll
      for (int j = 0; j < NJ; ++j) hv[j] += tile_val(j, i);  // (accumulate 0 / partial: hv is zero, 0 + v = v exactly)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int tile = (n0 >> 4) + wc * NJ + j;
        if (tile >= NTT || row >= M) continue;
        const size_t idx = (size_t)row * N + tile * 16 + 4 * q;
        if constexpr (MODE == MODE_PARTIAL) {
          *reinterpret_cast<f32x4*>(static_cast<float*>(out) + (size_t)split * M * N + idx) = hv[j];
        } else {
          *reinterpret_cast<f32x4*>(static_cast<float*>(out) + idx) = hv[j];
          if (mirror)
            *reinterpret_cast<u32x2*>(mirror + idx) = u32x2{pack2bf(hv[j][0], hv[j][1]), pack2bf(hv[j][2], hv[j][3])};
        }
      }
    }
  }
}

template <int MODE, int RMSM, int NJ = 8, int DIAG = 0, bool W3 = false>
__global__ void __launch_bounds__(256, 1)
    gemm4_kernel(const bf16_t* __restrict__ x, const u32x4* __restrict__ W, void* __restrict__ out, int M, int N,
                 int K, int accumulate, int out_f32, bf16_t* __restrict__ mirror, int kc, int tiles_m, int tiles_n,
                 float rms_eps, float* __restrict__ ssq_ws, QKVArgs qa, const float* __restrict__ rms_inv,
                 int group_m) {
  constexpr bool RMS = RMSM == 1;
  // the two K-tile slots (W3: two x + three W slots, all 160 KiB); after the loop: the epilogue's staging (128 KiB)
  // + 1 KiB of row scales
  __shared__ u32x4 lds[W3 ? 2 * G4_A_U4 + 3 * G4_B_U4 : 2 * G4_SLOT_U4 + 64];
  const int lane = threadIdx.x & 63;
  const int wu = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wr = wu >> 1, wc = wu & 1;
  // XCD-aware bijective remap, then (split, M-grouped tile) order (as gemm2)
  const int nwg = gridDim.x, orig = blockIdx.x;
  const int xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
  const int tiles = tiles_m * tiles_n;
  const int split = wgid / tiles, pid = wgid - split * tiles;
  int tm, tn;
  g4_tile_coords(pid, tiles_m, tiles_n, tm, tn, group_m);
  const int m0 = tm * G4_BM, n0 = tn * (32 * NJ);
  const int t0 = split * kc, KT = min(K >> 6, t0 + kc) - t0;

  f32x4 acc[NJ][8];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float ss[4] = {0.f, 0.f, 0.f, 0.f};
  const G4Args g{x, W, out, M, N, K, kc, tiles_m, tiles_n};
  if constexpr (NJ != 8) {
    static_assert(!RMS, "the 256 x 128 tile: precomputed statistic");
    g4n_mainloop<NJ, decltype(acc), W3>(g, lds, m0, n0, t0, KT, wu, lane, acc);
  } else {
    g4_mainloop<RMS, decltype(acc), DIAG, W3>(g, lds, m0, n0, t0, KT, wu, lane, acc, ss);
  }
  g4_epilogue<MODE, RMSM, decltype(acc), NJ>(
      acc, ss, lds, wu, lane, m0, n0, split,
      G4Epi{out, M, N, K, accumulate, out_f32, mirror, tiles_n, rms_eps, ssq_ws, rms_inv}, qa);
}

// Persistent gemm4 (tile config 13): one workgroup per CU walks the launch order round by round (tile wg, wg + CUs,
// ...), so a CU's next tile starts without a workgroup teardown and relaunch, and the CUs drift apart over the rounds:
// their epilogues (the residual's fp32 read-modify-write above all) stop arriving at HBM as one chip-wide burst.
template <int MODE, int RMSM>
__global__ void __launch_bounds__(256, 1)
    gemm4p_kernel(const bf16_t* __restrict__ x, const u32x4* __restrict__ W, void* __restrict__ out, int M, int N,
                  int K, int accumulate, int out_f32, bf16_t* __restrict__ mirror, int tiles_m, int tiles_n,
                  float rms_eps, QKVArgs qa, const float* __restrict__ rms_inv, int group_m) {
  constexpr bool RMS = RMSM == 1;
  __shared__ u32x4 lds[2 * G4_SLOT_U4 + 64];
  const int lane0 = threadIdx.x & 63;
  const int wu = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nwg = gridDim.x, orig = blockIdx.x;
  const int xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wg = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
  const int tiles = tiles_m * tiles_n;
  const G4Args g{x, W, out, M, N, K, K >> 6, tiles_m, tiles_n};
  const G4Epi ep{out, M, N, K, accumulate, out_f32, mirror, tiles_n, rms_eps, nullptr, rms_inv};
  for (int pid = wg; pid < tiles; pid += nwg) {
    int tm, tn;
    g4_tile_coords(pid, tiles_m, tiles_n, tm, tn, group_m);
    const int m0 = tm * G4_BM, n0 = tn * G4_BN;
    // the lane index laundered once per tile: the lane-dependent address math of the main loop and the unrolled
    // epilogue would otherwise be hoisted out of the tile loop and kept live (spills)
    int lane;
    asm volatile("v_mov_b32 %0, %1" : "=v"(lane) : "v"(lane0));
    f32x4 acc[8][8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float ss[4] = {0.f, 0.f, 0.f, 0.f};
    g4_mainloop<RMS>(g, lds, m0, n0, 0, K >> 6, wu, lane, acc, ss);
    g4_epilogue<MODE, RMSM>(acc, ss, lds, wu, lane, m0, n0, 0, ep, qa);
    __syncthreads();  // the epilogue's staging / row scales are done with LDS before the next tile's DMA
  }
}

// Tail-balanced gemm4 (tile configs 18 / 19): the columns [0, nb * 32 NJB) are cut into nb n-tiles of 32 NJB columns
// (NJB = 6 / 8: 192 / 256), the rest into nt n-tiles of 128 -- so that a grid whose last round would leave CUs idle
// (Llama-3-8B gate_up at M = 2048: 1200 tiles of 256 x 192 = 4.69 rounds of 256 CUs) becomes whole rounds of wide
// tiles plus one round of narrow ones (1024 + 256 workgroups). A workgroup is a body or a tail tile by its dispatch
// order (the tail workgroups are the last launched), each region with its own XCD remap and m-grouped order. Every
// workgroup is independent, and runs the main loop and epilogue of the uniform grids (same K order per output
// element: bit for bit the results of tiles 14 / 16 / 17). No K split, no QKV / argmax epilogue, the norm statistic
// precomputed (RMSM 0 / 2).
template <int MODE, int RMSM, int NJ>
JLA_DEV void g4t_tile(const G4Args& g, const G4Epi& ep, u32x4* lds, int m0, int n0, int wu, int lane) {
  f32x4 acc[NJ][8];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float ss[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (NJ != 8) {
    g4n_mainloop<NJ, decltype(acc), true>(g, lds, m0, n0, 0, g.K >> 6, wu, lane, acc);
  } else {
    g4_mainloop<false, decltype(acc), 0, true>(g, lds, m0, n0, 0, g.K >> 6, wu, lane, acc, ss);
  }
  g4_epilogue<MODE, RMSM, decltype(acc), NJ>(acc, ss, lds, wu, lane, m0, n0, 0, ep, QKVArgs{});
}

// XCD-aware bijective remap of workgroup `orig` of a region of nwg workgroups (as gemm4_kernel's over the grid; a
// region that starts at a multiple of 8 keeps orig & 7 = the XCD)
JLA_DEV int g4t_remap(int orig, int nwg) {
  const int xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
}

template <int MODE, int RMSM, int NJB>
__global__ void __launch_bounds__(256, 1)
    gemm4t_kernel(const bf16_t* __restrict__ x, const u32x4* __restrict__ W, void* __restrict__ out, int M, int N,
                  int K, int accumulate, int out_f32, bf16_t* __restrict__ mirror, int tiles_m, int nb, int nt,
                  float rms_eps, const float* __restrict__ rms_inv, int group_m) {
  static_assert(NJB == 6 || NJB == 8, "body tiles: 256 x 192 / 256 x 256");
  static_assert(RMSM != 1 && MODE != MODE_ARGMAX && MODE != MODE_QKV && MODE != MODE_PARTIAL, "see above");
  __shared__ u32x4 lds[2 * G4_A_U4 + 3 * G4_B_U4];  // two x + three W slots (160 KiB), both widths
  const int lane = threadIdx.x & 63;
  const int wu = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int body = tiles_m * nb, orig = blockIdx.x;
  const G4Epi ep{out, M, N, K, accumulate, out_f32, mirror, 0, rms_eps, nullptr, rms_inv};
  int tm, tn;
  if (orig < body) {
    g4_tile_coords(g4t_remap(orig, body), tiles_m, nb, tm, tn, group_m);
    const G4Args g{x, W, out, M, N, K, K >> 6, tiles_m, nb};
    g4t_tile<MODE, RMSM, NJB>(g, ep, lds, tm * G4_BM, tn * (32 * NJB), wu, lane);
  } else {
    g4_tile_coords(g4t_remap(orig - body, tiles_m * nt), tiles_m, nt, tm, tn, group_m);
    const G4Args g{x, W, out, M, N, K, K >> 6, tiles_m, nt};
    g4t_tile<MODE, RMSM, 4>(g, ep, lds, tm * G4_BM, nb * (32 * NJB) + tn * 128, wu, lane);
  }
}

// Sum of the ksplit fp32 slabs at float4 e4 in split order: the loads of up to 8 splits are issued before the first
// add (the round-4 loop waited on each split in turn: 12 dependent L2/HBM round trips for the 70B shard's qkv at M =
// 256, 9 us for 1.3 MB of output). Same addition order as before, so bit for bit the same sums.
__device__ __forceinline__ float4 sum_splits(const float* __restrict__ ws, int ksplit, size_t slab4, size_t e4) {
  const float4* p = reinterpret_cast<const float4*>(ws) + e4;
  float4 v = p[0];
  for (int s0 = 1; s0 < ksplit; s0 += 8) {
    float4 q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (s0 + j < ksplit) q[j] = p[(size_t)(s0 + j) * slab4];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (s0 + j < ksplit) {
        v.x += q[j].x;
        v.y += q[j].y;
        v.z += q[j].z;
        v.w += q[j].w;
      }
  }
  return v;
}

// Sum the split-K partials (fixed order) and apply the epilogue. One thread = 4 consecutive columns of one row (two
// RoPE pairs; a 16-column tile never straddles a float4); SwiGLU: 4 consecutive output columns, i.e. the gate float4
// and the up float4 16 columns to its right (the launch covers M * N / 8 threads there).
template <int MODE>
__global__ void __launch_bounds__(256)
    gemm_reduce_kernel(const float* __restrict__ ws, int ksplit, void* __restrict__ out, int M, int N,
                       int accumulate, int out_f32, bf16_t* __restrict__ mirror, QKVArgs qa,
                       const float* __restrict__ ssq, int K, float rms_eps) {
  const size_t t4 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t slab4 = (size_t)M * N / 4;
  if (t4 >= (MODE == MODE_SWIGLU ? slab4 >> 1 : slab4)) return;
  size_t e4 = t4;
  if constexpr (MODE == MODE_SWIGLU) {  // output float4 t4 -> the gate float4 of its 32-column (gate, up) tile pair
    const size_t oq = (size_t)N >> 3, mo = t4 / oq, c = (t4 - mo * oq) * 4;
    e4 = (mo * N + (c >> 4) * 32 + (c & 15)) >> 2;
  }
  const size_t idx = e4 * 4;
  const int m = (int)(idx / N), col = (int)(idx - (size_t)m * N);
  float4 v = sum_splits(ws, ksplit, slab4, e4);
  float rs = 1.f;  // fused RMSNorm: the splits' partial sums of squares of row m (fixed order)
  if (ssq) {
    float t = 0.f;
    for (int s = 0; s < ksplit; ++s) t += ssq[(size_t)s * M + m];
    rs = 1.f / sqrtf(t / (float)K + rms_eps);
    v.x *= rs;
    v.y *= rs;
    v.z *= rs;
    v.w *= rs;
  }
  float vv[4] = {v.x, v.y, v.z, v.w};
  if constexpr (MODE == MODE_SWIGLU) {
    // gate tile t = 2p holds columns [32p, 32p+16), the up tile the next 16: pair the two halves
    const int tile = col >> 4, c0 = col & 15;  // tile is even: the gate half of the pair
    float4 u = sum_splits(ws, ksplit, slab4, e4 + 4);
    u.x *= rs;
    u.y *= rs;
    u.z *= rs;
    u.w *= rs;
    const float uu[4] = {u.x, u.y, u.z, u.w};
    bf16_t* o = static_cast<bf16_t*>(out) + (size_t)m * (N >> 1) + (tile >> 1) * 16 + c0;
    const uint2 pk = make_uint2(pack2bf(silu(vv[0]) * uu[0], silu(vv[1]) * uu[1]),
                                pack2bf(silu(vv[2]) * uu[2], silu(vv[3]) * uu[3]));
    *reinterpret_cast<uint2*>(o) = pk;
    // decode M: also the packed copy (common.h pack_off) the next projection's packed-x GEMV reads
    if (qa.pack) *reinterpret_cast<uint2*>(qa.pack + pack_off(m, (tile >> 1) * 16 + c0, N >> 1)) = pk;
  } else if constexpr (MODE == MODE_RESIDUAL) {
    float4* o = reinterpret_cast<float4*>(static_cast<float*>(out) + idx);
    float4 r = *o;
    if (accumulate) {
      r.x += vv[0];
      r.y += vv[1];
      r.z += vv[2];
      r.w += vv[3];
    } else {
      r = make_float4(vv[0], vv[1], vv[2], vv[3]);
    }
    *o = r;
    if (mirror) {
      const uint2 pk = make_uint2(pack2bf(r.x, r.y), pack2bf(r.z, r.w));
      *reinterpret_cast<uint2*>(mirror + idx) = pk;
      if (qa.pack) *reinterpret_cast<uint2*>(qa.pack + pack_off(m, col, N)) = pk;  // packed copy of the mirror
    }
  } else if constexpr (MODE == MODE_QKV) {
    const int head = col / qa.Dh, d0 = col - head * qa.Dh;
    const int b = m / qa.S, sq = m - b * qa.S;
    if (head < qa.H + qa.Hkv) {
      int pos = qa.positions[m];
      if (pos < 0 || pos >= qa.table_len) JLA_FLAG(JLA_BOUNDS_ROPE_POS);
      pos = pos < 0 ? 0 : (pos >= qa.table_len ? qa.table_len - 1 : pos);
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const float2 cs = qa.table[(size_t)pos * (qa.Dh >> 1) + (d0 >> 1) + p];
        const float xr = vv[2 * p], xi = vv[2 * p + 1];
        vv[2 * p] = xr * cs.x - xi * cs.y;
        vv[2 * p + 1] = xr * cs.y + xi * cs.x;
      }
    }
    const uint2 packed = make_uint2(pack2bf(vv[0], vv[1]), pack2bf(vv[2], vv[3]));
    if (head < qa.H) {
      *reinterpret_cast<uint2*>(qa.q + ((size_t)m * qa.H + head) * qa.Dh + d0) = packed;
    } else {
      const int slot = qa.slot[0] + sq;
      if (slot < qa.T) {
        const bool is_k = head < qa.H + qa.Hkv;
        const int kh = is_k ? head - qa.H : head - qa.H - qa.Hkv;
        bf16_t* cache = is_k ? qa.kc : qa.vc;
        *reinterpret_cast<uint2*>(cache + (((size_t)b * qa.Hkv + kh) * qa.T + slot) * qa.Dh + d0) = packed;
      } else {
        JLA_FLAG(JLA_BOUNDS_KV_SLOT);
      }
    }
  } else {
    if (out_f32)
      *reinterpret_cast<float4*>(static_cast<float*>(out) + idx) = make_float4(vv[0], vv[1], vv[2], vv[3]);
    else
      *reinterpret_cast<uint2*>(static_cast<bf16_t*>(out) + idx) =
          make_uint2(pack2bf(vv[0], vv[1]), pack2bf(vv[2], vv[3]));
  }
}

// Split-K reduce of a row-parallel projection with the tensor-parallel all-reduce and the residual add in its epilogue
// (MODE_TPRESID: the tiled GEMM's counterpart of gemv.hip's fused epilogue, for decode batches past the GEMV's 64 rows;
// reference partition.py:67,70 -- the psum of the row-sharded wo / w2). Workgroup w sums the splits of elements
// [4096 w, 4096 (w + 1)) of the M x N output, rounds each pair to bf16 (the partial the unfused reduce stores) and
// pushes it as {2 x bf16, tag} granules into region w of every rank's buffer -- the GEMV workgroup w's TPRES_REGION and
// call counter, so every call that touches region w is ordered by one counter and allreduce.hip's parity argument
// holds -- then gathers the ranks' granules from its own buffer, sums them in rank order in fp32 and adds into h (and
// the bf16 mirror). Bit-identical to the bf16 partial + car_reduce_kernel; one launch and one HBM round trip of the
// partial fewer.
constexpr int TPR_ELEMS = 4096;  // elements per workgroup: 2048 granules of 8 bytes = one TPRES_REGION
static_assert(TPR_ELEMS / 2 * 8 == TPRES_REGION, "one fused-exchange region per workgroup");
__global__ void __launch_bounds__(256)
    gemm_reduce_tp_kernel(const float* __restrict__ ws, int ksplit, float* __restrict__ h, bf16_t* __restrict__ hb,
                          int M, int N, const CarDevice* __restrict__ dev) {
  const CarDevice& d = *dev;  // by reference (a by-value copy indexed with runtime p would live in scratch)
  const int w = blockIdx.x;
  const size_t slab4 = (size_t)M * N / 4;
  __shared__ int s_calls;
  if (threadIdx.x == 0) s_calls = __hip_atomic_load(d.wg_ctr + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1;
  // this thread's 4 float4 groups (coalesced: group j covers threads' consecutive float4s); h loaded now, its round trip
  // behind the exchange
  u32x2 gq[4];
  f32x4 hv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const size_t e4 = (size_t)w * (TPR_ELEMS / 4) + j * 256 + threadIdx.x;
    gq[j] = u32x2{0u, 0u};
    hv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (e4 < slab4) {
      const float4 v = sum_splits(ws, ksplit, slab4, e4);
      gq[j] = u32x2{pack2bf(v.x, v.y), pack2bf(v.z, v.w)};
      hv[j] = *reinterpret_cast<const f32x4*>(h + e4 * 4);
    }
  }
  __syncthreads();
  const int calls = s_calls;
  const unsigned tag = gran_tag_fused(calls);
  const long long wg_base = (long long)w * TPRES_REGION;
  const long long par_base = (long long)(calls & 1) * d.world * d.max_bytes;
  // granule (j, thread, half) at wg_base + ((j * 256 + thread) * 2 + half) * 8
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const size_t e4 = (size_t)w * (TPR_ELEMS / 4) + j * 256 + threadIdx.x;
    if (e4 >= slab4) continue;
    const long long g = wg_base + (long long)(j * 256 + threadIdx.x) * 16;
    for (int p = 0; p < d.world; ++p) {  // (8-byte stores: the unit the protocol relies on landing whole)
      const __amdgpu_buffer_rsrc_t rp = rsrc(d.buf[p]);
      const long long o = par_base + (long long)d.rank * d.max_bytes + g;
      st_sys8(rp, o, u32x2{gq[j][0], tag});
      st_sys8(rp, o + 8, u32x2{gq[j][1], tag});
    }
  }
  const bool give_up = __hip_atomic_load(d.error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
  const __amdgpu_buffer_rsrc_t mine = rsrc(d.buf[d.rank]);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const size_t e4 = (size_t)w * (TPR_ELEMS / 4) + j * 256 + threadIdx.x;
    if (e4 >= slab4) continue;
    const long long g = wg_base + (long long)(j * 256 + threadIdx.x) * 16;
    float sm[4] = {0.f, 0.f, 0.f, 0.f};
    u32x4 r[CAR_MAX_WORLD];
    car_gather16(d, mine, par_base + g, d.max_bytes, tag, give_up, r);
#pragma unroll
    for (int p = 0; p < CAR_MAX_WORLD; ++p) {
      if (p < d.world) {
        sm[0] += __uint_as_float(r[p][0] << 16);
        sm[1] += __uint_as_float(r[p][0] & 0xffff0000u);
        sm[2] += __uint_as_float(r[p][2] << 16);
        sm[3] += __uint_as_float(r[p][2] & 0xffff0000u);
      }
    }
    f32x4 n;
#pragma unroll
    for (int i = 0; i < 4; ++i) n[i] = hv[j][i] + sm[i];
    *reinterpret_cast<f32x4*>(h + e4 * 4) = n;
    *reinterpret_cast<u32x2*>(hb + e4 * 4) = u32x2{pack2bf(n[0], n[1]), pack2bf(n[2], n[3])};
  }
  if (threadIdx.x == 0) __hip_atomic_store(d.wg_ctr + w, calls, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
int gemm_tp_groups(int M, int N) { return (int)(((size_t)M * N + TPR_ELEMS - 1) / TPR_ELEMS); }

// The 256 x 256 gemm2 runs the full-line x staging pipeline (FA) with each K-tile's weight loads issued between the
// MFMAs (FAM = 2): 6-21 % faster than fragment-shaped x and 1-8 % faster than issuing the loads up front on the
// Llama-3-8B projections (profiles/r1_gemm2_fullline_x_ab.jsonl, r1_gemm2_fam_ab.jsonl). The other pipeline forms
// (early / late waits, 5 LDS buffers, two half phases, loads up front) and the 128 x 128 register-staged v1 kernel were
// never picked and were removed in round 4 (profiles/r4_variant_pruning.md).

static int g2_wm(int M) { return M <= 128 ? 1 : 2; }  // default tile rows / 128

// split-K plan: fill the chip with workgroups while keeping >= 4 K-tiles (gemm2: 1 WG per CU,
// target ~256 WGs) / >= 8 k-steps (gemm v1: ~512 WGs) per split.
int gemm_ksplit(int M, int N, int K) {
  const int KS = K >> 5;
  const int bm = 128 * g2_wm(M);
  const int tiles = ((N + G2_BN - 1) / G2_BN) * ((M + bm - 1) / bm);
  // one WG per CU, and the fp32 partial slabs (ks * M * N * 8 bytes written + read) kept within
  // ~2x the weight bytes (N * K * 2): measured optimum at M = 128..512 (profiles/README.md)
  int ks = min(256 / tiles, max(1, K / (2 * M)));
  ks = ks < 1 ? 1 : (ks > 16 ? 16 : ks);
  while (ks > 1 && KS / ks < 4) --ks;
  const int kc = (KS + ks - 1) / ks;
  return (KS + kc - 1) / kc;
}

size_t gemm_workspace_floats(int M, int N, int K) {
  const int ks = gemm_ksplit(M, N, K);
  return ks > 1 ? (size_t)ks * M * (N + 1) : 0;  // slabs + fused-RMS partial sums
}

static int num_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
      cus = prop.multiProcessorCount;
    if (cus <= 0) cus = 256;
  }
  return cus;
}
int gemm_num_cus() { return num_cus(); }

// The launchers below run a legal plan (gemm_plan.h: the tile ids, the kernel family of each and every rule): they
// check nothing themselves.
static bool g_g4_default = true;  // tile 0 resolves to gemm4 where it applies (tools switch it off for A/B)
void gemm_set_g4_default(int on) { g_g4_default = on != 0; }
int gemm_qkv_direct_ok(int M, int tile, int K) {
  const GemmPlanResult r = gemm_plan(M, 16, K, MODE_QKV, true, 1, tile, true, 0, 0, g_g4_default);
  return r.rc == 0 && !r.plan.reduce;
}
int gemm_plan_check(int M, int N, int K, int mode, int rms, int ksplit, int tile, int has_rms_ws, int n_body) {
  return gemm_plan(M, N, K, mode, rms != 0, ksplit, tile, has_rms_ws != 0, n_body, num_cus(), g_g4_default).rc;
}

// One launch of a tile kernel: the operands and epilogue arguments every family takes.
struct GemmArgs {
  const bf16_t* x;
  const u32x4* w;
  void* out;
  int M, N, K, accumulate, out_f32;
  bf16_t* mirror;
  float rms_eps;
  float* ssq;     // K split: the per-split sums of squares of the fused norm (behind the slabs)
  float* rms_ws;  // NORM_PRECOMPUTED: the row statistic's scratch
  QKVArgs qa;
  hipStream_t s;
};

// NORM_PRECOMPUTED: the row statistic into the scratch, ahead of the GEMM (inv: what the kernel reads; null otherwise).
// False: that launch failed.
static bool g4_row_stat(const GemmArgs& a, const GemmPlan& p, const float*& inv) {
  inv = p.norm == NORM_PRECOMPUTED ? a.rms_ws : nullptr;
  return inv == nullptr || rms_rowinv(a.x, a.rms_ws, a.M, a.K, a.rms_eps, a.s) == 0;  // (K % 8 == 0 always holds here)
}

// Tile rasterisation: the launch order walks groups of gm m-tiles across every n-tile (g4_tile_coords), so the 32
// workgroups an XCD runs at once cover gm m-tiles x 32 / gm n-tiles. gm = 4 (4 x 8 tiles per XCD) beat 8 (the
// round-4 order), 1, 2 and 16 on every Llama-3-8B projection at M = 2048 and 32768: qkv -7 / -9 %, o -3 / -8 %,
// gate_up -5 / 0 %, down -5 / -6 % (profiles/r5_gemm4_group_m.jsonl). gemm_set_g4_group pins another (tools).
static int g_g4_group = 0;
void gemm_set_g4_group(int gm) { g_g4_group = gm; }
static int g4_group_m(int tiles_m) {
  const int gm = g_g4_group > 0 ? g_g4_group : 4;
  return gm < tiles_m ? gm : tiles_m;
}
static int g_g5_diag = 0;  // tools only (gemm5ws.h diag bits 1-16; gemm4 store ablations 64 / 128: wrong results)
void gemm5_set_diag(int d) { g_g5_diag = d; }

// gemm4 on 256 x 32 NJ tiles; NJ = 6 / 4: the weights three K-tiles deep, the norm as the precomputed statistic only
template <int MODE, int NJ>
static void launch_g4(const GemmArgs& a, const GemmPlan& p) {
  const int tm = (a.M + G4_BM - 1) / G4_BM, tn = (a.N + 32 * NJ - 1) / (32 * NJ);
  const int grid = tm * tn * p.ksplit, gm = g4_group_m(tm);
  const float* inv;
  if (!g4_row_stat(a, p, inv)) return;
#define JLA_G4(R, DIAG, DEEP)                                                                                       \
  gemm4_kernel<MODE, R, NJ, DIAG, DEEP><<<grid, 256, 0, a.s>>>(a.x, a.w, a.out, a.M, a.N, a.K, a.accumulate, a.out_f32, \
                                                               a.mirror, p.kc, tm, tn, a.rms_eps, a.ssq, a.qa, inv, gm)
  if constexpr (NJ != 8) {
    if (inv)
      JLA_G4(2, 0, true);
    else
      JLA_G4(0, 0, true);
  } else {
    if constexpr (MODE == MODE_STORE) {  // ablation instances (tools only; wrong results)
      if (p.norm == NORM_NONE && (g_g5_diag & 192)) {
        if ((g_g5_diag & 192) == 64)
          JLA_G4(0, 1, false);
        else if ((g_g5_diag & 192) == 128)
          JLA_G4(0, 2, false);
        else
          JLA_G4(0, 3, false);
        return;
      }
    }
    if (p.norm == NORM_PRECOMPUTED) {
      if (p.deep) JLA_G4(2, 0, true); else JLA_G4(2, 0, false);
    } else if (p.norm == NORM_INLOOP) {
      if (p.deep) JLA_G4(1, 0, true); else JLA_G4(1, 0, false);
    } else {
      if (p.deep) JLA_G4(0, 0, true); else JLA_G4(0, 0, false);
    }
  }
#undef JLA_G4
}

// persistent gemm4: one workgroup per CU over every 256 x 256 tile
template <int MODE>
static void launch_g4p(const GemmArgs& a, const GemmPlan& p) {
  const int tm = (a.M + G4_BM - 1) / G4_BM, tn = (a.N + G4_BN - 1) / G4_BN;
  const int grid = min(tm * tn, num_cus()), gm = g4_group_m(tm);
  const float* inv;
  if (!g4_row_stat(a, p, inv)) return;
#define JLA_G4P(R)                                                                                                  \
  gemm4p_kernel<MODE, R><<<grid, 256, 0, a.s>>>(a.x, a.w, a.out, a.M, a.N, a.K, a.accumulate, a.out_f32, a.mirror, tm, \
                                                tn, a.rms_eps, a.qa, inv, gm)
  if (p.norm == NORM_PRECOMPUTED)
    JLA_G4P(2);
  else if (p.norm == NORM_INLOOP)
    JLA_G4P(1);
  else
    JLA_G4P(0);
#undef JLA_G4P
}

// tail-balanced gemm4: p.n_body body n-tiles of 32 NJB columns, the rest in 128-wide tiles
template <int MODE, int NJB>
static void launch_g4t(const GemmArgs& a, const GemmPlan& p) {
  const int tm = (a.M + G4_BM - 1) / G4_BM, nt = (a.N - p.n_body * 32 * NJB + 127) / 128;
  const int grid = tm * (p.n_body + nt), gm = g4_group_m(tm);
  const float* inv;
  if (!g4_row_stat(a, p, inv)) return;
  if (inv)
    gemm4t_kernel<MODE, 2, NJB><<<grid, 256, 0, a.s>>>(a.x, a.w, a.out, a.M, a.N, a.K, a.accumulate, a.out_f32,
                                                       a.mirror, tm, p.n_body, nt, a.rms_eps, inv, gm);
  else
    gemm4t_kernel<MODE, 0, NJB><<<grid, 256, 0, a.s>>>(a.x, a.w, a.out, a.M, a.N, a.K, a.accumulate, a.out_f32,
                                                       a.mirror, tm, p.n_body, nt, a.rms_eps, nullptr, gm);
}

// gemm2 tile configs 1 / 2 / 3 (p.family). The direct QKV and the argmax epilogues exist on the 256 x 256 tile only.
template <int MODE>
static void launch_g2(const GemmArgs& a, const GemmPlan& p) {
  const int cfg = p.family;
  const int bm = cfg == 1 ? 256 : 128, bn = cfg == 3 ? 128 : 256;
  const int tm = (a.M + bm - 1) / bm, tn = (a.N + bn - 1) / bn;
  const int grid = tm * tn * p.ksplit;
#define JLA_G2(WMV, LATE, R, MTV, NTV, FA, FM)                                                                     \
  gemm2_kernel<MODE, WMV, LATE, R, MTV, NTV, FA, FM><<<grid, 256 * WMV, 0, a.s>>>(                                 \
      a.x, a.w, a.out, a.M, a.N, a.K, a.accumulate, a.out_f32, a.mirror, p.kc, tm, tn, a.rms_eps, a.ssq, a.qa)
#define JLA_G2_CFG(R)                        \
  if (cfg == 2)                              \
    JLA_G2(1, false, R, 8, 4, false, 0);     \
  else if (cfg == 3)                         \
    JLA_G2(2, true, R, 4, 2, false, 0);      \
  else                                       \
    JLA_G2(2, true, R, 8, 4, true, 2)
  [[maybe_unused]] const bool rms = p.norm != NORM_NONE;  // the statistic summed in the main loop
  if constexpr (MODE == MODE_QKV) {
    JLA_G2(2, true, true, 8, 4, true, 2);
  } else if constexpr (MODE == MODE_ARGMAX) {
    if (rms)
      JLA_G2(2, true, true, 8, 4, true, 2);
    else
      JLA_G2(2, true, false, 8, 4, true, 2);
  } else if constexpr (MODE == MODE_RESIDUAL) {
    JLA_G2_CFG(false);
  } else {
    if (rms) {
      JLA_G2_CFG(true);
    } else {
      JLA_G2_CFG(false);
    }
  }
#undef JLA_G2_CFG
#undef JLA_G2
}

// gemm5: the weight-streaming partial kernel (a.out: the slab workspace); the reduce kernel follows for any split
static void launch_g5(const GemmArgs& a, const GemmPlan& p) {
  const int mt = a.M <= 128 ? 8 : 16, rows = 16 * mt, ntw = p.nj;
  const int tiles_m = (a.M + rows - 1) / rows, tiles_n = (a.N + 64 * ntw - 1) / (64 * ntw);
  const int grid = tiles_m * tiles_n * p.ksplit;
#define JLA_G5(MTV, NTV)                                                                                            \
  gemm5_partial_kernel<MTV, NTV><<<grid, 256, 0, a.s>>>(a.x, a.w, static_cast<float*>(a.out), a.M, a.N, a.K, p.kc, \
                                                        tiles_m, tiles_n, a.ssq, g_g5_diag)
  if (mt == 8 && ntw == 4)
    JLA_G5(8, 4);
  else if (mt == 8)
    JLA_G5(8, 2);
  else if (ntw == 4)
    JLA_G5(16, 4);
  else
    JLA_G5(16, 2);
#undef JLA_G5
}

// the tile kernel of the plan, epilogue MODE (MODE_PARTIAL: slabs for the reduce kernel)
template <int MODE>
static void launch_plan(const GemmArgs& a, const GemmPlan& p) {
  constexpr bool PLAIN = MODE == MODE_STORE || MODE == MODE_RESIDUAL || MODE == MODE_SWIGLU;
  switch (p.family) {
    case GEMM2_256x256:
    case GEMM2_128x256:
    case GEMM2_128x128:
      if constexpr (MODE != MODE_LOGPROB) launch_g2<MODE>(a, p);  // (gemm2 has no log-prob epilogue)
      break;
    case GEMM4:
      if (p.nj == 8) launch_g4<MODE, 8>(a, p);
      if constexpr (MODE != MODE_ARGMAX && MODE != MODE_LOGPROB) {
        if (p.nj == 6) launch_g4<MODE, 6>(a, p);
      }
      if constexpr (PLAIN || MODE == MODE_PARTIAL) {
        if (p.nj == 4) launch_g4<MODE, 4>(a, p);
      }
      break;
    case GEMM4_PERSISTENT:
      if constexpr (PLAIN || MODE == MODE_QKV) launch_g4p<MODE>(a, p);
      break;
    case GEMM4_TAIL:
      if constexpr (PLAIN) {
        if (p.nj == 6)
          launch_g4t<MODE, 6>(a, p);
        else
          launch_g4t<MODE, 8>(a, p);
      }
      break;
    case GEMM5:
      if constexpr (MODE == MODE_PARTIAL) launch_g5(a, p);
      break;
    case GEMM_NONE: break;
  }
}

// the split-K reduce + epilogue launch over [ksplit][M][N] partial slabs (+ [ksplit][M] sums of squares, fused norm)
static int launch_reduce(const float* ws, int ksplit, void* out, int M, int N, int K, int mode, int accumulate,
                         int out_f32, bf16_t* mirror, const QKVArgs* qkv, const float* ssq, float rms_eps,
                         hipStream_t s) {
  const size_t total4 = (size_t)M * N / (mode == MODE_SWIGLU ? 8 : 4);
  const int rgrid = (int)((total4 + 255) / 256);
  QKVArgs qa{};
  if (qkv) qa = *qkv;
  const float eps = ssq ? rms_eps : 0.f;
  switch (mode) {
    case MODE_STORE:
      gemm_reduce_kernel<MODE_STORE><<<rgrid, 256, 0, s>>>(ws, ksplit, out, M, N, accumulate, out_f32, nullptr, qa,
                                                           ssq, K, eps);
      break;
    case MODE_RESIDUAL:
      gemm_reduce_kernel<MODE_RESIDUAL><<<rgrid, 256, 0, s>>>(ws, ksplit, out, M, N, accumulate, 1, mirror, qa,
                                                              nullptr, K, eps);
      break;
    case MODE_SWIGLU:
      gemm_reduce_kernel<MODE_SWIGLU><<<rgrid, 256, 0, s>>>(ws, ksplit, out, M, N, accumulate, 0, nullptr, qa, ssq,
                                                            K, eps);
      break;
    case MODE_QKV:
      gemm_reduce_kernel<MODE_QKV><<<rgrid, 256, 0, s>>>(ws, ksplit, out, M, N, accumulate, 0, nullptr, qa, ssq, K,
                                                         eps);
      break;
    case MODE_TPRESID:  // out = h (fp32 residual), mirror = hb, qkv->tp = the TP group's CarDevice
      if (!qkv || !qa.tp || !mirror || ssq || (N & 3)) return -1;
      gemm_reduce_tp_kernel<<<gemm_tp_groups(M, N), 256, 0, s>>>(ws, ksplit, static_cast<float*>(out), mirror, M, N,
                                                                 static_cast<const CarDevice*>(qa.tp));
      break;
    default: return -1;
  }
  JLA_CHECK_LAUNCH();
  return 0;
}

int gemm(const bf16_t* x, const void* W, void* out, int M, int N, int K, int mode, int accumulate, int out_f32,
         bf16_t* mirror, const QKVArgs* qkv, float* ws, size_t ws_floats, int ksplit, hipStream_t s,
         float rms_eps, int tile, float* rms_ws, size_t rms_ws_floats, int n_body) {
  const bool has_rms_ws = rms_ws != nullptr && rms_ws_floats >= (size_t)M;  // too small: the in-loop statistic
  const GemmPlanResult r =
      gemm_plan(M, N, K, mode, rms_eps >= 0.f, ksplit, tile, has_rms_ws, n_body, num_cus(), g_g4_default);
  const GemmPlan& p = r.plan;
  if (r.rc != 0 || p.family == GEMM_NONE) return r.rc;
  // (gemm_argmax()'s and gemm_logprob()'s epilogues)
  if (mode == MODE_ARGMAX || mode == MODE_LOGPROB || (mode == MODE_QKV && !qkv)) return -1;
  const u32x4* w = static_cast<const u32x4*>(W);
  if (!p.reduce) {  // the epilogue in the tile kernel
    GemmArgs a{x, w, out, M, N, K, accumulate, out_f32, nullptr, rms_eps, nullptr, rms_ws, QKVArgs{}, s};
    switch (mode) {
      case MODE_QKV:
        a.out = nullptr, a.accumulate = a.out_f32 = 0, a.qa = *qkv;
        launch_plan<MODE_QKV>(a, p);
        break;
      case MODE_STORE: launch_plan<MODE_STORE>(a, p); break;
      case MODE_RESIDUAL:
        a.out_f32 = 1, a.mirror = mirror, a.rms_eps = -1.f;
        launch_plan<MODE_RESIDUAL>(a, p);
        break;
      case MODE_SWIGLU:
        a.out_f32 = 0;
        launch_plan<MODE_SWIGLU>(a, p);
        break;
      default: return -1;
    }
    JLA_CHECK_LAUNCH();
    return 0;
  }
  // workspace: [ksplit][M][N] fp32 partial slabs, then (fused norm) [ksplit][M] partial sums of squares
  const size_t slabs = (size_t)p.ksplit * M * N;
  if (ws == nullptr || ws_floats < slabs + (p.norm != NORM_NONE ? (size_t)p.ksplit * M : 0)) return -3;
  float* ssq = p.norm != NORM_NONE ? ws + slabs : nullptr;
  launch_plan<MODE_PARTIAL>(GemmArgs{x, w, ws, M, N, K, 0, 1, nullptr, rms_eps, ssq, nullptr, QKVArgs{}, s}, p);
  JLA_CHECK_LAUNCH();
  return launch_reduce(ws, p.ksplit, out, M, N, K, mode, accumulate, out_f32, mirror, qkv, ssq, rms_eps, s);
}

// ---- greedy lm_head: GEMM with the argmax in its epilogue (no fp32 logits round trip through HBM:
// at M = 2048, V = 128256 that is 1 GB written + 1 GB read per decode step), then the [M][P] partials are
// reduced per row. Ties go to the smaller index, so the result equals argmax_kernel's.
JLA_DEV void amax_merge(float& bv, int& bi, float ov, int oi) {
  if (ov > bv || (ov == bv && oi < bi)) {
    bv = ov;
    bi = oi;
  }
}

// TPR threads per row (64: one wave per row, 4 rows per 256-thread block; 1024: one block per row for the
// decode-sized M, where one wave walking ~8000 partials of a row with one dependent load per step took ~38 us).
// Each thread keeps 4 independent (value, index) candidates so 4 loads are in flight per step.
template <int TPR>
__global__ void __launch_bounds__(TPR == 64 ? 256 : TPR)
    argmax_partials_kernel(const float2* __restrict__ part, int P, int M, int32_t* __restrict__ idx,
                           float* __restrict__ val) {
  __shared__ float s_v[16];
  __shared__ int s_i[16];
  const int row = TPR == 64 ? blockIdx.x * 4 + (threadIdx.x >> 6) : blockIdx.x;
  const int t = TPR == 64 ? (threadIdx.x & 63) : threadIdx.x;
  if (row >= M) return;
  const float2* pr = part + (size_t)row * P;
  float bv[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int bi[4] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
  for (int k0 = t; k0 < P; k0 += 4 * TPR) {
    float2 e[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + u * TPR;
      e[u] = k < P ? pr[k] : make_float2(-INFINITY, __int_as_float(0x7fffffff));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) amax_merge(bv[u], bi[u], e[u].x, __float_as_int(e[u].y));
  }
#pragma unroll
  for (int u = 1; u < 4; ++u) amax_merge(bv[0], bi[0], bv[u], bi[u]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) amax_merge(bv[0], bi[0], __shfl_xor(bv[0], o, 64), __shfl_xor(bi[0], o, 64));
  if constexpr (TPR > 64) {
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
      s_v[w] = bv[0];
      s_i[w] = bi[0];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int ww = 1; ww < TPR / 64; ++ww) amax_merge(bv[0], bi[0], s_v[ww], s_i[ww]);
      idx[row] = bi[0] == 0x7fffffff ? 0 : bi[0];
      val[row] = bv[0];
    }
  } else if (t == 0) {
    idx[row] = bi[0] == 0x7fffffff ? 0 : bi[0];
    val[row] = bv[0];
  }
}

static void launch_argmax_partials(const float2* part, int P, int M, int32_t* idx, float* val, hipStream_t s) {
  if (M <= 512)
    argmax_partials_kernel<1024><<<M, 1024, 0, s>>>(part, P, M, idx, val);
  else
    argmax_partials_kernel<64><<<(M + 3) / 4, 256, 0, s>>>(part, P, M, idx, val);
}

int argmax_partials(const float* part, int P, int M, int32_t* idx, float* val, hipStream_t s) {
  if (M <= 0) return 0;
  launch_argmax_partials(reinterpret_cast<const float2*>(part), P, M, idx, val, s);
  JLA_CHECK_LAUNCH();
  return 0;
}

size_t gemm_argmax_workspace_floats(int M, int N) { return (size_t)M * ((N + G2_BN - 1) / G2_BN) * 4 * 2; }

int gemm_argmax(const bf16_t* x, const void* W, float* ws, size_t ws_floats, int M, int N, int K, float rms_eps,
                int32_t* idx, float* val, hipStream_t s, float* rms_ws, size_t rms_ws_floats) {
  const bool has_rms_ws = rms_ws != nullptr && rms_ws_floats >= (size_t)M;
  const GemmPlanResult r = gemm_plan(M, N, K, MODE_ARGMAX, rms_eps >= 0.f, 1, 0, has_rms_ws, 0, 0, g_g4_default);
  if (r.rc != 0 || r.plan.family == GEMM_NONE) return r.rc;
  if (ws == nullptr || ws_floats < gemm_argmax_workspace_floats(M, N)) return -3;
  launch_plan<MODE_ARGMAX>(
      GemmArgs{x, static_cast<const u32x4*>(W), ws, M, N, K, 0, 1, nullptr, rms_eps, nullptr, rms_ws, QKVArgs{}, s},
      r.plan);
  JLA_CHECK_LAUNCH();
  // one partial per wave column: 2 per 256-column gemm4 tile, 4 per gemm2 tile
  const int P = (N + G2_BN - 1) / G2_BN * (r.plan.family == GEMM4 ? 2 : 4);
  launch_argmax_partials(reinterpret_cast<const float2*>(ws), P, M, idx, val, s);
  JLA_CHECK_LAUNCH();
  return 0;
}

// ---- scoring lm_head: GEMM with the log-sum-exp in its epilogue (MODE_LOGPROB in g4_epilogue: no fp32 logits round
// trip through HBM, 16.8 GB written + read at M = 32768, V = 128256), then the [M][P] (max, sum) partials are merged
// per row. (m, s) stands for s * exp(m); (-inf, 0) is the identity and never meets an inf - inf.
JLA_DEV void lse_merge(float& m, float& s, float om, float os) {
  constexpr float LOG2E = 1.4426950408889634f;
  if (om == -INFINITY) return;
  if (m == -INFINITY) {
    m = om;
    s = os;
    return;
  }
  const float nm = fmaxf(m, om);
  s = s * __builtin_amdgcn_exp2f((m - nm) * LOG2E) + os * __builtin_amdgcn_exp2f((om - nm) * LOG2E);
  m = nm;
}

// The launch shapes of argmax_partials_kernel (TPR threads per row, 4 independent partials in flight per thread). The
// merge order is fixed by (P, TPR): per thread its strided partials in order, then the 4 candidates, the lanes of a
// wave by xor 32..1, the waves in order -- the same bits on every call.
template <int TPR>
__global__ void __launch_bounds__(TPR == 64 ? 256 : TPR)
    lse_partials_kernel(const float2* __restrict__ part, int P, int M, float* __restrict__ mx,
                        float* __restrict__ se) {
  __shared__ float s_m[16];
  __shared__ float s_s[16];
  const int row = TPR == 64 ? blockIdx.x * 4 + (threadIdx.x >> 6) : blockIdx.x;
  const int t = TPR == 64 ? (threadIdx.x & 63) : threadIdx.x;
  if (row >= M) return;
  const float2* pr = part + (size_t)row * P;
  float bm[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  float bs[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = t; k0 < P; k0 += 4 * TPR) {
    float2 e[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + u * TPR;
      e[u] = k < P ? pr[k] : make_float2(-INFINITY, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) lse_merge(bm[u], bs[u], e[u].x, e[u].y);
  }
#pragma unroll
  for (int u = 1; u < 4; ++u) lse_merge(bm[0], bs[0], bm[u], bs[u]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)  // (lane 0's chain is the row's result)
    lse_merge(bm[0], bs[0], __shfl_xor(bm[0], o, 64), __shfl_xor(bs[0], o, 64));
  if constexpr (TPR > 64) {
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
      s_m[w] = bm[0];
      s_s[w] = bs[0];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int ww = 1; ww < TPR / 64; ++ww) lse_merge(bm[0], bs[0], s_m[ww], s_s[ww]);
      mx[row] = bm[0];
      se[row] = bs[0];
    }
  } else if (t == 0) {
    mx[row] = bm[0];
    se[row] = bs[0];
  }
}

static void launch_lse_partials(const float2* part, int P, int M, float* mx, float* se, hipStream_t s) {
  if (M <= 512)
    lse_partials_kernel<1024><<<M, 1024, 0, s>>>(part, P, M, mx, se);
  else
    lse_partials_kernel<64><<<(M + 3) / 4, 256, 0, s>>>(part, P, M, mx, se);
}

// one (max, sum) pair per wave column of the 256 x 256 gemm4 tile
size_t gemm_logprob_workspace_floats(int M, int N) { return (size_t)M * ((N + G4_BN - 1) / G4_BN) * 2 * 2; }

int gemm_logprob(const bf16_t* x, const void* W, float* ws, size_t ws_floats, int M, int N, int K, float rms_eps,
                 const int32_t* targets, int col_offset, float* tgt, float* mx, float* se, hipStream_t s,
                 float* rms_ws, size_t rms_ws_floats) {
  const bool has_rms_ws = rms_ws != nullptr && rms_ws_floats >= (size_t)M;
  const GemmPlanResult r = gemm_plan(M, N, K, MODE_LOGPROB, rms_eps >= 0.f, 1, 0, has_rms_ws, 0, 0, g_g4_default);
  if (r.rc != 0 || r.plan.family == GEMM_NONE) return r.rc;
  if (ws == nullptr || ws_floats < gemm_logprob_workspace_floats(M, N)) return -3;
  if (targets == nullptr || tgt == nullptr || mx == nullptr || se == nullptr) return -1;
  // rows whose target is an ignored label or a column of another shard are written by nobody
  const hipError_t zeroed = hipMemsetAsync(tgt, 0, (size_t)M * sizeof(float), s);
  if (zeroed != hipSuccess) return (int)zeroed;
  GemmArgs a{x, static_cast<const u32x4*>(W), ws, M, N, K, 0, 1, nullptr, rms_eps, nullptr, rms_ws, QKVArgs{}, s};
  a.qa.lp_targets = targets, a.qa.lp_tgt = tgt, a.qa.lp_col_offset = col_offset;
  launch_plan<MODE_LOGPROB>(a, r.plan);
  JLA_CHECK_LAUNCH();
  launch_lse_partials(reinterpret_cast<const float2*>(ws), (N + G4_BN - 1) / G4_BN * 2, M, mx, se, s);
  JLA_CHECK_LAUNCH();
  return 0;
}

JLA_BOUNDS_ACCESSOR(gemm)

}  // namespace jla
