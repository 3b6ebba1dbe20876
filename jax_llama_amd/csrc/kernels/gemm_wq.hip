// The launch of the quantised-weight GEMM's partial kernel (gemm5q.h). A translation unit of its own: build.py compiles
// it without the packed fp32 VALU ops (its per-file flags), which the other kernels of gemm.hip keep. gemm_wq()
// (gemm.hip) resolves the plan, calls this and runs the reduce kernel with the caller's epilogue behind it.
#include "gemm5q.h"
#include "launchers.h"

namespace jla {

template <int FMT>
static void launch_g5q(const bf16_t* x, const void* Wq, const void* S, float* ws, int M, int N, int K, float* ssq,
                       int ntw, int ksplit, int kc, hipStream_t s) {
  const int mt = M <= 128 ? 8 : 16, rows = 16 * mt;
  const int tiles_m = (M + rows - 1) / rows, tiles_n = (N + 64 * ntw - 1) / (64 * ntw);
  const int grid = tiles_m * tiles_n * ksplit;
#define JLA_G5Q(MTV, NTV)                                                                                        \
  gemm5q_partial_kernel<FMT, MTV, NTV><<<grid, 256, 0, s>>>(x, static_cast<const u32x4*>(Wq), S, ws, M, N, K, kc, \
                                                            tiles_m, tiles_n, ssq)
  if (mt == 8 && ntw == 4)
    JLA_G5Q(8, 4);
  else if (mt == 8)
    JLA_G5Q(8, 2);
  else if (ntw == 4)
    JLA_G5Q(16, 4);
  else
    JLA_G5Q(16, 2);
#undef JLA_G5Q
}

int gemm5q_launch(const bf16_t* x, const void* Wq, const void* S, int fmt, float* ws, int M, int N, int K, float* ssq,
                  int ntw, int ksplit, int kc, hipStream_t s) {
  // (the shapes gemm_wq_plan() admits; checked again here because the kernel indexes by them)
  if (M <= 0 || N <= 0 || (N & 15) || K <= 0 || (K & (fmt == WQ_FP8 ? 63 : 127)) || (ntw != 2 && ntw != 4) ||
      ksplit < 1 || kc < 1 || (long long)ksplit * kc < (K >> 6) || (fmt != WQ_FP8 && fmt != WQ_MXFP4))
    return -1;
  if (fmt == WQ_FP8)
    launch_g5q<WQ_FP8>(x, Wq, S, ws, M, N, K, ssq, ntw, ksplit, kc, s);
  else
    launch_g5q<WQ_MXFP4>(x, Wq, S, ws, M, N, K, ssq, ntw, ksplit, kc, s);
  JLA_CHECK_LAUNCH();
  return 0;
}

}  // namespace jla
