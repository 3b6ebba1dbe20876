// In-register conversions of the quantised weight formats to bf16 MFMA fragments, shared by the decode GEMVs
// (gemv.hip) and the quantised-weight GEMM (gemm5q.h).
#pragma once
#include "common.h"

namespace jla {

// 8 e4m3 bytes (two dwords) -> the 8 bf16 of one B fragment, times the power-of-two `scale`: four
// v_cvt_scalef32_pk_bf16_fp8 (every e4m3 value is exact in bf16; at scale 1.0 the plain conversion)
JLA_DEV u32x4 fp8x8_to_bf16(unsigned lo, unsigned hi, float scale = 1.0f) {
  u32x4 r;
  r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, scale, false));
  r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, scale, true));
  r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, scale, false));
  r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, scale, true));
  return r;
}

// one dword of 8 e2m1 codes -> the 8 bf16 of one B fragment, times 2^(sbyte - 127): four v_cvt_scalef32_pk_bf16_fp4
// whose fp32 scale operand is the e8m0 byte moved into the exponent field (a zero byte: 0.0, and code 0 converts to 0)
JLA_DEV u32x4 fp4x8_to_bf16(unsigned q, unsigned sbyte) {
  const float sc = __uint_as_float(sbyte << 23);
  u32x4 r;
  r[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 0));
  r[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 1));
  r[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 2));
  r[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 3));
  return r;
}

}  // namespace jla
