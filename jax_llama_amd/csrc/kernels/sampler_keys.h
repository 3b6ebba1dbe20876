// What the two samplers (topk_sample.hip, nucleus_sample.hip) share: the order-preserving key of an fp32 logit and
// the counter-based generator behind their Gumbel noise.
#pragma once
#include "common.h"

namespace jla {

// -0.0 takes the key of +0.0: the two are equal logits (a tie goes to the lower index, like any other), not neighbours
JLA_DEV uint32_t fkey(float f) {
  uint32_t u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
JLA_DEV float kfloat(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

JLA_DEV uint4 philox4x32_10(uint4 ctr, uint2 k) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t lo0 = 0xD2511F53u * ctr.x, hi0 = __umulhi(0xD2511F53u, ctr.x);
    const uint32_t lo1 = 0xCD9E8D57u * ctr.z, hi1 = __umulhi(0xCD9E8D57u, ctr.z);
    ctr = make_uint4(hi1 ^ ctr.y ^ k.x, lo1, hi0 ^ ctr.w ^ k.y, lo0);
    k.x += 0x9E3779B9u;
    k.y += 0xBB67AE85u;
  }
  return ctr;
}

}  // namespace jla
