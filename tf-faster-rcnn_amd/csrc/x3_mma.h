// What the kernels on the exactly split bf16 pipe share (gemm_x3.hip, winograd2_fused.hip): the three-way split of an f32 fragment and
// the group of cross-term MFMAs of one 16-k step.  Two kernels that call both with the same operands in the same k order give the
// same bits -- the fused F(2x2,3x3) convolution relies on it.
#pragma once
#include "mfma_f32.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

// exact split of 8 consecutive k values (two float4) into three bf16x8 operands, every piece rounded to nearest-even
// (v_cvt_pk_bf16_f32): h = bf16(x), m = bf16(x - h), l = x - h - m.  Both subtractions are exact in f32 and l has at most 8
// significant bits left, so h + m + l == x; |m| <= 2^-8 |x|, |l| <= 2^-17 |x|, errors of either sign (truncation would bias every
// product towards zero and is 8x looser: tests/test_x3_math_cpu.py).
__device__ __forceinline__ void x3_split8(const float4 a, const float4 b, bf16x8& h, bf16x8& m, bf16x8& l) {
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const __bf16 hq = (__bf16)v[q];
    const float r = v[q] - (float)hq;
    const __bf16 mq = (__bf16)r;
    const float s = r - (float)mq;
    h[q] = hq; m[q] = mq; l[q] = (__bf16)s;
  }
}

// one 16-k step of a 32x32 block: the leading term onto acc, the five small cross terms onto acs, in this order (TERMS = 9: also
// al*wl, al*wm, am*wl -> every f32 product exact)
template <int TERMS>
__device__ __forceinline__ void x3_mma16(const bf16x8 ah, const bf16x8 am, const bf16x8 al, const bf16x8 bh, const bf16x8 bm, const bf16x8 bl,
                                         f32x16& acc, f32x16& acs) {
  acs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acs, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
  acs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acs, 0, 0, 0);
  acs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acs, 0, 0, 0);
  acs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acs, 0, 0, 0);
  acs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acs, 0, 0, 0);
  if (TERMS == 9) {
    acs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bl, acs, 0, 0, 0);
    acs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bm, acs, 0, 0, 0);
    acs = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bl, acs, 0, 0, 0);
  }
}

// the value k_gemm_x3 stores for a null bias, no residual and FRCNN_ACT_NONE: (acc + acs) + 0 through the open clamp
__device__ __forceinline__ float x3_combine_plain(float acc, float acs) {
  const float t = (acc + acs) + 0.f;
  return t < -__builtin_inff() ? -__builtin_inff() : (t > __builtin_inff() ? __builtin_inff() : t);
}
