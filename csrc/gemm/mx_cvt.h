// The MX quantisation rule as device code: one text for the streaming quantiser (mx_quant.hip)
// and the tiled GEMM's quantising epilogue (gemm_kernels.h). ddlb_amd/ops/mx.py
// quantize_mx_reference / quantize_mxfp4_reference are the specification.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ddlb {

// |x| as an integer: ordered as the floats are (exact, subnormals included).
__device__ __forceinline__ unsigned mx_abs_bits(float x) {
  return __builtin_bit_cast(unsigned, x) & 0x7FFFFFFFu;
}

// Scale exponent e (the block's scale byte is e + 127) from m = the integer image of the block's
// amax. amax = 1.f 2^(E - 127) = m' 2^(E - 126): m' <= 0.875 <=> fraction <= 0.75. A subnormal
// amax (E = 0) clamps to -127 either way; an all-zero block gets e = 0.
// (fp4: m' <= 0.75 <=> fraction <= 0.5, and 3 in place of 9)
template <bool FP4>
__device__ __forceinline__ int mx_scale_exp(unsigned m) {
  int e = FP4 ? (int)(m >> 23) - 129 + ((m & 0x7FFFFFu) > 0x400000u ? 1 : 0)
              : (int)(m >> 23) - 135 + ((m & 0x7FFFFFu) > 0x600000u ? 1 : 0);
  e = e < -127 ? -127 : (e > 127 ? 127 : e);
  if (m == 0) e = 0;
  return e;
}

// Four elements -> four e4m3 bytes (element 0 in the low byte): e4m3_rne(clamp(x 2^-e, +-448)).
__device__ __forceinline__ unsigned mx_cvt4_e4m3(float x0, float x1, float x2, float x3, int e) {
  const float y0 = __builtin_amdgcn_fmed3f(__builtin_ldexpf(x0, -e), -448.f, 448.f);
  const float y1 = __builtin_amdgcn_fmed3f(__builtin_ldexpf(x1, -e), -448.f, 448.f);
  const float y2 = __builtin_amdgcn_fmed3f(__builtin_ldexpf(x2, -e), -448.f, 448.f);
  const float y3 = __builtin_amdgcn_fmed3f(__builtin_ldexpf(x3, -e), -448.f, 448.f);
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(y0, y1, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(y2, y3, w, true);
  return (unsigned)w;
}

// The fp4 conversion's scale operand, 2^e (only its exponent field is read: the ldexp folds into
// the instruction, and e = -127 is the field 0).
__device__ __forceinline__ float mx_fp4_scale(int e) {
  return __builtin_bit_cast(float, (unsigned)(e + 127) << 23);
}

// Two elements -> one byte of E2M1 nibbles (x0 in the low nibble), written into byte SEL of w.
template <int SEL>
__device__ __forceinline__ unsigned mx_cvt2_e2m1(unsigned w, float x0, float x1, float sc) {
  return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, x0, x1, sc, SEL);
}

}  // namespace ddlb
