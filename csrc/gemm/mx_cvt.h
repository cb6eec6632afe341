// The MX quantisation rule as device code: one text for the streaming quantiser (mx_quant.hip)
// and the tiled GEMM's quantising epilogue (gemm_kernels.h). ddlb_amd/ops/mx.py
// quantize_mx_reference / quantize_mxfp4_reference are the specification.
//
// Non-finite input. The amax is taken over the finite elements only: NaN and +-Inf count as 0, so
// they cannot flush their finite neighbours to zero, and a block without a finite non-zero
// element gets the scale byte 127. MX-fp8 turns a non-finite element into the e4m3fn NaN byte
// with its sign (0x7F | sign << 7) at the conversion. E2M1 has no NaN: an MXFP4 block that holds
// a non-finite element gets the scale byte 255 (the E8M0 NaN; the block-scaled MFMA returns NaN
// for every product of such a block, tests/test_nonfinite_gpu.py test_scale_byte_255) and the
// element itself the nibble 0x7 | sign << 3. The fp4 amax word therefore carries a flag in bit
// 31, free because |x| as an integer is below 2^31: "the block holds a non-finite element".
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ddlb {

constexpr unsigned kMxNonFinite = 0x80000000u;  // the flag of an fp4 amax word
constexpr unsigned kMxInfBits = 0x7F800000u;    // |x| as an integer is below it <=> x is finite

// |x| as an integer: ordered as the floats are (exact, subnormals included).
__device__ __forceinline__ unsigned mx_abs_bits(float x) {
  return __builtin_bit_cast(unsigned, x) & 0x7FFFFFFFu;
}

// An element's contribution to its block's amax word: |x|, 0 (fp4: the flag) when not finite.
template <bool FP4>
__device__ __forceinline__ unsigned mx_amax_bits(float x) {
  const unsigned b = mx_abs_bits(x);
  return b < kMxInfBits ? b : (FP4 ? kMxNonFinite : 0u);
}

// Two amax words joined: the larger |x| and (fp4) the flag of either.
template <bool FP4>
__device__ __forceinline__ unsigned mx_amax_join(unsigned m, unsigned o) {
  if constexpr (FP4) {
    const unsigned a = m & ~kMxNonFinite, b = o & ~kMxNonFinite;
    return (a > b ? a : b) | ((m | o) & kMxNonFinite);
  } else {
    return o > m ? o : m;
  }
}

// Scale exponent e from m = the block's amax word. amax = 1.f 2^(E - 127) = m' 2^(E - 126):
// m' <= 0.875 <=> fraction <= 0.75. A subnormal amax (E = 0) clamps to -127 either way; an
// all-zero block gets e = 0. (fp4: m' <= 0.75 <=> fraction <= 0.5, and 3 in place of 9)
template <bool FP4>
__device__ __forceinline__ int mx_scale_exp(unsigned m) {
  if constexpr (FP4) m &= ~kMxNonFinite;
  int e = FP4 ? (int)(m >> 23) - 129 + ((m & 0x7FFFFFu) > 0x400000u ? 1 : 0)
              : (int)(m >> 23) - 135 + ((m & 0x7FFFFFu) > 0x600000u ? 1 : 0);
  e = e < -127 ? -127 : (e > 127 ? 127 : e);
  if (m == 0) e = 0;
  return e;
}

// The block's scale byte: e + 127, and 255 for an fp4 block whose amax word carries the flag.
template <bool FP4>
__device__ __forceinline__ unsigned mx_scale_byte(unsigned m, int e) {
  return FP4 && (m & kMxNonFinite) ? 255u : (unsigned)(e + 127);
}

// Bits [SH, SH + 8) of w replaced by the e4m3fn NaN byte with x's sign when x is not finite.
template <int SH>
__device__ __forceinline__ unsigned mx_nan_byte(unsigned w, float x) {
  const unsigned b = __builtin_bit_cast(unsigned, x);
  return (b & 0x7FFFFFFFu) < kMxInfBits
             ? w
             : (w & ~(0xFFu << SH)) | ((0x7Fu | ((b >> 24) & 0x80u)) << SH);
}

// Bits [SH, SH + 4) of w replaced by the nibble 0x7 | sign << 3 when x is not finite.
template <int SH>
__device__ __forceinline__ unsigned mx_nan_nibble(unsigned w, float x) {
  const unsigned b = __builtin_bit_cast(unsigned, x);
  return (b & 0x7FFFFFFFu) < kMxInfBits
             ? w
             : (w & ~(0xFu << SH)) | ((0x7u | ((b >> 28) & 0x8u)) << SH);
}

// Four elements -> four e4m3 bytes (element 0 in the low byte): e4m3_rne(clamp(x 2^-e, +-448)),
// a non-finite element the NaN byte with its sign.
__device__ __forceinline__ unsigned mx_cvt4_e4m3(float x0, float x1, float x2, float x3, int e) {
  const float y0 = __builtin_amdgcn_fmed3f(__builtin_ldexpf(x0, -e), -448.f, 448.f);
  const float y1 = __builtin_amdgcn_fmed3f(__builtin_ldexpf(x1, -e), -448.f, 448.f);
  const float y2 = __builtin_amdgcn_fmed3f(__builtin_ldexpf(x2, -e), -448.f, 448.f);
  const float y3 = __builtin_amdgcn_fmed3f(__builtin_ldexpf(x3, -e), -448.f, 448.f);
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(y0, y1, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(y2, y3, w, true);
  unsigned u = (unsigned)w;
  u = mx_nan_byte<0>(u, x0);
  u = mx_nan_byte<8>(u, x1);
  u = mx_nan_byte<16>(u, x2);
  u = mx_nan_byte<24>(u, x3);
  return u;
}

// The fp4 conversion's scale operand, 2^e (only its exponent field is read: the ldexp folds into
// the instruction, and e = -127 is the field 0).
__device__ __forceinline__ float mx_fp4_scale(int e) {
  return __builtin_bit_cast(float, (unsigned)(e + 127) << 23);
}

// Two elements -> one byte of E2M1 nibbles (x0 in the low nibble), written into byte SEL of w; a
// non-finite element the nibble 0x7 | sign << 3, whatever the instruction makes of it.
template <int SEL>
__device__ __forceinline__ unsigned mx_cvt2_e2m1(unsigned w, float x0, float x1, float sc) {
  w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, x0, x1, sc, SEL);
  w = mx_nan_nibble<8 * SEL>(w, x0);
  return mx_nan_nibble<8 * SEL + 4>(w, x1);
}

}  // namespace ddlb
