// The weight expansion of the A16 GEMMs (gemm_skinny_a16.hip, gemm_a16_kernels.h): MX weights to
// the activations' 16-bit dtype in registers, and the MFMA that multiplies them.
#pragma once
#include "gemm_kernels.h"

namespace ddlb {
namespace {

// The conversions and the MFMA of one activation dtype. B: the byte (fp4: two elements) or the
// half (fp8: two elements) of the source dword. The scale operand is the f32 2^(s - 127), built
// from the E8M0 byte as s << 23.
template <int DT> struct A16Ops;
template <> struct A16Ops<DT_BF16> {
  using Mma = MmaBF16;
  template <int B> static __device__ __forceinline__ int fp4(unsigned v, float sc) {
    return __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, sc, B));
  }
  template <bool HI> static __device__ __forceinline__ int fp8(unsigned v, float sc) {
    return __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, sc, HI));
  }
};
template <> struct A16Ops<DT_F16> {
  using Mma = MmaF16;
  template <int B> static __device__ __forceinline__ int fp4(unsigned v, float sc) {
    return __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(v, sc, B));
  }
  template <bool HI> static __device__ __forceinline__ int fp8(unsigned v, float sc) {
    return __builtin_bit_cast(int, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(v, sc, HI));
  }
};

// Eight elements of W in A's dtype, one MFMA operand: a dword of E2M1 nibbles, or two of e4m3.
template <int DT>
__device__ __forceinline__ i32x4 a16_expand_fp4(unsigned v, float sc) {
  using Ops = A16Ops<DT>;
  return i32x4{Ops::template fp4<0>(v, sc), Ops::template fp4<1>(v, sc),
               Ops::template fp4<2>(v, sc), Ops::template fp4<3>(v, sc)};
}
template <int DT>
__device__ __forceinline__ i32x4 a16_expand_fp8(unsigned v0, unsigned v1, float sc) {
  using Ops = A16Ops<DT>;
  return i32x4{Ops::template fp8<false>(v0, sc), Ops::template fp8<true>(v0, sc),
               Ops::template fp8<false>(v1, sc), Ops::template fp8<true>(v1, sc)};
}

}  // namespace
}  // namespace ddlb
