// What the MX quantisers (mx_quant.hip, mx_quant_t.hip) share: how 16 input bytes become fp32
// values, and the row-wise work on one such vector (a block's amax across the lanes that share
// it, the conversion, the packed store). The rule itself is mx_cvt.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm.h"
#include "mx_cvt.h"

namespace ddlb {

typedef __attribute__((ext_vector_type(4))) unsigned mxq_u32x4;

// The 16 bytes of one load as fp32 values; one element at p as fp32.
template <int DT> struct MxqIn;
template <> struct MxqIn<DT_F32> {
  static constexpr int kElems = 4;
  static __device__ __forceinline__ void cvt(const mxq_u32x4 v, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned u = v[i];  // (a bit_cast of the element lvalue itself reads element 0)
      f[i] = __builtin_bit_cast(float, u);
    }
  }
  static __device__ __forceinline__ float elem(const char* p) { return *(const float*)p; }
};
template <> struct MxqIn<DT_BF16> {
  static constexpr int kElems = 8;
  static __device__ __forceinline__ void cvt(const mxq_u32x4 v, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = __builtin_bit_cast(float, v[i] << 16);
      f[2 * i + 1] = __builtin_bit_cast(float, v[i] & 0xFFFF0000u);
    }
  }
  static __device__ __forceinline__ float elem(const char* p) {
    return __builtin_bit_cast(float, (unsigned)*(const unsigned short*)p << 16);
  }
};
template <> struct MxqIn<DT_F16> {
  static constexpr int kElems = 8;
  static __device__ __forceinline__ void cvt(const mxq_u32x4 v, float* f) {
    typedef __attribute__((ext_vector_type(2))) _Float16 h2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned u = v[i];
      const h2 h = __builtin_bit_cast(h2, u);
      f[2 * i] = (float)h.x;
      f[2 * i + 1] = (float)h.y;
    }
  }
  static __device__ __forceinline__ float elem(const char* p) {
    return (float)*(const _Float16*)p;
  }
};

// One lane's vector of a row: 32 / kElems neighbouring lanes hold one block (all of them must be
// active: the amax is a cross-lane max, on the integer image of |x|: exact, subnormals included).
// q points at this vector's packed output (kElems bytes, fp4: kElems / 2), s at the block's scale
// byte, which the block's first lane (lead) stores.
template <int DT, bool FP4>
__device__ __forceinline__ void mxq_rowwise_vec(const mxq_u32x4 v, char* q, uint8_t* s,
                                                bool lead) {
  using In = MxqIn<DT>;
  constexpr int EPV = In::kElems;   // elements per 16-byte vector
  constexpr int LPB = 32 / EPV;     // lanes that share a 32-element block
  float f[EPV];
  In::cvt(v, f);
  unsigned m = 0;  // |x| as an integer: ordered as the floats are
#pragma unroll
  for (int i = 0; i < EPV; ++i) {
    m = mx_amax_join<FP4>(m, mx_amax_bits<FP4>(f[i]));
  }
#pragma unroll
  for (int d = 1; d < LPB; d *= 2) {
    m = mx_amax_join<FP4>(m, (unsigned)__shfl_xor((int)m, d));
  }
  const int e = mx_scale_exp<FP4>(m);  // (mx_cvt.h: the rule, shared with the GEMM epilogue)
  if constexpr (FP4) {
    const float sc = mx_fp4_scale(e);
    unsigned w = 0;
    w = mx_cvt2_e2m1<0>(w, f[0], f[1], sc);
    w = mx_cvt2_e2m1<1>(w, f[2], f[3], sc);
    if constexpr (EPV == 8) {
      w = mx_cvt2_e2m1<2>(w, f[4], f[5], sc);
      w = mx_cvt2_e2m1<3>(w, f[6], f[7], sc);
      *(unsigned*)q = w;
    } else {
      *(unsigned short*)q = (unsigned short)w;
    }
  } else {
    unsigned out[EPV / 4];
#pragma unroll
    for (int i = 0; i < EPV / 4; ++i)
      out[i] = mx_cvt4_e4m3(f[4 * i], f[4 * i + 1], f[4 * i + 2], f[4 * i + 3], e);
    if constexpr (EPV == 8)
      *(uint2*)q = uint2{out[0], out[1]};
    else
      *(unsigned*)q = out[0];
  }
  if (lead) *s = (uint8_t)mx_scale_byte<FP4>(m, e);
}

}  // namespace ddlb
