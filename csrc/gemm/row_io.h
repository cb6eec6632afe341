// What the streaming row kernels share (moe_combine.hip, moe_combine_bwd.hip, moe_gather.hip,
// glu_act.hip): fp32 values to the output dtype as 16-byte stores, the workgroup size, and the
// grid cap taken from the CU count. The 16-byte loads are MxqIn<DT> (mx_quant_in.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_info.h"
#include "gemm.h"
#include "mx_quant_in.h"

namespace ddlb {

constexpr int kRowThreads = 256;

__device__ __forceinline__ unsigned row_bf16_rne(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0u;  // NaN
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// An f32 value that the compiler must materialise. A product that goes straight into row_store's
// f16 conversion is folded with it into v_fma_mixlo_f16 (with or without fp contract), which
// rounds the exact product once instead of to f32 and then to f16: not what (a * b).to(float16)
// computes in torch.
__device__ __forceinline__ float row_keep_f32(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// N f32 values -> the output dtype, one RNE rounding each, stored as 16-byte vectors (N = 4
// into f32 or N = 8 into 16 bits: one; N = 8 into f32: two)
template <int OUT, int N>
__device__ __forceinline__ void row_store(char* p, const float* acc) {
  if constexpr (OUT == DT_F32) {
#pragma unroll
    for (int i = 0; i < N; i += 4)
      *(float4*)(p + 4 * i) = float4{acc[i], acc[i + 1], acc[i + 2], acc[i + 3]};
  } else {
    static_assert(N == 8, "16-bit outputs are stored eight at a time");
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if constexpr (OUT == DT_BF16) {
        w[i] = row_bf16_rne(acc[2 * i]) | (row_bf16_rne(acc[2 * i + 1]) << 16);
      } else {
        const _Float16 lo = (_Float16)acc[2 * i], hi = (_Float16)acc[2 * i + 1];
        w[i] = (unsigned)__builtin_bit_cast(unsigned short, lo) |
               ((unsigned)__builtin_bit_cast(unsigned short, hi) << 16);
      }
    }
    *(mxq_u32x4*)p = mxq_u32x4{w[0], w[1], w[2], w[3]};
  }
}

// How a workgroup of kRowThreads lanes takes rows of vpr 16-byte vectors: 256 / vpr rows per pass
// when a row is shorter than the workgroup (lane -> row r_in, vector c0), one row striding
// otherwise. Lanes with r_in >= rows_pp have no row.
__host__ __device__ __forceinline__ int rows_per_pass(int vpr) {
  return vpr < kRowThreads ? kRowThreads / (vpr > 0 ? vpr : 1) : 1;
}
__device__ __forceinline__ void row_lane(int vpr, int tid, int& r_in, int& c0) {
  r_in = 0;
  c0 = tid;
  if (vpr < kRowThreads) {
    r_in = tid / vpr;
    c0 = tid - r_in * vpr;
  }
}

// a row-major operand the row kernels can take: rows of at least `cols` elements, 16-byte aligned
inline bool row_ptr_ok(const void* p, int64_t ld, int64_t cols, int esz) {
  return p != nullptr && ld >= cols && ((uintptr_t)p & 15) == 0 && (ld * esz) % 16 == 0;
}

// Workgroups for `rows` rows taken rows_pp per pass, grid-striding: at most 8 per CU.
inline unsigned row_grid(int64_t rows, int rows_pp) {
  int64_t grid = (rows + rows_pp - 1) / rows_pp;
  const int64_t cap = (int64_t)num_cus() * 8;
  if (grid > cap) grid = cap;
  return (unsigned)(grid < 1 ? 1 : grid);
}

}  // namespace ddlb
