// MoE combine for gfx950: the weighted un-permute out[t, :] = sum_j gate[t, j] * y[slot_row[t, j], :]
// (moe.h MoeCombineArgs has the contract).
//
// A gather through the inverted index slot_row, not a scatter: every output element is summed by
// one lane in the fixed order j = 0 .. k - 1 with a separate multiply and add, so the result is
// bitwise reproducible and equal to the same steps written with torch ops (no float atomics, no
// fma contraction). A streaming, memory-bound kernel shaped like the MX quantiser: one 16-byte
// load per lane and row of y, a workgroup takes 256 / (vectors per row) tokens per pass (one,
// striding along H, for long rows) and grid-strides over the tokens; the grid is sized by the CU
// count. The k row indices and gates of a token are read once, into registers, for k <= kCombineK;
// a larger k re-reads them per vector from the cache. No LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm/gemm.h"
#include "gemm/mx_quant_in.h"
#include "gemm/row_io.h"
#include "moe.h"

namespace ddlb {
namespace {

template <int DT, int N>
__device__ __forceinline__ void combine_add(float* acc, const MoeCombineArgs& a, int row, float g,
                                            int c) {
  if (row < 0 || row >= a.T) return;  // dropped or out of range: nothing is read
  constexpr int ESZ = 16 / N;
  const char* yr = (const char*)a.y + (int64_t)row * a.ldy * ESZ;
  const mxq_u32x4 v = *(const mxq_u32x4*)(yr + (int64_t)c * 16);
  float f[N];
  MxqIn<DT>::cvt(v, f);
  {
    // fmul_rn, then fadd_rn. (__fmul_rn / __fadd_rn are plain * and + inside the toolchain's
    // headers, where the compiler may still contract them into an fma: the operators are written
    // here, under the pragma that keeps the two roundings.)
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const float prod = g * f[i];
      acc[i] = acc[i] + prod;
    }
  }
}

template <int DT, int OUT, bool REGS>
__global__ __launch_bounds__(kRowThreads) void moe_combine_kernel(const MoeCombineArgs a,
                                                                      int rows_pp) {
  constexpr int N = MxqIn<DT>::kElems;  // elements per 16-byte vector of y
  constexpr int OSZ = OUT == DT_F32 ? 4 : 2;
  const int vpr = a.H / N;              // vectors per row
  int r_in, c0;
  row_lane(vpr, threadIdx.x, r_in, c0);
  if (r_in >= rows_pp) return;
  const int64_t step = (int64_t)gridDim.x * rows_pp;
  for (int64_t t = (int64_t)blockIdx.x * rows_pp + r_in; t < a.S; t += step) {
    const int* rows = a.slot_row + t * a.k;
    const float* gates = a.gate + t * a.k;
    char* orow = (char*)a.out + t * a.ldo * OSZ;
    int row[kCombineK];
    float g[kCombineK];
    if constexpr (REGS) {
#pragma unroll
      for (int j = 0; j < kCombineK; ++j) {
        row[j] = j < a.k ? rows[j] : -1;
        g[j] = j < a.k ? gates[j] : 0.0f;
      }
    }
    for (int c = c0; c < vpr; c += kRowThreads) {
      float acc[N];
#pragma unroll
      for (int i = 0; i < N; ++i) acc[i] = 0.0f;
      if constexpr (REGS) {
#pragma unroll
        for (int j = 0; j < kCombineK; ++j) combine_add<DT, N>(acc, a, row[j], g[j], c);
      } else {
        for (int j = 0; j < a.k; ++j) combine_add<DT, N>(acc, a, rows[j], gates[j], c);
      }
      row_store<OUT, N>(orow + (int64_t)c * N * OSZ, acc);
    }
  }
}

template <int DT, int OUT>
hipError_t combine_go(const MoeCombineArgs& a, hipStream_t s) {
  const int rows_pp = rows_per_pass(a.H / MxqIn<DT>::kElems);
  const dim3 grid(row_grid(a.S, rows_pp)), block(kRowThreads);
  if (a.k <= kCombineK)
    hipLaunchKernelGGL((moe_combine_kernel<DT, OUT, true>), grid, block, 0, s, a, rows_pp);
  else
    hipLaunchKernelGGL((moe_combine_kernel<DT, OUT, false>), grid, block, 0, s, a, rows_pp);
  return hipGetLastError();
}

}  // namespace

hipError_t moe_combine_launch(const MoeCombineArgs& a, int din, int dout, hipStream_t s) {
  if (din != DT_F32 && din != DT_F16 && din != DT_BF16) return hipErrorInvalidValue;
  if (dout != din && dout != DT_F32) return hipErrorInvalidValue;
  if (a.S < 0 || a.k < 1 || a.T < 0 || a.H < 0) return hipErrorInvalidValue;
  if (a.S == 0 || a.H == 0) return hipSuccess;
  const int esz = dtype_size(din), osz = dtype_size(dout);
  if (a.y == nullptr && a.T > 0) return hipErrorInvalidValue;
  if (a.slot_row == nullptr || a.gate == nullptr || a.out == nullptr || (a.H * esz) % 16 ||
      a.ldy < a.H || a.ldo < a.H || ((uintptr_t)a.y & 15) || (a.ldy * esz) % 16 ||
      ((uintptr_t)a.out & 15) || (a.ldo * osz) % 16)
    return hipErrorInvalidValue;
  if (din == DT_F32) return combine_go<DT_F32, DT_F32>(a, s);
  if (din == DT_F16)
    return dout == DT_F32 ? combine_go<DT_F16, DT_F32>(a, s) : combine_go<DT_F16, DT_F16>(a, s);
  return dout == DT_F32 ? combine_go<DT_BF16, DT_F32>(a, s) : combine_go<DT_BF16, DT_BF16>(a, s);
}

}  // namespace ddlb
