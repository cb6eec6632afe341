// Backward of the MoE combine for gfx950 (moe.h MoeCombineBwdArgs has the contract):
//   dy[slot_row[t, j], :] = gate[t, j] * dout[t, :]
//   dgate[t, j]           = <dout[t, :], y[slot_row[t, j], :]>
// and +0.0 in the padding rows of dy.
//
// Organised by token, as the forward is: a group of L lanes (L the power of two that holds a
// row's 16-byte vectors, at most the workgroup) takes token t, reads dout[t] once and, per choice
// j, writes the row of dy and reads the row of y for the dot product. Every row of dy is written
// by exactly one group (slot_row is injective where it is valid), so there is no scatter
// conflict and no atomic. The dot product is reduced in a fixed order: a lane sums its vectors in
// column order, the lanes of a group combine by xor shuffles (32, 16, .. 1, as far as L reaches)
// and, when the group spans waves (L = 128, 256), the waves' sums are added in wave order through
// LDS: the result is bitwise reproducible. No workgroup waits for another. The padding rows
// (row_token outside [0, S)) are zeroed in a second grid-stride phase of the same launch.
//
// Memory-bound and shaped like moe_combine.hip: 16-byte vectors of the narrower dtype (dy's; an
// f32 dout next to a 16-bit dy is read as two vectors), a grid-stride over the tokens, the grid
// sized by the CU count, 64-bit byte offsets, the k <= kCombineK choices of a token in registers
// or a loop over j for a larger k (which re-reads dout[t] per choice, from the cache).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm/gemm.h"
#include "gemm/mx_quant_in.h"
#include "gemm/row_io.h"
#include "moe.h"

namespace ddlb {
namespace {

constexpr int kWaves = kRowThreads / 64;

// vector c (N = 8 or 4 elements of the narrower dtype DO) of a dout row as fp32
template <int DI, int DO>
__device__ __forceinline__ void load_dout(const char* row, int c, float* f) {
  if constexpr (DI == DO) {
    MxqIn<DI>::cvt(*(const mxq_u32x4*)(row + (int64_t)c * 16), f);
  } else {  // f32 next to a 16-bit dy: eight floats
    MxqIn<DT_F32>::cvt(*(const mxq_u32x4*)(row + (int64_t)c * 32), f);
    MxqIn<DT_F32>::cvt(*(const mxq_u32x4*)(row + (int64_t)c * 32 + 16), f + 4);
  }
}

// One choice of one token, one vector: the dy store and this lane's part of the dot product.
template <int DO, int N, bool DG>
__device__ __forceinline__ void slot_vec(const MoeCombineBwdArgs& a, int row, float g,
                                         const float* f, int c, float& acc) {
  if (row < 0) return;  // dropped or out of range: nothing is read or written
  constexpr int OSZ = 16 / N;
  float p[N];  // fmul_rn to f32, then row_store's one rounding to dy's dtype
#pragma unroll
  for (int i = 0; i < N; ++i) p[i] = row_keep_f32(g * f[i]);
  row_store<DO, N>((char*)a.dy + ((int64_t)row * a.lddy * OSZ + (int64_t)c * 16), p);
  if constexpr (DG) {
    float yv[N];
    MxqIn<DO>::cvt(*(const mxq_u32x4*)((const char*)a.y +
                                        ((int64_t)row * a.ldy * OSZ + (int64_t)c * 16)), yv);
#pragma unroll
    for (int i = 0; i < N; ++i) acc += f[i] * yv[i];
  }
}

// the sum over the min(L, 64) lanes of a group that share a wave, in every one of them
__device__ __forceinline__ float group_wave_sum(float v, int L) {
  for (int d = (L < 64 ? L : 64) >> 1; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

template <int DI, int DO, bool REGS, bool DG>
__global__ __launch_bounds__(kRowThreads) void moe_combine_bwd_kernel(const MoeCombineBwdArgs a,
                                                                      int L) {
  constexpr int N = MxqIn<DO>::kElems;
  constexpr int ISZ = DI == DT_F32 ? 4 : 2, OSZ = 16 / N;
  __shared__ float red[kWaves][kCombineK];
  const int vpr = a.H / N;  // vectors per row, vpr <= L or L == kRowThreads
  const int tid = threadIdx.x, wave = tid >> 6;
  const int rows_pp = kRowThreads / L;
  const int r_in = tid / L, c0 = tid & (L - 1);
  const int64_t step = (int64_t)gridDim.x * rows_pp;

  // Phase 1, by token. The trip count is the workgroup's, not the lane's: every lane takes part
  // in the shuffles and barriers, a lane without a token or a vector adds zeros.
  for (int64_t base = (int64_t)blockIdx.x * rows_pp; base < a.S; base += step) {
    const int64_t t = base + r_in;
    const bool live = t < a.S;
    const int* rows = a.slot_row + (live ? t : 0) * a.k;
    const float* gates = a.gate + (live ? t : 0) * a.k;
    const char* drow = (const char*)a.dout + (live ? t : 0) * a.lddo * ISZ;
    if constexpr (REGS) {
      int row[kCombineK];
      float g[kCombineK], acc[kCombineK];
#pragma unroll
      for (int j = 0; j < kCombineK; ++j) {
        const int r = (live && j < a.k) ? rows[j] : -1;
        row[j] = (r >= 0 && r < a.T) ? r : -1;
        g[j] = (live && j < a.k) ? gates[j] : 0.0f;
        acc[j] = 0.0f;
      }
      if (live) {
        for (int c = c0; c < vpr; c += L) {
          float f[N];
          load_dout<DI, DO>(drow, c, f);
#pragma unroll
          for (int j = 0; j < kCombineK; ++j) slot_vec<DO, N, DG>(a, row[j], g[j], f, c, acc[j]);
        }
      }
      if constexpr (DG) {
#pragma unroll
        for (int j = 0; j < kCombineK; ++j)
          if (j < a.k) acc[j] = group_wave_sum(acc[j], L);  // (a.k and L are uniform)
        if (L > 64) {  // the group's waves, in wave order
          if ((tid & 63) == 0) {
#pragma unroll
            for (int j = 0; j < kCombineK; ++j)
              if (j < a.k) red[wave][j] = acc[j];
          }
          __syncthreads();
          if (c0 == 0) {
#pragma unroll
            for (int j = 0; j < kCombineK; ++j) {
              if (j >= a.k) continue;
              float v = red[wave][j];
              for (int w = 1; w < L / 64; ++w) v += red[wave + w][j];
              acc[j] = v;
            }
          }
          __syncthreads();
        }
        if (live && c0 == 0) {
#pragma unroll
          for (int j = 0; j < kCombineK; ++j)
            if (j < a.k) a.dgate[t * a.k + j] = acc[j];
        }
      }
    } else {
      for (int j = 0; j < a.k; ++j) {
        const int r = live ? rows[j] : -1;
        const int row = (r >= 0 && r < a.T) ? r : -1;
        const float g = live ? gates[j] : 0.0f;
        float acc = 0.0f;
        if (live) {
          for (int c = c0; c < vpr; c += L) {
            float f[N];
            load_dout<DI, DO>(drow, c, f);
            slot_vec<DO, N, DG>(a, row, g, f, c, acc);
          }
        }
        if constexpr (DG) {
          acc = group_wave_sum(acc, L);
          if (L > 64) {
            if ((tid & 63) == 0) red[wave][0] = acc;
            __syncthreads();
            if (c0 == 0) {
              float v = red[wave][0];
              for (int w = 1; w < L / 64; ++w) v += red[wave + w][0];
              acc = v;
            }
            __syncthreads();
          }
          if (live && c0 == 0) a.dgate[t * a.k + j] = acc;
        }
      }
    }
  }

  // Phase 2: +0.0 in the rows no token was sorted to (no barrier from here on).
  for (int64_t r = (int64_t)blockIdx.x * rows_pp + r_in; r < a.T; r += step) {
    const int tok = a.row_token[r];
    if (tok >= 0 && tok < a.S) continue;
    char* orow = (char*)a.dy + r * a.lddy * OSZ;
    for (int c = c0; c < vpr; c += L)
      *(mxq_u32x4*)(orow + (int64_t)c * 16) = mxq_u32x4{0u, 0u, 0u, 0u};
  }
}

template <int DI, int DO>
hipError_t combine_bwd_go(const MoeCombineBwdArgs& a, hipStream_t s) {
  const int vpr = a.H / MxqIn<DO>::kElems;
  int L = 1;
  while (L < vpr && L < kRowThreads) L *= 2;
  const int64_t rows = a.S > a.T ? a.S : a.T;
  const dim3 grid(row_grid(rows, kRowThreads / L)), block(kRowThreads);
  const bool regs = a.k <= kCombineK, dg = a.y != nullptr;
  if (regs && dg)
    hipLaunchKernelGGL((moe_combine_bwd_kernel<DI, DO, true, true>), grid, block, 0, s, a, L);
  else if (regs)
    hipLaunchKernelGGL((moe_combine_bwd_kernel<DI, DO, true, false>), grid, block, 0, s, a, L);
  else if (dg)
    hipLaunchKernelGGL((moe_combine_bwd_kernel<DI, DO, false, true>), grid, block, 0, s, a, L);
  else
    hipLaunchKernelGGL((moe_combine_bwd_kernel<DI, DO, false, false>), grid, block, 0, s, a, L);
  return hipGetLastError();
}

}  // namespace

hipError_t moe_combine_bwd_launch(const MoeCombineBwdArgs& a, int din, int dout, hipStream_t s) {
  if (din != DT_F32 && din != DT_F16 && din != DT_BF16) return hipErrorInvalidValue;
  if (dout != DT_F32 && dout != DT_F16 && dout != DT_BF16) return hipErrorInvalidValue;
  if (dout != din && din != DT_F32) return hipErrorInvalidValue;
  if (a.S < 0 || a.k < 1 || a.T < 0 || a.H < 0) return hipErrorInvalidValue;
  if ((a.y == nullptr) != (a.dgate == nullptr)) return hipErrorInvalidValue;
  if (a.H == 0 || (a.S == 0 && a.T == 0)) return hipSuccess;
  const int isz = dtype_size(din), osz = dtype_size(dout);
  if (((int64_t)a.H * osz) % 16) return hipErrorInvalidValue;
  if (a.S > 0 && (a.slot_row == nullptr || a.gate == nullptr ||
                  !row_ptr_ok(a.dout, a.lddo, a.H, isz)))
    return hipErrorInvalidValue;
  if (a.T > 0 && (a.row_token == nullptr || !row_ptr_ok(a.dy, a.lddy, a.H, osz) ||
                  (a.y != nullptr && !row_ptr_ok(a.y, a.ldy, a.H, osz))))
    return hipErrorInvalidValue;
  if (din == dout) {
    if (din == DT_F32) return combine_bwd_go<DT_F32, DT_F32>(a, s);
    return din == DT_F16 ? combine_bwd_go<DT_F16, DT_F16>(a, s)
                         : combine_bwd_go<DT_BF16, DT_BF16>(a, s);
  }
  return dout == DT_F16 ? combine_bwd_go<DT_F32, DT_F16>(a, s)
                        : combine_bwd_go<DT_F32, DT_BF16>(a, s);
}

}  // namespace ddlb
