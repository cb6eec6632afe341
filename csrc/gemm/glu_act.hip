// The gated activation on the packed [T, 2F] layout, forward and backward (glu_act.h has the
// contract). What the tiled GEMM's gated epilogue does to its accumulators, as an op that keeps
// the pre-activation c, so that a backward pass can read it.
//
// Streaming and memory-bound, shaped like moe_combine.hip: 16-byte loads, 256 / (vectors per
// row) rows per workgroup pass when rows are short, one row striding when long, a grid-stride
// over the rows, the grid sized by the CU count, 64-bit byte offsets. The groups of 32 gate and 32
// up columns are whole 16-byte vectors, so one lane loads a gate vector and the matching up
// vector 32 columns on: no LDS, no cross-lane traffic.
//
// act1 and x_sigmoid are the epilogue's own (gemm_kernels.h is included for them; none of its
// kernel templates is instantiated here). The derivative act' is written so that no finite gate
// gives NaN or Inf: sigmoid s and 1 - s both come from exp(-|z|), without cancellation, and gelu's
// polynomial is evaluated on the gate clamped to +-32, where s (1 - s) is already exactly 0 in
// fp32, so the limit (1 or 0) comes out instead of g * 0 * inf.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm.h"
#include "gemm_kernels.h"
#include "glu_act.h"
#include "mx_quant_in.h"
#include "row_io.h"

namespace ddlb {
namespace {

constexpr float kGeluC0 = 0.7978845608028654f, kGeluC1 = 0.044715f;
constexpr float kGeluClamp = 32.f;  // exp(-2 u(32)) = exp(-2389) is 0 in fp32

// s = sigmoid(z) and c = 1 - s, each with a small relative error: t = exp(-|z|) is in [0, 1]
__device__ __forceinline__ void sigmoid_pair(float z, float& s, float& c) {
  const float t = expf(-fabsf(z));
  const float hi = 1.f / (1.f + t), lo = t * hi;
  s = z >= 0.f ? hi : lo;
  c = z >= 0.f ? lo : hi;
}

// d act1(g) / dg; finite for every finite g, NaN for a NaN g
__device__ __forceinline__ float act1_grad(float g, int act) {
  float d, s, c;
  switch (act) {
    case ACT_GELU: {  // act1 = g sigmoid(2u): s + g s (1 - s) 2u'
      const float x = fminf(fmaxf(g, -kGeluClamp), kGeluClamp);
      const float u = kGeluC0 * (x + kGeluC1 * x * x * x);
      const float du = kGeluC0 * (1.f + 3.f * kGeluC1 * x * x);
      sigmoid_pair(2.f * u, s, c);
      d = s + x * s * c * (2.f * du);
      break;
    }
    case ACT_RELU: d = g <= 0.f ? 0.f : 1.f; break;
    case ACT_SILU:  // act1 = g sigmoid(g): s (1 + g (1 - s)); g (1 - s) cannot overflow
      sigmoid_pair(g, s, c);
      d = s * (1.f + g * c);
      break;
    default: d = 1.f; break;
  }
  return g != g ? g : d;
}

// byte offset of the gate vector that holds packed output column e (e % N == 0, N | 32)
template <int ESZ>
__device__ __forceinline__ int64_t gate_byte(int e) {
  return (int64_t)((e >> 5) * 64 + (e & 31)) * ESZ;
}

template <int DT, int OUT>
__global__ __launch_bounds__(kRowThreads) void glu_fwd_kernel(const GluArgs a, int rows_pp) {
  constexpr int N = MxqIn<DT>::kElems;
  constexpr int ESZ = 16 / N, OSZ = OUT == DT_F32 ? 4 : 2;
  const int vpr = a.F / N;  // vectors per row of h
  int r_in, c0;
  row_lane(vpr, threadIdx.x, r_in, c0);
  if (r_in >= rows_pp) return;
  const int64_t step = (int64_t)gridDim.x * rows_pp;
  for (int64_t t = (int64_t)blockIdx.x * rows_pp + r_in; t < a.T; t += step) {
    const char* crow = (const char*)a.c + t * a.ldc * ESZ;
    char* orow = (char*)a.out + t * a.ldo * OSZ;
    for (int v = c0; v < vpr; v += kRowThreads) {
      const char* gp = crow + gate_byte<ESZ>(v * N);
      float g[N], u[N], h[N];
      MxqIn<DT>::cvt(*(const mxq_u32x4*)gp, g);
      MxqIn<DT>::cvt(*(const mxq_u32x4*)(gp + 32 * ESZ), u);
#pragma unroll
      for (int i = 0; i < N; ++i) h[i] = row_keep_f32(act1(g[i], a.act) * u[i]);  // one f32 product
      row_store<OUT, N>(orow + (int64_t)v * N * OSZ, h);
    }
  }
}

template <int DT>
__global__ __launch_bounds__(kRowThreads) void glu_bwd_kernel(const GluArgs a, int rows_pp) {
  constexpr int N = MxqIn<DT>::kElems;
  constexpr int ESZ = 16 / N;
  const int vpr = a.F / N;  // vectors per row of dh
  int r_in, c0;
  row_lane(vpr, threadIdx.x, r_in, c0);
  if (r_in >= rows_pp) return;
  const int64_t step = (int64_t)gridDim.x * rows_pp;
  for (int64_t t = (int64_t)blockIdx.x * rows_pp + r_in; t < a.T; t += step) {
    const char* crow = (const char*)a.c + t * a.ldc * ESZ;
    const char* hrow = (const char*)a.dh + t * a.ldh * ESZ;
    char* orow = (char*)a.out + t * a.ldo * ESZ;
    for (int v = c0; v < vpr; v += kRowThreads) {
      const int64_t gb = gate_byte<ESZ>(v * N);
      float g[N], u[N], d[N], dg[N], du[N];
      MxqIn<DT>::cvt(*(const mxq_u32x4*)(crow + gb), g);
      MxqIn<DT>::cvt(*(const mxq_u32x4*)(crow + gb + 32 * ESZ), u);
      MxqIn<DT>::cvt(*(const mxq_u32x4*)(hrow + (int64_t)v * 16), d);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        dg[i] = row_keep_f32((d[i] * u[i]) * act1_grad(g[i], a.act));
        du[i] = row_keep_f32(d[i] * act1(g[i], a.act));
      }
      row_store<DT, N>(orow + gb, dg);
      row_store<DT, N>(orow + gb + 32 * ESZ, du);
    }
  }
}

template <int DT, int OUT>
hipError_t glu_fwd_go(const GluArgs& a, hipStream_t s) {
  const int rows_pp = rows_per_pass(a.F / MxqIn<DT>::kElems);
  hipLaunchKernelGGL((glu_fwd_kernel<DT, OUT>), dim3(row_grid(a.T, rows_pp)), dim3(kRowThreads),
                     0, s, a, rows_pp);
  return hipGetLastError();
}

template <int DT>
hipError_t glu_bwd_go(const GluArgs& a, hipStream_t s) {
  const int rows_pp = rows_per_pass(a.F / MxqIn<DT>::kElems);
  hipLaunchKernelGGL((glu_bwd_kernel<DT>), dim3(row_grid(a.T, rows_pp)), dim3(kRowThreads), 0, s,
                     a, rows_pp);
  return hipGetLastError();
}

bool glu_common_ok(const GluArgs& a, int din) {
  if (din != DT_F32 && din != DT_F16 && din != DT_BF16) return false;
  if (a.T < 0 || a.F < 0 || a.F % 32 || a.F > (1 << 29)) return false;
  return a.act == ACT_NONE || a.act == ACT_GELU || a.act == ACT_RELU || a.act == ACT_SILU;
}

}  // namespace

hipError_t glu_fwd_launch(const GluArgs& a, int din, int dout, hipStream_t s) {
  if (!glu_common_ok(a, din) || (dout != din && dout != DT_F32)) return hipErrorInvalidValue;
  if (a.T == 0 || a.F == 0) return hipSuccess;
  if (!row_ptr_ok(a.c, a.ldc, 2 * a.F, dtype_size(din)) ||
      !row_ptr_ok(a.out, a.ldo, a.F, dtype_size(dout)))
    return hipErrorInvalidValue;
  if (din == DT_F32) return glu_fwd_go<DT_F32, DT_F32>(a, s);
  if (din == DT_F16)
    return dout == DT_F32 ? glu_fwd_go<DT_F16, DT_F32>(a, s) : glu_fwd_go<DT_F16, DT_F16>(a, s);
  return dout == DT_F32 ? glu_fwd_go<DT_BF16, DT_F32>(a, s) : glu_fwd_go<DT_BF16, DT_BF16>(a, s);
}

hipError_t glu_bwd_launch(const GluArgs& a, int din, hipStream_t s) {
  if (!glu_common_ok(a, din)) return hipErrorInvalidValue;
  if (a.T == 0 || a.F == 0) return hipSuccess;
  const int esz = dtype_size(din);
  if (!row_ptr_ok(a.c, a.ldc, 2 * a.F, esz) || !row_ptr_ok(a.dh, a.ldh, a.F, esz) ||
      !row_ptr_ok(a.out, a.ldo, 2 * a.F, esz))
    return hipErrorInvalidValue;
  if (din == DT_F32) return glu_bwd_go<DT_F32>(a, s);
  return din == DT_F16 ? glu_bwd_go<DT_F16>(a, s) : glu_bwd_go<DT_BF16>(a, s);
}

}  // namespace ddlb
