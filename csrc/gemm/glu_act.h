// The gated activation as an op of its own, forward and backward (glu_act.hip), on the packed
// layout of the gated GEMM epilogue (GemmArgs::glu): in c[T, 2F] columns 64g .. 64g + 31 are gate
// columns and 64g + 32 .. 64g + 63 the matching up columns.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ddlb {

// c[T, 2F] (f32 / f16 / bf16, rows ldc ELEMENTS apart), act one of ACT_* (gemm.h).
//   forward:  out = h[T, F] in c's dtype or f32 (rows ldo apart):
//             h[t, 32g + j] = rne(act1(float(gate)) * float(up)), act1 the GEMM epilogue's.
//   backward: dh[T, F] in c's dtype (rows ldh apart), out = dc[T, 2F] in c's dtype (rows ldo
//             apart), in f32 with one rounding each:
//             dc[t, 64g + j] = (dh * up) * act'(gate), dc[t, 64g + 32 + j] = dh * act1(gate);
//             act' is finite for every finite gate, a NaN gate makes both NaN.
// 2F % 64 == 0; rows 16-byte aligned. T == 0 or F == 0 launches nothing.
struct GluArgs {
  const void* c = nullptr;
  const void* dh = nullptr;
  void* out = nullptr;
  int64_t ldc = 0, ldh = 0, ldo = 0;
  int T = 0, F = 0;
  int act = 0;
};
hipError_t glu_fwd_launch(const GluArgs& a, int din, int dout, hipStream_t s);
hipError_t glu_bwd_launch(const GluArgs& a, int din, hipStream_t s);

}  // namespace ddlb
