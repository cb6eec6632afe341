// MoE dispatch for gfx950: the routing sort (moe_route.hip) and the weighted un-permute
// (moe_combine.hip). docs/ARCHITECTURE.md "MoE dispatch" has the design.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ddlb {

// Stable counting sort of the n = S * k slots p = t * k + j of ids[S, k] (int32 or int64,
// contiguous) by expert, in three launches in stream order (count, scan, place); nothing waits on
// the host and no workgroup waits for another. All outputs int32, every element written:
//   offsets[E + 1]  offsets[0] = 0, offsets[e + 1] - offsets[e] = slots whose id is e
//   row_token[n]    the token p / k of the slot sorted to row r < offsets[E], -1 for the rows behind
//   slot_row[n]     the row of slot p, -1 when ids[p] is outside [0, E) (dropped, not counted)
// Rows are ordered by expert and, inside an expert, by ascending p. ws: route_workspace_words(n, E)
// int32 words (moe_route_map.h), content irrelevant before and after.
// 1 <= E <= kRouteMaxExperts, k >= 1, 0 <= n < 2^31, n % k == 0; n == 0 launches nothing (the
// caller then zeroes offsets).
struct MoeRouteArgs {
  const void* ids = nullptr;
  int* offsets = nullptr;
  int* row_token = nullptr;
  int* slot_row = nullptr;
  int* ws = nullptr;
  int64_t n = 0;
  int k = 0, E = 0;
  int ids64 = 0;
};
hipError_t moe_route_launch(const MoeRouteArgs& a, hipStream_t s);

// out[t, :] = sum_j gate[t, j] * y[slot_row[t, j], :] over y[T, H] (f32 / f16 / bf16, rows ldy
// ELEMENTS apart), gate[S, k] f32 and slot_row[S, k] int32 (both contiguous), out[S, H] in y's
// dtype or f32 (rows ldo ELEMENTS apart). Per element, in f32: acc = +0; for j = 0 .. k - 1 in
// order, if 0 <= slot_row[t, j] < T: acc = fadd_rn(acc, fmul_rn(gate, (float)y)), no contraction;
// one RNE rounding to the output dtype. Other slots contribute nothing and read nothing.
// H * element size % 16 == 0; y and out rows 16-byte aligned. S == 0 or H == 0 launches nothing.
struct MoeCombineArgs {
  const void* y = nullptr;
  const int* slot_row = nullptr;
  const float* gate = nullptr;
  void* out = nullptr;
  int64_t ldy = 0, ldo = 0;
  int S = 0, k = 0, T = 0, H = 0;
};
hipError_t moe_combine_launch(const MoeCombineArgs& a, int din, int dout, hipStream_t s);

}  // namespace ddlb
