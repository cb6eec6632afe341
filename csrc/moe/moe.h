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

// choices of a token that moe_combine and its backward hold in registers (a larger k loops)
constexpr int kCombineK = 8;

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

// The dense gather of the routed rows (moe_gather.hip): out[r, :] = x[row_token[r], :] over
// x[S, H] (f32 / f16 / bf16, rows ldx ELEMENTS apart) into out[T, H] of the same dtype (rows ldo
// apart); a row whose index is outside [0, S) is +0.0 and nothing is read for it. Bytes are
// copied, nothing is converted. H * element size % 16 == 0; rows 16-byte aligned. T == 0 or
// H == 0 launches nothing. Its backward is moe_combine with gates of 1.
struct MoeGatherArgs {
  const void* x = nullptr;
  const int* row_token = nullptr;
  void* out = nullptr;
  int64_t ldx = 0, ldo = 0;
  int S = 0, T = 0, H = 0;
};
hipError_t moe_gather_launch(const MoeGatherArgs& a, int dt, hipStream_t s);

// Backward of moe_combine (moe_combine_bwd.hip), by token, for (row_token, slot_row) mutually
// inverse as moe_route writes them. dout[S, H] f32 / f16 / bf16 (rows lddo apart); dy[T, H] in
// dout's dtype or, for f32 dout, any of the three (rows lddy apart); y[T, H] in dy's dtype (rows
// ldy apart) or null; gate[S, k] f32, slot_row[S, k] and row_token[T] int32, dgate[S, k] f32, all
// contiguous. For every slot (t, j) with 0 <= r = slot_row[t, j] < T:
//   dy[r, c]    = rne(fmul_rn(gate[t, j], (float)dout[t, c]))
//   dgate[t, j] = sum_c (float)dout[t, c] * (float)y[r, c] in f32: a lane sums its vectors in
//                 column order, the lanes of a row combine in a fixed tree (wave shuffles, then
//                 LDS when a row spans waves): bitwise reproducible, no atomics.
// Other slots read nothing and get dgate = +0.0. Rows r with row_token[r] outside [0, S) (the
// padding behind offsets[E]) are set to +0.0 in a second grid-stride phase of the same launch,
// so under the precondition every element of dy and dgate is written. Every index is
// range-checked before use: without the precondition nothing outside the tensors is addressed
// and the values are unspecified. y == nullptr (then dgate must be too) skips the dgate part.
// H * (dy element size) % 16 == 0; rows of dout, y and dy 16-byte aligned.
struct MoeCombineBwdArgs {
  const void* dout = nullptr;
  const int* slot_row = nullptr;
  const float* gate = nullptr;
  const int* row_token = nullptr;
  const void* y = nullptr;
  void* dy = nullptr;
  float* dgate = nullptr;
  int64_t lddo = 0, ldy = 0, lddy = 0;
  int S = 0, k = 0, T = 0, H = 0;
};
hipError_t moe_combine_bwd_launch(const MoeCombineBwdArgs& a, int din, int dout, hipStream_t s);

}  // namespace ddlb
