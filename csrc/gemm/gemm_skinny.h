// Skinny-M block-scaled GEMM (csrc/gemm/gemm_skinny.hip): C[M, N] = A[M, K] W[N, K]^T for decode
// shapes, M (or the rows of an expert) <= 64, where the work is one pass over the weights. Its
// arguments and the host-side arithmetic of its launch: strips, K-slices, the automatic slice
// count and the workspace, usable from host code (ddlb_amd/ops/gemm.py states the same rules).
//
// A workgroup is 4 waves, each owning kSkinnyNR 16-row tiles of W: a strip of 64 kSkinnyNR weight
// rows. It walks one K-slice of its strip; the grid is strips x S x groups. S > 1 writes f32
// partials [S, rows, N] that a second kernel sums in the order s = 0 .. S - 1 (no atomics: two
// runs write the same bytes). The epilogue, at the unsplit store or in that second kernel, is
// dense or gated (glu) and / or MX-quantising (c_scale): a decode FFN's fc1 in one call. Any M is
// correct; past 64 rows the weights are streamed once per 64 rows, which is what the tiled kernel
// is for.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm.h"

namespace ddlb {

// Compile-time choices, picked by measurement (docs/RESULTS.md "Skinny-M GEMM"). The W4A8 form
// keeps both numbers with their meanings apart: the ring is kSkinnyPanel W K-tiles (as fp4), the
// LDS panel kSkinnyPanel 128-byte K-rows of A (as fp8), which is kSkinnyPanel / 2 W K-tiles, so
// kSkinnyPanel is even for it. A panel as long as the ring would be 64 KiB at 64 rows, over the
// static LDS limit; a ring as short as the panel (2 tiles) would halve the bytes in flight per
// wave. This split is the only one timed (docs/RESULTS.md: at the MoE shapes 1.14 - 1.23 x the
// fp4 form's call time and 0.61 - 0.76 of the fp8 form's); the alternatives were not measured,
// and are the first thing to try against that gap (the panel barrier falls every two ring steps).
#ifndef DDLB_SKINNY_NR
#define DDLB_SKINNY_NR 2
#endif
#ifndef DDLB_SKINNY_PANEL
#define DDLB_SKINNY_PANEL 4
#endif
constexpr int kSkinnyNR = DDLB_SKINNY_NR;        // 16-row W tiles per wave (1 or 2)
constexpr int kSkinnyPanel = DDLB_SKINNY_PANEL;  // K-tiles per A panel in LDS = W K-tiles in flight
static_assert(kSkinnyPanel % 2 == 0, "the W4A8 panel is whole W K-tiles");
constexpr int kSkinnyWaves = 4;
constexpr int kSkinnyStrip = 16 * kSkinnyWaves * kSkinnyNR;  // W rows per workgroup
constexpr int kSkinnyMaxSlices = 16;             // the cap of the automatic slice count
static_assert(kSkinnyNR == 1 || kSkinnyNR == 2, "one or two W tiles per wave");

// Operand and scale layouts are GemmArgs' (gemm.h): leading dimensions in ELEMENTS (fp4: two per
// byte), scale rows in BYTES, one E8M0 byte per 32 K elements. din DT_FP8 (K % 128 == 0) or DT_FP4
// (K % 256 == 0); dout bf16 / f16 / f32 (c_scale: DT_FP8 / DT_FP4). Operand rows 16-byte aligned; scale base and row stride
// multiples of 4 (fp4: 8). Any N >= 1; M == 0 launches nothing.
// W4A8 (din DT_FP8, w_dtype DT_FP4): a is e4m3, w E2M1 pairs, K % 256 == 0; each operand keeps
// its own format's rules (lda in bytes = elements and a_scale 4-byte aligned; ldw / w_gstride even
// and w_scale, with its group stride, 8-byte aligned). fp4 a on fp8 w is refused.
struct SkinnyArgs {
  const void* a = nullptr;
  const void* w = nullptr;
  void* c = nullptr;
  const uint8_t* a_scale = nullptr;
  const uint8_t* w_scale = nullptr;
  int64_t lda = 0, ldw = 0, ldc = 0;
  int64_t a_scale_ld = 0, w_scale_ld = 0;
  int M = 0, N = 0, K = 0;  // grouped: M = T, the rows of a the launch may touch
  int act = 0;              // ACT_* (gemm.h), applied to the f32 sum before the one rounding
  // K-slices: 0 = automatic (skinny_auto_slices with the device's CUs), else 1 .. nk. With S > 1
  // ws holds S * M * N floats (skinny_workspace_floats), 16-byte aligned.
  int ksplit = 0;
  float* ws = nullptr;
  // Grouped form (optional): offs is a DEVICE array of ngroups + 1 int32 row offsets, clamped on
  // the device as GemmArgs::grp_offs is; group g multiplies its rows by the weight at
  // w + g * w_gstride ELEMENTS under the scales at w_scale + g * w_scale_gstride BYTES. Rows
  // outside [o'[0], o'[ngroups]) are not written. 1 <= ngroups <= kMaxGroups.
  const int* offs = nullptr;
  int ngroups = 0;
  int64_t w_gstride = 0, w_scale_gstride = 0;
  // Quantised output (optional; dout = DT_FP8 / DT_FP4 and only then), as GemmArgs::c_scale: the
  // epilogue quantises its f32 result by the MX rule (mx_cvt.h) in 32-column blocks of a row and
  // writes c as e4m3 bytes or E2M1 nibble pairs (ldc in ELEMENTS, even) with rows 16-byte
  // aligned, and the blocks' E8M0 bytes here, rows c_scale_ld BYTES apart (base and stride
  // multiples of 4; fp4 data: 8): the next GEMM's a and a_scale. Output columns % 128 == 0
  // (fp4: 256).
  uint8_t* c_scale = nullptr;
  int64_t c_scale_ld = 0;
  // Gated (GLU) epilogue (optional), as GemmArgs::glu: w is the [N, K] weight in the pack_glu
  // layout (rows 64g .. 64g + 31 gate, 64g + 32 .. 64g + 63 the matching up rows), N % 64 == 0,
  // and c has N / 2 columns: c[i, 32g + j] = act(sum[i, 64g + j]) * sum[i, 64g + 32 + j], one f32
  // multiply, then rounded once to dout or quantised (c_scale: [M, N / 64]). ldc >= N / 2. N
  // stays the rows of w: the strips, the slices and the workspace do not change.
  int glu = 0;
  // w's element type: DT_FP8 or DT_FP4; negative = as din.
  int w_dtype = -1;
};
hipError_t gemm_skinny_launch(const SkinnyArgs& p, int din, int dout, hipStream_t s);

// The A16 family (csrc/gemm/gemm_skinny_a16.hip): a is bf16 or f16 (din DT_BF16 / DT_F16), never
// quantised, a_scale null. w_dtype says what w is: DT_FP4 (MXFP4: E2M1 pairs, K % 256 == 0) or
// DT_FP8 (MX-fp8, K % 128 == 0), both under w_scale, expanded to din in registers as
// e * 2^(s - 127); or negative, w of din's own dtype (K % 64 == 0) and w_scale null. A K-tile
// (ksplit) stays 128 bytes of a row of W: 256 / 128 / 64 elements. lda, ldw, w_gstride in ELEMENTS
// as above, rows 16-byte aligned, w_scale 4-byte aligned (fp4: 8). dout is din or DT_F32; no
// quantised output (c_scale null). Strips, slices, the workspace, the grouped form, act and glu are
// as above.
hipError_t gemm_skinny_a16_launch(const SkinnyArgs& p, int din, int dout, hipStream_t s);

// strips of N weight rows (the last one may be ragged)
__host__ __device__ inline int skinny_strips(int N) {
  return (int)(((int64_t)N + kSkinnyStrip - 1) / kSkinnyStrip);
}

// K-tiles (128 bytes of a row of W: 128 fp8 or 256 fp4 elements) of slice s of S: contiguous, in
// order, covering [0, nk) exactly once; nk need not divide by S, and S <= nk leaves none empty
__host__ __device__ inline void skinny_slice(int nk, int S, int s, int& k0, int& k1) {
  k0 = (int)((int64_t)nk * s / S);
  k1 = (int)((int64_t)nk * (s + 1) / S);
}

// the automatic slice count: the smallest S <= min(nk, 16) whose grid has two workgroups per CU
__host__ __device__ inline int skinny_auto_slices(int strips, int nk, int groups, int cus) {
  const int cap = nk < kSkinnyMaxSlices ? nk : kSkinnyMaxSlices;
  for (int S = 1; S < cap; ++S)
    if ((int64_t)strips * S * groups >= 2 * (int64_t)cus) return S;
  return cap;
}

// floats of the workspace of S slices over `rows` rows (M, grouped: T)
__host__ __device__ inline int64_t skinny_workspace_floats(int S, int rows, int N) {
  return S > 1 ? (int64_t)S * rows * N : 0;
}

// Group g's clamped row range [r0, r1) (tile_map.h grouped_clamp: o'[0] = clamp(o[0], 0, T),
// o'[j + 1] = clamp(o[j + 1], o'[j], T), which is the running maximum of the offsets clamped to
// [0, T]); g = -1 gives [o'[0], o'[E]) with E = last. Uniform over a workgroup: scalar loads.
__host__ __device__ inline void skinny_group_rows(const int* offs, int T, int g, int last,
                                                  int& r0, int& r1) {
  const int first = offs[0] < 0 ? 0 : offs[0];
  int run = first;
  const int upto = g < 0 ? last : g;
  for (int j = 1; j <= upto; ++j) run = offs[j] > run ? offs[j] : run;
  r0 = g < 0 ? first : run;
  r1 = g < 0 ? run : (offs[g + 1] > run ? offs[g + 1] : run);
  r0 = r0 < T ? r0 : T;
  r1 = r1 < T ? r1 : T;
}

}  // namespace ddlb
