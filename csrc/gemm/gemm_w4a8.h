// Tiled W4A8 GEMM for prefill (csrc/gemm/gemm_w4a8_kernels.h): C[M, N] = A[M, K] W[N, K]^T with
// A MX-fp8 (e4m3) and W MXFP4 (E2M1 pairs), both under E8M0 block scales, one mixed-format scaled
// MFMA per 16x16 fragment pair and 128 K elements. The compute-bound sibling of the skinny kernel's
// W4A8 form (gemm_skinny.h), for M in the hundreds and up; a kernel of its own, not a flavour of
// gemm_tn_kernel, which keeps one format for both operands.
#pragma once
#include <hip/hip_runtime.h>

#include "gemm.h"

namespace ddlb {

// LDS stages of the K loop: 2 (one K-tile of DMA lead, the tiled kernel's loop) or 3 (two K-tiles
// of lead, counted vmcnt waits). A stage is BM * 128 + BN * 64 bytes: 40 KiB at 256x128, 24 KiB at
// 128x128. Three, by measurement (docs/RESULTS.md "W4A8 prefill": 0.83 - 0.91 of the two-stage
// call time at 256x128, 0.89 - 0.97 at 128x128 and 0.74 - 0.77 there at M = 512). The
// third stage costs no residency: registers hold both tiles to two waves per SIMD (one 8-wave
// or two 4-wave workgroups per CU), and 120 KiB once / 72 KiB twice fit the CU's 160 KiB.
#ifndef DDLB_W4A8_STAGES
#define DDLB_W4A8_STAGES 3
#endif
constexpr int kW4A8Stages = DDLB_W4A8_STAGES;
static_assert(kW4A8Stages == 2 || kW4A8Stages == 3, "two or three LDS stages");

// Tile codes the kernel is built for: 256x128 on 8 waves and 128x128 on 4, every wave a 64x64
// block (MR = NR = 4), so a 32-column MX block and a 64-column gate / up group stay in one wave.
// No instantiation of either spills (docs/ARCHITECTURE.md "W4A8 prefill kernel").
constexpr bool w4a8_offers(int tile) { return tile == TILE_256x128 || tile == TILE_128x128; }

// `auto`, from docs/RESULTS.md "W4A8 prefill" (three stages, one MI355X): 128x128 for the grouped
// form (0.78 - 0.93 of the 256x128 time at the E = 32 MoE shapes), for the gated quantised fc1
// (0.96 - 0.99; `fused`: glu or a quantised output, measured together only) and wherever 256x128
// has fewer tiles than the device CUs (M = 512: 0.54 - 0.58); 256x128 for a plain dense output
// on a grid of at least one tile per CU, where it leads by 0.7 - 1.2 % at 512 tiles and more and
// ties at 256.
inline int w4a8_auto_tile(int64_t M, int64_t N, bool grouped, bool fused, int cus) {
  const int64_t tiles = (M + 255) / 256 * ((N + 127) / 128);
  return !grouped && !fused && tiles >= cus ? TILE_256x128 : TILE_128x128;
}

// GemmArgs as gemm_launch takes them, with a e4m3 (lda in fp8 ELEMENTS = bytes) and b E2M1 pairs
// (ldb / b_gstride in fp4 ELEMENTS, even; the byte view is formed inside). K % 256 == 0; operand
// rows 16-byte aligned; a_scale / b_scale [rows, K / 32] E8M0 bytes, base, row stride (and
// b_scale_gstride) multiples of 4, rows * stride < 2^31. dout bf16 / f16 / f32 (any row pitch;
// 8-byte-aligned C rows get four-column stores), or DT_FP8 with c_scale and only then (MX-fp8 data, rows 16-byte aligned, and E8M0
// scales per 32 output columns; output columns % 128 == 0). act, glu (N % 64 == 0, N / 2 output
// columns) and the grouped form (grp_offs / ngroups / b_gstride / b_scale_gstride) are GemmArgs'.
// Plain rows only: row tables, row groups, flags, shards, ksplit and kgrouped are refused. tile:
// TILE_AUTO or a code of w4a8_offers(). Every refusal is hipErrorInvalidValue, nothing launched.
hipError_t gemm_w4a8_launch(const GemmArgs& p, int dout, int tile, hipStream_t s);

// The translation units behind it (dense ungrouped outputs live beside gemm_w4a8_launch).
hipError_t launch_w4a8_q(const GemmArgs& p, int tile, hipStream_t s);
hipError_t launch_w4a8_grouped(const GemmArgs& p, int dout, int tile, hipStream_t s);

}  // namespace ddlb
