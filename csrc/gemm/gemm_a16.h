// Tiled A16 GEMM for prefill (csrc/gemm/gemm_a16_kernels.h): C[M, N] = A[M, K] W[N, K]^T with A
// bf16 or f16, not quantised, and W MXFP4 (W4A16) or MX-fp8 (W8A16) under E8M0 block scales. W
// travels packed into LDS and is expanded to A's dtype in registers, between LDS and
// v_mfma_f32_16x16x32_{bf16,f16}. The compute-bound sibling of the skinny A16 kernel
// (gemm_skinny.h), for M in the hundreds and up; a kernel of its own, not a flavour of
// gemm_tn_kernel or of the W4A8 kernel, which feed one MFMA from two operands as stored.
#pragma once
#include <hip/hip_runtime.h>

#include "gemm.h"

namespace ddlb {

// Tile codes the kernel is built for, the W4A8 kernel's geometry: 128x128 on 4 waves and 256x128
// on 8, every wave a 64x64 block (MR = NR = 4). Two LDS stages of BM * 256 + BN * 64 (fp4) or
// BN * 128 (fp8) bytes: 80 / 96 KiB at 128x128, 144 / 160 KiB at 256x128, the last one the whole
// of a CU's 160 KiB. No instantiation spills (the table: gemm_a16_kernels.h).
constexpr bool a16_offers(int tile) { return tile == TILE_128x128 || tile == TILE_256x128; }

// `auto`, from docs/RESULTS.md "A16 prefill" (one MI355X; call time at 128x128 over call time at
// 256x128). MXFP4: 128x128 everywhere, two workgroups per CU: 0.92 - 0.97 dense and gated at
// M >= 2048, 0.66 - 0.72 at M = 512, 0.74 - 0.87 grouped at the E = 32 MoE shapes. MX-fp8: its
// 128x128 form is held to one wave per SIMD by its LDS, so 256x128 wherever that has at least one
// tile per CU (1.21 - 1.34 dense and gated at M >= 2048, 1.03 - 1.30 grouped) and 128x128 below
// (M = 512: 0.66 - 0.77). Grouped: the tiles of all M rows, which bounds the groups' tiles.
inline int a16_auto_tile(int64_t M, int64_t N, bool fp4, int cus) {
  const int64_t tiles = (M + 255) / 256 * ((N + 127) / 128);
  return !fp4 && tiles >= cus ? TILE_256x128 : TILE_128x128;
}

// GemmArgs as gemm_launch takes them. din: a's dtype, DT_BF16 or DT_F16 (lda in ELEMENTS). dw:
// DT_FP4 (b E2M1 pairs, ldb / b_gstride in fp4 ELEMENTS, even; K % 256 == 0) or DT_FP8 (b e4m3,
// K % 128 == 0); 16-bit weights are gemm_launch's and refused here. Operand rows 16-byte aligned;
// b_scale [N, K / 32] E8M0 bytes, base, row stride (and b_scale_gstride) multiples of 4,
// N * stride < 2^31; a_scale and c_scale null (no quantised input or output). dout din or DT_F32,
// any row pitch (8-byte-aligned C rows get four-column stores). act, glu (N % 64 == 0, N / 2
// output columns) and the grouped form (grp_offs / ngroups / b_gstride / b_scale_gstride) are
// GemmArgs'. Plain rows only: row tables, row groups, flags, shards, ksplit and kgrouped are
// refused. tile: TILE_AUTO or a code of a16_offers(). Every refusal is hipErrorInvalidValue,
// nothing launched.
hipError_t gemm_a16_launch(const GemmArgs& p, int din, int dout, int dw, int tile, hipStream_t s);

// The translation units behind it (the dense form lives beside gemm_a16_launch). p: the byte view.
hipError_t launch_a16_grouped(const GemmArgs& p, int din, int dout, int dw, int tile,
                              hipStream_t s);

}  // namespace ddlb
