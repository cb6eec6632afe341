// The M-grouped form of the tiled kernel (GemmArgs::grp_offs): its prologue and its launch
// template, included by the gemm_grouped_*.hip translation units only.
//
// The kernel is gemm_tn_kernel itself (gemm_kernels.h) with GRP = TILE_GROUPED_M: grouped_args
// below runs in front of its body, which then works on one tile of one group. The ungrouped
// instantiations do not see it (docs/ARCHITECTURE.md "One kernel template, three prologues").
#pragma once
#include "gemm_kernels.h"

namespace ddlb {
namespace {

// One workgroup per entry of the grid bound (grouped_grid_bound, tile_map.h). A workgroup finds
// its (group, m-tile, n-tile) by a scalar scan of the offsets, or finds none (false: the kernel
// returns before any barrier or LDS-DMA). pg is the launch's arguments re-based to the group:
// a, c and the scales of both at the group's first row, b and its scales at the group's weight,
// M the group's row count. The body's row loads clamp to M - 1 and its stores are guarded by M,
// so a tile never touches another group's rows. Every re-basing is 64-bit pointer arithmetic on
// workgroup-uniform values; the body's 32-bit scale offsets stay within one group. pl arrives as
// the byte view of launch_tiled_grouped (fp4: K, lda, ldb, b_gstride and / or ldc in bytes; a
// quantised output's ldc in bytes).
template <class Mma, int OUT, int BM, int BN>
__device__ __forceinline__ bool grouped_args(const GemmArgs& pl, GemmArgs& pg, int& wg) {
  const int tiles_n = (pl.N + BN - 1) / BN;
  GroupTile t;
  if (!grouped_tile(pl.grp_offs, pl.M, pl.ngroups, BM, tiles_n,
                    xcd_remap((int)blockIdx.x, (int)gridDim.x), t))
    return false;
  constexpr bool QOUT = OUT == DT_FP8 || OUT == DT_FP4;
  constexpr int64_t CSZ = QOUT ? 1 : out_size<OUT>();
  pg = pl;
  pg.a = (const char*)pl.a + (int64_t)t.row0 * pl.lda * Mma::kElem;
  pg.b = (const char*)pl.b + (int64_t)t.g * pl.b_gstride * Mma::kElem;
  pg.c = (char*)pl.c + (int64_t)t.row0 * pl.ldc * CSZ;
  if constexpr (is_scaled<Mma>::value) {
    pg.a_scale = pl.a_scale + (int64_t)t.row0 * pl.a_scale_ld;
    pg.b_scale = pl.b_scale + (int64_t)t.g * pl.b_scale_gstride;
  }
  if constexpr (QOUT) pg.c_scale = pl.c_scale + (int64_t)t.row0 * pl.c_scale_ld;
  pg.M = t.rows;
  pg.a_grp = pg.a_gstride = pg.c_grp = pg.c_gstride = t.rows;  // plain rows within the group
  wg = t.tm * tiles_n + t.tn;
  return true;
}

// launch_tiled's sibling for the M-grouped form, its one launch site (gated or not): the codes of
// mxs_offers() (NR = 4, no DMA interleave), anything else hipErrorInvalidValue; the byte view of
// fp4 operands / an fp4 output is formed here as launch_tiled forms it; the grid is the bound of
// tile_map.h, which gemm_launch has checked to be a grid.
template <class Mma, int OUT>
hipError_t launch_tiled_grouped(const GemmArgs& p_in, int tile, hipStream_t s) {
  constexpr bool in4 = is_fp4<Mma>::value, out4 = OUT == DT_FP4;
  static_assert(has_glu<Mma>::value, "grouped: bf16, f16, block-scaled fp8 / fp4 operands");
  const GemmArgs p = fp4_byte_view(p_in, in4, out4);
  return dispatch_int<kNumTileCfgs>(tile_slot(tile), [&](auto slot) {
    constexpr TileCfg c = kTileCfgs[decltype(slot)::value];
    if constexpr (!mxs_offers(c.code)) {
      return hipErrorInvalidValue;
    } else {
      static_assert(!c.ilv && c.cols / c.wn == 64, "grouped: 64 columns per wave, no interleave");
      const dim3 grid((unsigned)grouped_grid_bound(p.M, p.ngroups, c.rows,
                                                   (p.N + c.cols - 1) / c.cols));
      const dim3 block(c.wm * c.wn * 64);
      if (p.glu)
        hipLaunchKernelGGL((gemm_tn_kernel<Mma, OUT, c.rows, c.cols, c.wm, c.wn, false, true,
                                           TILE_GROUPED_M>), grid, block, 0, s, p);
      else
        hipLaunchKernelGGL((gemm_tn_kernel<Mma, OUT, c.rows, c.cols, c.wm, c.wn, false, false,
                                           TILE_GROUPED_M>), grid, block, 0, s, p);
      return hipGetLastError();
    }
  });
}

// One translation unit per operand flavour and output kind: IN is the operands' dtype code (the
// dense output a 16-bit flavour pairs with), QOUT the quantised outputs instead of the dense
// ones. gemm_launch has checked everything else.
template <class Mma, int IN, bool QOUT>
hipError_t launch_grouped_t(const GemmArgs& p, int dout, int tile, hipStream_t s) {
  if constexpr (QOUT) {
    if (dout == DT_FP8) return launch_tiled_grouped<Mma, DT_FP8>(p, tile, s);
    if (dout == DT_FP4) return launch_tiled_grouped<Mma, DT_FP4>(p, tile, s);
  } else {
    if (dout == DT_F32) return launch_tiled_grouped<Mma, DT_F32>(p, tile, s);
    if constexpr (is_scaled<Mma>::value) {
      if (dout == DT_BF16) return launch_tiled_grouped<Mma, DT_BF16>(p, tile, s);
      if (dout == DT_F16) return launch_tiled_grouped<Mma, DT_F16>(p, tile, s);
    } else {
      if (dout == IN) return launch_tiled_grouped<Mma, IN>(p, tile, s);
    }
  }
  return hipErrorInvalidValue;
}

}  // namespace
}  // namespace ddlb
