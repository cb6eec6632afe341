// The grouped form of the tiled kernel (GemmArgs::grp_offs) and its launch template, included by
// the gemm_grouped_*.hip translation units only.
//
// gemm_tn_grouped_kernel runs the body of gemm_tn_kernel (gemm_kernels.h), the SAME TEXT, on one
// tile of one group. gemm_kernels.h is not edited for it: the build (ddlb_amd/_build.py,
// grouped_body()) copies the body of gemm_tn_kernel, from the line behind its signature to its
// closing brace, into gemm_tn_grouped_body.gen.h and replaces exactly one line of it, the choice
// of the tile (`const int wg = tile_index(p, nwg);` becomes `const int wg = wg_group;`); a body
// that no longer holds that line exactly once fails the build. That file is included below,
// between this kernel's prologue and its closing brace. So the ungrouped instantiations are
// compiled from the text they always were, with no run-time branch and no template argument
// added, and their registers are the parent's (docs/ARCHITECTURE.md "Grouped GEMM").
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

template <class Mma, int OUT, int BM, int BN, int WM, int WN, bool GLU = false>
__global__ __launch_bounds__(WM* WN * 64) void gemm_tn_grouped_kernel(const GemmArgs p_launch) {
  constexpr bool ILV = false;  // the codes of mxs_offers(): never interleaved
  GemmArgs p_group;
  int wg_group;
  if (!grouped_args<Mma, OUT, BM, BN>(p_launch, p_group, wg_group)) return;
  const GemmArgs& p = p_group;
#include "gemm_tn_grouped_body.gen.h"
}

// launch_tiled's sibling for the grouped kernel, its one launch site (gated or not): the codes of
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
        hipLaunchKernelGGL((gemm_tn_grouped_kernel<Mma, OUT, c.rows, c.cols, c.wm, c.wn, true>),
                           grid, block, 0, s, p);
      else
        hipLaunchKernelGGL((gemm_tn_grouped_kernel<Mma, OUT, c.rows, c.cols, c.wm, c.wn>), grid,
                           block, 0, s, p);
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
