// The K-grouped form of the tiled kernel (GemmArgs::kgrouped): its prologue and its launch
// template, included by the gemm_kgrouped_*.hip translation units only.
//
// The kernel is gemm_tn_kernel itself (gemm_kernels.h) with GRP = TILE_GROUPED_K: kgrouped_args
// below runs in front of its body. Where the M-grouped prologue (gemm_grouped_kernels.h) re-bases
// the ROWS of a and c to a group, this one re-bases the COLUMNS of both operands and of both scale
// arrays to the group's range of the padded contraction axis (tile_map.h kgrouped_range) and the
// output to the group's own [M, N] matrix.
#pragma once
#include "gemm_kernels.h"

namespace ddlb {
namespace {

// One workgroup per (group, m-tile, n-tile): the grid is E * tiles_m * tiles_n, known on the
// host, groups slowest. pl arrives as the byte view of launch_tiled_kgrouped (fp4: K, lda, ldb in
// bytes). The prologue finds the group's columns [k0, k0 + kl) by a scalar scan of the offsets
// and re-bases a, b by k0 elements (fp4: k0 / 2 bytes), a_scale, b_scale by k0 / 32 bytes (a
// multiple of 4, fp4: of 8, as k0 is one of MOD: the body's aligned scale words stay aligned),
// c by g * c_kgstride elements, and sets K to kl (fp4: kl / 2 bytes): 64-bit pointer arithmetic
// on workgroup-uniform values. The body issues its first stage unconditionally, so a group
// without columns never enters it: its tile of c[g] is filled with +0.0 here, by guarded plain
// stores before any barrier, and the workgroup returns.
template <class Mma, int OUT, int BM, int BN, int NT>
__device__ __forceinline__ bool kgrouped_args(const GemmArgs& pl, GemmArgs& pg, int& wg) {
  constexpr bool in4 = is_fp4<Mma>::value;
  constexpr int MOD = in4 ? 256 : 128;  // the K-tile in elements
  constexpr int64_t CSZ = out_size<OUT>();
  const int tiles_n = (pl.N + BN - 1) / BN, tiles_m = (pl.M + BM - 1) / BM;
  const int per = tiles_m * tiles_n;
  const int g = (int)blockIdx.x / per;
  wg = xcd_remap((int)blockIdx.x - g * per, per);
  int64_t k0, kl;
  kgrouped_range(pl.grp_offs, pl.kgrp_rows, pl.ngroups, MOD, g, k0, kl);
  char* cg = (char*)pl.c + (int64_t)g * pl.c_kgstride * CSZ;
  if (kl == 0) {
    const int r0 = wg / tiles_n * BM, c0 = wg % tiles_n * BN;
    for (int i = (int)threadIdx.x; i < BM * BN; i += NT) {
      const int r = r0 + i / BN, c = c0 + i % BN;
      if (r < pl.M && c < pl.N) Store4<OUT>::st1(cg + ((int64_t)r * pl.ldc + c) * CSZ, 0.f);
    }
    return false;
  }
  pg = pl;
  pg.a = (const char*)pl.a + (in4 ? k0 / 2 : k0);
  pg.b = (const char*)pl.b + (in4 ? k0 / 2 : k0);
  pg.a_scale = pl.a_scale + k0 / 32;
  pg.b_scale = pl.b_scale + k0 / 32;
  pg.c = cg;
  pg.K = (int)(in4 ? kl / 2 : kl);
  return true;
}

// launch_tiled_grouped's sibling, the one launch site of the K-grouped form: the codes of
// mxs_offers(), anything else hipErrorInvalidValue; gemm_launch has checked that the grid is one.
template <class Mma, int OUT>
hipError_t launch_tiled_kgrouped(const GemmArgs& p_in, int tile, hipStream_t s) {
  static_assert(is_scaled<Mma>::value, "K-grouped: block-scaled fp8 / fp4 operands");
  const GemmArgs p = fp4_byte_view(p_in, is_fp4<Mma>::value, false);
  return dispatch_int<kNumTileCfgs>(tile_slot(tile), [&](auto slot) {
    constexpr TileCfg c = kTileCfgs[decltype(slot)::value];
    if constexpr (!mxs_offers(c.code)) {
      return hipErrorInvalidValue;
    } else {
      static_assert(!c.ilv && c.cols / c.wn == 64, "K-grouped: 64 columns per wave, no interleave");
      const int64_t tiles = (int64_t)((p.M + c.rows - 1) / c.rows) * ((p.N + c.cols - 1) / c.cols);
      const dim3 grid((unsigned)(tiles * p.ngroups));
      const dim3 block(c.wm * c.wn * 64);
      hipLaunchKernelGGL((gemm_tn_kernel<Mma, OUT, c.rows, c.cols, c.wm, c.wn, false, false,
                                         TILE_GROUPED_K>), grid, block, 0, s, p);
      return hipGetLastError();
    }
  });
}

template <class Mma>
hipError_t launch_kgrouped_t(const GemmArgs& p, int dout, int tile, hipStream_t s) {
  if (dout == DT_F32) return launch_tiled_kgrouped<Mma, DT_F32>(p, tile, s);
  if (dout == DT_BF16) return launch_tiled_kgrouped<Mma, DT_BF16>(p, tile, s);
  if (dout == DT_F16) return launch_tiled_kgrouped<Mma, DT_F16>(p, tile, s);
  return hipErrorInvalidValue;
}

}  // namespace
}  // namespace ddlb
