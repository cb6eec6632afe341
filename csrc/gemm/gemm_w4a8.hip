// Tiled W4A8 GEMM: the host entry with every refusal, and the dense ungrouped instantiations.
// The kernel: gemm_w4a8_kernels.h. It is not reached through gemm_launch.
#include "gemm_w4a8_kernels.h"

namespace ddlb {

hipError_t gemm_w4a8_launch(const GemmArgs& p, int dout, int tile, hipStream_t s) {
  const hipError_t bad = hipErrorInvalidValue;
  const bool qout = dout == DT_FP8;
  if (dout != DT_BF16 && dout != DT_F16 && dout != DT_F32 && !qout) return bad;
  if (p.M < 0 || p.N < 1 || p.K < 256 || p.K % 256) return bad;
  if (p.act < ACT_NONE || p.act > ACT_SILU) return bad;
  if (!p.a || !p.b || !p.c || !p.a_scale || !p.b_scale) return bad;
  // plain rows only: no row groups, row tables, arrival flags, shard order, in-kernel gather,
  // K-split or K-grouped form
  if ((p.a_grp != 0 && p.a_grp != p.M) || (p.c_grp != 0 && p.c_grp != p.M) || p.a_table ||
      p.c_table || p.flags || p.tile_order || p.ag_ctas || p.ksplit > 1 || p.kgrouped)
    return bad;
  const bool grouped = p.grp_offs != nullptr || p.ngroups != 0;
  if (grouped && (!p.grp_offs || p.ngroups < 1 || p.ngroups > kMaxGroups)) return bad;
  // the operands: K elements within a row, W's pitches even (whole bytes), rows 16-byte aligned
  if (p.lda < p.K || p.ldb < p.K || ((p.ldb | p.b_gstride) & 1)) return bad;
  if (((uintptr_t)p.a | (uintptr_t)p.b | (uint64_t)p.lda | (uint64_t)(p.ldb / 2)) & 15) return bad;
  if (grouped && ((p.b_gstride / 2) % 16 || p.b_scale_gstride % 4 ||
                  (p.ngroups > 1 && (p.b_gstride < (int64_t)(p.N - 1) * p.ldb + p.K ||
                                     p.b_scale_gstride < (int64_t)(p.N - 1) * p.b_scale_ld +
                                                             p.K / 32))))
    return bad;
  // the scales: one aligned 32-bit word per row and K-tile, rows addressed by 32-bit byte offsets
  // (sa_off / sw_off; grouped: from the group's base, at most M rows)
  if ((((uintptr_t)p.a_scale | (uintptr_t)p.b_scale | (uint64_t)p.a_scale_ld |
        (uint64_t)p.b_scale_ld) & 3) || p.a_scale_ld < p.K / 32 || p.b_scale_ld < p.K / 32 ||
      (int64_t)p.M * p.a_scale_ld >= (int64_t(1) << 31) ||
      (int64_t)p.N * p.b_scale_ld >= (int64_t(1) << 31))
    return bad;
  // the output: N columns, gated N / 2 from whole 64-row gate / up groups; quantised with its
  // scales and only then, in whole blocks as the next GEMM takes them per K-tile
  const int64_t cols = p.glu ? p.N / 2 : p.N;
  if ((p.glu && p.N % 64) || qout != (p.c_scale != nullptr) || p.ldc < cols) return bad;
  if (qout) {
    if (cols % 128 || (((uintptr_t)p.c | (uint64_t)p.ldc) & 15) ||
        (((uintptr_t)p.c_scale | (uint64_t)p.c_scale_ld) & 3) || p.c_scale_ld < cols / 32 ||
        (int64_t)p.M * p.c_scale_ld >= (int64_t(1) << 31))
      return bad;
  } else if ((uintptr_t)p.c & (dtype_size(dout) - 1)) {
    return bad;  // (any row pitch: rows that are not 8-byte aligned are stored one column at a time)
  }
  if (tile == TILE_AUTO) tile = w4a8_auto_tile(p.M, p.N, grouped, p.glu || qout, num_cus());
  if (!w4a8_offers(tile)) return bad;
  // the grid (grouped: its bound) is a 32-bit block count
  const int64_t tiles_n = (p.N + 127) / 128, bm = tile_rows_of(tile);
  const int64_t grid = grouped ? grouped_grid_bound(p.M, p.ngroups, (int)bm, (int)tiles_n)
                               : (p.M + bm - 1) / bm * tiles_n;
  if (grid >= (int64_t(1) << 31)) return bad;
  if (p.M == 0) return hipSuccess;
  if (qout) return launch_w4a8_q(p, tile, s);
  if (grouped) return launch_w4a8_grouped(p, dout, tile, s);
  return dispatch_out(dout, [&](auto o) {
    return launch_w4a8_t<decltype(o)::value, false>(p, tile, s);
  });
}

}  // namespace ddlb
