// Tiled A16 GEMM: the host entry with every refusal, and the dense ungrouped instantiations.
// The kernel: gemm_a16_kernels.h. It is not reached through gemm_launch.
#include "gemm_a16_kernels.h"

namespace ddlb {

hipError_t gemm_a16_launch(const GemmArgs& p_in, int din, int dout, int dw, int tile,
                           hipStream_t s) {
  const hipError_t bad = hipErrorInvalidValue;
  // a bf16 / f16, w MXFP4 / MX-fp8 (16-bit weights: gemm_launch), the output a's dtype or f32
  if (din != DT_BF16 && din != DT_F16) return bad;
  if (dw != DT_FP4 && dw != DT_FP8) return bad;
  if (dout != din && dout != DT_F32) return bad;
  const bool fp4 = dw == DT_FP4;
  const int kmod = fp4 ? 256 : 128;
  GemmArgs p = p_in;
  if (p.M < 0 || p.N < 1 || p.K < kmod || p.K % kmod) return bad;
  if (p.act < ACT_NONE || p.act > ACT_SILU) return bad;
  if (!p.a || !p.b || !p.c || !p.b_scale || p.a_scale || p.c_scale) return bad;
  // plain rows only: no row groups, row tables, arrival flags, shard order, in-kernel gather,
  // K-split or K-grouped form
  if ((p.a_grp != 0 && p.a_grp != p.M) || (p.c_grp != 0 && p.c_grp != p.M) || p.a_table ||
      p.c_table || p.flags || p.tile_order || p.ag_ctas || p.ksplit > 1 || p.kgrouped)
    return bad;
  const bool grouped = p.grp_offs != nullptr || p.ngroups != 0;
  if (grouped && (!p.grp_offs || p.ngroups < 1 || p.ngroups > kMaxGroups)) return bad;
  if (!grouped) p.b_gstride = p.b_scale_gstride = 0;
  // the operands: K elements within a row, fp4 pitches even (whole bytes); then the byte view,
  // rows 16-byte aligned
  if (p.lda < p.K || p.ldb < p.K || (fp4 && ((p.ldb | p.b_gstride) & 1))) return bad;
  const int64_t kw = fp4 ? p.K / 2 : p.K;  // bytes of a row of W
  p.lda *= 2;
  if (fp4) {
    p.ldb /= 2;
    p.b_gstride /= 2;
  }
  if (((uintptr_t)p.a | (uintptr_t)p.b | (uint64_t)p.lda | (uint64_t)p.ldb |
       (uint64_t)p.b_gstride) & 15)
    return bad;
  if (grouped && (p.b_scale_gstride % 4 ||
                  (p.ngroups > 1 && (p.b_gstride < (int64_t)(p.N - 1) * p.ldb + kw ||
                                     p.b_scale_gstride < (int64_t)(p.N - 1) * p.b_scale_ld +
                                                             p.K / 32))))
    return bad;
  // the scales: one aligned 32-bit word per row and K-tile, rows addressed by 32-bit byte offsets
  // (sw_off; grouped: from the group's base)
  if ((((uintptr_t)p.b_scale | (uint64_t)p.b_scale_ld) & 3) || p.b_scale_ld < p.K / 32 ||
      (int64_t)p.N * p.b_scale_ld >= (int64_t(1) << 31))
    return bad;
  // the output: N columns, gated N / 2 from whole 64-row gate / up groups, on any row pitch
  // (rows that are not 8-byte aligned are stored one column at a time)
  const int64_t cols = p.glu ? p.N / 2 : p.N;
  if ((p.glu && p.N % 64) || p.ldc < cols || ((uintptr_t)p.c & (dtype_size(dout) - 1)))
    return bad;
  if (tile == TILE_AUTO) tile = a16_auto_tile(p.M, p.N, fp4, num_cus());
  if (!a16_offers(tile)) return bad;
  // the grid (grouped: its bound) is a 32-bit block count
  const int64_t tiles_n = (p.N + 127) / 128, bm = tile_rows_of(tile);
  const int64_t grid = grouped ? grouped_grid_bound(p.M, p.ngroups, (int)bm, (int)tiles_n)
                               : (p.M + bm - 1) / bm * tiles_n;
  if (grid >= (int64_t(1) << 31)) return bad;
  if (p.M == 0) return hipSuccess;
  if (grouped) return launch_a16_grouped(p, din, dout, dw, tile, s);
  return launch_a16_forms<false>(p, din, dout, dw, tile, s);
}

}  // namespace ddlb
