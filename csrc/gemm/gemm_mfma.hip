// CDNA4 (gfx950) MFMA GEMM:  C[M,N] = A[M,K] * Bt[N,K]^T  ("TN": both operands K-contiguous).
//
// Replaces the cuBLAS GEMM the reference reaches through torch.matmul
// (ddlb/primitives/TPColumnwise/pytorch.py:97, TPRowwise/pytorch.py:82, compute_only.py:40).
//
// Design (see /opt/skills/guides/cdna_hip_programming.md §5):
//  * Operands staged global->LDS with LDS-DMA (`global_load_lds_dwordx4`, 16 B/lane, 1 KiB per
//    wave-instruction), double-buffered, one barrier per K-tile (the "minimum 2-phase" schedule).
//  * Every K-tile row is 128 bytes (BK = 64 for 16-bit types, 128 for fp8, 32 for fp32), so one
//    LDS layout serves every dtype. 16-byte chunks are XOR-swizzled with (row>>1)&7; because the
//    LDS-DMA destination is lane-linear, the swizzle is applied to the per-lane SOURCE address and
//    undone on the ds_read_b128 (rule 21). Conflict-free for the 16x16 fragment reads.
//  * MFMA 16x16x32 (bf16/f16), 2x 16x16x32 fp8 per 16 B, 4x 16x16x4 f32 per 16 B, or the
//    block-scaled 16x16x128 f8f6f4 (MX-fp8) that runs at 2x the bf16 rate: with unit scales, or
//    with real per-block E8M0 scales (GemmArgs::a_scale / b_scale, the tiled kernel's MmaMXS
//    flavour, gemm_mxs.hip; quantiser: mx_quant.hip). With E2M1 operands (MXFP4, MmaMX4S,
//    gemm_mx4.hip) the same instruction takes 16 bytes = 32 elements per lane, two per K-row,
//    at twice the MX-fp8 rate; there a lane group's 16 bytes are one block under its own scale.
//    Any k-permutation that is identical for A and B leaves the dot product unchanged, which is
//    what lets one 16-byte ds_read feed every instruction shape. For the 16x16x128 instruction
//    the order used (a lane's chunks fq and 4 + fq of the 128-byte K-row) is also the
//    instruction's own K order, so its 32-element scale blocks are the format's blocks; the
//    scale of block kb is supplied by lane group kb (measured; docs/ARCHITECTURE.md).
//  * Operands are swapped in the MFMA (D = Bt_frag x A_frag) so each lane ends with 4 consecutive
//    COLUMNS of one C row: the epilogue is one 8-byte (bf16) / 16-byte (f32) store per fragment.
//  * Grouped-row addressing for A and C: logical row i lives at physical row
//        base + (i / grp) * gstride + (i % grp)
//    so pipeline stages read strided row blocks of A and write straight to their final rows of C
//    (no permutation copy).
//  * Bijective XCD-aware block remap (8 XCDs, private L2s): blocks that share an A panel land on
//    the same XCD.
//  * Optional arrival flags: a tile whose A rows belong to shard s spins (bounded) until
//    flags[s] >= epoch before loading A, so one persistent-size GEMM launch can consume shards as
//    the copy engines deliver them (p2p pipeline).
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <stdint.h>


#include "gemm.h"
#include "gemm_entry.h"
#include "tile_map.h"

namespace ddlb {

int tile_rows(int tile) { return tile_rows_of(tile); }
int tile_cols(int tile) { return tile_cols_of(tile); }

bool gemm_fast_path_ok(const GemmArgs& p, int din, int dout) {
  const int esz = dtype_size(din);
  if (din == DT_F64 || (din == DT_FP8 && dout == DT_FP8)) return false;
  if (p.M <= 0 || p.N <= 0 || p.K <= 0) return false;
  if ((int64_t)p.K * esz % 128 != 0) return false;
  if (p.lda * esz % 16 || p.ldb * esz % 16) return false;
  if (((uintptr_t)p.a | (uintptr_t)p.b) & 15) return false;
  if ((p.ldc * dtype_size(dout)) % 8 || ((uintptr_t)p.c & 7)) return false;
  if (p.a_grp <= 0 || p.c_grp <= 0) return false;
  return true;
}

int choose_tile(int64_t M, int64_t N, int64_t K, int din) {
  // Measured on MI355X: among the ping-pong kernels, pt4 (t4 made persistent) leads t4 / t8 / pt8
  // on every shape and dtype measured once the C stores are non-temporal
  // (profiles/r01/s2/s2_41_tune_nt.txt: bf16 flagship 108.9 vs t4 121.1 us, 16384x8192x1024
  // 231.7 vs 251.9, 8192^3 695.7 vs 703.4; s2_44_fp8_tiles.txt: MX-fp8 flagship 63.6 vs pt8
  // 67.4 us, 8192^3 363 vs t8 380) whenever the grid covers most of the CUs; it falls back to t4
  // where it does not apply (a single K-tile, an odd K-tile count, activations). Long K with
  // fewer whole tiles prefers the 128-byte-row interleaved kernel; fewer tiles than CUs want
  // 128x128 blocks. (The LDS-ring, 256x256 ping-pong and persistent streaming families this
  // table once chose between were retired in round 4: pt4 had superseded them on every shape.)
  auto tiles = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((N + bn - 1) / bn); };
  (void)K;
  (void)din;
  // (down to half the CUs' worth of 256x256 tiles: at 128 tiles pt4 still beats the 128x128
  // kernel, 8192x1024x1024 bf16 22.5 vs 23.0 us, MX-fp8 14.8 vs 16.4, profiles/r04/r4_24_*)
  const bool whole = M % 256 == 0 && N % 256 == 0 && tiles(256, 256) >= 128;
  if (whole) return TILE_PT4;
  if (tiles(256, 256) >= 384) return TILE_I256;
  if (tiles(256, 128) >= 384) return TILE_256x128;
  if (tiles(128, 256) >= 384) return TILE_128x256;
  return TILE_128x128;
}

// Block-scale operands as every scaled flavour of the tiled kernel reads them: both present, base
// and row stride multiples of `align` (the scales of a row's K-tile are one aligned 32-bit load,
// align 4; 64-bit for fp4 data, align 8), a row's K / 32 bytes within its stride, rows addressed
// by 32-bit byte offsets.
static bool scale_operands_ok(const GemmArgs& p, int align) {
  return p.a_scale != nullptr && p.b_scale != nullptr &&
         (((uintptr_t)p.a_scale | (uintptr_t)p.b_scale) & (align - 1)) == 0 &&
         p.a_scale_ld % align == 0 && p.b_scale_ld % align == 0 && p.a_scale_ld >= p.K / 32 &&
         p.b_scale_ld >= p.K / 32 && (int64_t)p.M * p.a_scale_ld < (int64_t(1) << 31) &&
         (int64_t)p.N * p.b_scale_ld < (int64_t(1) << 31);
}

// The block-scaled and quantising flavours address plain operands only: no K-split, A row table,
// grouped A rows, arrival flags or in-kernel all-gather. `refusal` is the caller's code for it.
// What differs between the callers (a_grp / c_grp already defaulted by gemm_launch):
//  * plain_c_rows: grouped C rows are refused too (the quantising epilogue writes plain rows);
//  * plain_c_order: a C row table and a tile order are refused too (fp4 operands and quantised
//    output; fp8 operands with scales take both, as the tiled kernel does with unit scales).
static hipError_t plain_operands_only(const GemmArgs& p, bool plain_c_rows, bool plain_c_order,
                                      hipError_t refusal) {
  const int64_t rows = p.M > 0 ? p.M : 1;
  if (p.ksplit > 1 || p.a_table != nullptr || p.a_grp != rows || p.flags != nullptr ||
      p.ag_ctas > 0 || p.ag_mode != 0)
    return refusal;
  if (plain_c_rows && p.c_grp != rows) return refusal;
  if (plain_c_order && (p.c_table != nullptr || p.tile_order != 0)) return refusal;
  return hipSuccess;
}

// Grouped launches (GemmArgs::grp_offs): what a grouped launch adds to the checks of the flavour it
// runs (the functions below, with M = T, the rows the launch may touch). The offsets are device
// memory and are never read here. Plain rows in the launch's own order only, the tiled kernel's
// offered codes, no generic mode; the weights of consecutive groups b_gstride elements apart
// without overlap and as aligned as b itself, their scales b_scale_gstride bytes apart on the
// scale words' alignment; a grid bound (tile_map.h) that is a grid.
static bool grouped_launch(const GemmArgs& p) { return p.grp_offs != nullptr || p.ngroups != 0; }
static hipError_t grouped_operands_ok(const GemmArgs& p, int din, int tile, int mode) {
  if (p.grp_offs == nullptr || p.ngroups <= 0 || p.ngroups > kMaxGroups)
    return hipErrorInvalidValue;
  if (din != DT_BF16 && din != DT_F16 && din != DT_FP8 && din != DT_FP4)
    return hipErrorInvalidValue;
  if (mode == GEMM_MODE_GENERIC || (tile != TILE_AUTO && !mxs_offers(tile)))
    return hipErrorInvalidValue;
  if (p.M < 0 || p.N < 0) return hipErrorInvalidValue;
  const hipError_t e = plain_operands_only(p, true, true, hipErrorInvalidValue);
  if (e != hipSuccess) return e;
  const int64_t esz2 = din == DT_FP4 ? 1 : 2 * dtype_size(din);  // twice the element size
  if (p.b_gstride < 0 || p.b_gstride * esz2 % 32 ||
      (p.ngroups > 1 && p.b_gstride < (int64_t)p.N * p.ldb))
    return hipErrorInvalidValue;
  if (p.b_scale != nullptr) {
    const int align = din == DT_FP4 ? 8 : 4;
    if (p.b_scale_gstride < 0 || p.b_scale_gstride % align ||
        (p.ngroups > 1 && p.b_scale_gstride < (int64_t)p.N * p.b_scale_ld))
      return hipErrorInvalidValue;
  }
  if (grouped_grid_bound(p.M, p.ngroups, 128, (p.N + 127) / 128) > 0x7FFFFFFFLL)
    return hipErrorInvalidValue;
  return hipSuccess;
}
// The entry of a checked grouped launch (weak: gemm_entry.h).
static hipError_t launch_grouped_checked(const GemmArgs& p, int din, int dout, int tile,
                                         hipStream_t s) {
  if (launch_grouped == nullptr) return hipErrorNotSupported;
  return launch_grouped(p, din, dout, tile, s);
}

// DT_FP4 operands: the block-scaled MXFP4 flavour of the tiled kernel or hipErrorInvalidValue,
// never a launch with something substituted.
static hipError_t gemm_launch_fp4(const GemmArgs& p, int dout, int tile, int mode, hipStream_t s) {
  if (p.a_scale == nullptr || p.b_scale == nullptr) return hipErrorInvalidValue;
  if (dout != DT_BF16 && dout != DT_F16 && dout != DT_F32) return hipErrorInvalidValue;
  if (mode != GEMM_MODE_AUTO && mode != GEMM_MODE_MX) return hipErrorInvalidValue;
  if (tile != TILE_AUTO && !mx4_offers(tile)) return hipErrorInvalidValue;
  if (p.M < 0 || p.N < 0 || p.K <= 0 || p.K % 256 || p.lda % 2 || p.ldb % 2 || p.lda < p.K ||
      p.ldb < p.K)
    return hipErrorInvalidValue;
  const hipError_t e = plain_operands_only(p, false, true, hipErrorInvalidValue);
  if (e != hipSuccess) return e;
  if (p.M == 0 || p.N == 0) return hipSuccess;
  // the fast path's alignment, on the operands as the byte matrices the kernel reads
  if (p.a == nullptr || p.b == nullptr || p.c == nullptr || p.ldc < p.N ||
      !gemm_fast_path_ok(fp4_byte_view(p, true, false), DT_U8, dout))
    return hipErrorInvalidValue;
  if (!scale_operands_ok(p, 8)) return hipErrorInvalidValue;
  if (tile == TILE_AUTO) tile = mxs_tile_for(choose_tile(p.M, p.N, p.K, DT_FP4));
  if (tile < 0) return hipErrorInvalidValue;
  if (grouped_launch(p)) return launch_grouped_checked(p, DT_FP4, dout, tile, s);
  return launch_fast_mx4(p, dout, tile, s);
}

// Quantised output (dout = DT_FP8 / DT_FP4 with GemmArgs::c_scale): the tiled kernel's quantising
// epilogue or hipErrorInvalidValue, never a launch with something substituted.
static hipError_t gemm_launch_qout(const GemmArgs& p, int din, int dout, int tile, int mode,
                                   hipStream_t s) {
  const bool q4 = dout == DT_FP4, in4 = din == DT_FP4;
  if (p.c_scale == nullptr) return hipErrorInvalidValue;
  if (din != DT_BF16 && din != DT_F16 && din != DT_FP8 && !in4) return hipErrorInvalidValue;
  // fp8 / fp4 operands: block-scaled only (both scales); 16-bit operands carry none
  const bool scaled = din == DT_FP8 || in4;
  if (scaled ? (p.a_scale == nullptr || p.b_scale == nullptr)
             : (p.a_scale != nullptr || p.b_scale != nullptr))
    return hipErrorInvalidValue;
  if (mode == GEMM_MODE_GENERIC || mode < GEMM_MODE_AUTO || mode > GEMM_MODE_MX ||
      (!scaled && mode == GEMM_MODE_MX))
    return hipErrorInvalidValue;
  if (tile != TILE_AUTO && !mxs_offers(tile)) return hipErrorInvalidValue;
  // whole 32-column blocks, as many as the GEMM that reads them takes per K-tile row
  if (p.M < 0 || p.N < 0 || p.K <= 0 || p.N % (q4 ? 256 : 128)) return hipErrorInvalidValue;
  const hipError_t e = plain_operands_only(p, true, true, hipErrorInvalidValue);
  if (e != hipSuccess) return e;
  if (p.M == 0 || p.N == 0) return hipSuccess;
  // the fast path's alignment, on operands and output as the byte matrices the kernel touches;
  // output rows 16-byte aligned: what the GEMM that reads them as its A asks for
  if (in4 && (p.K % 256 || p.lda % 2 || p.ldb % 2)) return hipErrorInvalidValue;
  if (q4 && p.ldc % 2) return hipErrorInvalidValue;
  const GemmArgs q = fp4_byte_view(p, in4, q4);
  if (p.a == nullptr || p.b == nullptr || p.c == nullptr || p.lda < p.K || p.ldb < p.K ||
      p.ldc < p.N || q.ldc % 16 || ((uintptr_t)p.c & 15) ||
      !gemm_fast_path_ok(q, in4 ? DT_U8 : din, DT_U8))
    return hipErrorInvalidValue;
  if (scaled && !scale_operands_ok(p, in4 ? 8 : 4)) return hipErrorInvalidValue;
  // the output scales in the layout their reader takes (4-byte words; 8 for fp4 data)
  const int cal = q4 ? 8 : 4;
  if (((uintptr_t)p.c_scale & (cal - 1)) || p.c_scale_ld % cal || p.c_scale_ld < p.N / 32 ||
      (int64_t)p.M * p.c_scale_ld >= (int64_t(1) << 31))
    return hipErrorInvalidValue;
  if (tile == TILE_AUTO) tile = mxs_tile_for(choose_tile(p.M, p.N, p.K, din));
  if (tile < 0) return hipErrorInvalidValue;
  if (grouped_launch(p)) return launch_grouped_checked(p, din, dout, tile, s);
  return q4 ? launch_qout_fp4(p, din, tile, s) : launch_qout_fp8(p, din, tile, s);
}

// Gated (GLU) epilogue (GemmArgs::glu): the tiled kernel's offered codes, bf16 / f16 / block-scaled
// fp8 / block-scaled fp4 operands, a dense output the operands pair with or a quantised one, plain
// rows; or hipErrorInvalidValue, never a launch of something else. N counts the rows of b; the
// output, its scales and every bound on them have N / 2 columns.
static hipError_t gemm_launch_glu(const GemmArgs& p, int din, int dout, int tile, int mode,
                                  hipStream_t s) {
  const bool in4 = din == DT_FP4, scaled = din == DT_FP8 || in4;
  const bool q4 = dout == DT_FP4, qout = dout == DT_FP8 || q4;
  if (din != DT_BF16 && din != DT_F16 && !scaled) return hipErrorInvalidValue;
  // fp8 / fp4 operands: block-scaled only (both scales); 16-bit operands carry none
  if (scaled ? (p.a_scale == nullptr || p.b_scale == nullptr)
             : (p.a_scale != nullptr || p.b_scale != nullptr))
    return hipErrorInvalidValue;
  if (qout != (p.c_scale != nullptr)) return hipErrorInvalidValue;
  if (!qout && dout != DT_F32 && !(scaled ? dout == DT_BF16 || dout == DT_F16 : dout == din))
    return hipErrorInvalidValue;
  if (mode == GEMM_MODE_GENERIC || mode < GEMM_MODE_AUTO || mode > GEMM_MODE_MX ||
      (!scaled && mode == GEMM_MODE_MX))
    return hipErrorInvalidValue;
  if (tile != TILE_AUTO && !mxs_offers(tile)) return hipErrorInvalidValue;
  // whole 64-row gate / up groups; N / 2 in whole blocks as the GEMM that reads them takes them
  if (p.M < 0 || p.N < 0 || p.K <= 0 || p.N % (q4 ? 512 : qout ? 256 : 64))
    return hipErrorInvalidValue;
  const hipError_t e = plain_operands_only(p, true, true, hipErrorInvalidValue);
  if (e != hipSuccess) return e;
  if (p.M == 0 || p.N == 0) return hipSuccess;
  if (in4 && (p.K % 256 || p.lda % 2 || p.ldb % 2)) return hipErrorInvalidValue;
  if (q4 && p.ldc % 2) return hipErrorInvalidValue;
  const GemmArgs q = fp4_byte_view(p, in4, q4);
  if (p.a == nullptr || p.b == nullptr || p.c == nullptr || p.lda < p.K || p.ldb < p.K ||
      p.ldc < p.N / 2 || !gemm_fast_path_ok(q, in4 ? DT_U8 : din, qout ? DT_U8 : dout))
    return hipErrorInvalidValue;
  if (scaled && !scale_operands_ok(p, in4 ? 8 : 4)) return hipErrorInvalidValue;
  if (qout) {  // rows and scales as gemm_launch_qout asks for them, N / 64 scale bytes per row
    const int cal = q4 ? 8 : 4;
    if (q.ldc % 16 || ((uintptr_t)p.c & 15) || ((uintptr_t)p.c_scale & (cal - 1)) ||
        p.c_scale_ld % cal || p.c_scale_ld < p.N / 64 ||
        (int64_t)p.M * p.c_scale_ld >= (int64_t(1) << 31))
      return hipErrorInvalidValue;
  }
  if (tile == TILE_AUTO) tile = mxs_tile_for(choose_tile(p.M, p.N, p.K, din));
  if (tile < 0) return hipErrorInvalidValue;
  GemmArgs g = p;
  g.glu = 1;
  if (grouped_launch(p)) return launch_grouped_checked(g, din, dout, tile, s);
  if (qout) return q4 ? launch_qout_fp4(g, din, tile, s) : launch_qout_fp8(g, din, tile, s);
  if (in4) return launch_fast_mx4(g, dout, tile, s);
  if (scaled) return launch_fast_mxs(g, dout, tile, s);
  return launch_fast(g, din, dout, tile, s);
}

// A grouped launch with bf16 / f16 operands or block-scaled fp8 ones and a dense output (the gated,
// quantising and fp4 forms go through the functions above): the grouped tiled kernel or
// hipErrorInvalidValue. Unit-scale fp8 has no grouped form.
static hipError_t gemm_launch_grouped_dense(const GemmArgs& p, int din, int dout, int tile,
                                            int mode, hipStream_t s) {
  const bool scaled = din == DT_FP8;
  if (din != DT_BF16 && din != DT_F16 && !scaled) return hipErrorInvalidValue;
  if (scaled ? (p.a_scale == nullptr || p.b_scale == nullptr)
             : (p.a_scale != nullptr || p.b_scale != nullptr))
    return hipErrorInvalidValue;
  if (dout != DT_F32 && !(scaled ? dout == DT_BF16 || dout == DT_F16 : dout == din))
    return hipErrorInvalidValue;
  if (mode < GEMM_MODE_AUTO || mode > GEMM_MODE_MX || (!scaled && mode == GEMM_MODE_MX))
    return hipErrorInvalidValue;
  if (p.K <= 0) return hipErrorInvalidValue;
  if (p.M == 0 || p.N == 0) return hipSuccess;
  if (p.a == nullptr || p.b == nullptr || p.c == nullptr || p.lda < p.K || p.ldb < p.K ||
      p.ldc < p.N || !gemm_fast_path_ok(p, din, dout))
    return hipErrorInvalidValue;
  if (scaled && !scale_operands_ok(p, 4)) return hipErrorInvalidValue;
  if (tile == TILE_AUTO) tile = mxs_tile_for(choose_tile(p.M, p.N, p.K, din));
  if (tile < 0) return hipErrorInvalidValue;
  return launch_grouped_checked(p, din, dout, tile, s);
}

// K-grouped launches (GemmArgs::kgrouped): the K-grouped tiled kernel or hipErrorInvalidValue. The
// offsets are device memory and are never read here. What the M-grouped form refuses about flags,
// tables, grouped rows, K-split, all-gather, tile codes and the number of groups is refused here
// too, and so are an activation, a gate, a quantised output and unscaled operands. K is the
// operands' column extent: whole K-tiles, at least the capacity of (T, E, MOD), so no content of
// the offsets reaches a column outside an operand row (tile_map.h); rows and scales as the scaled
// flavour it runs asks for them. The groups' outputs lie c_kgstride elements apart without
// overlap, 8-byte aligned as c is.
static hipError_t gemm_launch_kgrouped(const GemmArgs& p, int din, int dout, int tile, int mode,
                                       hipStream_t s) {
  const bool in4 = din == DT_FP4;
  const int MOD = in4 ? 256 : 128;
  if (p.grp_offs == nullptr || p.ngroups <= 0 || p.ngroups > kMaxGroups)
    return hipErrorInvalidValue;
  if (din != DT_FP8 && !in4) return hipErrorInvalidValue;
  if (p.a_scale == nullptr || p.b_scale == nullptr) return hipErrorInvalidValue;
  if (dout != DT_F32 && dout != DT_BF16 && dout != DT_F16) return hipErrorInvalidValue;
  if (p.act != ACT_NONE || p.glu || p.c_scale != nullptr) return hipErrorInvalidValue;
  if (mode != GEMM_MODE_AUTO && mode != GEMM_MODE_MX) return hipErrorInvalidValue;
  if (tile != TILE_AUTO && !mxs_offers(tile)) return hipErrorInvalidValue;
  if (p.b_gstride != 0 || p.b_scale_gstride != 0) return hipErrorInvalidValue;
  if (p.M < 0 || p.N < 0 || p.K <= 0 || p.K % MOD || p.kgrp_rows < 0)
    return hipErrorInvalidValue;
  const hipError_t e = plain_operands_only(p, true, true, hipErrorInvalidValue);
  if (e != hipSuccess) return e;
  if (p.K < kgrouped_capacity(p.kgrp_rows, p.ngroups, MOD)) return hipErrorInvalidValue;
  if (p.M == 0 || p.N == 0) return hipSuccess;
  if (in4 && (p.lda % 2 || p.ldb % 2)) return hipErrorInvalidValue;
  if (p.a == nullptr || p.b == nullptr || p.c == nullptr || p.lda < p.K || p.ldb < p.K ||
      p.ldc < p.N || !gemm_fast_path_ok(fp4_byte_view(p, in4, false), in4 ? DT_U8 : din, dout))
    return hipErrorInvalidValue;
  if (!scale_operands_ok(p, in4 ? 8 : 4)) return hipErrorInvalidValue;
  if (p.c_kgstride < 0 || p.c_kgstride * dtype_size(dout) % 8 ||
      (p.ngroups > 1 && p.c_kgstride < (int64_t)p.M * p.ldc))
    return hipErrorInvalidValue;
  if (tile == TILE_AUTO) tile = mxs_tile_for(choose_tile(p.M, p.N, p.K, din));
  if (tile < 0) return hipErrorInvalidValue;
  const int64_t tiles = (int64_t)((p.M + tile_rows(tile) - 1) / tile_rows(tile)) *
                        ((p.N + tile_cols(tile) - 1) / tile_cols(tile));
  if (tiles * p.ngroups > 0x7FFFFFFFLL) return hipErrorInvalidValue;
  if (launch_kgrouped == nullptr) return hipErrorNotSupported;
  return launch_kgrouped(p, din, dout, tile, s);
}

hipError_t gemm_launch(const GemmArgs& p_in, int din, int dout, int tile, int mode,
                       hipStream_t s) {
  GemmArgs p = p_in;
  if (p.a_grp <= 0) { p.a_grp = p.M > 0 ? p.M : 1; p.a_gstride = p.a_grp; }
  if (p.c_grp <= 0) { p.c_grp = p.M > 0 ? p.M : 1; p.c_gstride = p.c_grp; }
  // known codes only (the retired families' codes are refused, not rerouted)
  if (tile != TILE_AUTO && tile_slot(tile) < 0) return hipErrorInvalidValue;
  if (p.kgrouped) return gemm_launch_kgrouped(p, din, dout, tile, mode, s);
  const bool grouped = grouped_launch(p);
  if (grouped) {
    const hipError_t e = grouped_operands_ok(p, din, tile, mode);
    if (e != hipSuccess) return e;
  }
  if (p.glu) return gemm_launch_glu(p, din, dout, tile, mode, s);
  // quantised output: dout fp8 / fp4 and output scales go together
  if (dout == DT_FP8 || dout == DT_FP4) return gemm_launch_qout(p, din, dout, tile, mode, s);
  if (p.c_scale != nullptr) return hipErrorInvalidValue;
  if (din == DT_FP4) return gemm_launch_fp4(p, dout, tile, mode, s);
  if (grouped) return gemm_launch_grouped_dense(p, din, dout, tile, mode, s);
  // MX block scales: both or neither; with them the tiled kernel's scaled flavour or a refusal,
  // never unit scales in their place
  if ((p.a_scale != nullptr) != (p.b_scale != nullptr)) return hipErrorInvalidValue;
  const bool scaled = p.a_scale != nullptr;
  if (scaled && p.M != 0 && p.N != 0) {
    if (din != DT_FP8 || mode == GEMM_MODE_GENERIC || (tile != TILE_AUTO && !mxs_offers(tile)) ||
        plain_operands_only(p, false, false, hipErrorNotSupported) != hipSuccess ||
        !gemm_fast_path_ok(p, din, dout) || !scale_operands_ok(p, 4))
      return hipErrorNotSupported;
    mode = GEMM_MODE_MX;
  }
  if (p.M == 0 || p.N == 0) return hipSuccess;
  if (p.ksplit > 1) {
    // K-split: slice j of K columns -> partial j at c + j * M * ldc (the caller sums them). pt4
    // runs every (slice, tile) pair in one launch; any other kernel runs the slices one by one.
    if (p.flags != nullptr || p.a_table != nullptr || p.c_table != nullptr || p.ag_ctas > 0 ||
        p.ag_mode != 0 || p.act != ACT_NONE || p.a_grp != p.M || p.c_grp != p.M || p.ksplit > 64)
      return hipErrorNotSupported;
    if (tile == TILE_AUTO || tile == TILE_PT4) {
      GemmArgs q = p;
      q.tile_order = 0;
      const bool fast = mode != GEMM_MODE_GENERIC && gemm_fast_path_ok(q, din, dout);
      hipError_t e = hipErrorNotSupported;
      if (fast && din == DT_FP8 && mode == GEMM_MODE_MX) e = launch_fast_mx(q, dout, TILE_PT4, s);
      else if (fast) e = launch_fast(q, din, dout, TILE_PT4, s);
      if (e != hipErrorNotSupported && e != hipErrorInvalidValue) return e;
    }
    const int esz = dtype_size(din), osz = dtype_size(dout);
    for (int j = 0; j < p.ksplit; ++j) {
      GemmArgs q = p;
      q.ksplit = 1;
      q.a = (const char*)p.a + (int64_t)j * p.K * esz;
      q.b = (const char*)p.b + (int64_t)j * p.K * esz;
      q.c = (char*)p.c + (int64_t)j * p.M * p.ldc * osz;
      const hipError_t e = gemm_launch(q, din, dout, tile == TILE_PT4 ? TILE_AUTO : tile, mode, s);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  if (p.a_table != nullptr) {
    // A through a row-block address table (direct access to the peers' shards, or the blocks of
    // a stage-major gather buffer): the ping-pong kernels (pt4 / t4 / t8 / pt8, whole 256-row
    // blocks; pt4 takes one panel base per tile) and the tiled kernels read A through it.
    // Arrival flags then index LOGICAL rows.
    if (p.shard_rows <= 0) return hipErrorInvalidValue;
    const bool whole = p.M % 256 == 0 && p.N % 256 == 0 && p.shard_rows % 256 == 0;
    if (tile == TILE_AUTO) {
      tile = choose_tile(p.M, p.N, p.K, din);
      if (tile != TILE_PT4 && tile != TILE_PT8 && tile != TILE_T4) tile = TILE_T8;
    }
    const bool ping = tile == TILE_T8 || tile == TILE_PT8 || tile == TILE_T4 || tile == TILE_PT4;
    if (ping && !whole) tile = TILE_128x128;
    // the tiled MX kernel addresses plain rows: block-scaled MFMAs on whole blocks only
    if (mode == GEMM_MODE_MX && !(ping && whole)) mode = GEMM_MODE_AUTO;
    if (p.flags != nullptr && !(ping && whole)) return hipErrorNotSupported;
    if (mode == GEMM_MODE_GENERIC || !gemm_fast_path_ok(p, din, dout)) return hipErrorNotSupported;
  }
  if (p.c_table != nullptr) {
    // direct-store C: every fast kernel addresses C rows through c_row(); the generic kernel
    // cannot, and an interleaved shard order needs whole tiles per shard
    if (p.c_shard_rows <= 0 || p.c_grp != p.M || mode == GEMM_MODE_GENERIC ||
        p.flags != nullptr || p.ag_ctas > 0 || !gemm_fast_path_ok(p, din, dout))
      return hipErrorNotSupported;
  }
  if (p.tile_order == 2 && (p.nshards <= 0 || p.M % p.nshards != 0))
    return hipErrorInvalidValue;
  if (p.ag_ctas > 0) {
    // in-kernel all-gather: only the gated persistent pt4 kernel carries the copy workgroups;
    // anything else would skip the copies, so refuse rather than fall back
    const int esz = dtype_size(din);
    if (p.flags == nullptr || p.a_table != nullptr || mode == GEMM_MODE_GENERIC ||
        !gemm_fast_path_ok(p, din, dout) || p.M % 256 || p.N % 256 || p.a_grp != p.M ||
        (int64_t)p.K * esz / 128 < 2 || ((int64_t)p.K * esz / 128) % 2 != 0 || p.act != ACT_NONE ||
        p.lda * esz > (1 << 22) || p.ldb * esz > (1 << 22) ||
        p.nsub < 1 || p.nshards % p.nsub || p.nshards / p.nsub > 32 || p.ag_parts < 1 ||
        p.ag_tab == nullptr || p.flag_rows * p.lda * esz / p.ag_parts >= (int64_t(1) << 30))
      return hipErrorNotSupported;  // (a copy unit is addressed by one 32-bit buffer descriptor)
    tile = TILE_PT4;
  } else if (p.ag_mode != 0) {
    return hipErrorNotSupported;  // agent-scope gate acquire only for flags this launch sets
  }
  if (mode < GEMM_MODE_AUTO || mode > GEMM_MODE_MX) return hipErrorInvalidValue;
  const bool fast = mode != GEMM_MODE_GENERIC && gemm_fast_path_ok(p, din, dout);
  if (p.tile_order && !fast) p.tile_order = 0;
  if (fast) {
    if (tile == TILE_AUTO) tile = choose_tile(p.M, p.N, p.K, din);
    if (scaled) {  // the tiled shape of that code, among the ones the scaled flavour is built for
      tile = mxs_tile_for(tile);
      if (tile < 0) return hipErrorNotSupported;
    }
    if (p.nsub < 1) p.nsub = 1;
    if (p.tile_order && (p.nshards <= 0 || p.M % p.nshards != 0 || p.nshards % p.nsub != 0 ||
                         (p.M / p.nshards) % tile_rows(tile) != 0)) {
      // tile_order 3 also means "the own blocks are not gated": never drop it silently
      if (p.tile_order == 3) return hipErrorNotSupported;
      p.tile_order = 0;
    }
    if (p.tile_order == 2 && p.N % tile_cols(tile) != 0) p.tile_order = 0;  // whole tiles/shard
    hipError_t e = hipErrorInvalidValue;
    if (scaled) return launch_fast_mxs(p, dout, tile, s);
    if (din == DT_FP8 && mode == GEMM_MODE_MX) e = launch_fast_mx(p, dout, tile, s);
    else e = launch_fast(p, din, dout, tile, s);
    if (e != hipErrorInvalidValue) return e;
  }
  if (p.flags != nullptr || p.c_table != nullptr)
    return hipErrorNotSupported;  // arrival flags / direct-store C need the tiled kernels
  return launch_generic(p, din, dout, s);
}

}  // namespace ddlb
