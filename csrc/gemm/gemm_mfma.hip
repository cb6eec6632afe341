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

static bool grouped_launch(const GemmArgs& p) { return p.grp_offs != nullptr || p.ngroups != 0; }

// Every form of the tiled kernel beyond the plain launch, checked in one place: fp4 operands, a
// quantised output (dout = DT_FP8 / DT_FP4 with GemmArgs::c_scale), a gated epilogue
// (GemmArgs::glu), grouped rows (GemmArgs::grp_offs) and K-grouped columns (GemmArgs::kgrouped),
// in any combination the kernel has. The answer is the launch of that form or
// hipErrorInvalidValue, never a launch with something substituted (hipErrorNotSupported: a host
// program linked without the grouped entries, gemm_entry.h). a_grp / c_grp are already defaulted
// by gemm_launch. Offsets are device memory and are never read here.
//  * Operands bf16 / f16 without scales, or fp8 / fp4 with both (block-scaled only); a dense
//    output is f32 or what the operands pair with, a quantised one comes with its scales.
//  * Plain rows in the launch's own order, the codes of mxs_offers(), mode auto (mx with scales).
//  * Every rule on the shape comes before the empty problem's hipSuccess, every rule on pointers
//    and layout after it: the fast path on the byte view (gemm.h fp4_byte_view), the scales, a
//    quantised output's rows 16-byte aligned and its scales in the layout their reader takes
//    (4-byte words; 8 for fp4 data), on cols = N / 2 columns with a gate.
//  * Grouped: the weights of consecutive groups b_gstride elements apart without overlap and as
//    aligned as b itself, their scales b_scale_gstride bytes apart on the scale words'
//    alignment; a grid bound (tile_map.h) that is a grid.
//  * K-grouped: scaled operands, a dense output, no activation or gate; K is the operands' column
//    extent, whole K-tiles and at least the capacity of (T, E, MOD), so no content of the offsets
//    reaches a column outside an operand row (tile_map.h); the groups' outputs lie c_kgstride
//    elements apart without overlap, 8-byte aligned as c is.
static hipError_t gemm_launch_form(GemmArgs p, int din, int dout, int tile, int mode,
                                   hipStream_t s) {
  constexpr hipError_t bad = hipErrorInvalidValue;
  const bool in4 = din == DT_FP4, scaled = din == DT_FP8 || in4;
  const bool q4 = dout == DT_FP4, qout = dout == DT_FP8 || q4;
  const bool glu = p.glu != 0, kgrouped = p.kgrouped != 0;
  const bool grouped = !kgrouped && grouped_launch(p);
  const int64_t cols = glu ? p.N / 2 : p.N;  // of the output and, over 32, of its scales
  const int sal = in4 ? 8 : 4, cal = q4 ? 8 : 4;
  if (din != DT_BF16 && din != DT_F16 && !scaled) return bad;
  if (scaled != (p.a_scale != nullptr) || scaled != (p.b_scale != nullptr)) return bad;
  if (qout != (p.c_scale != nullptr)) return bad;
  if (!qout && dout != DT_F32 && !(scaled ? dout == DT_BF16 || dout == DT_F16 : dout == din))
    return bad;
  if (mode != GEMM_MODE_AUTO && !(scaled && mode == GEMM_MODE_MX)) return bad;
  if (tile != TILE_AUTO && !mxs_offers(tile)) return bad;
  if (p.M < 0 || p.N < 0 || p.K <= 0 || p.lda < p.K || p.ldb < p.K) return bad;
  if (in4 && (p.K % 256 || p.lda % 2 || p.ldb % 2)) return bad;
  // whole 64-row gate / up groups; whole 32-column blocks, as many as the GEMM that reads them
  // takes per K-tile row
  if ((glu && p.N % 64) || (qout && cols % (q4 ? 256 : 128))) return bad;
  // (a dense fp4 launch without groups or a gate takes grouped C rows, as it always has)
  const bool plain_c_rows = !in4 || qout || glu || grouped || kgrouped;
  if (plain_operands_only(p, plain_c_rows, true, bad) != hipSuccess) return bad;
  if ((grouped || kgrouped) &&
      (p.grp_offs == nullptr || p.ngroups <= 0 || p.ngroups > kMaxGroups))
    return bad;
  if (grouped) {
    const int64_t esz2 = in4 ? 1 : 2 * dtype_size(din);  // twice the element size
    if (p.b_gstride < 0 || p.b_gstride * esz2 % 32 ||
        (p.ngroups > 1 && p.b_gstride < (int64_t)p.N * p.ldb))
      return bad;
    if (scaled && (p.b_scale_gstride < 0 || p.b_scale_gstride % sal ||
                   (p.ngroups > 1 && p.b_scale_gstride < (int64_t)p.N * p.b_scale_ld)))
      return bad;
    if (grouped_grid_bound(p.M, p.ngroups, 128, (p.N + 127) / 128) > 0x7FFFFFFFLL) return bad;
  }
  if (kgrouped) {
    const int MOD = in4 ? 256 : 128;
    if (!scaled || qout || glu || p.act != ACT_NONE) return bad;
    if (p.b_gstride != 0 || p.b_scale_gstride != 0 || p.kgrp_rows < 0 || p.K % MOD) return bad;
    if (p.K < kgrouped_capacity(p.kgrp_rows, p.ngroups, MOD)) return bad;
  }
  if (p.M == 0 || p.N == 0) return hipSuccess;
  const GemmArgs q = fp4_byte_view(p, in4, q4);
  if (p.a == nullptr || p.b == nullptr || p.c == nullptr || p.ldc < cols || (q4 && p.ldc % 2) ||
      !gemm_fast_path_ok(q, in4 ? DT_U8 : din, qout ? DT_U8 : dout))
    return bad;
  if (scaled && !scale_operands_ok(p, sal)) return bad;
  if (qout && (q.ldc % 16 || ((uintptr_t)p.c & 15) || ((uintptr_t)p.c_scale & (cal - 1)) ||
               p.c_scale_ld % cal || p.c_scale_ld < cols / 32 ||
               (int64_t)p.M * p.c_scale_ld >= (int64_t(1) << 31)))
    return bad;
  if (kgrouped && (p.c_kgstride < 0 || p.c_kgstride * dtype_size(dout) % 8 ||
                   (p.ngroups > 1 && p.c_kgstride < (int64_t)p.M * p.ldc)))
    return bad;
  if (tile == TILE_AUTO) tile = mxs_tile_for(choose_tile(p.M, p.N, p.K, din));
  if (tile < 0) return bad;
  p.glu = glu;
  if (kgrouped) {
    const int64_t tiles = (int64_t)((p.M + tile_rows(tile) - 1) / tile_rows(tile)) *
                          ((p.N + tile_cols(tile) - 1) / tile_cols(tile));
    if (tiles * p.ngroups > 0x7FFFFFFFLL) return bad;
    // (the grouped entries are weak: gemm_entry.h)
    return launch_kgrouped == nullptr ? hipErrorNotSupported : launch_kgrouped(p, din, dout, tile, s);
  }
  if (grouped)
    return launch_grouped == nullptr ? hipErrorNotSupported : launch_grouped(p, din, dout, tile, s);
  if (qout) return q4 ? launch_qout_fp4(p, din, tile, s) : launch_qout_fp8(p, din, tile, s);
  if (in4) return launch_fast_mx4(p, dout, tile, s);
  if (scaled) return launch_fast_mxs(p, dout, tile, s);
  return launch_fast(p, din, dout, tile, s);
}

hipError_t gemm_launch(const GemmArgs& p_in, int din, int dout, int tile, int mode,
                       hipStream_t s) {
  GemmArgs p = p_in;
  if (p.a_grp <= 0) { p.a_grp = p.M > 0 ? p.M : 1; p.a_gstride = p.a_grp; }
  if (p.c_grp <= 0) { p.c_grp = p.M > 0 ? p.M : 1; p.c_gstride = p.c_grp; }
  // known codes only (the retired families' codes are refused, not rerouted)
  if (tile != TILE_AUTO && tile_slot(tile) < 0) return hipErrorInvalidValue;
  // every form beyond the plain launch; a quantised output and its scales go together
  if (p.kgrouped || grouped_launch(p) || p.glu || din == DT_FP4 || dout == DT_FP8 ||
      dout == DT_FP4 || p.c_scale != nullptr)
    return gemm_launch_form(p, din, dout, tile, mode, s);
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
