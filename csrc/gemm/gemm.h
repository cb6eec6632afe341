// Public interface of the CDNA4 MFMA GEMM (csrc/gemm/gemm_mfma.hip).
//
// Non-finite values (every kernel and launch form; tests/test_nonfinite_gpu.py). The GEMM is
// IEEE 754 per element: an output element is NaN if any product of its dot is NaN (a NaN
// operand, Inf x 0, or +Inf and -Inf products both present), otherwise +-Inf if an infinite
// product is present, otherwise the sum, rounded once to the output dtype; a K-split keeps this
// through its partials and the reduce kernel. Elements outside a view (row padding, skipped
// grouped rows, columns no group owns) never influence anything, whatever bits they hold. The
// epilogue activations equal the f32 reference in class: relu(NaN) is NaN, gelu and silu give
// NaN at NaN and -Inf and +Inf at +Inf. A block-scale byte 255 (the E8M0 NaN) makes every
// product of its block NaN. The quantising epilogue and the MX quantisers below never hide a
// non-finite value: mx_cvt.h has the rule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ddlb {

// dtype codes shared with Python (ddlb_amd/ops/_dtypes.py)
// DT_FP4: OCP E2M1, two elements per byte (element 2j in the low nibble of byte j); dtype_size()
// is 0 for it, a row of K elements is K / 2 bytes.
enum DType : int { DT_F32 = 0, DT_F16 = 1, DT_BF16 = 2, DT_FP8 = 3, DT_F64 = 4, DT_U8 = 5,
                   DT_FP4 = 6 };
inline int dtype_size(int dt) {
  switch (dt) {
    case DT_F32: return 4;
    case DT_F16: case DT_BF16: return 2;
    case DT_FP8: case DT_U8: return 1;
    case DT_F64: return 8;
    default: return 0;
  }
}

// Codes 5 (pp256), 8 / 9 (p256 / p128), 13 / 14 (pi256 / pi256w4) and 15 (r256) belonged to
// kernel families retired in round 4 (no `auto` path reached them); they are refused.
enum Tile : int { TILE_AUTO = 0, TILE_256x256 = 1, TILE_256x128 = 2, TILE_128x256 = 3,
                  TILE_128x128 = 4, TILE_256x256_W4 = 6, TILE_256x128_W4 = 7,
                  TILE_I256 = 10, TILE_I128 = 11,    // I*: DMA interleaved into the MFMAs
                  TILE_I256W4 = 12,
                  TILE_T8 = 16,       // T8: 8-phase ping-pong, counted vmcnt (gemm_kernels.h)
                  TILE_PT8 = 17,      // PT8: persistent T8 (tiles streamed, C stores spread)
                  TILE_T4 = 18,       // T4: 2-phase ping-pong (32 MFMAs per section)
                  TILE_PT4 = 19 };    // PT4: persistent T4
// What each live code runs: the tile it covers and the tiled kernel's wave grid (wm x wn waves)
// and DMA interleave. The ping-pong codes (T8 .. PT4) run their own 256x256 kernels on whole
// tiles; their entry is the tiled kernel that takes every other shape (the interleaved 256x256).
// The block-scaled MX kernels use the same shapes, never interleaved.
struct TileCfg { int code, rows, cols, wm, wn; bool ilv; };
constexpr TileCfg kTileCfgs[] = {
    {TILE_256x256, 256, 256, 2, 4, false},    {TILE_256x128, 256, 128, 4, 2, false},
    {TILE_128x256, 128, 256, 2, 4, false},    {TILE_128x128, 128, 128, 2, 2, false},
    {TILE_256x256_W4, 256, 256, 2, 2, false}, {TILE_256x128_W4, 256, 128, 2, 2, false},
    {TILE_I256, 256, 256, 2, 4, true},        {TILE_I128, 128, 128, 2, 2, true},
    {TILE_I256W4, 256, 256, 2, 2, true},      {TILE_T8, 256, 256, 2, 4, true},
    {TILE_PT8, 256, 256, 2, 4, true},         {TILE_T4, 256, 256, 2, 4, true},
    {TILE_PT4, 256, 256, 2, 4, true}};
constexpr int kNumTileCfgs = sizeof(kTileCfgs) / sizeof(kTileCfgs[0]);
// Index of a tile code in kTileCfgs; -1 for TILE_AUTO, the retired codes and anything else.
constexpr int tile_slot(int tile) {
  for (int i = 0; i < kNumTileCfgs; ++i)
    if (kTileCfgs[i].code == tile) return i;
  return -1;
}
constexpr int tile_rows_of(int tile) {  // (256 for a code without a kernel, as tile_rows has said)
  const int i = tile_slot(tile);
  return i < 0 ? 256 : kTileCfgs[i].rows;
}
constexpr int tile_cols_of(int tile) {
  const int i = tile_slot(tile);
  return i < 0 ? 256 : kTileCfgs[i].cols;
}

// Tile codes the scaled (per-block E8M0 scales) flavour of the tiled kernel is built for. Both
// 256x256 forms are left out: on top of their accumulator and fragment registers the scale
// offsets, words and bytes (3 per fragment) do not fit, and the compiler spills to scratch
// (TILE_256x256, 2x4 waves: 292 bytes per lane; TILE_256x256_W4: 44; docs/ARCHITECTURE.md).
constexpr bool mxs_offers(int tile) {
  return tile == TILE_256x128 || tile == TILE_128x256 || tile == TILE_128x128 ||
         tile == TILE_256x128_W4;
}
// The scaled kernel for what choose_tile answers (`auto` only; an explicit code that is not
// offered, the ping-pong codes among them, is refused): an offered code is itself; any other
// live code maps to the offered code of its rows x cols, a 256x256 one to 256x128. -1: not a
// live code.
constexpr int mxs_tile_for(int tile) {
  if (mxs_offers(tile)) return tile;
  const int i = tile_slot(tile);
  if (i < 0) return -1;
  for (int j = 0; j < kNumTileCfgs; ++j)
    if (mxs_offers(kTileCfgs[j].code) && kTileCfgs[j].rows == kTileCfgs[i].rows &&
        kTileCfgs[j].cols == kTileCfgs[i].cols)
      return kTileCfgs[j].code;
  return TILE_256x128;
}

// Tile codes of the block-scaled fp4 flavour (MmaMX4S, gemm_mx4.hip): the set the fp8 scaled
// flavour offers, `auto` mapped the same way (mxs_tile_for). Both 256x256 forms stay out as they
// do for fp8: an instantiation that spills to scratch is not offered (TILE_256x256, 2x4 waves:
// 140 bytes per lane; TILE_256x256_W4: 228; docs/ARCHITECTURE.md has the register table).
constexpr bool mx4_offers(int tile) { return mxs_offers(tile); }

// (launch_tiled takes the DMA interleave from kTileCfgs for every flavour: the block-scaled and
// quantising ones are built without it, so no code they offer may carry it)
constexpr bool offered_tiles_not_interleaved() {
  for (int i = 0; i < kNumTileCfgs; ++i)
    if (kTileCfgs[i].ilv && (mxs_offers(kTileCfgs[i].code) || mx4_offers(kTileCfgs[i].code)))
      return false;
  return true;
}
static_assert(offered_tiles_not_interleaved(), "scaled flavours: plain tiled codes only");

constexpr bool tile_cfgs_distinct() {
  for (int i = 0; i < kNumTileCfgs; ++i)
    for (int j = i + 1; j < kNumTileCfgs; ++j)
      if (kTileCfgs[i].code == kTileCfgs[j].code) return false;
  return true;
}
// the rows x cols every live code has had since the table was three hand-written copies
constexpr bool tile_is(int tile, int rows, int cols) {
  return tile_slot(tile) >= 0 && tile_rows_of(tile) == rows && tile_cols_of(tile) == cols;
}
static_assert(kNumTileCfgs == 13 && tile_cfgs_distinct(), "thirteen distinct live tile codes");
static_assert(tile_is(TILE_256x256, 256, 256) && tile_is(TILE_256x128, 256, 128) &&
              tile_is(TILE_128x256, 128, 256) && tile_is(TILE_128x128, 128, 128) &&
              tile_is(TILE_256x256_W4, 256, 256) && tile_is(TILE_256x128_W4, 256, 128) &&
              tile_is(TILE_I256, 256, 256) && tile_is(TILE_I128, 128, 128) &&
              tile_is(TILE_I256W4, 256, 256) && tile_is(TILE_T8, 256, 256) &&
              tile_is(TILE_PT8, 256, 256) && tile_is(TILE_T4, 256, 256) &&
              tile_is(TILE_PT4, 256, 256), "tile_rows / tile_cols per code");
static_assert(tile_slot(TILE_AUTO) < 0 && tile_slot(5) < 0 && tile_slot(8) < 0 &&
              tile_slot(9) < 0 && tile_slot(13) < 0 && tile_slot(14) < 0 && tile_slot(15) < 0,
              "retired codes stay refused");
// Every mode runs one of this file's hand-written kernels: vendor libraries (hipBLASLt through
// torch.matmul) are only the comparison baseline of the `pytorch` slot, never behind `native`.
enum GemmMode : int { GEMM_MODE_AUTO = 0, GEMM_MODE_GENERIC = 1, GEMM_MODE_MX = 2 };

// C[M,N] = A[M,K] * Bt[N,K]^T. Leading dimensions in ELEMENTS.
// Logical row i of A (and of C) lives at physical row (i / grp) * gstride + (i % grp).
struct GemmArgs {
  const void* a = nullptr;
  const void* b = nullptr;
  void* c = nullptr;
  int64_t lda = 0, ldb = 0, ldc = 0;
  int64_t a_grp = 0, a_gstride = 0;  // 0 -> identity
  int64_t c_grp = 0, c_gstride = 0;
  int M = 0, N = 0, K = 0;
  // Arrival-ordered consumption (p2p pipeline): optional
  const unsigned* flags = nullptr;  // flags[shard] >= epoch once shard's A rows have landed
  unsigned epoch = 0;
  const unsigned* epoch_ptr = nullptr;  // if set: the epoch is read here (hipGraph replay)
  int64_t flag_rows = 1;            // physical A rows per shard
  unsigned* timeout_word = nullptr; // set to 1 if a spin gave up
  unsigned spin_limit = 1u << 26;   // polls before a bounded spin gives up (~30 s on uncached flags)
  int tile_order = 0, nshards = 1, first_shard = 0;
  // Row blocks per producer (tile_order): shard index = producer * nsub + block; dispatch is
  // block-major across producers (block 0 of every producer, own first, then block 1, ...),
  // i.e. the order chunked pulls from all peers arrive in. nsub = 1: plain shard order.
  int nsub = 1;
  int reserve_cus = 0;              // flag-gated persistent GEMMs: CUs left free (see launch_pt4)
  int raster_g = 4;                 // m-blocks per raster group of tile_mn (tile_map.h)
  // In-kernel all-gather (flag-gated pt4 only): workgroups [0, ag_ctas) of the launch pull the
  // peers' row blocks of A over xGMI into A (the same rows), count each (producer, block)
  // segment's ag_parts pieces and set its flag when the last lands, and ACK each producer once
  // all its rows are read; the other workgroups run the gated GEMM. ag_tab (device, 2*np+2
  // entries, np = nshards / nsub producers): [src A of producer 0..np-1 | address of my ACK word
  // at producer 0..np-1 | READY words (ready[p] >= epoch: p's rows may be read) | counters
  // (nshards per-segment, then np per-producer; monotonic across runs) | with AG_WAIT_ACKS: my
  // ACK word written by producer 0..np-1 (entry of my own rank unused)].
  int ag_ctas = 0, ag_parts = 1, ag_rank = 0;
  int ag_mode = 0;                  // AgMode bits below
  const uint64_t* ag_tab = nullptr;
  int act = 0;                      // fused epilogue activation: ACT_* below
  // Direct-access A (optional): row block s of shard_rows rows starts at a_table[s] (device
  // array of addresses, e.g. the peers' IPC-mapped shards read straight over xGMI).
  const uint64_t* a_table = nullptr;
  int64_t shard_rows = 0;
  // Direct-store C (optional): row block s of c_shard_rows rows is written at c_table[s] (device
  // array of addresses, e.g. the peers' IPC-mapped receive slots: a reduce-scatter's partials
  // stored straight over xGMI by the GEMM epilogue). tile_order = 2 interleaves the shards.
  const uint64_t* c_table = nullptr;
  int64_t c_shard_rows = 0;
  // K-split (optional): ksplit slices of K columns each (K is the SLICE length; lda / ldb the
  // full rows); slice s reads A / B columns [s K, (s + 1) K) and writes its partial product at
  // c + s * M * ldc elements (the caller sums the partials). pt4 runs every (slice, tile) in one
  // launch; other kernels run the slices one after another.
  int ksplit = 1;
  // MX block scales (optional, fp8 inputs; both or neither): one E8M0 byte (value 2^(s - 127))
  // per 32 consecutive K elements of a row, row-major [rows, K / 32] with a row stride of
  // a_scale_ld / b_scale_ld BYTES (a multiple of 4, base 4-byte aligned), so the four scales of a
  // row's 128-byte K-tile are one aligned 32-bit word. Null: unit scales, the kernels above.
  // DT_FP4 operands (E2M1, lda / ldb in ELEMENTS and even, K % 256 == 0) always carry scales, in
  // the same layout; base and row stride are then multiples of 8, so the eight scales of a row's
  // 128-byte K-tile (256 elements) are one aligned 64-bit load.
  const uint8_t* a_scale = nullptr;
  const uint8_t* b_scale = nullptr;
  int64_t a_scale_ld = 0, b_scale_ld = 0;
  // Quantised output (optional; dout = DT_FP8 / DT_FP4 and only then): the tiled kernel's
  // epilogue quantises act(acc) by the MX rule in 32-column blocks of a C row and writes c as
  // e4m3 bytes [M, N] (N % 128 == 0) or E2M1 nibble pairs [M, N / 2] (N % 256 == 0; ldc in
  // ELEMENTS and even) and the blocks' E8M0 bytes here, [M, N / 32] with rows c_scale_ld BYTES
  // apart: the layout the next GEMM reads as its A and a_scale. Plain C rows only.
  uint8_t* c_scale = nullptr;
  int64_t c_scale_ld = 0;
  // Gated (GLU) epilogue (optional; the tiled kernel, codes of mxs_offers()): b is [N, K] with
  // gate and up rows interleaved in groups of 32 (rows 64g .. 64g + 31 gate, 64g + 32 .. 64g + 63
  // the matching up rows) and c has N / 2 columns, c[i, 32g + j] = act(acc[i, 64g + j]) *
  // acc[i, 64g + 32 + j] in f32, then rounded to dout or quantised (c_scale: [M, N / 64]). N stays
  // the number of b rows; N % 64 == 0 (whole blocks as the reader takes them for a quantised
  // output: N % 256, fp4 N % 512); ldc >= N / 2. Plain rows only.
  int glu = 0;
  // Grouped form (optional; the tiled kernel, codes of mxs_offers()): grp_offs is a DEVICE array of
  // ngroups + 1 int32 row offsets, read by the kernel only (no host sync). Group g is rows
  // [o'[g], o'[g + 1]) of a, a_scale, c and c_scale and multiplies by the weight at
  // b + g * b_gstride ELEMENTS with the scales at b_scale + g * b_scale_gstride BYTES; every
  // flavour the tiled kernel has (dense, block-scaled, act, quantised output, glu) per group, bit
  // for bit what the ungrouped launch writes for those rows. M is the number of rows of a the
  // launch may touch (T). The offsets are clamped as they are read, o'[0] = clamp(o[0], 0, T),
  // o'[g + 1] = clamp(o[g + 1], o'[g], T): no content of the array addresses a row >= T, rows
  // outside [o'[0], o'[ngroups]) are not written, empty groups are legal anywhere.
  // 1 <= ngroups <= kMaxGroups. Plain rows only.
  const int* grp_offs = nullptr;
  int ngroups = 0;
  int64_t b_gstride = 0, b_scale_gstride = 0;
  // K-grouped form (optional; grp_offs / ngroups as above, block-scaled fp8 / fp4 operands, codes
  // of mxs_offers(), dense output): the groups lie along the CONTRACTION axis. With the offsets
  // clamped to kgrp_rows (T) as above, n_g = o'[g + 1] - o'[g] and MOD = 128 (fp4: 256) elements,
  // group g owns columns [k0_g, k0_g + kl_g) of a, b and (over 32) of both scale arrays,
  //   kl_g = MOD ceil(n_g / MOD),  k0_g = MOD sum_{j < g} ceil(n_j / MOD)   (tile_map.h),
  // and writes c + g * c_kgstride ELEMENTS: c[g] = a[:, cols g] b[:, cols g]^T, [M, N] with rows
  // ldc apart; a group without columns writes +0.0. K is the operands' column extent and is at
  // least kgrouped_capacity(T, ngroups, MOD), so no content of the offsets addresses a column
  // outside it. M and N are the ordinary extents of a and b here. The wgrad of a routed layer.
  int kgrouped = 0;
  int kgrp_rows = 0;
  int64_t c_kgstride = 0;
};
constexpr int kMaxGroups = 1024;
// The byte view of a launch whose operands and / or output are fp4: the kernels address bytes (two
// E2M1 elements each), so K, lda and ldb of fp4 operands and ldc of an fp4 output are halved.
// GemmArgs stay in ELEMENTS up to the launch entries (gemm_entry.h); the view is formed inside.
constexpr GemmArgs fp4_byte_view(GemmArgs p, bool fp4_in, bool fp4_out) {
  if (fp4_in) { p.K /= 2; p.lda /= 2; p.ldb /= 2; p.b_gstride /= 2; }
  if (fp4_out) p.ldc /= 2;
  return p;
}
enum Act : int { ACT_NONE = 0, ACT_GELU = 1, ACT_RELU = 2, ACT_SILU = 3 };
// In-kernel all-gather variants (GemmArgs::ag_mode bits; 0 = write-through publication, 8 loads
// in flight per lane, system-scope acquire in the GEMM gate; the plan builders pick the default,
// ddlb_amd/parallel/algorithms.py AlgoConfig.ag_mode).
enum AgMode : int {
  AG_LEGACY_PUBLISH = 1,   // plain stores + agent release fence per unit (the first version)
  AG_AGENT_ACQUIRE = 2,    // the gated tiles acquire at agent scope (flags set by this launch)
  AG_DEEP_LOADS = 4,       // 16 loads in flight per lane instead of 8
  AG_FILL_ROUNDS = 8,      // grow ag_ctas while the GEMM's number of tile rounds stays the same
  AG_WAIT_ACKS = 16,       // copy workgroup 0 waits for every peer's ACK before the launch ends
                           // (ag_tab then has np more entries: my local ACK word per producer)
};

// MX quantiser (csrc/gemm/mx_quant.hip): x[R, K] (f32 / f16 / bf16 rows, ldx ELEMENTS apart) ->
// q[R, K] e4m3 (rows ldq bytes apart) and s[R, K / 32] E8M0 bytes (rows lds bytes apart), one
// scale per 32 consecutive K elements: the smallest power of two 2^e with amax / 2^e <= 448
// (e clamped to [-127, 127], an all-zero block gets e = 0), s = e + 127, q = rne(x / 2^e).
// amax is taken over the finite elements; a NaN or +-Inf element becomes the e4m3fn NaN byte
// with its sign (fp4: the nibble 0x7 | sign << 3, and its block's scale byte 255).
// K % 128 == 0; x rows 16-byte and q rows 8-byte aligned (checked by the caller, and here).
struct MxQuantArgs {
  const void* x = nullptr;
  void* q = nullptr;
  uint8_t* s = nullptr;
  int64_t ldx = 0, ldq = 0, lds = 0;
  int R = 0, K = 0;
};
hipError_t mx_quantize_launch(const MxQuantArgs& a, int din, hipStream_t s);
// The MXFP4 flavour: q[R, K / 2] bytes of E2M1 nibble pairs (element 2j in the low nibble of byte
// j; rows ldq BYTES apart, 4-byte aligned), the same scale array; the rule with 6 in place of 448
// (e = ex - 3 if m <= 0.75 else ex - 2), ties to the even code. K % 256 == 0.
hipError_t mxfp4_quantize_launch(const MxQuantArgs& a, int din, hipStream_t s);
// The gathering flavour (a routed layer's dispatch): src is a DEVICE array of R int32 row indices
// and output row r is, byte for byte, what the launches above write for row src[r] of x[X, K];
// an index outside [0, X) gives a zero row (zero data, scale byte 127) and reads nothing, so no
// content of src addresses outside x. Either format (fp4: q[R, K / 2]); the same alignment and
// K % 128 (fp4: 256) rules. R == 0 launches nothing.
struct MxQuantGatherArgs {
  const void* x = nullptr;
  void* q = nullptr;
  uint8_t* s = nullptr;
  const int* src = nullptr;
  int64_t ldx = 0, ldq = 0, lds = 0;
  int R = 0, K = 0, X = 0;
};
hipError_t mx_quantize_gather_launch(const MxQuantGatherArgs& a, int din, bool fp4,
                                     hipStream_t s);

// Transposing MX quantiser (csrc/gemm/mx_quant_t.hip): x[R, C] (rows ldx ELEMENTS apart) ->
// qt[C, R] e4m3 (fp4: [C, R / 2] nibble pairs; rows ldqt BYTES apart) and st[C, R / 32] E8M0
// bytes (rows ldst bytes apart). A block is x[32 b .. 32 b + 31, c]: the result is the row-wise
// quantisation of x.T, byte for byte, for a GEMM that contracts over R.
// R % 128 == 0 (fp4: 256); C * element size % 16 == 0; x and qt rows 16-byte aligned; st base
// and ldst multiples of 4 (fp4: 8). R == 0 or C == 0 launches nothing.
// two = true: the same pass also writes the row-wise pair q[R, C] (fp4: [R, C / 2]; rows ldq
// bytes apart, 8-byte aligned, fp4: 4) and s[R, C / 32], as mx_quantize_launch would;
// C % 128 == 0 (fp4: 256) then. q and s are not read otherwise.
struct MxQuantTArgs {
  const void* x = nullptr;
  void* qt = nullptr;
  uint8_t* st = nullptr;
  void* q = nullptr;
  uint8_t* s = nullptr;
  int64_t ldx = 0, ldqt = 0, ldst = 0, ldq = 0, lds = 0;
  int R = 0, C = 0;
};
hipError_t mx_quantize_t_launch(const MxQuantTArgs& a, int din, bool fp4, bool two,
                                hipStream_t s);

// Grouped transposing MX quantiser (csrc/gemm/mx_quant_t.hip, the grouped form): x[T, C], sorted
// into ngroups groups by the DEVICE array offs (ngroups + 1 int32, clamped to T as a grouped GEMM
// clamps them, read by the kernel only) -> qt[C, cap] (fp4: [C, cap / 2]) and st[C, cap / 32],
// cap = kgrouped_capacity(T, ngroups, MOD), MOD = 128 (fp4: 256): columns [k0_g, k0_g + kl_g) of
// row c hold the blocks of x[o'[g] : o'[g + 1], c], zero-extended to kl_g rows (tile_map.h
// kgrouped_range has the layout), i.e. mx_quantize_t_launch of the group's rows padded with zero
// rows, byte for byte: the operands of a K-grouped GEMM. Columns at or past k0_E are not written.
// stacked_rows = R > 0 (R % MOD == 0): group g goes to the slab qt + g * qt_gstride /
// st + g * st_gstride BYTES instead, from column 0 of the slab, [C, R] / [C, R / 32]; a tile of
// the group at or past row R is dropped. Alignment as for mx_quantize_t_launch; ldqt / ldst hold
// the capacity (stacked: R); 1 <= ngroups <= kMaxGroups. T == 0 or C == 0 launches nothing.
struct MxQuantTGroupedArgs {
  const void* x = nullptr;
  void* qt = nullptr;
  uint8_t* st = nullptr;
  const int* offs = nullptr;
  int64_t ldx = 0, ldqt = 0, ldst = 0;
  int64_t qt_gstride = 0, st_gstride = 0;
  int T = 0, C = 0, ngroups = 0, stacked_rows = 0;
};
hipError_t mx_quantize_t_grouped_launch(const MxQuantTGroupedArgs& a, int din, bool fp4,
                                        hipStream_t s);

hipError_t gemm_launch(const GemmArgs& p, int din, int dout, int tile, int mode, hipStream_t s);
bool gemm_fast_path_ok(const GemmArgs& p, int din, int dout);
int choose_tile(int64_t M, int64_t N, int64_t K, int din);
int tile_rows(int tile);
int tile_cols(int tile);

}  // namespace ddlb
