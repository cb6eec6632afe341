// The tiled W4A8 kernel (device code, header-only): MX-fp8 A on MXFP4 W for prefill shapes.
// Included by gemm_w4a8.hip (dense outputs), gemm_w4a8_q.hip (MX-fp8 output, plain and grouped)
// and gemm_w4a8_grouped.hip (dense outputs, grouped). gemm_w4a8.h has the interface.
//
// Geometry. A workgroup owns a BM x BN tile of C, 256x128 on 8 waves (4 x 2) or 128x128 on 4
// (2 x 2); every wave owns 64x64: MR = NR = 4 fragments of 16x16, 16 accumulator quads. A K-tile
// is 128 K elements: 128 bytes of an A row (e4m3) and 64 bytes of a W row (E2M1 pairs), and one
// v_mfma_scale_f32_16x16x128_f8f6f4 with format codes 4 (W, first operand) and 0 (A) per fragment
// pair (MmaMX84S::step48s), 16 per wave per K-tile.
//
// Staging. Both operands go global -> LDS by LDS-DMA (global_load_lds_dwordx4: 64 lanes x 16
// bytes = 1 KiB, written lane-contiguously), NS stages of BM * 128 + BN * 64 bytes.
//   A: eight 128-byte rows per instruction, lane l -> row l >> 3, LDS slot l & 7, which holds the
//      row's chunk (l & 7) ^ ((row >> 1) & 7): the tiled kernel's layout. Lane (frow, fq) reads
//      chunks fq and 4 + fq of its row: the fp8 K order of the scaled MFMA (eight registers).
//   W: sixteen 64-byte rows per instruction, lane l -> row l >> 2, LDS slot l & 3, which holds
//      the row's chunk (l & 3) ^ ((row >> 2) & 3). Lane (frow, fq) reads the ONE chunk fq of its
//      row, a whole 32-element block: the first four registers of the fp4 operand.
// The permutation sits on the global-address side (which 16 bytes a lane fetches), because the
// DMA's LDS side is fixed: lane-contiguous, 256 dwords over the 64 banks four times, no conflict.
// The ds_read_b128 side, by counting banks (64 banks x 4 bytes = a 256-byte bank row, 16 lanes of
// 16 bytes per pass, lanes 16 g .. 16 g + 15 together, i.e. all frow of one fq: the model under
// which the tiled kernel's (row >> 1) & 7 was measured at 0 conflicts): a W row is 64 bytes, so
// rows r, r + 4, r + 8, r + 12 of a fragment start on the same 16 banks and the 16-byte slot
// within the bank row is 4 (frow & 3) + (fq ^ x(frow)). With x = frow >> 2 the four rows that
// share banks take four different slots: frow -> 4 (frow & 3) + (fq ^ (frow >> 2)) is a bijection
// of 0..15 for every fq, one lane per 4-bank group, no conflict. (Unpermuted, x = 0, it is a 4-way
// conflict: four rows x the same slot.) Counted, not measured with the LDS conflict counter.
//
// Scales. One 32-bit word (four E8M0 bytes) per row per K-tile and operand, loaded from global
// memory beside the DMA of its K-tile and first touched after the wait that covers it; lane
// (frow, fq) supplies byte fq of its row's word for both operands. Rows are clamped to M - 1 /
// N - 1 for data and scales alike; only stores are predicated.
//
// K loop. K % 256 == 0, so the number of K-tiles is even and at least 2; the loop is unrolled by
// two and the scale words of the K-tiles in flight sit in registers with static indices. NS = 2:
// the tiled kernel's loop (stage kt + 1, compute kt, vmcnt(0), barrier). NS = 3: two K-tiles in
// flight; every wave issues the same PER = LA + LW + 8 vector-memory instructions per K-tile, they
// complete in order, so vmcnt(PER) at the end of iteration kt means "K-tile kt + 1 has landed".
#pragma once
#include "gemm_kernels.h"
#include "gemm_w4a8.h"

namespace ddlb {
namespace {

// The grouped form's prologue (the contract of gemm_grouped: tile_map.h grouped_tile): the launch's
// arguments re-based to the workgroup's group, 64-bit arithmetic on uniform values; false for the
// surplus of the grid bound (the kernel returns before any barrier or LDS-DMA). pl is the byte
// view: lda, ldb, b_gstride in bytes; a quantised output's ldc in bytes (CSZ = 1).
template <int BM, int BN, int CSZ>
__device__ __forceinline__ bool w4a8_grouped_args(const GemmArgs& pl, GemmArgs& pg, int& wg) {
  const int tiles_n = (pl.N + BN - 1) / BN;
  GroupTile t;
  if (!grouped_tile(pl.grp_offs, pl.M, pl.ngroups, BM, tiles_n,
                    xcd_remap((int)blockIdx.x, (int)gridDim.x), t))
    return false;
  pg = pl;
  pg.a = (const char*)pl.a + (int64_t)t.row0 * pl.lda;
  pg.b = (const char*)pl.b + (int64_t)t.g * pl.b_gstride;
  pg.c = (char*)pl.c + (int64_t)t.row0 * pl.ldc * CSZ;
  pg.a_scale = pl.a_scale + (int64_t)t.row0 * pl.a_scale_ld;
  pg.b_scale = pl.b_scale + (int64_t)t.g * pl.b_scale_gstride;
  if (pl.c_scale != nullptr) pg.c_scale = pl.c_scale + (int64_t)t.row0 * pl.c_scale_ld;
  pg.M = t.rows;
  wg = t.tm * tiles_n + t.tn;
  return true;
}

// Two waves per SIMD (at most 256 registers): what the 8-wave tile needs to be resident at all,
// and two workgroups of the 4-wave tile per CU (left alone the compiler takes 190 VGPRs + 72
// AGPRs for it, one wave per SIMD). No instantiation spills under it.
template <int OUT, int BM, int BN, int WM, int WN, bool GLU, bool GROUPED, int NS = kW4A8Stages>
__global__ __launch_bounds__(WM* WN * 64) __attribute__((amdgpu_waves_per_eu(2)))
void gemm_w4a8_kernel(const GemmArgs p_launch) {
  constexpr bool QOUT = OUT == DT_FP8;
  constexpr int OSZ = QOUT ? 1 : out_size<OUT>();
  [[maybe_unused]] GemmArgs p_group;
  [[maybe_unused]] int wg_group;
  if constexpr (GROUPED) {
    if (!w4a8_grouped_args<BM, BN, OSZ>(p_launch, p_group, wg_group)) return;
  }
  const GemmArgs& p = GROUPED ? p_group : p_launch;
  constexpr int NW = WM * WN;
  constexpr int A_ROWB = 128, W_ROWB = 64;  // bytes of a row per K-tile
  constexpr int A_BYTES = BM * A_ROWB, W_BYTES = BN * W_ROWB, STAGE = A_BYTES + W_BYTES;
  constexpr int TM = BM / WM, TN = BN / WN, MR = TM / 16, NR = TN / 16;
  constexpr int LA = BM / 8 / NW, LW = BN / 16 / NW;  // LDS-DMA instructions per wave per K-tile
  static_assert(MR == 4 && NR == 4, "64x64 per wave");
  static_assert(LA * NW * 8 == BM && LW * NW * 16 == BN, "tile rows must split over waves");
  static_assert(STAGE % 1024 == 0, "stages keep the DMA's 1 KiB alignment");
  __shared__ __attribute__((aligned(1024))) char smem[NS * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
  const int wg = GROUPED ? wg_group : xcd_remap((int)blockIdx.x, tiles_m * tiles_n);
  const int tm = wg / tiles_n, tn = wg % tiles_n;
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;

  // Per-lane source pointers of the rows this wave stages (the permutations: see the top).
  const char* aptr[LA];
  const char* wptr[LW];
#pragma unroll
  for (int i = 0; i < LA; ++i) {
    const int row = (wave * LA + i) * 8 + (lane >> 3);
    int64_t gr = m0 + row;
    gr = gr < p.M ? gr : p.M - 1;
    aptr[i] = (const char*)p.a + gr * p.lda + ((lane & 7) ^ ((row >> 1) & 7)) * 16;
  }
#pragma unroll
  for (int i = 0; i < LW; ++i) {
    const int row = (wave * LW + i) * 16 + (lane >> 2);
    int64_t gr = n0 + row;
    gr = gr < p.N ? gr : p.N - 1;
    wptr[i] = (const char*)p.b + gr * p.ldb + ((lane & 3) ^ ((row >> 2) & 3)) * 16;
  }
  auto stage = [&](int buf, int kt) __attribute__((always_inline)) {
    char* base = smem + buf * STAGE;
#pragma unroll
    for (int i = 0; i < LA; ++i)
      glds16(aptr[i] + (int64_t)kt * A_ROWB, base + (wave * LA + i) * 1024);
#pragma unroll
    for (int i = 0; i < LW; ++i)
      glds16(wptr[i] + (int64_t)kt * W_ROWB, base + A_BYTES + (wave * LW + i) * 1024);
  };

  const int wm = wave / WN, wn = wave % WN;
  const int frow = lane & 15, fq = lane >> 4;
  f32x4 acc[MR][NR];
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j < NR; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // Scale rows: 32-bit byte offsets from the (group's) base, kept in range by the host's gate
  // rows * scale_ld < 2^31. LEAD sets of words in flight, one per K-tile of DMA lead.
  constexpr int LEAD = NS - 1;
  constexpr int PER = LA + LW + MR + NR;  // vector-memory instructions per wave per K-tile
  unsigned sa_off[MR], sw_off[NR];
  unsigned sa_w[LEAD][MR], sw_w[LEAD][NR];
  int sa[MR], sw[NR];
#pragma unroll
  for (int i = 0; i < MR; ++i) {
    int64_t gr = m0 + wm * TM + i * 16 + frow;
    gr = gr < p.M ? gr : p.M - 1;
    sa_off[i] = (unsigned)(gr * p.a_scale_ld);
  }
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    int64_t gr = n0 + wn * TN + j * 16 + frow;
    gr = gr < p.N ? gr : p.N - 1;
    sw_off[j] = (unsigned)(gr * p.b_scale_ld);
  }
  auto issue = [&](int kt, auto slot) __attribute__((always_inline)) {
    constexpr int S = decltype(slot)::value;
    stage(kt % NS, kt);
    const GLB_AS char* ga = (const GLB_AS char*)p.a_scale + kt * 4;
    const GLB_AS char* gw = (const GLB_AS char*)p.b_scale + kt * 4;
#pragma unroll
    for (int i = 0; i < MR; ++i) sa_w[S][i] = *(const GLB_AS unsigned*)(ga + sa_off[i]);
#pragma unroll
    for (int j = 0; j < NR; ++j) sw_w[S][j] = *(const GLB_AS unsigned*)(gw + sw_off[j]);
  };
  auto take_scales = [&](auto slot) __attribute__((always_inline)) {
    constexpr int S = decltype(slot)::value;
    // (the fences keep these uses between the barrier and the next stage's DMA)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < MR; ++i) sa[i] = (int)__builtin_amdgcn_ubfe(sa_w[S][i], fq * 8, 8);
#pragma unroll
    for (int j = 0; j < NR; ++j) sw[j] = (int)__builtin_amdgcn_ubfe(sw_w[S][j], fq * 8, 8);
    __builtin_amdgcn_sched_barrier(0);
  };

  const int a_c0 = (fq ^ (frow >> 1)) * 16, a_c1 = ((4 + fq) ^ (frow >> 1)) * 16;
  const int w_c = (fq ^ (frow >> 2)) * 16;
  auto compute = [&](int buf) __attribute__((always_inline)) {
    const char* As = smem + buf * STAGE + (wm * TM + frow) * A_ROWB;
    const char* Ws = smem + buf * STAGE + A_BYTES + (wn * TN + frow) * W_ROWB + w_c;
    i32x8 af[MR];
    i32x4 wf[NR];
#pragma unroll
    for (int i = 0; i < MR; ++i) {
      const i32x4 lo = *(const i32x4*)(As + i * 16 * A_ROWB + a_c0);
      const i32x4 hi = *(const i32x4*)(As + i * 16 * A_ROWB + a_c1);
      af[i] = i32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) wf[j] = *(const i32x4*)(Ws + j * 16 * W_ROWB);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
      for (int j = 0; j < NR; ++j) MmaMX84S::step48s(acc[i][j], wf[j], af[i], sw[j], sa[i]);
    __builtin_amdgcn_s_setprio(0);
  };
  // One K-tile: its scales, the DMA of K-tile kt + LEAD into the buffer iteration kt - 1 read
  // (every wave is past that iteration's barrier), the MFMAs, then the wait for K-tile kt + 1.
  auto step = [&](int kt, auto slot, bool more) __attribute__((always_inline)) {
    take_scales(slot);
    if (more) issue(kt + LEAD, slot);
    compute(kt % NS);
    if (more) wait_vm<(LEAD - 1) * PER>();
    else wait_vm<0>();
    __builtin_amdgcn_s_barrier();
  };
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1 % LEAD>;

  const int nk = p.K / 128;  // even, >= 2
  issue(0, S0{});
  if constexpr (LEAD == 2) issue(1, S1{});
  wait_vm<(LEAD - 1) * PER>();
  __builtin_amdgcn_s_barrier();
  int kt = 0;
  for (; kt < nk - 2; kt += 2) {
    step(kt, S0{}, true);
    step(kt + 1, S1{}, true);
  }
  step(kt, S0{}, LEAD == 1);
  take_scales(S1{});
  compute((kt + 1) % NS);

  // Epilogue: lane holds C[row = .. + frow][col = .. + 4 fq + r], r = 0..3, of fragment (i, j).
  if constexpr (QOUT) {
    // MX-fp8 output (GemmArgs::c_scale): a block is 32 consecutive columns of a C row, fragments
    // 2b, 2b + 1 (gated: the products of 4b, 4b + 1 with 4b + 2, 4b + 3) of the four lanes
    // frow + 16 g: the lane's 8 values, then a max across lanes ^16 and ^32. Every lane takes
    // part (rows are clamped, only the stores are predicated); a block is wholly inside or
    // outside N. ldc in BYTES. The rule and the conversions: mx_cvt.h.
#pragma unroll
    for (int i = 0; i < MR; ++i) {
      const int64_t row = m0 + wm * TM + i * 16 + frow;
      const bool rok = row < p.M;
      const int64_t rc = rok ? row : p.M - 1;
      char* crow = (char*)p.c + rc * p.ldc;
      uint8_t* srow = p.c_scale + rc * p.c_scale_ld;
      auto block = [&](const f32x4 v0, const f32x4 v1, const int64_t col, const bool ok)
                       __attribute__((always_inline)) {
        const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        unsigned m = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) m = mx_amax_join<false>(m, mx_amax_bits<false>(v[r]));
#pragma unroll
        for (int d = 16; d <= 32; d *= 2) m = mx_amax_join<false>(m, (unsigned)__shfl_xor((int)m, d));
        const int e = mx_scale_exp<false>(m);
        const unsigned w0 = mx_cvt4_e4m3(v[0], v[1], v[2], v[3], e);
        const unsigned w1 = mx_cvt4_e4m3(v[4], v[5], v[6], v[7], e);
        if (ok) {
          *(unsigned*)(crow + col + fq * 4) = w0;
          *(unsigned*)(crow + col + 16 + fq * 4) = w1;
          if (fq == 0) srow[col / 32] = (uint8_t)mx_scale_byte<false>(m, e);
        }
      };
      if constexpr (GLU) {
        const int64_t col = (n0 + wn * TN) / 2;
        block(act4(acc[i][0], p.act) * acc[i][2], act4(acc[i][1], p.act) * acc[i][3], col,
              rok && 2 * col < p.N);
      } else {
#pragma unroll
        for (int b = 0; b < NR / 2; ++b) {
          const int64_t col = n0 + wn * TN + b * 32;
          block(act4(acc[i][2 * b], p.act), act4(acc[i][2 * b + 1], p.act), col,
                rok && col < p.N);
        }
      }
    }
  } else {
    // four columns per store where every C row is 8-byte aligned, else one by one (uniform)
    const bool vec = (((uintptr_t)p.c | (uint64_t)(p.ldc * OSZ)) & 7) == 0;
    auto store4 = [&](char* crow, const int64_t col, const int64_t ncols, const f32x4 v4)
                      __attribute__((always_inline)) {
      if (vec && col + 3 < ncols) {
        Store4<OUT>::st(crow + col * OSZ, v4);
      } else {
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
        for (int r = 0; r < 4; ++r)
          if (col + r < ncols) Store4<OUT>::st1(crow + (col + r) * OSZ, v[r]);
      }
    };
#pragma unroll
    for (int i = 0; i < MR; ++i) {
      const int64_t row = m0 + wm * TM + i * 16 + frow;
      if (row >= p.M) continue;
      char* crow = (char*)p.c + row * p.ldc * OSZ;
      if constexpr (GLU) {
        // Gated: the wave's 64 columns are 32 gate and the 32 matching up columns; fragments h
        // (gate) and 2 + h (up) of the same lane give 4 of the N / 2 output columns. N % 64 == 0:
        // the group is wholly inside or outside.
        if (n0 + wn * TN >= p.N) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int64_t col = (n0 + wn * TN) / 2 + h * 16 + fq * 4;
          store4(crow, col, p.N / 2, act4(acc[i][h], p.act) * acc[i][2 + h]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < NR; ++j)
          store4(crow, n0 + wn * TN + j * 16 + fq * 4, p.N, act4(acc[i][j], p.act));
      }
    }
  }
}

// The one launch site: the byte view of W (two E2M1 elements per byte), the tile code's geometry,
// plain or grouped grid (grouped: the bound of tile_map.h, which gemm_w4a8_launch has checked to be
// a grid). A code that w4a8_offers() does not list is hipErrorInvalidValue.
template <int OUT, bool GROUPED>
hipError_t launch_w4a8_t(const GemmArgs& p_in, int tile, hipStream_t s) {
  GemmArgs p = p_in;
  p.ldb /= 2;
  p.b_gstride /= 2;
  auto go = [&](auto bm, auto glu) {
    constexpr int BM = decltype(bm)::value, WM = BM / 64;
    constexpr bool GLU = decltype(glu)::value;
    const int tiles_n = (p.N + 127) / 128;
    const int64_t grid = GROUPED ? grouped_grid_bound(p.M, p.ngroups, BM, tiles_n)
                                 : (int64_t)((p.M + BM - 1) / BM) * tiles_n;
    hipLaunchKernelGGL((gemm_w4a8_kernel<OUT, BM, 128, WM, 2, GLU, GROUPED>), dim3((unsigned)grid),
                       dim3(WM * 2 * 64), 0, s, p);
    return hipGetLastError();
  };
  auto by_glu = [&](auto bm) {
    return p.glu ? go(bm, std::true_type{}) : go(bm, std::false_type{});
  };
  if (tile == TILE_256x128) return by_glu(std::integral_constant<int, 256>{});
  if (tile == TILE_128x128) return by_glu(std::integral_constant<int, 128>{});
  return hipErrorInvalidValue;
}

}  // namespace
}  // namespace ddlb
