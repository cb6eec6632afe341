// The tiled A16 kernel (device code, header-only): bf16 / f16 A on MXFP4 or MX-fp8 W for prefill
// shapes. Included by gemm_a16.hip (dense form) and gemm_a16_grouped.hip (grouped form).
// gemm_a16.h has the interface.
//
// Geometry: the W4A8 kernel's (gemm_w4a8_kernels.h). A workgroup owns a BM x 128 tile of C, 128x128
// on 4 waves (2 x 2) or 256x128 on 8 (4 x 2); every wave owns 64x64: MR = NR = 4 fragments of
// 16x16, 16 accumulator quads. A K-tile is 128 K elements: 256 bytes of an A row, 64 (fp4) or 128
// (fp8) bytes of a W row and one 32-bit word of W's scales, and four v_mfma_f32_16x16x32 per
// fragment pair, 64 per wave.
//
// Staging. Both operands go global -> LDS by LDS-DMA (glds16: 64 lanes x 16 bytes = 1 KiB,
// lane-contiguous), W still packed; two stages of BM * 256 + 128 * 64 (fp4) / 128 * 128 (fp8).
//   W, fp4: the W4A8 kernel's W staging. Sixteen 64-byte rows per instruction, LDS slot l & 3 of
//      row l >> 2 holds the row's chunk (l & 3) ^ ((row >> 2) & 3); lane (frow, fq) reads the one
//      chunk fq of its row.
//   W, fp8: the W4A8 kernel's A staging. Eight 128-byte rows per instruction, slot l & 7 of row
//      l >> 3 holds chunk (l & 7) ^ ((row >> 1) & 7); lane (frow, fq) reads chunks fq and 4 + fq.
//   A: two 128-byte K-rows per row and K-tile, kept as two planes [kp][BM rows][128 bytes], each
//      staged like the fp8 W: slot l & 7 of row l >> 3 holds chunk (l & 7) ^ ((row >> 1) & 7) ^
//      2 kp. The K-row parity term is the skinny A16 kernel's: the fp4 form's lane groups fq and
//      fq ^ 2 read the same chunk of adjacent K-rows, which would otherwise be the same banks.
// The permutations sit on the global-address side (the DMA's LDS side is lane-contiguous). Bank
// counting of the ds_read_b128 side for both W maps: gemm_w4a8_kernels.h. For A, the 16 lanes of
// one fq share kp and the chunk ch, a 256-byte bank row holds rows 2 r and 2 r + 1, and lane frow
// reads its 16-byte slot 8 (frow & 1) + (ch ^ 2 kp ^ (frow >> 1)): sixteen different slots, no
// conflict. Counted, not measured with the LDS conflict counter.
//
// Expansion: in registers, once per wave per K-tile. v_mfma_f32_16x16x32 takes K elements
// 8 g .. 8 g + 7 from lane group g of both operands, so any assignment of K elements to (MFMA,
// lane group, slot) is right as long as W and A use the same one; W's is given by how a lane reads
// it (the skinny A16 kernel's map, gemm_skinny_a16.hip, for one chunk per h):
//   fp4: chunk fq is elements 32 fq .. 32 fq + 31, one scale block, byte fq of the row's word.
//        Dword t of it is MFMA t's operand (4 v_cvt_scalef32_pk_*_fp4, one per byte); its A
//        fragment is K-row fq >> 1, chunk 4 (fq & 1) + t.
//   fp8: chunk 4 h + fq (h = 0, 1) is 16 elements of block 2 h + (fq >> 1), that byte of the word.
//        Dwords 2 t, 2 t + 1 are MFMA 2 h + t's operand (4 v_cvt_scalef32_pk_*_fp8, one per half
//        dword); its A fragment is K-row h, chunk 2 fq + t.
// The scale operand is the f32 2^(s - 127) built as s << 23. Each expanded W fragment (4 VGPRs)
// is used by the wave's four A fragments: one packed conversion per MFMA issued.
//
// Scale byte 255: the conversion is given the f32 Inf for it and what it returns is not relied
// on. Every lane keeps the largest scale byte its W rows met, and the epilogue sets the output
// columns of every W row that met 255 to NaN (a ballot: W row r's bytes live in the lanes with
// frow = r, its column in lane group r >> 2). e4m3 NaN bytes and NaN / Inf of A go through the
// conversion and the MFMA as values.
//
// K loop: any number of K-tiles >= 1 (MX-fp8 allows K = 128). Two stages: stage kt + 1, compute
// kt, vmcnt(0), barrier; the scale words of K-tile kt + 1 are loaded beside its DMA and turned
// into the f32 operands after the barrier, before the next DMA is issued.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; the 64 instantiations: bf16 and
// f16, dense and grouped, plain and gated, both outputs): no scratch and no spills anywhere.
//                   VGPRs        AGPRs   LDS (two stages)   waves per SIMD
//   fp4  128x128    162 .. 166     0      80 KiB            2 (two workgroups per CU)
//   fp4  256x128    160 .. 164     0     144 KiB            2 (one 8-wave workgroup)
//   fp8  128x128    121 .. 125    64      96 KiB            1 (LDS: one 4-wave workgroup per CU)
//   fp8  256x128    182 .. 186     0     160 KiB            2 (one 8-wave workgroup)
// The fp8 form at 128x128 is held to one wave per SIMD by its LDS, not by registers, and is
// built for that (the compiler then parks the accumulators in AGPRs).
#pragma once
#include "gemm_a16.h"
#include "gemm_a16_ops.h"
#include "gemm_w4a8_kernels.h"

namespace ddlb {
namespace {

// Two waves per SIMD (at most 256 registers): what the 8-wave tile needs to be resident at all;
// one where the LDS allows no more (fp8 at 128x128).
// GROUPED: the prologue of the W4A8 kernel (w4a8_grouped_args; there is no a_scale to re-base).
template <bool FP4, int DT, int OUT, int BM, int BN, int WM, int WN, bool GLU, bool GROUPED>
__global__ __launch_bounds__(WM* WN * 64)
__attribute__((amdgpu_waves_per_eu(FP4 || BM == 256 ? 2 : 1)))
void gemm_a16_kernel(const GemmArgs p_launch) {
  using Ops = A16Ops<DT>;
  static_assert(OUT == DT || OUT == DT_F32, "the output is a's dtype or f32");
  constexpr int OSZ = out_size<OUT>();
  [[maybe_unused]] GemmArgs p_group;
  [[maybe_unused]] int wg_group;
  if constexpr (GROUPED) {
    if (!w4a8_grouped_args<BM, BN, OSZ>(p_launch, p_group, wg_group)) return;
  }
  const GemmArgs& p = GROUPED ? p_group : p_launch;
  constexpr int NW = WM * WN, NS = 2;
  constexpr int A_ROWB = 128, W_ROWB = FP4 ? 64 : 128;  // bytes of an A K-row, of a W row per K-tile
  constexpr int A_PLANE = BM * A_ROWB, A_BYTES = 2 * A_PLANE, W_BYTES = BN * W_ROWB;
  constexpr int STAGE = A_BYTES + W_BYTES;
  constexpr int WROWS = 1024 / W_ROWB;  // W rows per LDS-DMA instruction
  constexpr int TM = BM / WM, TN = BN / WN, MR = TM / 16, NR = TN / 16;
  constexpr int LA = 2 * BM / 8 / NW, LW = BN / WROWS / NW;  // LDS-DMA instructions per wave
  constexpr int NH = FP4 ? 1 : 2;                            // W chunks per lane and fragment
  static_assert(MR == 4 && NR == 4, "64x64 per wave");
  static_assert(LA * NW * 8 == 2 * BM && LW * NW * WROWS == BN, "tile rows must split over waves");
  static_assert(NS * STAGE <= 160 * 1024, "two stages fit the CU's LDS");
  __shared__ __attribute__((aligned(1024))) char smem[NS * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
  const int wg = GROUPED ? wg_group : xcd_remap((int)blockIdx.x, tiles_m * tiles_n);
  const int tm = wg / tiles_n, tn = wg % tiles_n;
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;

  // Per-lane source pointers of the rows this wave stages (the permutations: see the top). A's
  // instruction q of a K-tile is row block q >> 1, K-row q & 1.
  const char* aptr[LA];
  const char* wptr[LW];
#pragma unroll
  for (int i = 0; i < LA; ++i) {
    const int q = wave * LA + i, kp = q & 1, row = (q >> 1) * 8 + (lane >> 3);
    int64_t gr = m0 + row;
    gr = gr < p.M ? gr : p.M - 1;
    aptr[i] = (const char*)p.a + gr * p.lda + kp * A_ROWB +
              ((lane & 7) ^ ((row >> 1) & 7) ^ (kp << 1)) * 16;
  }
#pragma unroll
  for (int i = 0; i < LW; ++i) {
    const int row = (wave * LW + i) * WROWS + (FP4 ? lane >> 2 : lane >> 3);
    int64_t gr = n0 + row;
    gr = gr < p.N ? gr : p.N - 1;
    const int chunk = FP4 ? (lane & 3) ^ ((row >> 2) & 3) : (lane & 7) ^ ((row >> 1) & 7);
    wptr[i] = (const char*)p.b + gr * p.ldb + chunk * 16;
  }
  auto stage = [&](int buf, int kt) __attribute__((always_inline)) {
    char* base = smem + buf * STAGE;
#pragma unroll
    for (int i = 0; i < LA; ++i) {
      const int q = wave * LA + i;
      glds16(aptr[i] + (int64_t)kt * (2 * A_ROWB), base + (q & 1) * A_PLANE + (q >> 1) * 1024);
    }
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

  // W's scale rows: 32-bit byte offsets from the (group's) base, kept in range by the host's gate
  // N * b_scale_ld < 2^31. One set of words in flight, for the K-tile the DMA is fetching.
  unsigned sw_off[NR], sw_w[NR], smax[NR];
  float sc[NH][NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    int64_t gr = n0 + wn * TN + j * 16 + frow;
    gr = gr < p.N ? gr : p.N - 1;
    sw_off[j] = (unsigned)(gr * p.b_scale_ld);
    smax[j] = 0;
  }
  auto issue = [&](int kt) __attribute__((always_inline)) {
    stage(kt % NS, kt);
    const GLB_AS char* gw = (const GLB_AS char*)p.b_scale + kt * 4;
#pragma unroll
    for (int j = 0; j < NR; ++j) sw_w[j] = *(const GLB_AS unsigned*)(gw + sw_off[j]);
  };
  // this lane's scale bytes of the K-tile that has landed: the f32 operands, and the running
  // maximum (the fences keep these uses between the barrier and the next stage's DMA)
  auto take_scales = [&]() __attribute__((always_inline)) {
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int h = 0; h < NH; ++h)
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        const unsigned b = __builtin_amdgcn_ubfe(sw_w[j], (FP4 ? fq : 2 * h + (fq >> 1)) * 8, 8);
        smax[j] = b > smax[j] ? b : smax[j];
        sc[h][j] = __builtin_bit_cast(float, b << 23);
      }
    __builtin_amdgcn_sched_barrier(0);
  };

  const int swz = (frow >> 1) & 7;  // (row >> 1) & 7 of every fragment's row frow
  const int w_c0 = FP4 ? (fq ^ (frow >> 2)) * 16 : (fq ^ swz) * 16;
  const int w_c1 = ((4 + fq) ^ swz) * 16;  // (fp8 only)
  auto compute = [&](int buf) __attribute__((always_inline)) {
    const char* As = smem + buf * STAGE + (wm * TM + frow) * A_ROWB;
    const char* Ws = smem + buf * STAGE + A_BYTES + (wn * TN + frow) * W_ROWB;
    i32x4 raw[NH][NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      raw[0][j] = *(const i32x4*)(Ws + j * 16 * W_ROWB + w_c0);
      if constexpr (!FP4) raw[NH - 1][j] = *(const i32x4*)(Ws + j * 16 * W_ROWB + w_c1);
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      // this chunk's place in A: K-row, and the chunk of MFMA 0
      const int kp = FP4 ? fq >> 1 : h, ch0 = FP4 ? 4 * (fq & 1) : 2 * fq;
      const char* ap = As + kp * A_PLANE;
      const int px = swz ^ (kp << 1);
#pragma unroll
      for (int t = 0; t < 4 / NH; ++t) {
        i32x4 wf[NR], af[MR];
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          if constexpr (FP4)
            wf[j] = a16_expand_fp4<DT>((unsigned)raw[h][j][t], sc[h][j]);
          else
            wf[j] = a16_expand_fp8<DT>((unsigned)raw[h][j][2 * t], (unsigned)raw[h][j][2 * t + 1],
                                       sc[h][j]);
        }
#pragma unroll
        for (int i = 0; i < MR; ++i)
          af[i] = *(const i32x4*)(ap + i * 16 * A_ROWB + ((ch0 + t) ^ px) * 16);
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
          for (int j = 0; j < NR; ++j) Ops::Mma::step(acc[i][j], wf[j], af[i]);
      }
    }
    __builtin_amdgcn_s_setprio(0);
  };

  // One K-tile: its scales, the DMA of K-tile kt + 1 into the buffer iteration kt - 1 read (every
  // wave is past that iteration's barrier), the MFMAs, then the wait for K-tile kt + 1.
  const int nk = p.K / 128;  // >= 1
  issue(0);
  wait_vm<0>();
  __builtin_amdgcn_s_barrier();
  for (int kt = 0; kt < nk; ++kt) {
    take_scales();
    if (kt + 1 < nk) issue(kt + 1);
    compute(kt % NS);
    wait_vm<0>();  // (and never leave an LDS-DMA in flight past the end of the workgroup)
    __builtin_amdgcn_s_barrier();
  }

  // scale byte 255: NaN in the output columns of the W rows that met it. W row frow of fragment j
  // lives in the four lanes (frow, *); this lane stores columns 4 fq .. 4 fq + 3 of the fragment.
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const unsigned long long b = __builtin_amdgcn_ballot_w64(smax[j] == 255u);
    const unsigned rows = (unsigned)(b | (b >> 16) | (b >> 32) | (b >> 48)) & 0xffffu;
    if (rows != 0) {  // (uniform)
      const unsigned mine = rows >> (4 * fq);
      const float nan = __builtin_nanf("");
#pragma unroll
      for (int i = 0; i < MR; ++i) {
        if (mine & 1) acc[i][j].x = nan;
        if (mine & 2) acc[i][j].y = nan;
        if (mine & 4) acc[i][j].z = nan;
        if (mine & 8) acc[i][j].w = nan;
      }
    }
  }

  // Epilogue: lane holds C[row = .. + frow][col = .. + 4 fq + r], r = 0..3, of fragment (i, j).
  // Four columns per store where every C row is 8-byte aligned, else one by one (uniform).
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

// The one launch site. p: the byte view gemm_a16_launch forms (lda, ldb, b_gstride in bytes). The
// tile code's geometry, plain or grouped grid (grouped: the bound of tile_map.h, which
// gemm_a16_launch has checked to be a grid). A code a16_offers() does not list is
// hipErrorInvalidValue.
template <bool FP4, int DT, int OUT, bool GROUPED>
hipError_t launch_a16_t(const GemmArgs& p, int tile, hipStream_t s) {
  auto go = [&](auto bm, auto glu) {
    constexpr int BM = decltype(bm)::value, WM = BM / 64;
    constexpr bool GLU = decltype(glu)::value;
    const int tiles_n = (p.N + 127) / 128;
    const int64_t grid = GROUPED ? grouped_grid_bound(p.M, p.ngroups, BM, tiles_n)
                                 : (int64_t)((p.M + BM - 1) / BM) * tiles_n;
    hipLaunchKernelGGL((gemm_a16_kernel<FP4, DT, OUT, BM, 128, WM, 2, GLU, GROUPED>),
                       dim3((unsigned)grid), dim3(WM * 2 * 64), 0, s, p);
    return hipGetLastError();
  };
  auto by_glu = [&](auto bm) {
    return p.glu ? go(bm, std::true_type{}) : go(bm, std::false_type{});
  };
  if (tile == TILE_256x128) return by_glu(std::integral_constant<int, 256>{});
  if (tile == TILE_128x128) return by_glu(std::integral_constant<int, 128>{});
  return hipErrorInvalidValue;
}

// din x dw x dout -> the instantiation (dout: din or f32; gemm_a16_launch has checked all three).
template <bool GROUPED>
hipError_t launch_a16_forms(const GemmArgs& p, int din, int dout, int dw, int tile,
                            hipStream_t s) {
  auto by_out = [&](auto fp4, auto dt) {
    constexpr bool F = decltype(fp4)::value;
    constexpr int DT = decltype(dt)::value;
    return dout == DT_F32 ? launch_a16_t<F, DT, DT_F32, GROUPED>(p, tile, s)
                          : launch_a16_t<F, DT, DT, GROUPED>(p, tile, s);
  };
  auto by_dt = [&](auto fp4) {
    return din == DT_BF16 ? by_out(fp4, std::integral_constant<int, DT_BF16>{})
                          : by_out(fp4, std::integral_constant<int, DT_F16>{});
  };
  return dw == DT_FP4 ? by_dt(std::true_type{}) : by_dt(std::false_type{});
}

}  // namespace
}  // namespace ddlb
