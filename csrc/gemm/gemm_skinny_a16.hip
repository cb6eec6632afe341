// Skinny-M GEMM for bf16 / f16 activations on gfx950 (gemm_skinny.h, gemm_skinny_a16_launch): the
// weight-streaming split-K kernel of gemm_skinny.hip for an A that is not quantised. W is MXFP4
// (W4A16), MX-fp8 (W8A16) or A's own 16-bit dtype; it is streamed in its stored form, expanded to
// A's dtype in registers and multiplied by v_mfma_f32_16x16x32_{bf16,f16} with f32 accumulation.
//
// What is the same as gemm_skinny.hip: strips of kSkinnyStrip W rows over 4 waves of kSkinnyNR
// 16-row tiles, the grid strips x S x groups, the K-tile of 128 bytes of a row of W (here 256 fp4,
// 128 fp8 or 64 16-bit elements), lane (fr = lane & 15, fq = lane >> 4) loading the 16-byte chunks
// fq and 4 + fq of its row's K-tile and the row's scale word(s) into a register ring of
// kSkinnyPanel K-tiles, W never in LDS, MFMA operand order W, A (a lane owns 4 consecutive output
// columns of one row), acc[MC][NR], the row maps (plain and gated), and everything behind the
// K-loop (gemm_skinny_tail.h: the store tail, skinny_reduce_kernel, skinny_epilogue_kernel).
//
// What is its own:
//   * The expansion. v_mfma_f32_16x16x32 takes K elements 8 g .. 8 g + 7 from lane group g of
//     both operands, so any assignment of K elements to (MFMA, lane group, slot) is right as long
//     as W and A use the same one. W's is given by how it was loaded: chunk c = 4 h + fq (h = 0
//     for the first load, 1 for the second) becomes
//       fp4:    32 elements, one scale block (byte fq of scale word h). Dword t of the chunk is
//               MFMA t's operand: 4 v_cvt_scalef32_pk_*_fp4 (one per byte, two elements each).
//       fp8:    16 elements of block 2 h + (fq >> 1) (that byte of the one scale word). Dwords
//               2 t, 2 t + 1 are MFMA t's operand: 4 v_cvt_scalef32_pk_*_fp8 (one per half dword).
//       16-bit: 8 elements, the MFMA's operand as loaded.
//     The scale operand is the f32 2^(s - 127), built as s << 23. MFMA t of chunk c therefore
//     multiplies the K-tile's elements E c + 8 t .. + 7 (E = 32 / 16 / 8 elements per chunk), and
//     its A fragment is the 16 bytes at 2 (E c + 8 t) of the row's 512 / 256 / 128 bytes:
//       fp4:    128-byte K-row 2 h + (fq >> 1), chunk 4 (fq & 1) + t
//       fp8:    K-row h, chunk 2 fq + t
//       16-bit: K-row 0, chunk 4 h + fq
//     (tests/test_gemm_skinny_a16_gpu.py, one block at a time, pins this map down).
//   * A in LDS. 16 MC rows (MC = 1: M <= 16, else 4) in 128-byte K-rows, AR = 4 / 2 / 1 of them
//     per W K-tile, rows past the range zero-filled and never read from memory. The 16-byte chunk
//     ch of panel K-row kp, row r is stored at chunk ch ^ ((r >> 1) & 7) ^ 2 (kp & 1): the tiled
//     kernel's swizzle, and the K-row's parity so that the fp4 form's lane groups fq and fq ^ 2
//     (same chunk, adjacent K-rows) read different banks. The next panel's global loads are issued
//     before the current panel's MFMAs.
//     Panel length. One W K-tile of A at 64 rows is 32 / 16 / 8 KiB, so a panel as long as the
//     ring (4 K-tiles) would be 128 KiB for fp4. The panel is 32 KiB at most:
//       MC = 4: PK / AR K-tiles = 1 (fp4), 2 (fp8), 4 (16-bit): 32 KiB each;
//       MC = 1: the ring's PK = 4 K-tiles: 32 (fp4), 16 (fp8), 8 KiB (16-bit).
//     32 KiB is the largest size that keeps the panel on its way to LDS in 8 i32x4 per thread
//     (32 VGPRs; 64 KiB would take 64 next to the 72 - 80 of the ring) and leaves room for more
//     than one workgroup per CU; for MC = 1 it already makes the panel barrier as rare as the
//     ring allows. At MC = 4 the fp4 form has a barrier pair per K-tile: it moves 2 bytes of A
//     through LDS per byte of W, and nothing is promised for it there (docs/RESULTS.md).
//   * Scale byte 255. The conversion is given the f32 Inf for it; what it returns is not relied
//     on. Each lane keeps the largest scale byte its W rows met, and the epilogue sets the output
//     columns of every W row that met 255 to NaN (a ballot: W row r's bytes live in the lanes with
//     fr = r, its column in lane group r >> 2). A split launch does so in the slice that met it.
//     e4m3 NaN bytes and NaN / Inf of A go through the conversion and the MFMA as values.
//
// Numerics: the weight multiplied is e 2^(s - 127) in A's dtype, exact whenever that is zero or a
// normal number of the dtype; f32 accumulation in MFMA order; one rounding at the store. Outside
// that range (and scale byte 0, whose f32 operand is +0) the result is the conversion's.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, the 60 instantiations of the
// main kernel; bf16 and f16 are alike): no scratch anywhere; static LDS 32 KiB (MC = 4, and fp4 at
// MC = 1), 16 KiB (fp8, MC = 1), 8 KiB (16-bit, MC = 1). VGPRs + AGPRs, waves per SIMD:
//               MC = 1                      MC = 4
//   fp4     256 + 72 .. 80, 1 wave      256 + 84 .. 92, 1 wave
//   fp8     245 .. 256 + 0, 2 waves     256 + 74 .. 82, 1 wave
//   16-bit  172 .. 180 + 0, 2 waves     232 .. 256 + 32 .. 62, 1 wave
// The MC = 1 fp8 and 16-bit kernels ask for two waves per SIMD (left alone fp8 takes 252 + 8 and
// runs one); fp4 at MC = 1 spills 208 - 240 bytes per lane when asked, so it is not. Where AGPRs
// appear the compiler parks ring registers in them (v_accvgpr moves, no memory traffic).
// Built with the flags of gemm_skinny.hip (no packed-f32 VALU): the two files share the epilogue
// tail and the reduce kernels as source, and the gated test compares their arithmetic byte for
// byte with the f32 path; the K-loop here has no f32 VALU arithmetic either way.
#include "gemm_a16_ops.h"
#include "gemm_skinny_tail.h"

namespace ddlb {
namespace {

constexpr int PK = kSkinnyPanel, NR = kSkinnyNR, SNT = 64 * kSkinnyWaves;
constexpr int A16_W4 = 0, A16_W8 = 1, A16_W16 = 2;  // the weight forms

// p arrives as the byte view gemm_skinny_a16_launch forms: lda, ldw, w_gstride in bytes, K in
// elements. PART / OUT / GLU and the W row map: as gemm_skinny_kernel.
template <int WF, int DT, int OUT, int MC, bool PART, bool GLU = false>
__global__ __launch_bounds__(SNT)
__attribute__((amdgpu_waves_per_eu(MC == 1 && WF != A16_W4 ? 2 : 1)))
void gemm_skinny_a16_kernel(const SkinnyArgs p) {
  using Ops = A16Ops<DT>;
  constexpr int AR = WF == A16_W4 ? 4 : WF == A16_W8 ? 2 : 1;  // A K-rows (128 bytes) per K-tile
  constexpr int SW = WF == A16_W4 ? 2 : WF == A16_W8 ? 1 : 0;  // W scale words per K-tile
  constexpr int NT = AR;                                       // MFMAs per chunk
  constexpr int PW = MC == 1 || PK < AR ? (MC == 1 ? PK : 1) : PK / AR;  // K-tiles per A panel
  constexpr int PA = PW * AR;                                  // its 128-byte K-rows
  static_assert(PK % PW == 0, "the ring is whole A panels");
  static_assert(!PART || (OUT == DT_F32 && !GLU), "partials: f32 in W-row order");
  static_assert(!GLU || NR == 2, "a wave's two tiles: a gate / up pair");
  static_assert(OUT == DT || OUT == DT_F32, "the output is a's dtype or f32");
  constexpr int TJ = GLU ? 32 : 16;         // W rows from tile j to tile j + 1
  constexpr int ROWS = 16 * MC;             // A rows per super-chunk
  constexpr int NA = ROWS * PA * 8 / SNT;   // 16-byte chunks of an A panel per thread
  static_assert(NA * SNT == ROWS * PA * 8, "an A panel splits evenly over the threads");
  static_assert(PA * ROWS * 128 <= 32 * 1024, "the panel rule of the header comment");
  __shared__ __attribute__((aligned(16))) char As[PA * ROWS * 128];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int g = blockIdx.z;
  int r0 = 0, r1 = p.M;
  if (p.offs != nullptr) skinny_group_rows(p.offs, p.M, g, p.ngroups, r0, r1);
  if (r0 >= r1) return;  // an empty group: before any barrier
  int kt0, kt1;
  skinny_slice(p.K / (64 * AR), (int)gridDim.y, (int)blockIdx.y, kt0, kt1);

  // this lane's W rows (one per tile), at its first chunk, and their scale rows
  const int n0 = blockIdx.x * kSkinnyStrip +
                 (GLU ? 64 * (wave >> 1) + 16 * (wave & 1) : wave * 16 * NR);
  const GLB_AS char* wp[NR];
  const GLB_AS char* wsp[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    int64_t n = (int64_t)n0 + j * TJ + fr;
    n = n < p.N ? n : p.N - 1;
    wp[j] = (const GLB_AS char*)p.w + (int64_t)g * p.w_gstride + n * p.ldw + fq * 16;
    wsp[j] = nullptr;
    if constexpr (SW > 0)
      wsp[j] = (const GLB_AS char*)p.w_scale + (int64_t)g * p.w_scale_gstride + n * p.w_scale_ld;
  }

  i32x4 wlo[PK][NR], whi[PK][NR];   // the ring: K-tile kt lives in slot (kt - kt0) % PK
  unsigned wsc[PK][NR][SW ? SW : 1];
  auto load_w = [&](int d, int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const GLB_AS char* t = wp[j] + (int64_t)kt * 128;
      wlo[d][j] = *(const GLB_AS i32x4*)t;
      whi[d][j] = *(const GLB_AS i32x4*)(t + 64);
      if constexpr (SW == 2) {
        const u32x2 v = *(const GLB_AS u32x2*)(wsp[j] + (int64_t)kt * 8);
        wsc[d][j][0] = v.x;
        wsc[d][j][SW - 1] = v.y;
      } else if constexpr (SW == 1) {
        wsc[d][j][0] = *(const GLB_AS unsigned*)(wsp[j] + (int64_t)kt * 4);
      }
    }
  };

  i32x4 areg[NA];        // the next A panel on its way to LDS
  int m0 = r0;
  const int ka1 = AR * kt1;  // A is counted in its 128-byte K-rows
  auto load_a = [&](int base) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int q = i * SNT + tid, c = q & 7, row = (q >> 3) % ROWS, kr = base + q / (8 * ROWS);
      const int64_t gr = (int64_t)m0 + row;
      areg[i] = i32x4{0, 0, 0, 0};
      if (gr < r1 && kr < ka1)
        areg[i] = *(const GLB_AS i32x4*)((const GLB_AS char*)p.a + gr * p.lda +
                                         (int64_t)kr * 128 + c * 16);
    }
  };
  auto store_a = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int q = i * SNT + tid, c = q & 7, prow = q >> 3;  // prow = kp * ROWS + row
      const int pos = c ^ ((prow >> 1) & 7) ^ (((prow / ROWS) & 1) << 1);
      *(i32x4*)(As + prow * 128 + pos * 16) = areg[i];
    }
  };

  const int swz = (fr >> 1) & 7;  // (16 mc + fr) >> 1 & 7: the same for every row chunk
  unsigned smax[NR];              // the largest scale byte this lane's W rows met
#pragma unroll
  for (int j = 0; j < NR; ++j) smax[j] = 0;
  for (; m0 < r1; m0 += ROWS) {
    f32x4 acc[MC][NR];
#pragma unroll
    for (int i = 0; i < MC; ++i)
#pragma unroll
      for (int j = 0; j < NR; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // A first, then the ring (a slot whose K-tile lies past the slice stays empty)
    load_a(AR * kt0);
#pragma unroll
    for (int d = 0; d < PK; ++d)
      if (kt0 + d < kt1) load_w(d, kt0 + d);

    for (int base = kt0; base < kt1; base += PK) {
#pragma unroll
      for (int d = 0; d < PK; ++d) {
        const int kt = base + d;
        if (kt >= kt1) break;  // (uniform)
        if (d % PW == 0) {   // the next A panel: K-tiles kt .. kt + PW - 1
          __syncthreads();  // every wave is done with the previous panel
          store_a();
          __syncthreads();
          load_a(AR * (kt + PW));
        }
        i32x4 raw[2][NR];
        unsigned sw[NR][SW ? SW : 1];
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          raw[0][j] = wlo[d][j];
          raw[1][j] = whi[d][j];
#pragma unroll
          for (int w = 0; w < SW; ++w) sw[j][w] = wsc[d][j][w];
        }
        if (kt + PK < kt1) load_w(d, kt + PK);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          float sc[NR];
          if constexpr (SW > 0) {
#pragma unroll
            for (int j = 0; j < NR; ++j) {
              const unsigned b = WF == A16_W4
                  ? __builtin_amdgcn_ubfe(sw[j][SW == 2 ? h : 0], fq * 8, 8)
                  : __builtin_amdgcn_ubfe(sw[j][0], (2 * h + (fq >> 1)) * 8, 8);
              smax[j] = b > smax[j] ? b : smax[j];
              sc[j] = __builtin_bit_cast(float, b << 23);
            }
          }
          // this chunk's place in the A panel: K-row, and the chunk of MFMA 0
          const int kr = WF == A16_W4 ? 2 * h + (fq >> 1) : WF == A16_W8 ? h : 0;
          const int ch0 = WF == A16_W4 ? 4 * (fq & 1) : WF == A16_W8 ? 2 * fq : 4 * h + fq;
          const int kp = (d % PW) * AR + kr;
          const char* ap = As + (kp * ROWS + fr) * 128;
          const int px = swz ^ ((kp & 1) << 1);
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            i32x4 wf[NR];
#pragma unroll
            for (int j = 0; j < NR; ++j) {
              if constexpr (WF == A16_W4) {
                const unsigned v = (unsigned)raw[h][j][t];
                wf[j] = i32x4{Ops::template fp4<0>(v, sc[j]), Ops::template fp4<1>(v, sc[j]),
                              Ops::template fp4<2>(v, sc[j]), Ops::template fp4<3>(v, sc[j])};
              } else if constexpr (WF == A16_W8) {
                const unsigned v0 = (unsigned)raw[h][j][2 * t], v1 = (unsigned)raw[h][j][2 * t + 1];
                wf[j] = i32x4{Ops::template fp8<false>(v0, sc[j]), Ops::template fp8<true>(v0, sc[j]),
                              Ops::template fp8<false>(v1, sc[j]), Ops::template fp8<true>(v1, sc[j])};
              } else {
                wf[j] = raw[h][j];
              }
            }
            i32x4 af[MC];
#pragma unroll
            for (int i = 0; i < MC; ++i)
              af[i] = *(const i32x4*)(ap + i * 16 * 128 + (((ch0 + t) ^ px) * 16));
#pragma unroll
            for (int i = 0; i < MC; ++i)
#pragma unroll
              for (int j = 0; j < NR; ++j) Ops::Mma::step(acc[i][j], wf[j], af[i]);
          }
        }
      }
    }

    // scale byte 255: NaN in the output columns of the W rows that met it. W row fr of tile j
    // lives in the four lanes (fr, *); this lane stores columns 4 fq .. 4 fq + 3 of the tile.
    if constexpr (SW > 0) {
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        const unsigned long long b = __builtin_amdgcn_ballot_w64(smax[j] == 255u);
        const unsigned rows = (unsigned)(b | (b >> 16) | (b >> 32) | (b >> 48)) & 0xffffu;
        if (rows != 0) {  // (uniform)
          const unsigned mine = rows >> (4 * fq);
#pragma unroll
          for (int i = 0; i < MC; ++i) {
            const float nan = __builtin_nanf("");
            if (mine & 1) acc[i][j].x = nan;
            if (mine & 2) acc[i][j].y = nan;
            if (mine & 4) acc[i][j].z = nan;
            if (mine & 8) acc[i][j].w = nan;
          }
        }
      }
    }

    // a lane holds C[m0 + 16 i + fr][n0 + TJ j + 4 fq + 0 .. 3]; gated: one quad of the N / 2
    // output columns from its two tiles
    constexpr int EO = PART ? DT_F32 : OUT;
    constexpr int B4 = skinny_bytes4<EO>();
    constexpr int NV = GLU ? 1 : NR;  // quads per lane and row
    const int64_t ncols = GLU ? p.N / 2 : p.N;
    const int64_t col0 = (GLU ? (int64_t)blockIdx.x * (kSkinnyStrip / 2) + 32 * (wave >> 1) +
                                    16 * (wave & 1) : (int64_t)n0) + fq * 4;
    const bool vec = PART ? (p.N & 3) == 0 : skinny_vec<EO>(p);
#pragma unroll
    for (int i = 0; i < MC; ++i) {
      const int64_t row = (int64_t)m0 + i * 16 + fr;
      if (row >= r1) continue;
      char* crow = PART ? (char*)(p.ws + ((int64_t)blockIdx.y * p.M + row) * p.N)
                        : (char*)p.c + row * p.ldc * B4 / 4;
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        f32x4 v;
        if constexpr (GLU) v = skinny_gate(acc[i][0], acc[i][1], p.act);
        else v = PART ? acc[i][j] : act4(acc[i][j], p.act);
        skinny_store4<EO>(crow, col0 + j * 16, ncols, vec, nullptr, v, 0u);
      }
    }
  }
}

template <int WF, int DT, int MC>
hipError_t launch_a16(const SkinnyArgs& p, int dout, int S, int groups, hipStream_t s) {
  const dim3 grid((unsigned)skinny_strips(p.N), (unsigned)S, (unsigned)groups), block(SNT);
  auto out = [&](auto&& f) {  // dout: a's dtype or f32
    return dout == DT_F32 ? f(std::integral_constant<int, DT_F32>{})
                          : f(std::integral_constant<int, DT>{});
  };
  if (S > 1) {
    hipLaunchKernelGGL((gemm_skinny_a16_kernel<WF, DT, DT_F32, MC, true>), grid, block, 0, s, p);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    return out([&](auto o) {
      constexpr int O = decltype(o)::value;
      return p.glu ? skinny_launch_epilogue<O, true>(p, S, s) : skinny_launch_reduce<O>(p, S, s);
    });
  }
  return out([&](auto o) {
    constexpr int O = decltype(o)::value;
    if (!p.glu) {
      hipLaunchKernelGGL((gemm_skinny_a16_kernel<WF, DT, O, MC, false>), grid, block, 0, s, p);
    } else if constexpr (NR == 2) {
      hipLaunchKernelGGL((gemm_skinny_a16_kernel<WF, DT, O, MC, false, true>), grid, block, 0, s,
                         p);
    } else {
      return hipErrorInvalidValue;
    }
    return hipGetLastError();
  });
}

template <int WF, int DT>
hipError_t launch_a16_rows(const SkinnyArgs& p, int dout, int S, int groups, hipStream_t s) {
  // one 16-row chunk, or four: one pass over W for up to 64 rows
  return p.M > 16 ? launch_a16<WF, DT, 4>(p, dout, S, groups, s)
                  : launch_a16<WF, DT, 1>(p, dout, S, groups, s);
}

}  // namespace

// Every refusal of the A16 skinny GEMM (hipErrorInvalidValue, nothing launched): the rules of
// gemm_skinny.h. gemm_skinny_launch is not involved.
hipError_t gemm_skinny_a16_launch(const SkinnyArgs& p_in, int din, int dout, hipStream_t s) {
  if (din != DT_BF16 && din != DT_F16) return hipErrorInvalidValue;
  const bool w4 = p_in.w_dtype == DT_FP4, w8 = p_in.w_dtype == DT_FP8, mx = w4 || w8;
  if (!mx && p_in.w_dtype >= 0 && p_in.w_dtype != din) return hipErrorInvalidValue;
  if (dout != din && dout != DT_F32) return hipErrorInvalidValue;
  SkinnyArgs p = p_in;
  if (p.M < 0 || p.N < 1 || p.K < 1 || p.K % (w4 ? 256 : w8 ? 128 : 64))
    return hipErrorInvalidValue;
  if (p.act < ACT_NONE || p.act > ACT_SILU) return hipErrorInvalidValue;
  if (!p.a || !p.w || !p.c || p.a_scale || p.c_scale || mx != (p.w_scale != nullptr))
    return hipErrorInvalidValue;
  const int64_t cols = p.glu ? p.N / 2 : p.N;
  if (p.glu && p.N % 64) return hipErrorInvalidValue;
  if (p.lda < p.K || p.ldw < p.K || p.ldc < cols) return hipErrorInvalidValue;
  const bool grouped = p.offs != nullptr || p.ngroups != 0;
  if (grouped && (!p.offs || p.ngroups < 1 || p.ngroups > kMaxGroups)) return hipErrorInvalidValue;
  if (!grouped) p.w_gstride = p.w_scale_gstride = 0;
  // the byte view: a in 2-byte elements, w by its own format
  const int64_t kw = w4 ? p.K / 2 : w8 ? p.K : 2 * (int64_t)p.K;  // bytes of a row of W
  p.lda *= 2;
  if (w4) {
    if ((p.ldw | p.w_gstride) & 1) return hipErrorInvalidValue;
    p.ldw /= 2; p.w_gstride /= 2;
  } else if (!w8) {
    p.ldw *= 2; p.w_gstride *= 2;
  }
  if (grouped && p.ngroups > 1 && p.w_gstride < (int64_t)(p.N - 1) * p.ldw + kw)
    return hipErrorInvalidValue;
  if (((uintptr_t)p.a | (uintptr_t)p.w | (uint64_t)p.lda | (uint64_t)p.ldw |
       (uint64_t)p.w_gstride) & 15)
    return hipErrorInvalidValue;
  if (mx) {
    if (((uintptr_t)p.w_scale | (uint64_t)p.w_scale_ld | (uint64_t)p.w_scale_gstride) &
        (w4 ? 7 : 3))
      return hipErrorInvalidValue;
    if (p.w_scale_ld < p.K / 32) return hipErrorInvalidValue;
  }
  const int nk = (int)(kw / 128);
  const int groups = grouped ? p.ngroups : 1;
  const int S = p.ksplit == 0 ? skinny_auto_slices(skinny_strips(p.N), nk, groups, num_cus())
                              : p.ksplit;
  if (S < 1 || S > nk || S > 65535 || (p.N + 255) / 256 > 65535) return hipErrorInvalidValue;
  if (S > 1 && (!p.ws || ((uintptr_t)p.ws & 15))) return hipErrorInvalidValue;
  if (p.M == 0) return hipSuccess;
  const bool bf = din == DT_BF16;
  if (w4) return bf ? launch_a16_rows<A16_W4, DT_BF16>(p, dout, S, groups, s)
                    : launch_a16_rows<A16_W4, DT_F16>(p, dout, S, groups, s);
  if (w8) return bf ? launch_a16_rows<A16_W8, DT_BF16>(p, dout, S, groups, s)
                    : launch_a16_rows<A16_W8, DT_F16>(p, dout, S, groups, s);
  return bf ? launch_a16_rows<A16_W16, DT_BF16>(p, dout, S, groups, s)
            : launch_a16_rows<A16_W16, DT_F16>(p, dout, S, groups, s);
}

}  // namespace ddlb
