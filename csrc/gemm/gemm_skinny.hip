// Skinny-M block-scaled GEMM for gfx950 (gemm_skinny.h): a weight-streaming split-K kernel for
// decode shapes, dense and grouped, MX-fp8, MXFP4 and MX-fp8 activations on MXFP4 weights (W4A8),
// and the kernel that sums its K-slices.
//
// The work is bound by reading W once, so the design is about that stream:
//   * W never touches LDS. Each byte is used once, so lane (r = lane & 15, g = lane >> 4) loads
//     the 16-byte chunks g and 4 + g of row r's 128-byte K-tile straight into the registers the
//     scaled MFMA reads them from (the layouts measured for the tiled kernel, gemm_kernels.h:
//     fp8 takes both chunks in one MFMA; fp4 takes chunk g, then 4 + g, in two format-4 MFMAs,
//     each chunk one 32-element block). The row's scale word (fp4: two) is loaded the same way
//     and lane (r, g) passes byte g. A ring of kSkinnyPanel K-tiles per wave is kept in flight:
//     a tile's registers are refilled with the tile kSkinnyPanel further on as soon as it is
//     consumed. W4A8 walks W as fp4 and A as fp8, two A K-rows to a W K-tile: see the kernel.
//   * A goes through LDS once per workgroup: 16 MC rows (MC = 1 or 4) by kSkinnyPanel K-tiles,
//     data and scale words, rows past the row range zero-filled with scale byte 127 and never
//     read from memory. The next panel's global loads are issued before the current panel's
//     MFMAs, so they are older than the W refills and waiting for them leaves those in flight.
//     Rows are 128 bytes apart with the tiled kernel's XOR swizzle on the 16-byte chunks.
//   * One W fragment feeds MC MFMAs (acc[MC][NR]): up to 64 rows cost one weight stream. More
//     rows loop over super-chunks of 16 MC rows and stream W again for each (correct, slow).
//   * MFMA operand order W, A: a lane holds 4 consecutive N-columns of one C row.
//   * S == 1: the epilogue applies act, rounds once, stores C. S > 1: slice s stores f32 partials
//     at ws[s], skinny_reduce_kernel sums them in the order 0 .. S - 1, applies act, rounds once.
//   * The gated (SkinnyArgs::glu) and MX-quantising (SkinnyArgs::c_scale) epilogues sit at the
//     same two sites: the unsplit kernel's final store and, for S > 1, skinny_epilogue_kernel in
//     place of skinny_reduce_kernel (the partial kernel is the same). At both a lane owns four
//     consecutive output columns and ends in skinny_store4; only the way a 32-column block's
//     amax word is joined differs. Unsplit and gated, a wave's two W tiles are a gate tile and its
//     up tile (the row map below), so the product is lane-local.
// W rows >= N are clamped to row N - 1 for the loads and dropped at the store; nothing reads
// outside a view; every row address is 64-bit. Non-finite values: the rule of gemm.h.
#include "gemm_skinny_tail.h"  // the epilogue tail and the reduce kernels, shared with the A16 form

namespace ddlb {
namespace {

constexpr int PK = kSkinnyPanel, NR = kSkinnyNR, SNT = 64 * kSkinnyWaves;
// The operand forms: both e4m3, both E2M1, or e4m3 A on E2M1 W (W4A8).
constexpr int SK_F8 = 0, SK_F4 = 1, SK_W4A8 = 2;

// p arrives as the byte view gemm_skinny_launch forms (fp4: K, lda, ldw, w_gstride in bytes;
// W4A8: ldw and w_gstride only, K stays A's).
// PART: the f32 partial of slice blockIdx.y, no activation; otherwise the whole K and the final
// store: OUT dense or quantised, GLU gated.
// W rows. Tile j of wave w is rows 128 strip + 32 w + 16 j + fr. GLU (unsplit only): rows
// 128 strip + 64 (w >> 1) + 32 j + 16 (w & 1) + fr, the gate tile (j = 0) and its up tile of
// output columns 64 strip + 32 (w >> 1) + 16 (w & 1) + 4 fq .. + 3: waves w, w ^ 1 share a block.
//
// W4A8. A K-tile is W's: 128 bytes, 256 elements, two scale words, walked and kept in the ring
// exactly as the fp4 form's. A is walked as the fp8 form's, in 128-byte K-rows of 128 elements
// with one scale word: K-rows 2 kt and 2 kt + 1 belong to K-tile kt, and MFMA h of the tile takes
// W chunk 4 h + fq under byte fq of W scale word h against the fp8 fragment of K-row 2 kt + h
// (chunks fq and 4 + fq) under byte fq of that K-row's word (MmaMX84S). The LDS panel stays PK
// K-rows (the fp8 form's 32 KiB at MC = 4: PK K-tiles of it would be 64 KiB), so it covers
// PK / 2 K-tiles and the panel barrier falls every PK / 2 ring steps; the ring stays PK K-tiles.
// Its MC = 1 kernels ask for two waves per SIMD, as the other forms' MC = 1 kernels get unasked:
// left alone the dense and partial ones take 242 VGPRs + 14 AGPRs, two registers over, and run one
// wave; asked, all take at most 256 VGPRs, no AGPRs and no scratch. (Every other instantiation
// asks for one, which is what 256 threads have by default: their code is the same without it.)
template <int FORM, int OUT, int MC, bool PART, bool GLU = false>
__global__ __launch_bounds__(SNT)
__attribute__((amdgpu_waves_per_eu(FORM == SK_W4A8 && MC == 1 ? 2 : 1)))
void gemm_skinny_kernel(const SkinnyArgs p) {
  constexpr bool F4 = FORM == SK_F4, W4A8 = FORM == SK_W4A8;
  constexpr int SW = FORM == SK_F8 ? 1 : 2;  // W scale words per K-tile
  constexpr int SA = F4 ? 2 : 1;             // A scale words per panel row
  constexpr int AP = W4A8 ? 2 : 1;           // A panel rows (128 bytes of K) per K-tile
  constexpr int PW = PK / AP;                // K-tiles an A panel covers
  static_assert(!PART || (OUT == DT_F32 && !GLU), "partials: f32 in W-row order");
  static_assert(!(GLU || skinny_qout<OUT>()) || NR == 2, "a wave's two tiles: a pair, or a block");
  static_assert(!(GLU && skinny_qout<OUT>()) || PK * SA >= kSkinnyWaves,
                "Ss holds an amax word per wave and row");
  static_assert(PW * AP == PK, "an A panel is whole K-tiles");
  constexpr int TJ = GLU ? 32 : 16;         // W rows from tile j to tile j + 1
  constexpr int ROWS = 16 * MC;             // A rows per super-chunk
  constexpr int NA = ROWS * PK * 8 / SNT;   // 16-byte chunks of an A panel per thread
  constexpr int NS = (ROWS * PK + SNT - 1) / SNT;  // scale rows of a panel per thread
  static_assert(NA * SNT == ROWS * PK * 8, "an A panel splits evenly over the threads");
  __shared__ __attribute__((aligned(16))) char As[PK * ROWS * 128];
  __shared__ unsigned Ss[PK * ROWS * SA];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int g = blockIdx.z;
  int r0 = 0, r1 = p.M;
  if (p.offs != nullptr) skinny_group_rows(p.offs, p.M, g, p.ngroups, r0, r1);
  if (r0 >= r1) return;  // an empty group: before any barrier
  int kt0, kt1;
  skinny_slice(p.K / (128 * AP), (int)gridDim.y, (int)blockIdx.y, kt0, kt1);

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
    wsp[j] = (const GLB_AS char*)p.w_scale + (int64_t)g * p.w_scale_gstride + n * p.w_scale_ld;
  }

  i32x4 wlo[PK][NR], whi[PK][NR];   // the ring: K-tile kt lives in slot (kt - kt0) % PK
  unsigned wsc[PK][NR][SW];
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
      } else {
        wsc[d][j][0] = *(const GLB_AS unsigned*)(wsp[j] + (int64_t)kt * 4);
      }
    }
  };

  i32x4 areg[NA];        // the next A panel on its way to LDS
  unsigned asc[NS][SA];
  int m0 = r0;
  const int ka1 = AP * kt1;  // panel rows are counted in A's 128-byte K-rows (kt here)
  auto load_a = [&](int base) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int q = i * SNT + tid, c = q & 7, row = (q >> 3) % ROWS, kt = base + q / (8 * ROWS);
      const int64_t gr = (int64_t)m0 + row;
      areg[i] = i32x4{0, 0, 0, 0};
      if (gr < r1 && kt < ka1)
        areg[i] = *(const GLB_AS i32x4*)((const GLB_AS char*)p.a + gr * p.lda +
                                         (int64_t)kt * 128 + c * 16);
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int q = i * SNT + tid, row = q % ROWS, kt = base + q / ROWS;
      const int64_t gr = (int64_t)m0 + row;
#pragma unroll
      for (int w = 0; w < SA; ++w) asc[i][w] = 0x7f7f7f7fu;  // padding rows: unit scales
      if (q < ROWS * PK && gr < r1 && kt < ka1) {
        const GLB_AS char* t = (const GLB_AS char*)p.a_scale + gr * p.a_scale_ld +
                               (int64_t)kt * (4 * SA);
        if constexpr (F4) {
          const u32x2 v = *(const GLB_AS u32x2*)t;
          asc[i][0] = v.x;
          asc[i][SA - 1] = v.y;
        } else {
          asc[i][0] = *(const GLB_AS unsigned*)t;
        }
      }
    }
  };
  auto store_a = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int q = i * SNT + tid, c = q & 7, prow = q >> 3;  // prow = d * ROWS + row
      *(i32x4*)(As + prow * 128 + ((c ^ ((prow >> 1) & 7)) * 16)) = areg[i];
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int q = i * SNT + tid;
      if (q < ROWS * PK) {
#pragma unroll
        for (int w = 0; w < SA; ++w) Ss[q * SA + w] = asc[i][w];
      }
    }
  };

  const int swz = (fr >> 1) & 7;  // (16 mc + fr) >> 1 & 7: the same for every row chunk
  const int ca = (fq ^ swz) * 16, cb = ((4 + fq) ^ swz) * 16;
  for (; m0 < r1; m0 += ROWS) {
    f32x4 acc[MC][NR];
#pragma unroll
    for (int i = 0; i < MC; ++i)
#pragma unroll
      for (int j = 0; j < NR; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // A first, then the ring (a slot whose K-tile lies past the slice stays empty)
    load_a(AP * kt0);
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
          load_a(AP * (kt + PW));
        }
        i32x4 blo[NR], bhi[NR];
        int sb[NR][SW];
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          blo[j] = wlo[d][j];
          bhi[j] = whi[d][j];
#pragma unroll
          for (int w = 0; w < SW; ++w)
            sb[j][w] = (int)__builtin_amdgcn_ubfe(wsc[d][j][w], fq * 8, 8);
        }
        if (kt + PK < kt1) load_w(d, kt + PK);
        if constexpr (W4A8) {
#pragma unroll
          for (int h = 0; h < 2; ++h) {  // panel row 2 (d % PW) + h: A K-row 2 kt + h
            i32x8 a8[MC];
            int sa[MC];
#pragma unroll
            for (int i = 0; i < MC; ++i) {
              const int prow = ((d % PW) * 2 + h) * ROWS + i * 16 + fr;
              const i32x4 lo = *(const i32x4*)(As + prow * 128 + ca);
              const i32x4 hi = *(const i32x4*)(As + prow * 128 + cb);
              a8[i] = i32x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
              sa[i] = (int)__builtin_amdgcn_ubfe(Ss[prow], fq * 8, 8);
            }
#pragma unroll
            for (int i = 0; i < MC; ++i)
#pragma unroll
              for (int j = 0; j < NR; ++j)
                MmaMX84S::step48s(acc[i][j], h ? bhi[j] : blo[j], a8[i], sb[j][h], sa[i]);
          }
        } else {
          i32x4 alo[MC], ahi[MC];
          int sa[MC][SA];
#pragma unroll
          for (int i = 0; i < MC; ++i) {
            const int prow = d * ROWS + i * 16 + fr;
            alo[i] = *(const i32x4*)(As + prow * 128 + ca);
            ahi[i] = *(const i32x4*)(As + prow * 128 + cb);
#pragma unroll
            for (int w = 0; w < SA; ++w)
              sa[i][w] = (int)__builtin_amdgcn_ubfe(Ss[prow * SA + w], fq * 8, 8);
          }
#pragma unroll
          for (int i = 0; i < MC; ++i)
#pragma unroll
            for (int j = 0; j < NR; ++j) {
              if constexpr (F4) {
                MmaMX4S::step4s(acc[i][j], blo[j], alo[i], sb[j][0], sa[i][0]);
                MmaMX4S::step4s(acc[i][j], bhi[j], ahi[i], sb[j][SW - 1], sa[i][SW - 1]);
              } else {
                const i32x8 b8 = {blo[j].x, blo[j].y, blo[j].z, blo[j].w,
                                  bhi[j].x, bhi[j].y, bhi[j].z, bhi[j].w};
                const i32x8 a8 = {alo[i].x, alo[i].y, alo[i].z, alo[i].w,
                                  ahi[i].x, ahi[i].y, ahi[i].z, ahi[i].w};
                MmaMXS::step8s(acc[i][j], b8, a8, sb[j][0], sa[i][0]);
              }
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
    f32x4 v[MC][NV];
    unsigned am[MC];
#pragma unroll
    for (int i = 0; i < MC; ++i) {
      am[i] = 0;
      if constexpr (GLU) {
        v[i][0] = skinny_gate(acc[i][0], acc[i][1], p.act);
      } else {
#pragma unroll
        for (int j = 0; j < NR; ++j) v[i][j] = PART ? acc[i][j] : act4(acc[i][j], p.act);
      }
      // the row's block: the wave's 32 columns (gated: its 16), over the four fq lanes
#pragma unroll
      for (int j = 0; j < NV; ++j) am[i] = skinny_amax4<EO>(am[i], v[i][j]);
      am[i] = skinny_amax_xor<EO>(skinny_amax_xor<EO>(am[i], 16), 32);
    }
    if constexpr (GLU && skinny_qout<EO>()) {
      // the other half of the block is wave ^ 1's: the words change hands through Ss, which
      // every wave is done with behind the first barrier (all waves get here: rows past the
      // range are dropped at the stores)
      __syncthreads();
#pragma unroll
      for (int i = 0; i < MC; ++i) Ss[wave * ROWS + i * 16 + fr] = am[i];
      __syncthreads();
#pragma unroll
      for (int i = 0; i < MC; ++i)
        am[i] = mx_amax_join<EO == DT_FP4>(am[i], Ss[(wave ^ 1) * ROWS + i * 16 + fr]);
    }
#pragma unroll
    for (int i = 0; i < MC; ++i) {
      const int64_t row = (int64_t)m0 + i * 16 + fr;
      if (row >= r1) continue;
      char* crow = PART ? (char*)(p.ws + ((int64_t)blockIdx.y * p.M + row) * p.N)
                        : (char*)p.c + row * p.ldc * B4 / 4;
      uint8_t* sdst = nullptr;  // the scale byte: one lane per (row, block)
      if constexpr (skinny_qout<EO>())
        if (fq == 0 && !(GLU && (wave & 1))) sdst = p.c_scale + row * p.c_scale_ld + (col0 >> 5);
#pragma unroll
      for (int j = 0; j < NV; ++j)
        skinny_store4<EO>(crow, col0 + j * 16, ncols, vec, j == 0 ? sdst : nullptr, v[i][j],
                          am[i]);
    }
  }
}

// dout over the dense and the quantised outputs
template <class F>
hipError_t skinny_dispatch_out(int dout, F&& f) {
  if (dout == DT_FP8) return f(std::integral_constant<int, DT_FP8>{});
  if (dout == DT_FP4) return f(std::integral_constant<int, DT_FP4>{});
  return dispatch_out(dout, f);
}

template <int FORM, int MC>
hipError_t launch_skinny(const SkinnyArgs& p, int dout, int S, int groups, hipStream_t s) {
  const dim3 grid((unsigned)skinny_strips(p.N), (unsigned)S, (unsigned)groups), block(SNT);
  const bool fused = p.glu != 0 || dout == DT_FP8 || dout == DT_FP4;
  if (S > 1) {
    hipLaunchKernelGGL((gemm_skinny_kernel<FORM, DT_F32, MC, true>), grid, block, 0, s, p);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (!fused)
      return dispatch_out(dout, [&](auto o) {
        return skinny_launch_reduce<decltype(o)::value>(p, S, s);
      });
  }
  if (!fused)
    return dispatch_out(dout, [&](auto o) {
      hipLaunchKernelGGL((gemm_skinny_kernel<FORM, decltype(o)::value, MC, false>), grid, block, 0,
                         s, p);
      return hipGetLastError();
    });
  if constexpr (NR == 2) {  // (a wave's two tiles are what the fused epilogues pair up)
    return skinny_dispatch_out(dout, [&](auto o) {
      constexpr int O = decltype(o)::value;
      auto go = [&](auto glu) {
        constexpr bool G = decltype(glu)::value;
        if constexpr (G || skinny_qout<O>()) {
          if (S > 1) return skinny_launch_epilogue<O, G>(p, S, s);
          hipLaunchKernelGGL((gemm_skinny_kernel<FORM, O, MC, false, G>), grid, block, 0, s, p);
        }
        return hipGetLastError();
      };
      return p.glu ? go(std::true_type{}) : go(std::false_type{});
    });
  }
  return hipErrorInvalidValue;
}

}  // namespace

// Every refusal of the skinny GEMM (hipErrorInvalidValue, nothing launched): the rules of
// SkinnyArgs. The tiled kernel's gemm_launch is not involved.
hipError_t gemm_skinny_launch(const SkinnyArgs& p_in, int din, int dout, hipStream_t s) {
  const int dw = p_in.w_dtype < 0 ? din : p_in.w_dtype;
  const bool f4 = din == DT_FP4, w4 = dw == DT_FP4;  // W4A8: w4 && !f4
  if ((din != DT_FP8 && !f4) || (dw != DT_FP8 && !w4) || (f4 && !w4)) return hipErrorInvalidValue;
  const bool q4 = dout == DT_FP4, qout = dout == DT_FP8 || q4;
  if (dout != DT_BF16 && dout != DT_F16 && dout != DT_F32 && !qout) return hipErrorInvalidValue;
  SkinnyArgs p = p_in;
  if (p.M < 0 || p.N < 1 || p.K < 1 || p.K % (w4 ? 256 : 128)) return hipErrorInvalidValue;
  if (p.act < ACT_NONE || p.act > ACT_SILU) return hipErrorInvalidValue;
  if (!p.a || !p.w || !p.c || !p.a_scale || !p.w_scale) return hipErrorInvalidValue;
  // the output: N columns, gated N / 2 from whole 64-row gate / up groups; quantised with its
  // scales and only then, in whole blocks as the GEMM that reads them takes per K-tile, rows
  // and scale words aligned as that GEMM's a and a_scale (above)
  const int64_t cols = p.glu ? p.N / 2 : p.N;
  if ((p.glu && p.N % 64) || qout != (p.c_scale != nullptr)) return hipErrorInvalidValue;
  if (p.lda < p.K || p.ldw < p.K || p.ldc < cols) return hipErrorInvalidValue;
  if (qout) {
    const int cal = q4 ? 8 : 4;
    if (cols % (q4 ? 256 : 128) || (q4 && (p.ldc & 1))) return hipErrorInvalidValue;
    if ((((uintptr_t)p.c | (uint64_t)(q4 ? p.ldc / 2 : p.ldc)) & 15) ||
        (((uintptr_t)p.c_scale | (uint64_t)p.c_scale_ld) & (cal - 1)) ||
        p.c_scale_ld < cols / 32 || (int64_t)p.M * p.c_scale_ld >= (int64_t(1) << 31))
      return hipErrorInvalidValue;
  }
  const bool grouped = p.offs != nullptr || p.ngroups != 0;
  if (grouped && (!p.offs || p.ngroups < 1 || p.ngroups > kMaxGroups)) return hipErrorInvalidValue;
  if (!grouped) p.w_gstride = p.w_scale_gstride = 0;
  // the byte view: two fp4 elements per byte, each operand's quantities by its own format (K
  // is A's; W4A8 leaves it and lda alone)
  const int scale_row = p.K / 32;       // bytes of a row of either operand's scales
  const int kw = w4 ? p.K / 2 : p.K;    // bytes of a row of W
  if (f4) {
    if (p.lda & 1) return hipErrorInvalidValue;
    p.K /= 2; p.lda /= 2;
  }
  if (w4) {
    if ((p.ldw | p.w_gstride) & 1) return hipErrorInvalidValue;
    p.ldw /= 2; p.w_gstride /= 2;
  }
  if (grouped && p.ngroups > 1 && p.w_gstride < (int64_t)(p.N - 1) * p.ldw + kw)
    return hipErrorInvalidValue;
  if (((uintptr_t)p.a | (uintptr_t)p.w | (uint64_t)p.lda | (uint64_t)p.ldw |
       (uint64_t)p.w_gstride) & 15)
    return hipErrorInvalidValue;
  if ((((uintptr_t)p.a_scale | (uint64_t)p.a_scale_ld) & (f4 ? 7 : 3)) ||
      (((uintptr_t)p.w_scale | (uint64_t)p.w_scale_ld | (uint64_t)p.w_scale_gstride) &
       (w4 ? 7 : 3)))
    return hipErrorInvalidValue;
  if (p.a_scale_ld < scale_row || p.w_scale_ld < scale_row) return hipErrorInvalidValue;
  const int nk = kw / 128;  // K-tiles are W's
  const int groups = grouped ? p.ngroups : 1;
  const int S = p.ksplit == 0 ? skinny_auto_slices(skinny_strips(p.N), nk, groups, num_cus())
                              : p.ksplit;
  if (S < 1 || S > nk || S > 65535 || (p.N + 255) / 256 > 65535) return hipErrorInvalidValue;
  if (S > 1 && (!p.ws || ((uintptr_t)p.ws & 15))) return hipErrorInvalidValue;
  if (p.M == 0) return hipSuccess;
  const bool wide = p.M > 16;  // one 16-row chunk, or four: one pass over W for up to 64 rows
  if (f4) return wide ? launch_skinny<SK_F4, 4>(p, dout, S, groups, s)
                      : launch_skinny<SK_F4, 1>(p, dout, S, groups, s);
  if (w4) return wide ? launch_skinny<SK_W4A8, 4>(p, dout, S, groups, s)
                      : launch_skinny<SK_W4A8, 1>(p, dout, S, groups, s);
  return wide ? launch_skinny<SK_F8, 4>(p, dout, S, groups, s)
              : launch_skinny<SK_F8, 1>(p, dout, S, groups, s);
}

}  // namespace ddlb
