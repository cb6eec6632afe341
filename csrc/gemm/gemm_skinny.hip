// Skinny-M block-scaled GEMM for gfx950 (gemm_skinny.h): a weight-streaming split-K kernel for
// decode shapes, dense and grouped, MX-fp8 and MXFP4, and the kernel that sums its K-slices.
//
// The work is bound by reading W once, so the design is about that stream:
//   * W never touches LDS. Each byte is used once, so lane (r = lane & 15, g = lane >> 4) loads
//     the 16-byte chunks g and 4 + g of row r's 128-byte K-tile straight into the registers the
//     scaled MFMA reads them from (the layouts measured for the tiled kernel, gemm_kernels.h:
//     fp8 takes both chunks in one MFMA; fp4 takes chunk g, then 4 + g, in two format-4 MFMAs,
//     each chunk one 32-element block). The row's scale word (fp4: two) is loaded the same way
//     and lane (r, g) passes byte g. A ring of kSkinnyPanel K-tiles per wave is kept in flight:
//     a tile's registers are refilled with the tile kSkinnyPanel further on as soon as it is
//     consumed.
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
// W rows >= N are clamped to row N - 1 for the loads and dropped at the store; nothing reads
// outside a view; every row address is 64-bit. Non-finite values: the rule of gemm.h.
#include "gemm_skinny.h"

#include "gemm_kernels.h"

namespace ddlb {
namespace {

constexpr int PK = kSkinnyPanel, NR = kSkinnyNR, SNT = 64 * kSkinnyWaves;

// p arrives as the byte view gemm_skinny_launch forms (fp4: K, lda, ldw, w_gstride in bytes).
// PART: the f32 partial of slice blockIdx.y, no activation; otherwise the whole K and the final
// store in OUT.
template <bool F4, int OUT, int MC, bool PART>
__global__ __launch_bounds__(SNT) void gemm_skinny_kernel(const SkinnyArgs p) {
  constexpr int ROWS = 16 * MC;             // A rows per super-chunk
  constexpr int NA = ROWS * PK * 8 / SNT;   // 16-byte chunks of an A panel per thread
  constexpr int NS = (ROWS * PK + SNT - 1) / SNT;  // scale rows of a panel per thread
  constexpr int SW = F4 ? 2 : 1;            // scale words per row per K-tile
  static_assert(NA * SNT == ROWS * PK * 8, "an A panel splits evenly over the threads");
  __shared__ __attribute__((aligned(16))) char As[PK * ROWS * 128];
  __shared__ unsigned Ss[PK * ROWS * SW];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int g = blockIdx.z;
  int r0 = 0, r1 = p.M;
  if (p.offs != nullptr) skinny_group_rows(p.offs, p.M, g, p.ngroups, r0, r1);
  if (r0 >= r1) return;  // an empty group: before any barrier
  int kt0, kt1;
  skinny_slice(p.K / 128, (int)gridDim.y, (int)blockIdx.y, kt0, kt1);

  // this lane's W rows (one per tile), at its first chunk, and their scale rows
  const int n0 = blockIdx.x * kSkinnyStrip + wave * 16 * NR;
  const GLB_AS char* wp[NR];
  const GLB_AS char* wsp[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    int64_t n = (int64_t)n0 + j * 16 + fr;
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
      if constexpr (F4) {
        const u32x2 v = *(const GLB_AS u32x2*)(wsp[j] + (int64_t)kt * 8);
        wsc[d][j][0] = v.x;
        wsc[d][j][SW - 1] = v.y;
      } else {
        wsc[d][j][0] = *(const GLB_AS unsigned*)(wsp[j] + (int64_t)kt * 4);
      }
    }
  };

  i32x4 areg[NA];        // the next A panel on its way to LDS
  unsigned asc[NS][SW];
  int m0 = r0;
  auto load_a = [&](int base) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int q = i * SNT + tid, c = q & 7, row = (q >> 3) % ROWS, kt = base + q / (8 * ROWS);
      const int64_t gr = (int64_t)m0 + row;
      areg[i] = i32x4{0, 0, 0, 0};
      if (gr < r1 && kt < kt1)
        areg[i] = *(const GLB_AS i32x4*)((const GLB_AS char*)p.a + gr * p.lda +
                                         (int64_t)kt * 128 + c * 16);
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int q = i * SNT + tid, row = q % ROWS, kt = base + q / ROWS;
      const int64_t gr = (int64_t)m0 + row;
#pragma unroll
      for (int w = 0; w < SW; ++w) asc[i][w] = 0x7f7f7f7fu;  // padding rows: unit scales
      if (q < ROWS * PK && gr < r1 && kt < kt1) {
        const GLB_AS char* t = (const GLB_AS char*)p.a_scale + gr * p.a_scale_ld +
                               (int64_t)kt * (4 * SW);
        if constexpr (F4) {
          const u32x2 v = *(const GLB_AS u32x2*)t;
          asc[i][0] = v.x;
          asc[i][SW - 1] = v.y;
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
        for (int w = 0; w < SW; ++w) Ss[q * SW + w] = asc[i][w];
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
    load_a(kt0);
#pragma unroll
    for (int d = 0; d < PK; ++d)
      if (kt0 + d < kt1) load_w(d, kt0 + d);

    for (int base = kt0; base < kt1; base += PK) {
      __syncthreads();  // every wave is done with the previous panel
      store_a();
      __syncthreads();
      load_a(base + PK);
#pragma unroll
      for (int d = 0; d < PK; ++d) {
        const int kt = base + d;
        if (kt >= kt1) break;  // (uniform)
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
        {
          i32x4 alo[MC], ahi[MC];
          int sa[MC][SW];
#pragma unroll
          for (int i = 0; i < MC; ++i) {
            const int prow = d * ROWS + i * 16 + fr;
            alo[i] = *(const i32x4*)(As + prow * 128 + ca);
            ahi[i] = *(const i32x4*)(As + prow * 128 + cb);
#pragma unroll
            for (int w = 0; w < SW; ++w)
              sa[i][w] = (int)__builtin_amdgcn_ubfe(Ss[prow * SW + w], fq * 8, 8);
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

    // a lane holds C[m0 + 16 i + fr][n0 + 16 j + 4 fq + 0 .. 3]
    constexpr int OSZ = PART ? 4 : out_size<OUT>();
    const bool vec = PART ? (p.N & 3) == 0
                          : ((((uintptr_t)p.c | (uint64_t)(p.ldc * OSZ)) & (4 * OSZ - 1)) == 0);
#pragma unroll
    for (int i = 0; i < MC; ++i) {
      const int64_t row = (int64_t)m0 + i * 16 + fr;
      if (row >= r1) continue;
      char* crow = PART ? (char*)(p.ws + ((int64_t)blockIdx.y * p.M + row) * p.N)
                        : (char*)p.c + row * p.ldc * OSZ;
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        const int64_t col = (int64_t)n0 + j * 16 + fq * 4;
        const f32x4 v4 = PART ? acc[i][j] : act4(acc[i][j], p.act);
        if (col + 3 < p.N && vec) {
          Store4<PART ? DT_F32 : OUT>::st(crow + col * OSZ, v4);
        } else {
          const float v[4] = {v4.x, v4.y, v4.z, v4.w};
          for (int r = 0; r < 4; ++r)
            if (col + r < p.N) Store4<PART ? DT_F32 : OUT>::st1(crow + (col + r) * OSZ, v[r]);
        }
      }
    }
  }
}

// C[row, col] = round(act(sum over s = 0 .. S - 1, in that order, of ws[s][row][col])): one
// workgroup per (row, 256 columns). Grouped: rows [o'[0], o'[E]) only, read from the offsets here.
template <int OUT>
__global__ __launch_bounds__(256) void skinny_reduce_kernel(const SkinnyArgs p, const int S) {
  int r0 = 0, r1 = p.M;
  if (p.offs != nullptr) skinny_group_rows(p.offs, p.M, -1, p.ngroups, r0, r1);
  const int64_t row = (int64_t)r0 + blockIdx.x;
  const int64_t col = (int64_t)blockIdx.y * 256 + threadIdx.x;
  if (row >= r1 || col >= p.N) return;
  const GLB_AS float* src = (const GLB_AS float*)p.ws + row * p.N + col;
  const int64_t step = (int64_t)p.M * p.N;
  float acc = src[0];
#pragma unroll 4
  for (int s = 1; s < S; ++s) acc += src[s * step];
  constexpr int OSZ = out_size<OUT>();
  Store4<OUT>::st1((char*)p.c + (row * p.ldc + col) * OSZ, act1(acc, p.act));
}

template <bool F4, int MC>
hipError_t launch_skinny(const SkinnyArgs& p, int dout, int S, int groups, hipStream_t s) {
  const dim3 grid((unsigned)skinny_strips(p.N), (unsigned)S, (unsigned)groups), block(SNT);
  if (S > 1) {
    hipLaunchKernelGGL((gemm_skinny_kernel<F4, DT_F32, MC, true>), grid, block, 0, s, p);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const dim3 rgrid((unsigned)p.M, (unsigned)((p.N + 255) / 256));
    return dispatch_out(dout, [&](auto o) {
      hipLaunchKernelGGL((skinny_reduce_kernel<decltype(o)::value>), rgrid, dim3(256), 0, s, p, S);
      return hipGetLastError();
    });
  }
  return dispatch_out(dout, [&](auto o) {
    hipLaunchKernelGGL((gemm_skinny_kernel<F4, decltype(o)::value, MC, false>), grid, block, 0, s,
                       p);
    return hipGetLastError();
  });
}

}  // namespace

// Every refusal of the skinny GEMM (hipErrorInvalidValue, nothing launched): the rules of
// SkinnyArgs. The tiled kernel's gemm_launch is not involved.
hipError_t gemm_skinny_launch(const SkinnyArgs& p_in, int din, int dout, hipStream_t s) {
  const bool f4 = din == DT_FP4;
  if (din != DT_FP8 && !f4) return hipErrorInvalidValue;
  if (dout != DT_BF16 && dout != DT_F16 && dout != DT_F32) return hipErrorInvalidValue;
  SkinnyArgs p = p_in;
  if (p.M < 0 || p.N < 1 || p.K < 1 || p.K % (f4 ? 256 : 128)) return hipErrorInvalidValue;
  if (p.act < ACT_NONE || p.act > ACT_SILU) return hipErrorInvalidValue;
  if (!p.a || !p.w || !p.c || !p.a_scale || !p.w_scale) return hipErrorInvalidValue;
  if (p.lda < p.K || p.ldw < p.K || p.ldc < p.N) return hipErrorInvalidValue;
  const bool grouped = p.offs != nullptr || p.ngroups != 0;
  if (grouped && (!p.offs || p.ngroups < 1 || p.ngroups > kMaxGroups)) return hipErrorInvalidValue;
  if (!grouped) p.w_gstride = p.w_scale_gstride = 0;
  if (f4) {  // the byte view: two elements per byte
    if ((p.lda | p.ldw | p.w_gstride) & 1) return hipErrorInvalidValue;
    p.K /= 2; p.lda /= 2; p.ldw /= 2; p.w_gstride /= 2;
  }
  if (grouped && p.ngroups > 1 && p.w_gstride < (int64_t)(p.N - 1) * p.ldw + p.K)
    return hipErrorInvalidValue;
  if (((uintptr_t)p.a | (uintptr_t)p.w | (uint64_t)p.lda | (uint64_t)p.ldw |
       (uint64_t)p.w_gstride) & 15)
    return hipErrorInvalidValue;
  const int sal = f4 ? 8 : 4;
  if (((uintptr_t)p.a_scale | (uintptr_t)p.w_scale | (uint64_t)p.a_scale_ld |
       (uint64_t)p.w_scale_ld | (uint64_t)p.w_scale_gstride) & (sal - 1))
    return hipErrorInvalidValue;
  const int nk = p.K / 128;
  if (p.a_scale_ld < 4 * (int64_t)nk * (f4 ? 2 : 1) || p.w_scale_ld < 4 * (int64_t)nk * (f4 ? 2 : 1))
    return hipErrorInvalidValue;
  const int groups = grouped ? p.ngroups : 1;
  const int S = p.ksplit == 0 ? skinny_auto_slices(skinny_strips(p.N), nk, groups, num_cus())
                              : p.ksplit;
  if (S < 1 || S > nk || S > 65535 || (p.N + 255) / 256 > 65535) return hipErrorInvalidValue;
  if (S > 1 && (!p.ws || ((uintptr_t)p.ws & 15))) return hipErrorInvalidValue;
  if (p.M == 0) return hipSuccess;
  const bool wide = p.M > 16;  // one 16-row chunk, or four: one pass over W for up to 64 rows
  if (f4) return wide ? launch_skinny<true, 4>(p, dout, S, groups, s)
                      : launch_skinny<true, 1>(p, dout, S, groups, s);
  return wide ? launch_skinny<false, 4>(p, dout, S, groups, s)
              : launch_skinny<false, 1>(p, dout, S, groups, s);
}

}  // namespace ddlb
