// Grouped transposing MX quantiser for gfx950: x[T, C] (f32 / f16 / bf16), its rows sorted into
// E groups by a device array of offsets -> qt[C, cap] OCP e4m3 (or [C, cap / 2] E2M1 nibble pairs)
// + st[C, cap / 32] E8M0 in the padded K layout of a K-grouped GEMM (tile_map.h kgrouped_range):
// group g's blocks start at the group's first row, run down the columns of x and fill the columns
// [k0_g, k0_g + kl_g) of qt, the group's last tile zero-extended. Byte for byte that is
// mx_quant_t.hip's output for the group's rows padded with zero rows to a multiple of TR
// (ddlb_amd/ops/mx.py quantize_mx_t_grouped_reference is the specification). An all-zero block
// gets the scale byte 127 and zero data (mx_cvt.h), so the padding contributes exact zeros to a
// contraction over it.
//
// The kernel is mx_quant_t_kernel's sibling (one-way form) and keeps its two steps, its LDS
// swizzle and its stores; mx_quant_t.hip has the reasoning. What differs:
//   * the grid is the bound (T / TR + E) * ctiles of tile_map.h: a workgroup finds its
//     (group, row tile of the group) with grouped_tile (BM = TR), or finds none and returns
//     before the barrier;
//   * step 1 predicates a source row at or past the group's end off (it stands for zeros, as a
//     vector past column C does), and a tile starts at any row of x, not at a multiple of TR;
//   * step 2's destination column is TR times the LAUNCH-WIDE row tile index, which is k0_g plus
//     the tile's offset in the group, below the capacity because the grid is.
// Stacked form (stacked_rows = R > 0): group g is written to its own slab, from column 0, and a
// tile at or past row R of the group is dropped: with x = w.reshape(E * N, K), offsets
// arange(E + 1) * N and R = N, one launch writes the column-wise quantisation [E, K, N] of every
// expert's weight.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm.h"
#include "mx_cvt.h"
#include "mx_quant_in.h"
#include "tile_map.h"

namespace ddlb {
namespace {

constexpr int kMxtgThreads = 256;
constexpr int kMxtgCols = 64;  // tile width in elements

template <int DT, bool FP4>
__global__ __launch_bounds__(kMxtgThreads) __attribute__((amdgpu_waves_per_eu(4, 8)))
void mx_quant_t_grouped_kernel(const MxQuantTGroupedArgs a, int ctiles) {
  using In = MxqIn<DT>;
  constexpr int EPV = In::kElems;           // elements per 16-byte vector
  constexpr int ESZ = 16 / EPV;
  constexpr int TR = FP4 ? 256 : 128;       // tile rows
  constexpr int NB = TR / 32;               // 32-row blocks per tile column
  constexpr int VPR = kMxtgCols / EPV;      // vectors (chunks) per tile row: 8 or 16
  constexpr int NV = TR * VPR / kMxtgThreads;  // vectors per lane: 4 .. 16
  constexpr int SK = FP4 ? 1 : 2;           // the swizzle's step in chunks per row block
  __shared__ mxq_u32x4 tile[TR * VPR];      // 16, 32 or 64 KiB

  const int tid = threadIdx.x;
  GroupTile t;
  if (!grouped_tile(a.offs, a.T, a.ngroups, TR, ctiles, (int)blockIdx.x, t)) return;
  const int tr0 = t.tm * TR;                // the tile's first row within the group
  const int nrows = t.rows - tr0;           // the group's rows from there on (> 0)
  const int64_t r0 = (int64_t)t.row0 + tr0; // ... and within x
  const int c0 = t.tn * kMxtgCols;
  // destination: the padded layout's column, or the group's slab
  int64_t d0 = (int64_t)((int)blockIdx.x / ctiles) * TR;
  char* qt = (char*)a.qt;
  uint8_t* st = a.st;
  if (a.stacked_rows > 0) {
    if (tr0 >= a.stacked_rows) return;
    d0 = tr0;
    qt += (int64_t)t.g * a.qt_gstride;
    st += (int64_t)t.g * a.st_gstride;
  }

  // 1. global -> registers (all loads in flight), then -> LDS
  mxq_u32x4 v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int idx = tid + i * kMxtgThreads;
    const int r = idx / VPR, k = idx % VPR;
    const int col = c0 + k * EPV;  // C % EPV == 0: a vector lies wholly inside or outside
    v[i] = mxq_u32x4{0u, 0u, 0u, 0u};
    if (col < a.C && r < nrows)
      v[i] = *(const mxq_u32x4*)((const char*)a.x + ((r0 + r) * a.ldx + col) * ESZ);
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int idx = tid + i * kMxtgThreads;
    const int r = idx / VPR, k = idx % VPR;
    tile[r * VPR + (k ^ ((r >> 5) * SK))] = v[i];
  }
  __syncthreads();

  // 2. one (column, row block) per lane and trip; every lane runs every trip (the shuffles)
#pragma unroll 1
  for (int u = tid; u < kMxtgCols * NB; u += kMxtgThreads) {
    const int b = u % NB, c = u / NB;
    const char* p = (const char*)tile + (b * 32 * VPR + ((c / EPV) ^ (b * SK))) * 16 +
                    (c % EPV) * ESZ;
    float f[32];
    unsigned m = 0;  // |x| as an integer: ordered as the floats are
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      f[i] = In::elem(p + i * VPR * 16);
      m = mx_amax_join<FP4>(m, mx_amax_bits<FP4>(f[i]));
    }
    const int e = mx_scale_exp<FP4>(m);
    const int col = c0 + c;
    const bool ok = col < a.C;
    if constexpr (FP4) {
      const float sc = mx_fp4_scale(e);
      unsigned w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned q = 0;
        q = mx_cvt2_e2m1<0>(q, f[8 * j], f[8 * j + 1], sc);
        q = mx_cvt2_e2m1<1>(q, f[8 * j + 2], f[8 * j + 3], sc);
        q = mx_cvt2_e2m1<2>(q, f[8 * j + 4], f[8 * j + 5], sc);
        q = mx_cvt2_e2m1<3>(q, f[8 * j + 6], f[8 * j + 7], sc);
        w[j] = q;
      }
      if (ok)
        *(mxq_u32x4*)(qt + (int64_t)col * a.ldqt + (d0 + 32 * b) / 2) =
            mxq_u32x4{w[0], w[1], w[2], w[3]};
    } else {
      unsigned w[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        w[j] = mx_cvt4_e4m3(f[4 * j], f[4 * j + 1], f[4 * j + 2], f[4 * j + 3], e);
      if (ok) {
        mxq_u32x4* dst = (mxq_u32x4*)(qt + (int64_t)col * a.ldqt + d0 + 32 * b);
        dst[0] = mxq_u32x4{w[0], w[1], w[2], w[3]};
        dst[1] = mxq_u32x4{w[4], w[5], w[6], w[7]};
      }
    }
    // four neighbouring blocks' scale bytes -> one aligned 32-bit word (NB % 4 == 0)
    unsigned sw = mx_scale_byte<FP4>(m, e) << (8 * (b & 3));
    sw |= (unsigned)__shfl_xor((int)sw, 1);
    sw |= (unsigned)__shfl_xor((int)sw, 2);
    if (ok && (b & 3) == 0)
      *(unsigned*)(st + (int64_t)col * a.ldst + d0 / 32 + b) = sw;
  }
}

template <bool FP4>
hipError_t mxtg_launch(const MxQuantTGroupedArgs& a, int din, hipStream_t s) {
  if (din != DT_F32 && din != DT_F16 && din != DT_BF16) return hipErrorInvalidValue;
  constexpr int MOD = FP4 ? 256 : 128;      // the tile rows: a K-grouped GEMM's K-tile
  constexpr int SALIGN = FP4 ? 8 : 4;       // st: one word per tile and row
  const int esz = dtype_size(din);
  if (a.T < 0 || a.C < 0 || ((int64_t)a.C * esz) % 16) return hipErrorInvalidValue;
  if (a.ngroups < 1 || a.ngroups > kMaxGroups) return hipErrorInvalidValue;
  if (a.stacked_rows < 0 || a.stacked_rows % MOD) return hipErrorInvalidValue;
  if (a.T == 0 || a.C == 0) return hipSuccess;
  const bool stacked = a.stacked_rows > 0;
  const int64_t cols = stacked ? a.stacked_rows : kgrouped_capacity(a.T, a.ngroups, MOD);
  if (a.x == nullptr || a.qt == nullptr || a.st == nullptr || a.offs == nullptr ||
      ((uintptr_t)a.offs & 3) || a.ldx < a.C || a.ldqt < (FP4 ? cols / 2 : cols) ||
      a.ldst < cols / 32 || ((uintptr_t)a.x & 15) || (a.ldx * esz) % 16 ||
      ((uintptr_t)a.qt & 15) || a.ldqt % 16 || ((uintptr_t)a.st & (SALIGN - 1)) ||
      a.ldst % SALIGN)
    return hipErrorInvalidValue;
  if (stacked && (a.qt_gstride < 0 || a.qt_gstride % 16 || a.st_gstride < 0 ||
                  a.st_gstride % SALIGN ||
                  (a.ngroups > 1 && (a.qt_gstride < (int64_t)a.C * a.ldqt ||
                                     a.st_gstride < (int64_t)a.C * a.ldst))))
    return hipErrorInvalidValue;
  const int ctiles = (a.C + kMxtgCols - 1) / kMxtgCols;
  const int64_t grid = grouped_grid_bound(a.T, a.ngroups, MOD, ctiles);
  if (grid > 0x7FFFFFFF) return hipErrorInvalidValue;
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kMxtgThreads), 0, s, a, ctiles);
    return hipGetLastError();
  };
  if (din == DT_F32) return go(mx_quant_t_grouped_kernel<DT_F32, FP4>);
  if (din == DT_F16) return go(mx_quant_t_grouped_kernel<DT_F16, FP4>);
  return go(mx_quant_t_grouped_kernel<DT_BF16, FP4>);
}

}  // namespace

hipError_t mx_quantize_t_grouped_launch(const MxQuantTGroupedArgs& a, int din, bool fp4,
                                        hipStream_t s) {
  return fp4 ? mxtg_launch<true>(a, din, s) : mxtg_launch<false>(a, din, s);
}

}  // namespace ddlb
