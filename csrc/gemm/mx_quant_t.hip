// Transposing MX quantiser for gfx950: x[R, C] (f32 / f16 / bf16) -> qt[C, R] OCP e4m3 (or
// [C, R / 2] E2M1 nibble pairs) + st[C, R / 32] E8M0, with the blocks DOWN the columns of x: a
// block is x[32 b .. 32 b + 31, c]. The result is mx_quant.hip's output for x.T, byte for byte
// (ddlb_amd/ops/mx.py quantize_mx_t_reference is the specification): the operand layout of a GEMM
// that contracts over R, which is what a linear layer's dgrad (over N) and wgrad (over M) do.
// It is a second quantisation of the tensor, not a transpose of the row-wise one.
//
// One pass over x, 3 bytes moved per 16-bit element. A workgroup of 256 threads takes a tile of
// TR = 128 rows (fp4: 256; R % TR == 0, so a row of st gets one aligned 32-bit (64-bit) word per
// tile) by 64 columns:
//   1. every lane loads 16-byte vectors along the input rows (a tile row is 128 or 256 contiguous
//      bytes; a vector past column C is predicated off and stands for zeros) and stores them to
//      LDS;
//   2. after the barrier one lane owns one (column, 32-row block): it reads the block's 32
//      elements down the column, takes the amax on the integer image of |x|, converts, and stores
//      the block's 32 (16) bytes into row c of qt. The lanes of a column's TR / 32 blocks are
//      adjacent, so a column's 128 bytes leave as one contiguous run, and its scale bytes are
//      gathered across those lanes into 32-bit words.
// LDS layout: rows at their natural pitch (64 elements, no padding), the 16-byte chunk index of
// a row XORed with (row / 32) * SK, SK = 2 (fp4: 1). The column reads of step 2 are 2- or 4-byte
// LDS reads, banked per 32-lane half. A half holds 32 / NB columns x NB blocks (NB = TR / 32):
// unswizzled, its blocks are 32 rows = a multiple of 4 KiB apart and all land on the same banks
// (NB-way conflict, whatever 16-byte-aligned pitch is chosen). The columns of a half span
// 32 / NB dwords or fewer, inside one chunk pair (fp8) or one chunk (fp4), and the XOR moves block
// b's chunk by 2 b (b) chunks = 8 b (4 b) dwords: NB disjoint dword ranges, at most 32 dwords in
// all, so every lane of the half has a bank of its own (two 16-bit lanes in one dword read the
// same dword). The step from row to row adds the same offset to every lane. Step 1's 16-byte
// writes stay a permutation of a row's chunks.
//
// TWO = true: step 1 also quantises its vectors row-wise, straight from the registers, exactly
// as mx_quant.hip does (mx_quant_in.h holds that code for both), and writes q[R, C], s[R, C / 32]:
// x is read once for both layouts. C % 128 == 0 (fp4: 256) then, so no vector is predicated off
// and the lanes that share a row block are all active.
//
// The grid is one workgroup per tile, column tiles fastest (two-way: permuted within groups of
// 16 or 32 workgroups, see the kernel); no grid cap, no scratch.
//
// The grouped form (Args = MxQuantTGroupedArgs, one-way) is the same kernel template behind
// another prologue: x[T, C], its rows sorted into E groups by a device array of offsets ->
// qt[C, cap], st[C, cap / 32] in the padded K layout of a K-grouped GEMM (tile_map.h
// kgrouped_range): group g's blocks start at the group's first row, run down the columns of x and
// fill the columns [k0_g, k0_g + kl_g) of qt, the group's last tile zero-extended. Byte for byte
// that is the plain form's output for the group's rows padded with zero rows to a multiple of TR
// (ddlb_amd/ops/mx.py quantize_mx_t_grouped_reference is the specification). An all-zero block
// gets the scale byte 127 and zero data (mx_cvt.h), so the padding contributes exact zeros to a
// contraction over it. The prologue:
//   * the grid is the bound (T / TR + E) * ctiles of tile_map.h: a workgroup finds its
//     (group, row tile of the group) with grouped_tile (BM = TR), or finds none and returns
//     before the barrier; a tile starts at any row of x, not at a multiple of TR, and has nrows
//     source rows left in its group: step 1 predicates a row at or past that off (it stands for
//     zeros, as a vector past column C does);
//   * step 2's destination column d0 is TR times the LAUNCH-WIDE row tile index, which is k0_g
//     plus the tile's offset in the group, below the capacity because the grid is;
//   * stacked form (stacked_rows = R > 0): group g is written to its own slab, from column 0, and
//     a tile at or past row R of the group is dropped: with x = w.reshape(E * N, K), offsets
//     arange(E + 1) * N and R = N, one launch writes the column-wise quantisation [E, K, N] of
//     every expert's weight.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "gemm.h"
#include "mx_cvt.h"
#include "mx_quant_in.h"
#include "tile_map.h"

namespace ddlb {
namespace {

constexpr int kMxtThreads = 256;
constexpr int kMxtCols = 64;  // tile width in elements

// (waves per SIMD: without the hint the register allocator spends 240 VGPRs on three of the
// twelve plain instantiations and halves what their LDS footprint would let a CU hold)
template <int DT, bool FP4, bool TWO, class Args = MxQuantTArgs>
__global__ __launch_bounds__(kMxtThreads) __attribute__((amdgpu_waves_per_eu(4, 8)))
void mx_quant_t_kernel(const Args a, int ctiles) {
  constexpr bool GROUPED = std::is_same<Args, MxQuantTGroupedArgs>::value;
  static_assert(!(GROUPED && TWO), "the grouped form is one-way");
  using In = MxqIn<DT>;
  constexpr int EPV = In::kElems;           // elements per 16-byte vector
  constexpr int ESZ = 16 / EPV;
  constexpr int TR = FP4 ? 256 : 128;       // tile rows
  constexpr int NB = TR / 32;               // 32-row blocks per tile column
  constexpr int VPR = kMxtCols / EPV;       // vectors (chunks) per tile row: 8 or 16
  constexpr int NV = TR * VPR / kMxtThreads;  // vectors per lane: 4 .. 16
  constexpr int SK = FP4 ? 1 : 2;           // the swizzle's step in chunks per row block
  constexpr int LPB = 32 / EPV;             // lanes that share a row-wise block
  __shared__ mxq_u32x4 tile[TR * VPR];      // 16, 32 or 64 KiB

  const int tid = threadIdx.x;
  int64_t r0;                   // the tile's first row in x
  int64_t d0;                   // ... and its first column in qt (st: d0 / 32)
  int c0;                       // the tile's first column in x
  int nrows = TR;               // grouped: rows of x from r0 to its group's end (> 0)
  char* qt = (char*)a.qt;
  uint8_t* st = a.st;
  if constexpr (GROUPED) {
    GroupTile t;
    if (!grouped_tile(a.offs, a.T, a.ngroups, TR, ctiles, (int)blockIdx.x, t)) return;
    const int tr0 = t.tm * TR;  // the tile's first row within the group
    nrows = t.rows - tr0;
    r0 = (int64_t)t.row0 + tr0;
    c0 = t.tn * kMxtCols;
    d0 = (int64_t)((int)blockIdx.x / ctiles) * TR;  // the padded layout's column
    if (a.stacked_rows > 0) {                       // ... or the group's slab
      if (tr0 >= a.stacked_rows) return;
      d0 = tr0;
      qt += (int64_t)t.g * a.qt_gstride;
      st += (int64_t)t.g * a.st_gstride;
    }
  } else {
    unsigned bid = blockIdx.x;
    if constexpr (TWO) {
      // A tile's row of q is 64 bytes (fp4: 32), half (a quarter) of a 128-byte line, and
      // workgroups b and b + 8 share an XCD and its L2 (observed dispatch order; only speed rests
      // on it). So within every whole group of 8 P workgroups, P = 2 (4), the P column tiles that
      // complete a line go to workgroups 8 apart and the line leaves one L2 whole.
      // ctiles % P == 0.
      constexpr unsigned P = FP4 ? 4 : 2;
      const unsigned grp = bid / (8 * P), i = bid % (8 * P);
      if ((grp + 1) * (8 * P) <= gridDim.x) bid = grp * (8 * P) + (i % 8) * P + i / 8;
    }
    r0 = d0 = (int64_t)(bid / (unsigned)ctiles) * TR;
    c0 = (int)(bid % (unsigned)ctiles) * kMxtCols;
  }

  // 1. global -> registers (all loads in flight), then -> LDS (and the row-wise outputs)
  mxq_u32x4 v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int idx = tid + i * kMxtThreads;
    const int r = idx / VPR, k = idx % VPR;
    const int col = c0 + k * EPV;  // C % EPV == 0: a vector lies wholly inside or outside
    v[i] = mxq_u32x4{0u, 0u, 0u, 0u};
    if ((TWO || col < a.C) && (!GROUPED || r < nrows))
      v[i] = *(const mxq_u32x4*)((const char*)a.x + ((r0 + r) * a.ldx + col) * ESZ);
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int idx = tid + i * kMxtThreads;
    const int r = idx / VPR, k = idx % VPR;
    tile[r * VPR + (k ^ ((r >> 5) * SK))] = v[i];
    if constexpr (TWO) {
      const int col = c0 + k * EPV;
      mxq_rowwise_vec<DT, FP4>(v[i], (char*)a.q + (r0 + r) * a.ldq + (FP4 ? col / 2 : col),
                               a.s + (r0 + r) * a.lds + col / 32, (tid & (LPB - 1)) == 0);
    }
  }
  __syncthreads();

  // 2. one (column, row block) per lane and trip; every lane runs every trip (the shuffles)
#pragma unroll 1
  for (int u = tid; u < kMxtCols * NB; u += kMxtThreads) {
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
        unsigned t = 0;
        t = mx_cvt2_e2m1<0>(t, f[8 * j], f[8 * j + 1], sc);
        t = mx_cvt2_e2m1<1>(t, f[8 * j + 2], f[8 * j + 3], sc);
        t = mx_cvt2_e2m1<2>(t, f[8 * j + 4], f[8 * j + 5], sc);
        t = mx_cvt2_e2m1<3>(t, f[8 * j + 6], f[8 * j + 7], sc);
        w[j] = t;
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

// What the two launches below check alike. The input: a dtype with a 16-byte vector load, C
// columns that are whole vectors.
bool mxt_input_ok(int din, int C) {
  if (din != DT_F32 && din != DT_F16 && din != DT_BF16) return false;
  return C >= 0 && ((int64_t)C * dtype_size(din)) % 16 == 0;
}

// x[., C] and qt, st with `cols` quantised columns: present, wide enough, aligned for the
// kernel's 16-byte loads and stores and for st's one word per tile and row.
template <bool FP4, class Args>
bool mxt_operands_ok(const Args& a, int din, int64_t cols) {
  constexpr int SALIGN = FP4 ? 8 : 4;
  return a.x != nullptr && a.qt != nullptr && a.st != nullptr && a.ldx >= a.C &&
         a.ldqt >= (FP4 ? cols / 2 : cols) && a.ldst >= cols / 32 && !((uintptr_t)a.x & 15) &&
         (a.ldx * dtype_size(din)) % 16 == 0 && !((uintptr_t)a.qt & 15) && a.ldqt % 16 == 0 &&
         !((uintptr_t)a.st & (SALIGN - 1)) && a.ldst % SALIGN == 0;
}

// `grid` workgroups (a 31-bit grid, or refused) of the input dtype's kernel
template <bool FP4, bool TWO, class Args>
hipError_t mxt_go(const Args& a, int din, int64_t grid, int ctiles, hipStream_t s) {
  if (grid > 0x7FFFFFFF) return hipErrorInvalidValue;
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kMxtThreads), 0, s, a, ctiles);
    return hipGetLastError();
  };
  if (din == DT_F32) return go(mx_quant_t_kernel<DT_F32, FP4, TWO, Args>);
  if (din == DT_F16) return go(mx_quant_t_kernel<DT_F16, FP4, TWO, Args>);
  return go(mx_quant_t_kernel<DT_BF16, FP4, TWO, Args>);
}

template <bool FP4, bool TWO>
hipError_t mxt_launch(const MxQuantTArgs& a, int din, hipStream_t s) {
  constexpr int MOD = FP4 ? 256 : 128;      // R (and, two-way, C) as a GEMM's K
  constexpr int QALIGN = FP4 ? 4 : 8;       // q: the row-wise kernel's packed store
  if (!mxt_input_ok(din, a.C) || a.R < 0 || a.R % MOD) return hipErrorInvalidValue;
  if (TWO && a.C % MOD) return hipErrorInvalidValue;
  if (a.R == 0 || a.C == 0) return hipSuccess;
  if (!mxt_operands_ok<FP4>(a, din, a.R)) return hipErrorInvalidValue;
  if (TWO && (a.q == nullptr || a.s == nullptr || a.ldq < (FP4 ? a.C / 2 : a.C) ||
              a.lds < a.C / 32 || ((uintptr_t)a.q & (QALIGN - 1)) || a.ldq % QALIGN))
    return hipErrorInvalidValue;
  const int ctiles = (a.C + kMxtCols - 1) / kMxtCols;
  return mxt_go<FP4, TWO>(a, din, (int64_t)(a.R / MOD) * ctiles, ctiles, s);
}

template <bool FP4>
hipError_t mxtg_launch(const MxQuantTGroupedArgs& a, int din, hipStream_t s) {
  constexpr int MOD = FP4 ? 256 : 128;      // the tile rows: a K-grouped GEMM's K-tile
  constexpr int SALIGN = FP4 ? 8 : 4;
  if (!mxt_input_ok(din, a.C) || a.T < 0) return hipErrorInvalidValue;
  if (a.ngroups < 1 || a.ngroups > kMaxGroups) return hipErrorInvalidValue;
  if (a.stacked_rows < 0 || a.stacked_rows % MOD) return hipErrorInvalidValue;
  if (a.T == 0 || a.C == 0) return hipSuccess;
  const bool stacked = a.stacked_rows > 0;
  const int64_t cols = stacked ? a.stacked_rows : kgrouped_capacity(a.T, a.ngroups, MOD);
  if (!mxt_operands_ok<FP4>(a, din, cols) || a.offs == nullptr || ((uintptr_t)a.offs & 3))
    return hipErrorInvalidValue;
  if (stacked && (a.qt_gstride < 0 || a.qt_gstride % 16 || a.st_gstride < 0 ||
                  a.st_gstride % SALIGN ||
                  (a.ngroups > 1 && (a.qt_gstride < (int64_t)a.C * a.ldqt ||
                                     a.st_gstride < (int64_t)a.C * a.ldst))))
    return hipErrorInvalidValue;
  const int ctiles = (a.C + kMxtCols - 1) / kMxtCols;
  return mxt_go<FP4, false>(a, din, grouped_grid_bound(a.T, a.ngroups, MOD, ctiles), ctiles, s);
}

}  // namespace

hipError_t mx_quantize_t_launch(const MxQuantTArgs& a, int din, bool fp4, bool two,
                                hipStream_t s) {
  if (fp4) return two ? mxt_launch<true, true>(a, din, s) : mxt_launch<true, false>(a, din, s);
  return two ? mxt_launch<false, true>(a, din, s) : mxt_launch<false, false>(a, din, s);
}

hipError_t mx_quantize_t_grouped_launch(const MxQuantTGroupedArgs& a, int din, bool fp4,
                                        hipStream_t s) {
  return fp4 ? mxtg_launch<true>(a, din, s) : mxtg_launch<false>(a, din, s);
}

}  // namespace ddlb
