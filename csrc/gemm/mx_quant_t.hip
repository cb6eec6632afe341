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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm.h"
#include "mx_cvt.h"
#include "mx_quant_in.h"

namespace ddlb {
namespace {

constexpr int kMxtThreads = 256;
constexpr int kMxtCols = 64;  // tile width in elements

// (waves per SIMD: without the hint the register allocator spends 240 VGPRs on three of the
// twelve instantiations and halves what their LDS footprint would let a CU hold)
template <int DT, bool FP4, bool TWO>
__global__ __launch_bounds__(kMxtThreads) __attribute__((amdgpu_waves_per_eu(4, 8)))
void mx_quant_t_kernel(const MxQuantTArgs a, int ctiles) {
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
  unsigned bid = blockIdx.x;
  if constexpr (TWO) {
    // A tile's row of q is 64 bytes (fp4: 32), half (a quarter) of a 128-byte line, and workgroups
    // b and b + 8 share an XCD and its L2 (observed dispatch order; only speed rests on it). So
    // within every whole group of 8 P workgroups, P = 2 (4), the P column tiles that complete a
    // line go to workgroups 8 apart and the line leaves one L2 whole. ctiles % P == 0.
    constexpr unsigned P = FP4 ? 4 : 2;
    const unsigned grp = bid / (8 * P), i = bid % (8 * P);
    if ((grp + 1) * (8 * P) <= gridDim.x) bid = grp * (8 * P) + (i % 8) * P + i / 8;
  }
  const int ct = (int)(bid % (unsigned)ctiles);
  const int64_t r0 = (int64_t)(bid / (unsigned)ctiles) * TR;
  const int c0 = ct * kMxtCols;

  // 1. global -> registers (all loads in flight), then -> LDS (and the row-wise outputs)
  mxq_u32x4 v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int idx = tid + i * kMxtThreads;
    const int r = idx / VPR, k = idx % VPR;
    const int col = c0 + k * EPV;  // C % EPV == 0: a vector lies wholly inside or outside
    v[i] = mxq_u32x4{0u, 0u, 0u, 0u};
    if (TWO || col < a.C)
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
        *(mxq_u32x4*)((char*)a.qt + (int64_t)col * a.ldqt + (r0 + 32 * b) / 2) =
            mxq_u32x4{w[0], w[1], w[2], w[3]};
    } else {
      unsigned w[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        w[j] = mx_cvt4_e4m3(f[4 * j], f[4 * j + 1], f[4 * j + 2], f[4 * j + 3], e);
      if (ok) {
        mxq_u32x4* dst = (mxq_u32x4*)((char*)a.qt + (int64_t)col * a.ldqt + r0 + 32 * b);
        dst[0] = mxq_u32x4{w[0], w[1], w[2], w[3]};
        dst[1] = mxq_u32x4{w[4], w[5], w[6], w[7]};
      }
    }
    // four neighbouring blocks' scale bytes -> one aligned 32-bit word (NB % 4 == 0)
    unsigned sw = mx_scale_byte<FP4>(m, e) << (8 * (b & 3));
    sw |= (unsigned)__shfl_xor((int)sw, 1);
    sw |= (unsigned)__shfl_xor((int)sw, 2);
    if (ok && (b & 3) == 0)
      *(unsigned*)(a.st + (int64_t)col * a.ldst + r0 / 32 + b) = sw;
  }
}

template <bool FP4, bool TWO>
hipError_t mxt_launch(const MxQuantTArgs& a, int din, hipStream_t s) {
  if (din != DT_F32 && din != DT_F16 && din != DT_BF16) return hipErrorInvalidValue;
  constexpr int MOD = FP4 ? 256 : 128;      // R (and, two-way, C) as a GEMM's K
  constexpr int SALIGN = FP4 ? 8 : 4;       // st: one word per tile and row
  constexpr int QALIGN = FP4 ? 4 : 8;       // q: the row-wise kernel's packed store
  const int esz = dtype_size(din);
  if (a.R < 0 || a.C < 0 || a.R % MOD || ((int64_t)a.C * esz) % 16) return hipErrorInvalidValue;
  if (TWO && a.C % MOD) return hipErrorInvalidValue;
  if (a.R == 0 || a.C == 0) return hipSuccess;
  if (a.x == nullptr || a.qt == nullptr || a.st == nullptr || a.ldx < a.C ||
      a.ldqt < (FP4 ? a.R / 2 : a.R) || a.ldst < a.R / 32 || ((uintptr_t)a.x & 15) ||
      (a.ldx * esz) % 16 || ((uintptr_t)a.qt & 15) || a.ldqt % 16 ||
      ((uintptr_t)a.st & (SALIGN - 1)) || a.ldst % SALIGN)
    return hipErrorInvalidValue;
  if (TWO && (a.q == nullptr || a.s == nullptr || a.ldq < (FP4 ? a.C / 2 : a.C) ||
              a.lds < a.C / 32 || ((uintptr_t)a.q & (QALIGN - 1)) || a.ldq % QALIGN))
    return hipErrorInvalidValue;
  const int ctiles = (a.C + kMxtCols - 1) / kMxtCols;
  const int64_t grid = (int64_t)(a.R / (FP4 ? 256 : 128)) * ctiles;
  if (grid > 0x7FFFFFFF) return hipErrorInvalidValue;
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kMxtThreads), 0, s, a, ctiles);
    return hipGetLastError();
  };
  if (din == DT_F32) return go(mx_quant_t_kernel<DT_F32, FP4, TWO>);
  if (din == DT_F16) return go(mx_quant_t_kernel<DT_F16, FP4, TWO>);
  return go(mx_quant_t_kernel<DT_BF16, FP4, TWO>);
}

}  // namespace

hipError_t mx_quantize_t_launch(const MxQuantTArgs& a, int din, bool fp4, bool two,
                                hipStream_t s) {
  if (fp4) return two ? mxt_launch<true, true>(a, din, s) : mxt_launch<true, false>(a, din, s);
  return two ? mxt_launch<false, true>(a, din, s) : mxt_launch<false, false>(a, din, s);
}

}  // namespace ddlb
