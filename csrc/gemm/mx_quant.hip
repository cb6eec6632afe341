// MX quantiser for gfx950: x[R, K] (f32 / f16 / bf16) -> q[R, K] OCP e4m3 + s[R, K / 32] E8M0.
//
// The format (docs/ARCHITECTURE.md "MX block scaling"): one scale byte s per 32 consecutive K
// elements of a row, value 2^(s - 127). The rule rounds the scale UP so nothing saturates:
//   amax = max|x| over the block (fp32);  amax == 0: s = 127, q = 0;  otherwise amax = m 2^ex with
//   m in [0.5, 1):  e = ex - 9 if m <= 0.875 else ex - 8  (the smallest e with amax / 2^e <= 448),
//   e clamped to [-127, 127], s = e + 127, q = e4m3_rne(clamp(x 2^-e, -448, 448)).
// Non-finite input is unspecified. ddlb_amd/ops/mx.py quantize_mx_reference is the specification.
//
// A streaming, memory-bound kernel: one 16-byte load per lane (8 16-bit or 4 f32 elements), so 4
// (8) neighbouring lanes share a block and its amax is a cross-lane max over them (on the integer
// image of |x|: exact, subnormals included); two v_cvt_pk_fp8_f32 per four elements, one packed
// 8-byte (4-byte) store per lane, the block's first lane stores the scale byte. A workgroup takes
// 256 / (vectors per row) rows per pass (one, striding along K, for long rows) and grid-strides
// over the rows; the grid is sized by the CU count. No LDS.
//
// The MXFP4 flavour (FP4 = true) is the same streaming kernel with OCP E2M1 elements: 6 in place
// of 448 (e = ex - 3 if m <= 0.75 else ex - 2), q = e2m1_rne(clamp(x 2^-e, -6, 6)) with ties to the
// even code, two elements per byte (element 2j in the low nibble of byte j), so a lane packs its
// 8 (4) elements into 4 (2) bytes. One v_cvt_scalef32_pk_fp4_f32 converts two elements and takes
// the block's scale 2^e as an operand (only its exponent field is read: the ldexp folds into
// it, and e = -127 is the field 0). It is used because it matches the specification,
// ddlb_amd/ops/mx.py quantize_mxfp4_reference, nibble for nibble on the GPU: the seven ties in
// both signs, -0 and negative values that round to zero (0x8), subnormal inputs, s = 0
// (tests/test_mxfp4_gpu.py). K % 256 == 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "device_info.h"
#include "gemm.h"
#include "mx_cvt.h"
#include "mx_quant_in.h"

namespace ddlb {
namespace {

constexpr int kMxqThreads = 256;

// The gathering form (Args = MxQuantGatherArgs): output row r is the quantisation of x[src[r]] (a
// routed layer's dispatch: the permuted 16-bit copy of x is never written). A lane reads its row's
// index once per row, and an index outside [0, X) makes the row a zero row: zero data, scale byte
// 127, nothing read.
template <int DT, bool FP4, class Args = MxQuantArgs>
__global__ __launch_bounds__(kMxqThreads) void mx_quant_kernel(const Args a, int rows_pp) {
  constexpr bool GATHER = std::is_same<Args, MxQuantGatherArgs>::value;
  using In = MxqIn<DT>;
  constexpr int EPV = In::kElems;   // elements per 16-byte vector
  constexpr int LPB = 32 / EPV;     // lanes that share a 32-element block
  constexpr int ESZ = 16 / EPV;
  const int vpr = a.K / EPV;        // vectors per row: a multiple of 16 (K % 128 == 0)
  const int tid = threadIdx.x;
  int r_in = 0, c0 = tid;
  if (vpr < kMxqThreads) {
    r_in = tid / vpr;
    c0 = tid - r_in * vpr;
  }
  if (r_in >= rows_pp) return;  // whole blocks' lanes leave together (vpr % LPB == 0)
  const int64_t row_step = (int64_t)gridDim.x * rows_pp;
  for (int64_t row = (int64_t)blockIdx.x * rows_pp + r_in; row < a.R; row += row_step) {
    int64_t from = row;
    bool real = true;  // (the lanes of a row agree)
    if constexpr (GATHER) {
      const int src = a.src[row];
      real = src >= 0 && src < a.X;
      from = real ? src : 0;
    }
    const char* xr = (const char*)a.x + from * a.ldx * ESZ;
    char* qr = (char*)a.q + row * a.ldq;
    uint8_t* sr = a.s + row * a.lds;
    for (int c = c0; c < vpr; c += kMxqThreads) {  // (lanes of a block share their trip count)
      mxq_u32x4 v = mxq_u32x4{0u, 0u, 0u, 0u};
      if (real) v = *(const mxq_u32x4*)(xr + (int64_t)c * 16);
      mxq_rowwise_vec<DT, FP4>(v, qr + (int64_t)c * (FP4 ? EPV / 2 : EPV), sr + c / LPB,
                               (tid & (LPB - 1)) == 0);
    }
  }
}

// Both forms: the same refusals and the same grid over the R output rows. Gathering, x needs
// X >= 0 rows (X = 0: every row is a zero row and x is not read) and src is required.
template <bool FP4, class Args>
hipError_t mxq_launch(const Args& a, int din, hipStream_t s) {
  constexpr bool GATHER = std::is_same<Args, MxQuantGatherArgs>::value;
  if (din != DT_F32 && din != DT_F16 && din != DT_BF16) return hipErrorInvalidValue;
  // fp4: q rows are K / 2 bytes, stored 4 (2) bytes per lane
  constexpr int KMOD = FP4 ? 256 : 128, QALIGN = FP4 ? 4 : 8;
  if (a.R < 0 || a.K <= 0 || a.K % KMOD) return hipErrorInvalidValue;
  bool x_needed = true;
  if constexpr (GATHER) {
    if (a.X < 0) return hipErrorInvalidValue;
    x_needed = a.X > 0;
  }
  if (a.R == 0) return hipSuccess;
  const int esz = dtype_size(din);
  if ((a.x == nullptr && x_needed) || a.q == nullptr || a.s == nullptr || a.ldx < a.K ||
      a.ldq < (FP4 ? a.K / 2 : a.K) || a.lds < a.K / 32 || ((uintptr_t)a.x & 15) ||
      (a.ldx * esz) % 16 || ((uintptr_t)a.q & (QALIGN - 1)) || a.ldq % QALIGN)
    return hipErrorInvalidValue;
  if constexpr (GATHER) {
    if (a.src == nullptr) return hipErrorInvalidValue;
  }
  const int vpr = a.K / (16 / esz);
  const int rows_pp = vpr < kMxqThreads ? kMxqThreads / vpr : 1;
  // eight 256-thread workgroups fill a CU's wave slots; the rest of the rows by grid stride
  int64_t grid = ((int64_t)a.R + rows_pp - 1) / rows_pp;
  const int64_t cap = (int64_t)num_cus() * 8;
  if (grid > cap) grid = cap;
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kMxqThreads), 0, s, a, rows_pp);
    return hipGetLastError();
  };
  if (din == DT_F32) return go(mx_quant_kernel<DT_F32, FP4, Args>);
  if (din == DT_F16) return go(mx_quant_kernel<DT_F16, FP4, Args>);
  return go(mx_quant_kernel<DT_BF16, FP4, Args>);
}

}  // namespace

hipError_t mx_quantize_gather_launch(const MxQuantGatherArgs& a, int din, bool fp4,
                                     hipStream_t s) {
  return fp4 ? mxq_launch<true>(a, din, s) : mxq_launch<false>(a, din, s);
}

hipError_t mx_quantize_launch(const MxQuantArgs& a, int din, hipStream_t s) {
  return mxq_launch<false>(a, din, s);
}
hipError_t mxfp4_quantize_launch(const MxQuantArgs& a, int din, hipStream_t s) {
  return mxq_launch<true>(a, din, s);
}

}  // namespace ddlb
