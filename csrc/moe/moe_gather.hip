// Dense gather of the routed rows for gfx950: out[r, :] = x[row_token[r], :], +0.0 rows for an
// index outside [0, S) (moe.h MoeGatherArgs has the contract). The training path's permuted copy:
// mx_grouped_linear quantises its 16-bit rows twice (row-wise and grouped-transposed), so they
// are written once here; the inference path's quantize_mx_gather writes no such copy.
//
// A byte copy in 16-byte vectors, shaped like moe_combine.hip: 256 / (vectors per row) rows per
// workgroup pass when rows are short, one row striding when long, a grid-stride over the rows,
// the grid sized by the CU count, 64-bit byte offsets. No LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm/gemm.h"
#include "gemm/row_io.h"
#include "moe.h"

namespace ddlb {
namespace {

__global__ __launch_bounds__(kRowThreads) void moe_gather_kernel(const MoeGatherArgs a, int esz,
                                                                 int rows_pp) {
  const int vpr = (int)((int64_t)a.H * esz / 16);  // vectors per row
  int r_in, c0;
  row_lane(vpr, threadIdx.x, r_in, c0);
  if (r_in >= rows_pp) return;
  const int64_t step = (int64_t)gridDim.x * rows_pp;
  for (int64_t r = (int64_t)blockIdx.x * rows_pp + r_in; r < a.T; r += step) {
    const int tok = a.row_token[r];
    const bool valid = tok >= 0 && tok < a.S;  // otherwise nothing is read
    const char* xrow = (const char*)a.x + (int64_t)(valid ? tok : 0) * a.ldx * esz;
    char* orow = (char*)a.out + r * a.ldo * esz;
    for (int c = c0; c < vpr; c += kRowThreads) {
      mxq_u32x4 v = {0u, 0u, 0u, 0u};
      if (valid) v = *(const mxq_u32x4*)(xrow + (int64_t)c * 16);
      *(mxq_u32x4*)(orow + (int64_t)c * 16) = v;
    }
  }
}

}  // namespace

hipError_t moe_gather_launch(const MoeGatherArgs& a, int dt, hipStream_t s) {
  if (dt != DT_F32 && dt != DT_F16 && dt != DT_BF16) return hipErrorInvalidValue;
  if (a.S < 0 || a.T < 0 || a.H < 0) return hipErrorInvalidValue;
  if (a.T == 0 || a.H == 0) return hipSuccess;
  const int esz = dtype_size(dt);
  if (a.x == nullptr && a.S > 0) return hipErrorInvalidValue;
  if (a.row_token == nullptr || a.out == nullptr || ((int64_t)a.H * esz) % 16 || a.ldx < a.H ||
      a.ldo < a.H || ((uintptr_t)a.x & 15) || (a.ldx * esz) % 16 || ((uintptr_t)a.out & 15) ||
      (a.ldo * esz) % 16)
    return hipErrorInvalidValue;
  const int rows_pp = rows_per_pass((int)((int64_t)a.H * esz / 16));
  hipLaunchKernelGGL(moe_gather_kernel, dim3(row_grid(a.T, rows_pp)), dim3(kRowThreads), 0, s, a,
                     esz, rows_pp);
  return hipGetLastError();
}

}  // namespace ddlb
