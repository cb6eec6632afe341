// gemm_qout_fp4: the tiled kernel with the MXFP4 quantising epilogue (E2M1 nibble pairs + E8M0
// block scales out; bf16 / f16 / block-scaled fp8 / block-scaled fp4 in; see gemm_kernels.h).
#include "gemm_kernels.h"
#include "gemm_entry.h"

namespace ddlb {
hipError_t launch_qout_fp4(const GemmArgs& p, int din, int tile, hipStream_t s) {
  return launch_qout<DT_FP4>(p, din, p.a_scale != nullptr, tile, s);
}
}  // namespace ddlb
