// gemm_qout_fp8: the tiled kernel with the MX-fp8 quantising epilogue (e4m3 bytes + E8M0 block
// scales out; bf16 / f16 / block-scaled fp8 / block-scaled fp4 in; see gemm_kernels.h).
#include "gemm_kernels.h"
#include "gemm_entry.h"

namespace ddlb {
hipError_t launch_qout_fp8(const GemmArgs& p, int din, int tile, hipStream_t s) {
  return launch_qout<DT_FP8>(p, din, p.a_scale != nullptr, tile, s);
}
}  // namespace ddlb
