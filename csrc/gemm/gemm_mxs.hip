// gemm_mxs: the tiled kernel's block-scaled MX-fp8 instantiations (MmaMXS, see gemm_mfma.hip).
#include "gemm_kernels.h"
#include "gemm_entry.h"

namespace ddlb {
hipError_t launch_fast_mxs(const GemmArgs& p, int dout, int tile, hipStream_t s) {
  if (dout == DT_BF16) return launch_mxs_cfg<DT_BF16>(p, tile, s);
  if (dout == DT_F16) return launch_mxs_cfg<DT_F16>(p, tile, s);
  if (dout == DT_F32) return launch_mxs_cfg<DT_F32>(p, tile, s);
  return hipErrorInvalidValue;
}
}  // namespace ddlb
