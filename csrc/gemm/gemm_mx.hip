// gemm_mx: instantiations of the MFMA GEMM kernels (see gemm_mfma.hip).
#include "gemm_kernels.h"
#include "gemm_entry.h"

namespace ddlb {
hipError_t launch_fast_mx(const GemmArgs& p, int dout, int tile, hipStream_t s) {
  return dispatch_out(dout, [&](auto o) { return launch_mx_cfg<decltype(o)::value>(p, tile, s); });
}
}  // namespace ddlb
