// gemm_kgrouped: the entry of the K-grouped launches (GemmArgs::kgrouped), which sends a launch
// that gemm_launch has checked to the translation unit that holds its kernels. Host code only.
#include "gemm_entry.h"

namespace ddlb {
hipError_t launch_kgrouped(const GemmArgs& p, int din, int dout, int tile, hipStream_t s) {
  if (din == DT_FP8) return launch_kgrouped_mxs(p, dout, tile, s);
  if (din == DT_FP4) return launch_kgrouped_mx4(p, dout, tile, s);
  return hipErrorInvalidValue;
}
}  // namespace ddlb
