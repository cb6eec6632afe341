// Tiled W4A8 GEMM: the MX-fp8 output (GemmArgs::c_scale), plain and grouped.
#include "gemm_w4a8_kernels.h"

namespace ddlb {

hipError_t launch_w4a8_q(const GemmArgs& p, int tile, hipStream_t s) {
  return p.grp_offs ? launch_w4a8_t<DT_FP8, true>(p, tile, s)
                    : launch_w4a8_t<DT_FP8, false>(p, tile, s);
}

}  // namespace ddlb
