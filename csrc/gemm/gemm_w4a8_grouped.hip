// Tiled W4A8 GEMM: the grouped form (GemmArgs::grp_offs) with a dense output.
#include "gemm_w4a8_kernels.h"

namespace ddlb {

hipError_t launch_w4a8_grouped(const GemmArgs& p, int dout, int tile, hipStream_t s) {
  return dispatch_out(dout, [&](auto o) {
    return launch_w4a8_t<decltype(o)::value, true>(p, tile, s);
  });
}

}  // namespace ddlb
