// gemm_mxs: the tiled kernel's block-scaled MX-fp8 instantiations (MmaMXS, see gemm_mfma.hip).
#include "gemm_kernels.h"
#include "gemm_entry.h"

namespace ddlb {
hipError_t launch_fast_mxs(const GemmArgs& p, int dout, int tile, hipStream_t s) {
  // gemm_launch has checked the operands and mapped the tile code (mxs_tile_for)
  return dispatch_out(dout, [&](auto o) {
    return launch_tiled<MmaMXS, decltype(o)::value, mxs_offers>(p, tile, s);
  });
}
}  // namespace ddlb
