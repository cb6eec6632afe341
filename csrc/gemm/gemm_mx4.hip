// gemm_mx4: the tiled kernel's block-scaled MXFP4 instantiations (MmaMX4S, see gemm_mfma.hip).
#include "gemm_kernels.h"
#include "gemm_entry.h"

namespace ddlb {
hipError_t launch_fast_mx4(const GemmArgs& p, int dout, int tile, hipStream_t s) {
  // gemm_launch has checked the operands and mapped the tile code (mxs_tile_for)
  return dispatch_out(dout, [&](auto o) {
    return launch_tiled<MmaMX4S, decltype(o)::value, mx4_offers>(p, tile, s);
  });
}
}  // namespace ddlb
