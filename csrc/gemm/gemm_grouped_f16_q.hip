// gemm_grouped_f16_q: the grouped form of the tiled kernel (GemmArgs::grp_offs;
// gemm_tn_kernel<.., TILE_GROUPED_M>, gemm_grouped_kernels.h), ungated and gated, the four codes of
// mxs_offers(): f16 operands, MX-fp8 / MXFP4 out.
#include "gemm_grouped_kernels.h"
#include "gemm_entry.h"

namespace ddlb {
hipError_t launch_grouped_f16_q(const GemmArgs& p, int dout, int tile, hipStream_t s) {
  return launch_grouped_t<MmaF16, DT_F16, true>(p, dout, tile, s);
}
}  // namespace ddlb
