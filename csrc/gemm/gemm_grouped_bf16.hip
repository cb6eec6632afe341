// gemm_grouped_bf16: the grouped form of the tiled kernel (GemmArgs::grp_offs;
// gemm_tn_kernel<.., TILE_GROUPED_M>, gemm_grouped_kernels.h), ungated and gated, the four codes of
// mxs_offers(): bf16 operands, bf16 / f32 out.
#include "gemm_grouped_kernels.h"
#include "gemm_entry.h"

namespace ddlb {
hipError_t launch_grouped_bf16(const GemmArgs& p, int dout, int tile, hipStream_t s) {
  return launch_grouped_t<MmaBF16, DT_BF16, false>(p, dout, tile, s);
}
}  // namespace ddlb
