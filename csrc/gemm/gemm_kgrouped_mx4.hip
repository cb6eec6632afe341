// gemm_kgrouped_mx4: the K-grouped form of the tiled kernel (GemmArgs::kgrouped;
// gemm_tn_kernel<.., TILE_GROUPED_K>, gemm_kgrouped_kernels.h), the four codes of mxs_offers():
// block-scaled fp4 operands, bf16 / f16 / f32 out.
#include "gemm_kgrouped_kernels.h"
#include "gemm_entry.h"

namespace ddlb {
hipError_t launch_kgrouped_mx4(const GemmArgs& p, int dout, int tile, hipStream_t s) {
  return launch_kgrouped_t<MmaMX4S>(p, dout, tile, s);
}
}  // namespace ddlb
