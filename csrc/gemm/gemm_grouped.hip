// gemm_grouped: the entry of the grouped launches (GemmArgs::grp_offs), which sends a launch that
// gemm_launch has checked to the translation unit that holds its kernels. Host code only.
#include "gemm_entry.h"

namespace ddlb {
hipError_t launch_grouped(const GemmArgs& p, int din, int dout, int tile, hipStream_t s) {
  const bool q = dout == DT_FP8 || dout == DT_FP4, scaled = p.a_scale != nullptr;
  if (din == DT_BF16 && !scaled)
    return q ? launch_grouped_bf16_q(p, dout, tile, s) : launch_grouped_bf16(p, dout, tile, s);
  if (din == DT_F16 && !scaled)
    return q ? launch_grouped_f16_q(p, dout, tile, s) : launch_grouped_f16(p, dout, tile, s);
  if (din == DT_FP8 && scaled)
    return q ? launch_grouped_mxs_q(p, dout, tile, s) : launch_grouped_mxs(p, dout, tile, s);
  if (din == DT_FP4 && scaled)
    return q ? launch_grouped_mx4_q(p, dout, tile, s) : launch_grouped_mx4(p, dout, tile, s);
  return hipErrorInvalidValue;
}
}  // namespace ddlb
