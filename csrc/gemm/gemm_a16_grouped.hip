// Tiled A16 GEMM: the grouped form (GemmArgs::grp_offs).
#include "gemm_a16_kernels.h"

namespace ddlb {

hipError_t launch_a16_grouped(const GemmArgs& p, int din, int dout, int dw, int tile,
                              hipStream_t s) {
  return launch_a16_forms<true>(p, din, dout, dw, tile, s);
}

}  // namespace ddlb
