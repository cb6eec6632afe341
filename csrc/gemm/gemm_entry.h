// Per-(input, output)-dtype launch entry points (one translation unit each), used by
// gemm_launch() in gemm_mfma.hip.
#pragma once
#include "gemm.h"

namespace ddlb {
hipError_t launch_fast_bf16_bf16(const GemmArgs& p, int tile, hipStream_t s);
hipError_t launch_fast_bf16_f32(const GemmArgs& p, int tile, hipStream_t s);
hipError_t launch_fast_f16_f16(const GemmArgs& p, int tile, hipStream_t s);
hipError_t launch_fast_f16_f32(const GemmArgs& p, int tile, hipStream_t s);
hipError_t launch_fast_fp8_bf16(const GemmArgs& p, int tile, hipStream_t s);
hipError_t launch_fast_fp8_f16(const GemmArgs& p, int tile, hipStream_t s);
hipError_t launch_fast_fp8_f32(const GemmArgs& p, int tile, hipStream_t s);
hipError_t launch_fast_f32_f32(const GemmArgs& p, int tile, hipStream_t s);
hipError_t launch_fast_mx(const GemmArgs& p, int dout, int tile, hipStream_t s);
// MX-fp8 with block scales (GemmArgs::a_scale / b_scale): the tiled kernel, offered tiles only
hipError_t launch_fast_mxs(const GemmArgs& p, int dout, int tile, hipStream_t s);
// MXFP4 with block scales (DT_FP4 operands): the tiled kernel, offered tiles only
hipError_t launch_fast_mx4(const GemmArgs& p, int dout, int tile, hipStream_t s);
// Quantised output (GemmArgs::c_scale): MX-fp8 / MXFP4 data and block scales out of the tiled
// kernel's epilogue; din bf16 / f16 / fp8 with scales / fp4 with scales, offered tiles only
hipError_t launch_qout_fp8(const GemmArgs& p, int din, int tile, hipStream_t s);
hipError_t launch_qout_fp4(const GemmArgs& p, int din, int tile, hipStream_t s);
hipError_t launch_generic(const GemmArgs& p, int din, int dout, hipStream_t s);
// Grouped launches (GemmArgs::grp_offs): gemm_launch calls launch_grouped (gemm_grouped.hip), which
// picks the translation unit by operands (bf16, f16, fp8 with scales, fp4 with scales) and output
// (dense: gemm_grouped_<in>.hip; fp8 / fp4 with c_scale: gemm_grouped_<in>_q.hip).
// launch_grouped is declared weak so that a host program which links gemm_mfma.hip against its own
// set of entries without this one still links; gemm_launch answers hipErrorNotSupported for a
// grouped launch where it is absent, and the extension always holds it.
hipError_t launch_grouped(const GemmArgs& p, int din, int dout, int tile, hipStream_t s)
    __attribute__((weak));
hipError_t launch_grouped_bf16(const GemmArgs& p, int dout, int tile, hipStream_t s);
hipError_t launch_grouped_f16(const GemmArgs& p, int dout, int tile, hipStream_t s);
hipError_t launch_grouped_mxs(const GemmArgs& p, int dout, int tile, hipStream_t s);
hipError_t launch_grouped_mx4(const GemmArgs& p, int dout, int tile, hipStream_t s);
hipError_t launch_grouped_bf16_q(const GemmArgs& p, int dout, int tile, hipStream_t s);
hipError_t launch_grouped_f16_q(const GemmArgs& p, int dout, int tile, hipStream_t s);
hipError_t launch_grouped_mxs_q(const GemmArgs& p, int dout, int tile, hipStream_t s);
hipError_t launch_grouped_mx4_q(const GemmArgs& p, int dout, int tile, hipStream_t s);
// K-grouped launches (GemmArgs::kgrouped): gemm_launch calls launch_kgrouped (gemm_kgrouped.hip),
// which picks the translation unit by operands (fp8 / fp4 with scales: gemm_kgrouped_<in>.hip).
// Weak for the same reason as launch_grouped.
hipError_t launch_kgrouped(const GemmArgs& p, int din, int dout, int tile, hipStream_t s)
    __attribute__((weak));
hipError_t launch_kgrouped_mxs(const GemmArgs& p, int dout, int tile, hipStream_t s);
hipError_t launch_kgrouped_mx4(const GemmArgs& p, int dout, int tile, hipStream_t s);

// Dispatch of the fast (MFMA) family by dtype pair; hipErrorInvalidValue if not provided.
inline hipError_t launch_fast(const GemmArgs& p, int din, int dout, int tile, hipStream_t s) {
  if (din == DT_BF16 && dout == DT_BF16) return launch_fast_bf16_bf16(p, tile, s);
  if (din == DT_BF16 && dout == DT_F32) return launch_fast_bf16_f32(p, tile, s);
  if (din == DT_F16 && dout == DT_F16) return launch_fast_f16_f16(p, tile, s);
  if (din == DT_F16 && dout == DT_F32) return launch_fast_f16_f32(p, tile, s);
  if (din == DT_FP8 && dout == DT_BF16) return launch_fast_fp8_bf16(p, tile, s);
  if (din == DT_FP8 && dout == DT_F16) return launch_fast_fp8_f16(p, tile, s);
  if (din == DT_FP8 && dout == DT_F32) return launch_fast_fp8_f32(p, tile, s);
  if (din == DT_F32 && dout == DT_F32) return launch_fast_f32_f32(p, tile, s);
  return hipErrorInvalidValue;
}
}  // namespace ddlb
