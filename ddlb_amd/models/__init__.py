"""Model-level building blocks on top of the primitives.

* :mod:`ddlb_amd.models.shapes`  — TP GEMM shapes of real transformer layers (Llama 3, GPT-3,
  Qwen2, Mixtral) -> benchmark sweeps (``python -m ddlb_amd.models``).
* :mod:`ddlb_amd.models.tp_mlp`  — sequence-parallel TP MLP block (AG+GEMM+act -> GEMM+RS).
* :mod:`ddlb_amd.models.mx_mlp`  — one-GPU MLP on the block-scaled matrix pipe (MX-fp8 / MXFP4):
  fc1 writes its activation quantised from the GEMM epilogue, fc2 reads it.
* :mod:`ddlb_amd.models.mx_moe`  — one-GPU routed (mixture-of-experts) gated FFN: tokens sorted by
  expert on the device, one grouped GEMM launch per layer (``ops.gemm.gemm_grouped``).
* :mod:`ddlb_amd.models.mx_moe_ffn` — the trainable routed gated FFN: autograd through the
  dispatch, the GLU and the combine around two ``mx_grouped_linear`` layers.
* :mod:`ddlb_amd.models.mx_linear` — a trainable one-GPU MX linear layer: forward, dgrad and
  wgrad on the block-scaled GEMMs, operands quantised along each GEMM's own contraction axis.
"""

from ddlb_amd.models.shapes import MODELS, LayerGemm, ModelSpec, benchmark_configs, layer_gemms

__all__ = ["MODELS", "ModelSpec", "LayerGemm", "layer_gemms", "benchmark_configs"]
