"""compute_only TP-Rowwise: the K-sharded partial GEMM alone (no reduce-scatter).

Not present in the reference (``ddlb/benchmark.py:51-55`` registers none for tp_rowwise); added
so the GEMM share of the rowwise pipelines can be measured on its own. ``size=sharded`` runs
``[m, k/d] x [k/d, n]`` (this rank's real work); ``unsharded`` runs the full ``[m, k] x [k, n]``.
Validation compares against the matching fp32 product. ``quant=mx``: the activation is quantised
to MX-fp8 inside the timed step and multiplied by the block-scaled GEMM, validated against the
product of the dequantised operands (see the columnwise slot and :class:`MxQuantGemm`);
``quant=mxfp4`` does the same through MXFP4 and the block-scaled fp4 GEMM.
"""

from __future__ import annotations

from ddlb_amd.primitives.gemm_select import QUANT_CHOICES, GemmBackend, MxQuantGemm
from ddlb_amd.primitives.tp_rowwise.base import TPRowwise


class ComputeOnlyTPRowwise(TPRowwise):
    DEFAULT_OPTIONS = {"size": "sharded", "gemm": "auto", "quant": "none"}
    ALLOWED_VALUES = {"size": ["sharded", "unsharded"], "gemm": ["auto", "hip", "torch", "torch_nt"],
                      "quant": QUANT_CHOICES}

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.size = self.options["size"]
        self.gemm = GemmBackend(self.options["gemm"], self.device, self.dtype)
        if self.size == "unsharded":
            self.a_in, b = self.A_unsharded, self.B_unsharded
        else:
            self.a_in, b = self.A, self.B
        self._b_ref = b
        quant = self.options["quant"]
        self.mx = MxQuantGemm(self.gemm, b.shape[0], quant) if quant != "none" else None
        self.w = (self.mx or self.gemm).prepare_weight(b)
        self.out = self.gemm.alloc_out(self.m, self.n)

    def run(self):
        if self.mx is not None:
            return self.mx(self.a_in, self.out)
        return self.gemm(self.a_in, self.w, self.out)

    def expected(self):
        """fp32 reference; with ``quant=mx`` the product of the DEQUANTISED reference-quantised
        operands (:meth:`MxQuantGemm.expected` says why)."""
        if self.mx is not None:
            return self.mx.expected(self.a_in, self._b_ref)
        return self._ref_matmul(self.a_in, self._b_ref)
