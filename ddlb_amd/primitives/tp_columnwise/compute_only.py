"""compute_only TP-Columnwise: the GEMM alone, no communication.

Parity: ``ddlb/primitives/TPColumnwise/compute_only.py:8-55`` (option ``size``).
Added option ``gemm``: ``hip`` = our MFMA kernel (weight stored ``[n, k]``), ``torch`` =
``torch.matmul`` (hipBLASLt on GPU, the only choice on CPU), ``auto`` = hip on GPU.
Added option ``quant``: ``none``, or ``mx`` = the bf16 / f16 activation is quantised to MX-fp8
(e4m3 + one E8M0 scale per 32 K elements) inside the timed step and multiplied with the weight
quantised at set-up by the block-scaled GEMM (:class:`MxQuantGemm`): what an fp8 linear layer
pays. It is validated against the product of the dequantised operands. ``mxfp4`` is the same
through MXFP4 (E2M1 elements, the block-scaled fp4 GEMM; ``k % 256 == 0``).

Unlike the reference, ``size=sharded`` is validated too (against the local rows) instead of
being skipped (``compute_only.py:52-53``). Its TFLOPS keeps the reference's ``2*m*n*k``
numerator, which over-counts by ``d`` — kept for comparability.
"""

from __future__ import annotations

from ddlb_amd.primitives.tp_columnwise.base import TPColumnwise
from ddlb_amd.primitives.gemm_select import QUANT_CHOICES, GemmBackend, MxQuantGemm


class ComputeOnlyTPColumnwise(TPColumnwise):
    DEFAULT_OPTIONS = {"size": "sharded", "gemm": "auto", "quant": "none"}
    ALLOWED_VALUES = {"size": ["sharded", "unsharded"], "gemm": ["auto", "hip", "torch", "torch_nt"],
                      "quant": QUANT_CHOICES}

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.size = self.options["size"]
        self.a_in = self.A_unsharded if self.size == "unsharded" else self.A
        self.gemm = GemmBackend(self.options["gemm"], self.device, self.dtype)
        quant = self.options["quant"]
        self.mx = MxQuantGemm(self.gemm, self.k, quant) if quant != "none" else None
        self.w = (self.mx or self.gemm).prepare_weight(self.B)
        self.out = self.gemm.alloc_out(self.a_in.shape[0], self.n)

    def run(self):
        if self.mx is not None:
            return self.mx(self.a_in, self.out)
        return self.gemm(self.a_in, self.w, self.out)

    def expected(self):
        """fp32 reference of this rank's rows; with ``quant=mx`` the product of the DEQUANTISED
        reference-quantised operands (:meth:`MxQuantGemm.expected` says why)."""
        if self.mx is not None:
            return self.mx.expected(self.a_in, self.B)
        if self.size == "unsharded":
            return self._ref_matmul(self.A_unsharded, self.B)
        return self._ref_matmul(self.A, self.B)
