"""Select and drive the local GEMM used by the compute_only / pytorch / native slots.

``hip``   : our CDNA4 MFMA kernels (:mod:`ddlb_amd.ops.gemm`); weights are stored ``[n, k]``
            (K-contiguous, the layout both MFMA operands want — the same layout
            ``te.Linear`` keeps its weight in).
``torch`` : ``torch.matmul`` (hipBLASLt / rocBLAS on GPU, ATen on CPU) — the vendor baseline, with
            the reference's ``[k, n]`` weight (``TPColumnwise/pytorch.py:97``).
``torch_nt``: ``F.linear`` on the ``[n, k]`` weight — hipBLASLt's fastest layout (the one our
            kernels use), so the vendor comparison is like for like.
``auto``  : ``hip`` on a GPU, ``torch`` on the CPU. On a GPU ``auto`` never silently falls back:
            a missing extension raises (the driver checks the native library really ran).
"""

from __future__ import annotations

from ddlb_amd.primitives.base import output_dtype


class GemmBackend:
    def __init__(self, choice: str, device, dtype_name: str):
        self.device = device
        self.dtype_name = dtype_name
        self.out_dtype = output_dtype(dtype_name)
        if choice == "auto":
            choice = "hip" if device.type == "cuda" else "torch"
        if choice == "hip" and device.type != "cuda":
            raise RuntimeError("gemm=hip needs a ROCm GPU; use gemm=torch on the CPU")
        self.choice = choice
        if choice == "hip":
            from ddlb_amd.ops import gemm as _g

            _g.check_supported(dtype_name)
            self._hip = _g

    def prepare_weight(self, b):
        """``b`` is ``[k, n]``; the HIP kernel (and F.linear) consume ``[n, k]``."""
        if self.choice in ("hip", "torch_nt"):
            return b.t().contiguous()
        return b

    def alloc_out(self, rows: int, cols: int):
        import torch

        return torch.empty((rows, cols), dtype=self.out_dtype, device=self.device)

    def __call__(self, a, w, out=None):
        if self.choice == "hip":
            return self._hip.gemm(a, w, out=out)
        import torch

        if a.dtype == torch.float8_e4m3fn:
            a, w = a.to(torch.bfloat16), w.to(torch.bfloat16)
        if self.choice == "torch_nt":
            return torch.nn.functional.linear(a, w)
        if out is not None:
            return torch.matmul(a, w, out=out)
        return torch.matmul(a, w)


QUANT_CHOICES = ["none", "mx"]


class MxQuantGemm:
    """``quant=mx`` of the compute_only slots: a bf16 / f16 activation through the fp8 matrix
    pipe, as an fp8 linear layer runs it. The ``[n, k]`` weight is quantised once at set-up
    (:func:`ddlb_amd.ops.mx.quantize_mx`); every call quantises the activation and runs the
    block-scaled GEMM, both on the clock. Output in the benchmark dtype. HIP kernels only: it
    raises at construction on a CPU device, with ``gemm=torch`` or for another dtype."""

    def __init__(self, backend: GemmBackend, k: int):
        if backend.dtype_name not in ("bfloat16", "float16"):
            raise ValueError(f"quant=mx quantises bfloat16 or float16 inputs, not "
                             f"{backend.dtype_name}")
        if backend.device.type != "cuda":
            raise ValueError("quant=mx needs a ROCm GPU (the quantiser and the scaled GEMM are "
                             "HIP kernels)")
        if backend.choice != "hip":
            raise ValueError(f"quant=mx runs the hip GEMM, not gemm={backend.choice}")
        if k % 128:
            raise ValueError(f"quant=mx needs the GEMM's K ({k}) to be a multiple of 128")
        from ddlb_amd.ops import gemm as _g
        from ddlb_amd.ops import mx as _mx

        self._g, self._mx = _g, _mx
        self.wq = self.ws = None

    def prepare_weight(self, b):
        """``b`` is ``[k, n]``; quantised as the ``[n, k]`` weight the kernel reads."""
        self.wq, self.ws = self._mx.quantize_mx(b.t().contiguous())
        return self.wq

    def __call__(self, a, out):
        aq, a_s = self._mx.quantize_mx(a)
        return self._g.gemm(aq, self.wq, out=out, a_scale=a_s, w_scale=self.ws)

    def expected(self, a, b):
        """fp32 product of the DEQUANTISED reference-quantised operands: what the scaled GEMM
        is asked to compute. Against the unquantised product the format's own error (up to 1.85
        at k = 1024 with U[-1, 1) inputs) exceeds DDLB's ``atol = 1e-3 k``, so that rule would
        judge the number format and not the kernels."""
        ref = self._mx.quantize_mx_reference
        a_dq = self._mx.dequantize_mx(*ref(a))
        w_dq = self._mx.dequantize_mx(*ref(b.t().contiguous()))
        return a_dq @ w_dq.t()
