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


QUANT_CHOICES = ["none", "mx", "mxfp4"]


class MxQuantGemm:
    """``quant=mx`` of the compute_only slots: a bf16 / f16 activation through the fp8 matrix
    pipe, as an fp8 linear layer runs it. The ``[n, k]`` weight is quantised once at set-up
    (:func:`ddlb_amd.ops.mx.quantize_mx`); every call quantises the activation and runs the
    block-scaled GEMM, both on the clock. Output in the benchmark dtype. HIP kernels only: it
    raises at construction on a CPU device, with ``gemm=torch`` or for another dtype.

    ``quant=mxfp4`` is the same recipe through MXFP4 (E2M1 elements, ``k % 256 == 0``):
    :func:`ddlb_amd.ops.mx.quantize_mxfp4` and the block-scaled fp4 GEMM."""

    def __init__(self, backend: GemmBackend, k: int, quant: str = "mx"):
        if quant not in ("mx", "mxfp4"):
            raise ValueError(f"quant={quant} is not a block-scaled format (mx, mxfp4)")
        name = f"quant={quant}"
        if backend.dtype_name not in ("bfloat16", "float16"):
            raise ValueError(f"{name} quantises bfloat16 or float16 inputs, not "
                             f"{backend.dtype_name}")
        if backend.device.type != "cuda":
            raise ValueError(f"{name} needs a ROCm GPU (the quantiser and the scaled GEMM are "
                             "HIP kernels)")
        if backend.choice != "hip":
            raise ValueError(f"{name} runs the hip GEMM, not gemm={backend.choice}")
        kmod = 256 if quant == "mxfp4" else 128
        if k % kmod:
            raise ValueError(f"{name} needs the GEMM's K ({k}) to be a multiple of {kmod}")
        from ddlb_amd.ops import gemm as _g
        from ddlb_amd.ops import mx as _mx

        self._g, self._mx = _g, _mx
        if quant == "mxfp4":
            self._quant, self._ref, self._dq = (_mx.quantize_mxfp4, _mx.quantize_mxfp4_reference,
                                                _mx.dequantize_mxfp4)
        else:
            self._quant, self._ref, self._dq = (_mx.quantize_mx, _mx.quantize_mx_reference,
                                                _mx.dequantize_mx)
        self.wq = self.ws = None

    def prepare_weight(self, b):
        """``b`` is ``[k, n]``; quantised as the ``[n, k]`` weight the kernel reads."""
        self.wq, self.ws = self._quant(b.t().contiguous())
        return self.wq

    def __call__(self, a, out):
        aq, a_s = self._quant(a)
        return self._g.gemm(aq, self.wq, out=out, a_scale=a_s, w_scale=self.ws)

    def expected(self, a, b):
        """fp32 product of the DEQUANTISED reference-quantised operands: what the scaled GEMM
        is asked to compute. Against the unquantised product the format's own error (up to 1.85
        at k = 1024 with U[-1, 1) inputs) exceeds DDLB's ``atol = 1e-3 k``, so that rule would
        judge the number format and not the kernels."""
        a_dq = self._dq(*self._ref(a))
        w_dq = self._dq(*self._ref(b.t().contiguous()))
        return a_dq @ w_dq.t()
