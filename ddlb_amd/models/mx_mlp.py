"""One-GPU MLP block on the block-scaled matrix pipe, end to end in MX-fp8 or MXFP4.

    Xq, sX = quantise(X)                                   per forward (streaming quantiser)
    Hq, sH = act(Xq @ W1q.T)   quantised in the epilogue   fc1: block-scaled GEMM, (q, s) out
    Y      = Hq @ W2q.T                                    fc2: block-scaled GEMM, bf16 out

``X [S, H]``, ``W1 [F, H]``, ``W2 [H, F]`` (weights K-contiguous, quantised once at set-up). With
``fused=True`` fc1's epilogue writes the ``[S, F]`` activation as quantised data and E8M0 scales
(``ops.gemm.gemm(..., out_quant=)``), blocks along F, the layout fc2 reads along its K. With
``fused=False`` fc1 writes bf16 and the streaming quantiser reads it back: one more launch, and
one more rounding (to bf16, before the quantisation).

``gated=True`` is the Llama-style block ``h = act(X Wg.T) * (X Wu.T)``: ``W1 = pack_glu(Wg, Wu)``
is ``[2F, H]`` (gate and up rows interleaved in groups of 32, quantised once like any weight) and
fc1 runs with ``glu=True``, so the product is formed in the GEMM's epilogue and ``h`` is still
``[S, F]``; fused or not as above.

``reference()`` is the torch chain on the dequantised operands in fp32:
``dequantize(quantize_reference(act(Xd @ W1d.T))) @ W2d.T`` (gated: ``glu_reference`` of the
``[S, 2F]`` product in place of ``act``).
"""

from __future__ import annotations

FMTS = ("mx", "mxfp4")


def _fmt_ops(fmt: str):
    """(HIP quantiser, torch reference quantiser, dequantiser) of a format."""
    from ddlb_amd.ops import mx

    if fmt == "mx":
        return mx.quantize_mx, mx.quantize_mx_reference, mx.dequantize_mx
    if fmt == "mxfp4":
        return mx.quantize_mxfp4, mx.quantize_mxfp4_reference, mx.dequantize_mxfp4
    raise ValueError(f"fmt must be one of {FMTS}, not {fmt!r}")


class MxMLP:
    gated = False  # the ungated block unless the constructor is told otherwise

    def __init__(self, hidden: int, ffn: int, seq: int, dtype: str = "bfloat16",
                 act: str = "gelu", fmt: str = "mx", fused: bool = True, tile: str = "auto",
                 seed: int = 0, gated: bool = False):
        import torch

        from ddlb_amd.ops.gemm import ACTS, pack_glu
        from ddlb_amd.primitives.base import torch_dtype, uniform_pm1

        _fmt_ops(fmt)
        if act not in ACTS:
            raise ValueError(f"act must be one of {tuple(ACTS)}, not {act!r}")
        if dtype not in ("bfloat16", "float16"):
            raise TypeError(f"MxMLP takes bfloat16 / float16 activations, not {dtype}")
        mod = 256 if fmt == "mxfp4" else 128
        if hidden % mod or ffn % mod:
            raise ValueError(f"fmt={fmt!r} needs hidden and ffn to be multiples of {mod} "
                             f"(hidden = {hidden}, ffn = {ffn})")
        if seq <= 0:
            raise ValueError("seq must be positive")
        if not torch.cuda.is_available():
            raise RuntimeError("MxMLP runs the native block-scaled GEMMs: it needs a ROCm GPU "
                               "(MxMLP.reference_chain runs anywhere)")
        self.H, self.F, self.S = hidden, ffn, seq
        self.dtype, self.act, self.fmt, self.fused, self.tile = dtype, act, fmt, bool(fused), tile
        self.gated = bool(gated)
        dev = torch.device("cuda", torch.cuda.current_device())
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        tdt = torch_dtype(dtype)
        self.X = uniform_pm1((seq, hidden), dtype, g, dev)
        self.W1 = (uniform_pm1((ffn, hidden), "float32", g, dev) * hidden ** -0.5).to(tdt)
        if self.gated:  # W1 above is the gate; the up rows follow it, interleaved in groups of 32
            up = (uniform_pm1((ffn, hidden), "float32", g, dev) * hidden ** -0.5).to(tdt)
            self.W1 = pack_glu(self.W1, up)
        self.W2 = (uniform_pm1((hidden, ffn), "float32", g, dev) * ffn ** -0.5).to(tdt)
        quant, _, _ = _fmt_ops(fmt)
        self.w1q, self.w1s = quant(self.W1)
        self.w2q, self.w2s = quant(self.W2)
        self.out = torch.empty((seq, hidden), dtype=torch.bfloat16, device=dev)
        torch.cuda.synchronize()

    @property
    def flops(self) -> float:
        """FLOPs of one forward: 2 S H F for each of the two GEMMs (gated: fc1 has 2F rows)."""
        return (6.0 if self.gated else 4.0) * self.S * self.H * self.F

    def forward(self):
        import torch

        from ddlb_amd.ops.gemm import gemm

        quant, _, _ = _fmt_ops(self.fmt)
        xq, xs = quant(self.X)
        glu = {"glu": True} if self.gated else {}
        if self.fused:
            hq, hs = gemm(xq, self.w1q, a_scale=xs, w_scale=self.w1s, act=self.act,
                          tile=self.tile, out_quant=self.fmt, **glu)
        else:
            h = gemm(xq, self.w1q, a_scale=xs, w_scale=self.w1s, act=self.act, tile=self.tile,
                     out_dtype=torch.bfloat16, **glu)
            hq, hs = quant(h)
        gemm(hq, self.w2q, self.out, a_scale=hs, w_scale=self.w2s, tile=self.tile)
        return self.out

    @staticmethod
    def reference_chain(X, W1, W2, act: str = "gelu", fmt: str = "mx", gated: bool = False):
        """The fp32 torch chain on dequantised operands (any device):
        ``dequantize(quantize_reference(act(Xd @ W1d.T))) @ W2d.T``. ``gated``: ``W1`` is the
        packed ``[2F, H]`` weight and ``glu_reference`` stands in place of ``act``."""
        import torch

        from ddlb_amd.ops.gemm import ACTS, glu_reference
        from ddlb_amd.parallel.sim import apply_act

        _, qref, deq = _fmt_ops(fmt)
        xd, w1d, w2d = (deq(*qref(t)) for t in (X, W1, W2))
        c = (xd @ w1d.t()).to(torch.float32)
        h = glu_reference(c, act) if gated else apply_act(c, ACTS[act]).to(torch.float32)
        return deq(*qref(h)) @ w2d.t()

    def reference(self):
        return self.reference_chain(self.X, self.W1, self.W2, self.act, self.fmt, self.gated)

    def validate(self, out=None) -> None:
        """The benchmark's own bound for 8-bit types: ``rtol = 0, atol = 1e-3 k`` with ``k`` the
        reduction length of the GEMM that produced the result (fc2: ``ffn``)."""
        import torch

        out = self.out if out is None else out
        torch.testing.assert_close(out.float(), self.reference(), rtol=0, atol=1e-3 * self.F)
