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

``kernel="skinny"`` (decode: ``seq <= 64``) runs both layers on the weight-streaming
``ops.gemm.gemm_skinny`` instead of the tiled kernel: fc1 with the quantised output, gated or
``act`` only, straight into fc2. ``fused=False`` there is the chain the fused epilogue replaces
(gated: f32 fc1, ``ops.glu.glu``, the row quantiser; else bf16 fc1 and the row quantiser).

``fmt="w4a8"`` (``kernel="skinny"``, or ``"mixed"`` below) keeps the weights in MXFP4 and the activations in
MX-fp8: ``X`` is quantised with ``quantize_mx``, fc1 writes MX-fp8 (``out_quant="mx"``), and both
layers run ``gemm_skinny``'s mixed pair, so they stream the fp4 bytes and only the weights pay
the 4-bit error.

``kernel="mixed"`` (``fmt="w4a8"`` only, any ``seq``: prefill) runs the same chain on the tiled
W4A8 kernel, ``ops.gemm.gemm_w4a8``: fc1 with ``act`` / ``glu`` and ``out_quant="mx"``, then
fc2. ``fused=False`` there is bf16 fc1 and the row quantiser (gated: f32 fc1, ``ops.glu.glu``,
the row quantiser).

``fmt="w4a16"`` / ``"w8a16"`` (``kernel="skinny"``, or ``"a16"`` below) is weight-only
quantisation: MXFP4 / MX-fp8 weights, ``X`` and ``H`` stay 16-bit and nothing is quantised per
forward. Both layers run ``ops.gemm.gemm_skinny_a16`` (fc1 with ``act`` / ``glu``, writing ``H``
in ``X``'s dtype). ``reference_chain`` for them: the dequantised weights, ``H`` rounded to ``X``'s
dtype between the layers.

``kernel="a16"`` (``fmt="w4a16"`` / ``"w8a16"`` only, any ``seq``: prefill) runs the same chain on
the tiled A16 kernel, ``ops.gemm.gemm_a16``: fc1 with ``act`` / ``glu`` and ``H`` in ``X``'s
dtype, then fc2.

``reference()`` is the torch chain on the dequantised operands in fp32:
``dequantize(quantize_reference(act(Xd @ W1d.T))) @ W2d.T`` (gated: ``glu_reference`` of the
``[S, 2F]`` product in place of ``act``).
"""

from __future__ import annotations

FMTS = ("mx", "mxfp4", "w4a8", "w4a16", "w8a16")
A16 = "a16"  # the activation "format" of the weight-only formats: not quantised
KERNELS = ("tiled", "skinny", "mixed", "a16")
SKINNY_ROWS = 64  # the rows one pass over the weights serves (gemm_skinny)


def _fmt_ops(fmt: str):
    """(HIP quantiser, torch reference quantiser, dequantiser) of a format."""
    from ddlb_amd.ops import mx

    if fmt == "mx":
        return mx.quantize_mx, mx.quantize_mx_reference, mx.dequantize_mx
    if fmt == "mxfp4":
        return mx.quantize_mxfp4, mx.quantize_mxfp4_reference, mx.dequantize_mxfp4
    raise ValueError(f"fmt must be one of {FMTS}, not {fmt!r}")


def _fmt_pair(fmt: str):
    """``(activation format, weight format)`` of a model format: the same but for ``"w4a8"`` and
    the weight-only formats (activations :data:`A16`)."""
    if fmt not in FMTS:
        raise ValueError(f"fmt must be one of {FMTS}, not {fmt!r}")
    mixed = {"w4a8": ("mx", "mxfp4"), "w4a16": (A16, "mxfp4"), "w8a16": (A16, "mx")}
    return mixed.get(fmt, (fmt, fmt))


def _check_fmt_kernel(fmt: str, kernel: str) -> int:
    """The format's refusals that the models share; returns what hidden and ffn are multiples
    of (the K-tile of the narrower operand)."""
    afmt, wfmt = _fmt_pair(fmt)
    if kernel == "mixed":
        if fmt != "w4a8":
            raise ValueError(f"kernel='mixed' is the tiled W4A8 GEMM: it takes fmt='w4a8' only, "
                             f"not fmt={fmt!r}")
    elif kernel == "a16":
        if afmt != A16:
            raise ValueError(f"kernel='a16' is the tiled A16 GEMM: it takes fmt='w4a16' / "
                             f"'w8a16' only, not fmt={fmt!r}")
    elif afmt != wfmt and kernel != "skinny":
        raise ValueError(f"fmt={fmt!r} needs kernel='skinny': only the skinny GEMMs multiply "
                         "MX-fp8 or 16-bit activations by narrower MX weights, the tiled kernel "
                         "takes one format for both operands (fmt='w4a8' also runs at any seq "
                         "with kernel='mixed', the tiled W4A8 GEMM; fmt='w4a16' / 'w8a16' with "
                         "kernel='a16', the tiled A16 GEMM)")
    return 256 if wfmt == "mxfp4" else 128


class MxMLP:
    gated = False  # the ungated block unless the constructor is told otherwise

    def __init__(self, hidden: int, ffn: int, seq: int, dtype: str = "bfloat16",
                 act: str = "gelu", fmt: str = "mx", fused: bool = True, tile: str = "auto",
                 seed: int = 0, gated: bool = False, kernel: str = "tiled"):
        import torch

        from ddlb_amd.ops.gemm import ACTS, pack_glu
        from ddlb_amd.primitives.base import torch_dtype, uniform_pm1

        self.afmt, self.wfmt = _fmt_pair(fmt)
        if act not in ACTS:
            raise ValueError(f"act must be one of {tuple(ACTS)}, not {act!r}")
        if dtype not in ("bfloat16", "float16"):
            raise TypeError(f"MxMLP takes bfloat16 / float16 activations, not {dtype}")
        if kernel not in KERNELS:
            raise ValueError(f"kernel must be one of {KERNELS}, not {kernel!r}")
        mod = _check_fmt_kernel(fmt, kernel)
        if hidden % mod or ffn % mod:
            raise ValueError(f"fmt={fmt!r} needs hidden and ffn to be multiples of {mod} "
                             f"(hidden = {hidden}, ffn = {ffn})")
        if seq <= 0:
            raise ValueError("seq must be positive")
        if kernel == "skinny" and seq > SKINNY_ROWS:
            raise ValueError(f"kernel='skinny' is for seq <= {SKINNY_ROWS}, not {seq}: past that "
                             "the tiled kernel is the one to use")
        if not torch.cuda.is_available():
            raise RuntimeError("MxMLP runs the native block-scaled GEMMs: it needs a ROCm GPU "
                               "(MxMLP.reference_chain runs anywhere)")
        self.H, self.F, self.S = hidden, ffn, seq
        self.dtype, self.act, self.fmt, self.fused, self.tile = dtype, act, fmt, bool(fused), tile
        self.gated, self.kernel = bool(gated), kernel
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
        quant, _, _ = _fmt_ops(self.wfmt)
        self.w1q, self.w1s = quant(self.W1)
        self.w2q, self.w2s = quant(self.W2)
        odt = tdt if self.afmt == A16 else torch.bfloat16  # weight-only: X's dtype throughout
        self.out = torch.empty((seq, hidden), dtype=odt, device=dev)
        torch.cuda.synchronize()

    @property
    def flops(self) -> float:
        """FLOPs of one forward: 2 S H F for each of the two GEMMs (gated: fc1 has 2F rows)."""
        return (6.0 if self.gated else 4.0) * self.S * self.H * self.F

    def forward(self):
        import torch

        from ddlb_amd.ops.gemm import gemm

        if self.kernel == "a16":  # weight-only at any seq: the tiled A16 GEMM
            from ddlb_amd.ops.gemm import gemm_a16

            h = gemm_a16(self.X, self.w1q, w_scale=self.w1s, act=self.act, glu=self.gated,
                         tile=self.tile)
            return gemm_a16(h, self.w2q, self.out, w_scale=self.w2s, tile=self.tile)
        if self.afmt == A16:  # weight-only: nothing is quantised per forward
            from ddlb_amd.ops.gemm import gemm_skinny_a16

            h = gemm_skinny_a16(self.X, self.w1q, w_scale=self.w1s, act=self.act, glu=self.gated)
            return gemm_skinny_a16(h, self.w2q, self.out, w_scale=self.w2s)
        quant, _, _ = _fmt_ops(self.afmt)
        xq, xs = quant(self.X)
        glu = {"glu": True} if self.gated else {}
        if self.kernel == "skinny":
            return self._forward_skinny(xq, xs)
        if self.kernel == "mixed":
            return self._forward_mixed(xq, xs)
        if self.fused:
            hq, hs = gemm(xq, self.w1q, a_scale=xs, w_scale=self.w1s, act=self.act,
                          tile=self.tile, out_quant=self.fmt, **glu)
        else:
            h = gemm(xq, self.w1q, a_scale=xs, w_scale=self.w1s, act=self.act, tile=self.tile,
                     out_dtype=torch.bfloat16, **glu)
            hq, hs = quant(h)
        gemm(hq, self.w2q, self.out, a_scale=hs, w_scale=self.w2s, tile=self.tile)
        return self.out

    def _forward_skinny(self, xq, xs):
        import torch

        from ddlb_amd.ops.gemm import gemm_skinny

        quant, _, _ = _fmt_ops(self.afmt)
        fc1 = dict(a_scale=xs, w_scale=self.w1s)
        if self.fused:
            hq, hs = gemm_skinny(xq, self.w1q, act=self.act, glu=self.gated, out_quant=self.afmt,
                                 **fc1)
        elif self.gated:
            from ddlb_amd.ops.glu import glu

            hq, hs = quant(glu(gemm_skinny(xq, self.w1q, out_dtype=torch.float32, **fc1),
                               self.act))
        else:
            hq, hs = quant(gemm_skinny(xq, self.w1q, act=self.act, **fc1))
        gemm_skinny(hq, self.w2q, self.out, a_scale=hs, w_scale=self.w2s)
        return self.out

    def _forward_mixed(self, xq, xs):
        import torch

        from ddlb_amd.ops.gemm import gemm_w4a8
        from ddlb_amd.ops.mx import quantize_mx

        fc1 = dict(a_scale=xs, w_scale=self.w1s, tile=self.tile)
        if self.fused:
            hq, hs = gemm_w4a8(xq, self.w1q, act=self.act, glu=self.gated, out_quant="mx", **fc1)
        elif self.gated:
            from ddlb_amd.ops.glu import glu

            hq, hs = quantize_mx(glu(gemm_w4a8(xq, self.w1q, out_dtype=torch.float32, **fc1),
                                     self.act))
        else:
            hq, hs = quantize_mx(gemm_w4a8(xq, self.w1q, act=self.act, **fc1))
        gemm_w4a8(hq, self.w2q, self.out, a_scale=hs, w_scale=self.w2s, tile=self.tile)
        return self.out

    @staticmethod
    def reference_chain(X, W1, W2, act: str = "gelu", fmt: str = "mx", gated: bool = False):
        """The fp32 torch chain on dequantised operands (any device):
        ``dequantize(quantize_reference(act(Xd @ W1d.T))) @ W2d.T``. ``gated``: ``W1`` is the
        packed ``[2F, H]`` weight and ``glu_reference`` stands in place of ``act``. Each operand
        goes through its own format (``"w4a8"``: ``X`` and ``h`` MX-fp8, the weights MXFP4)."""
        import torch

        from ddlb_amd.ops.gemm import ACTS, glu_reference
        from ddlb_amd.parallel.sim import apply_act

        afmt, wfmt = _fmt_pair(fmt)
        _, wqref, wdeq = _fmt_ops(wfmt)
        if afmt == A16:  # not quantised: X as it is, h rounded to X's dtype between the layers
            def through(t):
                return t.to(X.dtype).to(torch.float32)
        else:
            _, qref, deq = _fmt_ops(afmt)

            def through(t):
                return deq(*qref(t))
        xd = through(X)
        w1d, w2d = (wdeq(*wqref(t)) for t in (W1, W2))
        c = (xd @ w1d.t()).to(torch.float32)
        h = glu_reference(c, act) if gated else apply_act(c, ACTS[act]).to(torch.float32)
        return through(h) @ w2d.t()

    def reference(self):
        return self.reference_chain(self.X, self.W1, self.W2, self.act, self.fmt, self.gated)

    def validate(self, out=None) -> None:
        """The benchmark's own bound for 8-bit types: ``rtol = 0, atol = 1e-3 k`` with ``k`` the
        reduction length of the GEMM that produced the result (fc2: ``ffn``)."""
        import torch

        out = self.out if out is None else out
        torch.testing.assert_close(out.float(), self.reference(), rtol=0, atol=1e-3 * self.F)
