"""A trainable one-GPU linear layer on the block-scaled matrix pipe (MX-fp8 or MXFP4).

    Y  = X  @ W.T     forward, contracts K:  Xq  [M, K] x Wq  [N, K]
    dX = dY @ W       dgrad,   contracts N:  dYq [M, N] x Wtq [K, N]
    dW = dY.T @ X     wgrad,   contracts M:  dYtq [N, M] x Xtq [K, M]

``X [M, K]``, ``W [N, K]``, ``dY [M, N]``, bf16 or f16. MX scales lie along the contraction axis,
so every tensor is quantised twice, once along each of its axes; the second copy is stored
transposed, which makes its blocks K-contiguous rows for ``ops.gemm.gemm``. One two-way launch
(``ops.mx.quantize_mx_2way``) writes both copies and reads the tensor once: ``X`` and ``W`` in the
forward pass, ``dY`` in the backward pass. Saved for backward: the transposed copies of ``X`` and
``W`` (1 or 0.5 byte per element plus scales, not the bf16 tensors).

M, N and K are multiples of 128 (MXFP4: 256); another shape raises, nothing falls back to bf16.
There is no K-split: a wgrad with a long M and a small N x K runs on few tiles
(docs/RESULTS.md "Transposed MX quantiser / MX backward").

:func:`mx_linear_reference` is the same chain in torch on dequantised reference quantisations.
"""

from __future__ import annotations

import torch

FMTS = ("mx", "mxfp4")


def _mod(fmt: str) -> int:
    if fmt not in FMTS:
        raise ValueError(f"fmt must be one of {FMTS}, not {fmt!r}")
    return 256 if fmt == "mxfp4" else 128


def check_shapes(x, w, fmt: str, dy=None):
    """The layer's own refusals (any device). Returns ``(M, N, K)``."""
    mod = _mod(fmt)
    if x.dim() != 2 or w.dim() != 2:
        raise ValueError(f"mx_linear expects x [M, K] and w [N, K], not {tuple(x.shape)} and "
                         f"{tuple(w.shape)}")
    for name, t in (("x", x), ("w", w)):
        if t.dtype not in (torch.bfloat16, torch.float16):
            raise TypeError(f"mx_linear takes bfloat16 / float16 tensors, {name} is {t.dtype}")
    (M, K), (N, Kw) = x.shape, w.shape
    if K != Kw:
        raise ValueError(f"K mismatch: x {tuple(x.shape)} vs w {tuple(w.shape)}")
    if M % mod or N % mod or K % mod or 0 in (M, N, K):
        raise ValueError(f"mx_linear(fmt={fmt!r}) needs M, N and K to be positive multiples of "
                         f"{mod}: each is the contraction length of one of the three GEMMs "
                         f"(M, N, K = {M}, {N}, {K})")
    if dy is not None and tuple(dy.shape) != (M, N):
        raise ValueError(f"dy must have shape {(M, N)}, not {tuple(dy.shape)}")
    return M, N, K


class _MxLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, fmt, tile, w_quant):
        from ddlb_amd.ops.gemm import gemm
        from ddlb_amd.ops.mx import quantize_mx_2way

        check_shapes(x, w, fmt)
        xq, xs, xtq, xts = quantize_mx_2way(x.detach(), fmt=fmt)
        if w_quant is None:
            w_quant = quantize_mx_2way(w.detach(), fmt=fmt)
        wq, ws, wtq, wts = w_quant
        y = gemm(xq, wq, out_dtype=x.dtype, a_scale=xs, w_scale=ws, tile=tile)
        ctx.save_for_backward(xtq, xts, wtq, wts)
        ctx.fmt, ctx.tile, ctx.x_dtype, ctx.w_dtype = fmt, tile, x.dtype, w.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        from ddlb_amd.ops.gemm import gemm
        from ddlb_amd.ops.mx import quantize_mx_2way

        xtq, xts, wtq, wts = ctx.saved_tensors
        dyq, dys, dytq, dyts = quantize_mx_2way(dy.contiguous(), fmt=ctx.fmt)
        dx = dw = None
        if ctx.needs_input_grad[0]:  # [M, N] x [K, N] -> [M, K]
            dx = gemm(dyq, wtq, out_dtype=ctx.x_dtype, a_scale=dys, w_scale=wts, tile=ctx.tile)
        if ctx.needs_input_grad[1]:  # [N, M] x [K, M] -> [N, K]
            dw = gemm(dytq, xtq, out_dtype=ctx.w_dtype, a_scale=dyts, w_scale=xts,
                      tile=ctx.tile)
        return dx, dw, None, None, None


def mx_linear(x, w, fmt: str = "mx", tile: str = "auto", *, w_quant=None):
    """``y = x @ w.T`` on the block-scaled GEMM, differentiable in ``x`` and ``w``: backward runs
    dgrad and wgrad on the block-scaled GEMM as well (module docstring). ``w_quant``: the result
    of ``quantize_mx_2way(w, fmt=fmt)`` when the caller keeps it (:class:`MxLinear` does)."""
    return _MxLinearFn.apply(x, w, fmt, tile, w_quant)


class MxLinear(torch.nn.Module):
    """``y = x @ weight.T`` (no bias) through :func:`mx_linear`. The weight's two quantised
    copies are kept between calls and made again when the parameter's ``_version`` has moved
    (an optimiser step, any in-place write); ``n_quant`` counts the quantisations."""

    def __init__(self, in_features: int, out_features: int, fmt: str = "mx", tile: str = "auto",
                 dtype=torch.bfloat16, device=None, seed: int = 0):
        super().__init__()
        mod = _mod(fmt)
        if in_features % mod or out_features % mod or in_features <= 0 or out_features <= 0:
            raise ValueError(f"MxLinear(fmt={fmt!r}) needs in_features and out_features to be "
                             f"positive multiples of {mod} (got {in_features}, {out_features})")
        if dtype not in (torch.bfloat16, torch.float16):
            raise TypeError(f"MxLinear takes bfloat16 / float16 weights, not {dtype}")
        self.in_features, self.out_features, self.fmt, self.tile = (in_features, out_features,
                                                                    fmt, tile)
        g = torch.Generator().manual_seed(seed)
        w = (torch.rand(out_features, in_features, generator=g) * 2 - 1) * in_features ** -0.5
        self.weight = torch.nn.Parameter(w.to(device=device, dtype=dtype))
        self.n_quant = 0
        self._w_quant = None
        self._w_key = None

    def _quantised_weight(self):
        from ddlb_amd.ops.mx import quantize_mx_2way

        w = self.weight
        key = (w._version, w.data_ptr(), w.dtype)
        if self._w_key != key:
            self._w_quant = quantize_mx_2way(w.detach(), fmt=self.fmt)
            self._w_key = key
            self.n_quant += 1
        return self._w_quant

    def forward(self, x):
        check_shapes(x, self.weight, self.fmt)
        return mx_linear(x, self.weight, self.fmt, self.tile, w_quant=self._quantised_weight())


def mx_linear_reference(x, w, dy, fmt: str = "mx"):
    """``(y, dx, dw)`` in fp32 (any device): the products of the dequantised reference
    quantisations, each operand quantised along the axis its GEMM contracts, the transposed
    quantisations included."""
    from ddlb_amd.ops import mx

    check_shapes(x, w, fmt, dy)
    if fmt == "mxfp4":
        qref, deq = mx.quantize_mxfp4_reference, mx.dequantize_mxfp4
    else:
        qref, deq = mx.quantize_mx_reference, mx.dequantize_mx

    def rows(t):   # blocks along the rows of t
        return deq(*qref(t))

    def cols(t):   # blocks down the columns of t, stored transposed
        return deq(*mx.quantize_mx_t_reference(t, fmt))

    y = rows(x) @ rows(w).t()          # [M, K] x [N, K]
    dx = rows(dy) @ cols(w).t()        # [M, N] x [K, N]
    dw = cols(dy) @ cols(x).t()        # [N, M] x [K, M]
    return y, dx, dw
