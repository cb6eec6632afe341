"""A trainable routed (per-expert) linear layer on the block-scaled matrix pipe (MX-fp8 or MXFP4).

``X [T, K]`` holds the tokens sorted by expert, ``W [E, N, K]`` one weight per expert and
``offsets [E + 1]`` (int32, on the device, read by the kernels only) the row ranges: expert ``g``
owns rows ``[o'[g], o'[g + 1])`` with the offsets clamped as ``ops.gemm.clamp_offsets`` does.

    Y[rows g]  = X[rows g]  @ W[g].T     forward, M-grouped, contracts K:  Xq [T, K] x Wq [E, N, K]
    dX[rows g] = dY[rows g] @ W[g]       dgrad,   M-grouped, contracts N:  dYq [T, N] x Wtq [E, K, N]
    dW[g]      = dY[rows g].T @ X[rows g]  wgrad, K-grouped, contracts the group's rows:
                                                  dYtq [N, cap] x Xtq [K, cap] -> [E, N, K]

Forward and dgrad are ``ops.gemm.gemm_grouped``; the wgrad is ``ops.gemm.gemm_kgrouped`` on the
padded K layout that ``ops.mx.quantize_mx_t_grouped`` writes for ``X`` and ``dY`` (each group's
blocks start at the group's first row, its tail is zero-padded to a whole K-tile). ``Wtq`` is the
stacked form of the same quantiser: one launch for all experts. Nothing waits for the device
(a graph capture that holds autograd's backward is another matter: see
``ddlb_amd.models.mx_moe_ffn.refuse_captured_backward``). Saved for backward: the grouped-transposed ``X`` and
``Wtq`` (1 or 0.5 byte per element plus scales), not the 16-bit tensors.

``T`` is free; ``K`` and ``N`` are multiples of 128 (MXFP4: 256), being the contraction lengths of
forward and dgrad. Rows outside ``[o'[0], o'[E])`` get zero ``Y`` and zero ``dX``; an expert
without rows gets a zero ``dW``. ``X`` and ``dY`` are each read twice (row-wise and
grouped-transposed quantisation are separate launches; a two-way grouped quantiser is not built).

:func:`mx_grouped_linear_reference` is the same chain in torch on dequantised reference
quantisations.
"""

from __future__ import annotations

import torch

from ddlb_amd.models.mx_linear import FMTS, _mod  # noqa: F401  (FMTS re-exported)


def check_shapes(x, w, offsets, fmt: str, dy=None):
    """The layer's own refusals (any device; the offsets' content is not read). Returns
    ``(T, N, K, E)``."""
    mod = _mod(fmt)
    if x.dim() != 2 or w.dim() != 3:
        raise ValueError(f"mx_grouped_linear expects x [T, K] and w [E, N, K], not "
                         f"{tuple(x.shape)} and {tuple(w.shape)}")
    for name, t in (("x", x), ("w", w)):
        if t.dtype not in (torch.bfloat16, torch.float16):
            raise TypeError(f"mx_grouped_linear takes bfloat16 / float16 tensors, {name} is "
                            f"{t.dtype}")
    (T, K), (E, N, Kw) = x.shape, w.shape
    if K != Kw:
        raise ValueError(f"K mismatch: x {tuple(x.shape)} vs w {tuple(w.shape)}")
    if E < 1:
        raise ValueError("mx_grouped_linear needs at least one expert")
    if N % mod or K % mod or 0 in (N, K):
        raise ValueError(f"mx_grouped_linear(fmt={fmt!r}) needs N and K to be positive multiples "
                         f"of {mod}: the contraction lengths of dgrad and forward (N, K = {N}, "
                         f"{K})")
    if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int32:
        raise TypeError(f"offsets must be an int32 tensor, not "
                        f"{getattr(offsets, 'dtype', type(offsets))}")
    if offsets.dim() != 1 or offsets.shape[0] != E + 1 or not offsets.is_contiguous():
        raise ValueError(f"offsets must be contiguous with shape ({E + 1},) for {E} experts, not "
                         f"{tuple(offsets.shape)}")
    if dy is not None and tuple(dy.shape) != (T, N):
        raise ValueError(f"dy must have shape {(T, N)}, not {tuple(dy.shape)}")
    return T, N, K, E


def quantize_weight(w, fmt: str = "mx"):
    """Both quantisations of ``w [E, N, K]``: ``(wq [E, N, K], ws [E, N, K / 32], wtq [E, K, N],
    wts [E, K, N / 32])`` (fp4: data of half the columns): the row-wise one for the forward pass
    and, in one launch of the stacked grouped transposer, the column-wise one for dgrad."""
    from ddlb_amd.ops.mx import quantize_mx, quantize_mx_t_grouped, quantize_mxfp4

    E, N, K = w.shape
    w2 = w.detach().contiguous().reshape(E * N, K)
    q, s = (quantize_mxfp4 if fmt == "mxfp4" else quantize_mx)(w2)
    slabs = torch.arange(E + 1, dtype=torch.int32, device=w.device) * N
    wtq, wts = quantize_mx_t_grouped(w2, slabs, fmt=fmt, stacked_rows=N)
    wq = q.view(torch.uint8).reshape(E, N, q.shape[1]).view(q.dtype)
    return wq, s.reshape(E, N, s.shape[1]), wtq, wts


class _MxGroupedLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, offsets, fmt, tile, w_quant):
        from ddlb_amd.ops.gemm import gemm_grouped
        from ddlb_amd.ops.mx import quantize_mx, quantize_mx_t_grouped, quantize_mxfp4

        T, N, K, E = check_shapes(x, w, offsets, fmt)
        xd = x.detach().contiguous()
        xq, xs = (quantize_mxfp4 if fmt == "mxfp4" else quantize_mx)(xd)
        if w_quant is None:
            w_quant = quantize_weight(w, fmt)
        wq, ws, wtq, wts = w_quant
        y = torch.zeros((T, N), dtype=x.dtype, device=x.device)
        if T:
            gemm_grouped(xq, wq, offsets, y, a_scale=xs, w_scale=ws, tile=tile)
        saved = [wtq, wts, offsets]
        ctx.need_w = w.requires_grad
        if ctx.need_w:  # the wgrad's operand, quantised down the rows of every group
            saved += list(quantize_mx_t_grouped(xd, offsets, fmt=fmt))
        ctx.save_for_backward(*saved)
        ctx.fmt, ctx.tile, ctx.x_dtype, ctx.w_dtype = fmt, tile, x.dtype, w.dtype
        ctx.dims = (T, N, K, E)
        return y

    @staticmethod
    def backward(ctx, dy):
        from ddlb_amd.ops.gemm import gemm_grouped, gemm_kgrouped
        from ddlb_amd.ops.mx import quantize_mx, quantize_mx_t_grouped, quantize_mxfp4

        wtq, wts, offsets = ctx.saved_tensors[:3]
        T, N, K, E = ctx.dims
        dy = dy.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:  # [T, N] x [E, K, N] -> [T, K]
            dyq, dys = (quantize_mxfp4 if ctx.fmt == "mxfp4" else quantize_mx)(dy)
            dx = torch.zeros((T, K), dtype=ctx.x_dtype, device=dy.device)
            if T:
                gemm_grouped(dyq, wtq, offsets, dx, a_scale=dys, w_scale=wts, tile=ctx.tile)
        if ctx.needs_input_grad[1] and ctx.need_w:  # [N, cap] x [K, cap] -> [E, N, K]
            xtq, xts = ctx.saved_tensors[3:]
            if T:
                dytq, dyts = quantize_mx_t_grouped(dy, offsets, fmt=ctx.fmt)
                dw = gemm_kgrouped(dytq, xtq, offsets, T, a_scale=dyts, w_scale=xts,
                                   out_dtype=ctx.w_dtype, tile=ctx.tile)
            else:
                dw = torch.zeros((E, N, K), dtype=ctx.w_dtype, device=dy.device)
        return dx, dw, None, None, None, None


def mx_grouped_linear(x, w, offsets, fmt: str = "mx", tile: str = "auto", *, w_quant=None):
    """``y[rows g] = x[rows g] @ w[g].T`` on the grouped block-scaled GEMM, differentiable in ``x``
    and ``w``: backward runs the grouped dgrad and the K-grouped wgrad on the block-scaled GEMM as
    well (module docstring), each only when its gradient is needed. ``w_quant``: the result of
    :func:`quantize_weight` when the caller keeps it (:class:`MxGroupedLinear` does)."""
    return _MxGroupedLinearFn.apply(x, w, offsets, fmt, tile, w_quant)


class MxGroupedLinear(torch.nn.Module):
    """``y[rows g] = x[rows g] @ weight[g].T`` (no bias) through :func:`mx_grouped_linear`. The
    weight's two quantised copies are kept between calls and made again when the parameter's
    ``_version`` has moved (an optimiser step, any in-place write); ``n_quant`` counts the
    quantisations."""

    def __init__(self, experts: int, in_features: int, out_features: int, fmt: str = "mx",
                 tile: str = "auto", dtype=torch.bfloat16, device=None, seed: int = 0):
        super().__init__()
        mod = _mod(fmt)
        if experts < 1:
            raise ValueError(f"MxGroupedLinear needs at least one expert (got {experts})")
        if in_features % mod or out_features % mod or in_features <= 0 or out_features <= 0:
            raise ValueError(f"MxGroupedLinear(fmt={fmt!r}) needs in_features and out_features "
                             f"to be positive multiples of {mod} (got {in_features}, "
                             f"{out_features})")
        if dtype not in (torch.bfloat16, torch.float16):
            raise TypeError(f"MxGroupedLinear takes bfloat16 / float16 weights, not {dtype}")
        self.experts, self.in_features, self.out_features = experts, in_features, out_features
        self.fmt, self.tile = fmt, tile
        g = torch.Generator().manual_seed(seed)
        w = (torch.rand(experts, out_features, in_features, generator=g) * 2 - 1) \
            * in_features ** -0.5
        self.weight = torch.nn.Parameter(w.to(device=device, dtype=dtype))
        self.n_quant = 0
        self._w_quant = None
        self._w_key = None

    def _quantised_weight(self):
        w = self.weight
        key = (w._version, w.data_ptr(), w.dtype)
        if self._w_key != key:
            self._w_quant = quantize_weight(w, self.fmt)
            self._w_key = key
            self.n_quant += 1
        return self._w_quant

    def forward(self, x, offsets):
        check_shapes(x, self.weight, offsets, self.fmt)
        return mx_grouped_linear(x, self.weight, offsets, self.fmt, self.tile,
                                 w_quant=self._quantised_weight())


def mx_grouped_linear_reference(x, w, dy, offsets, fmt: str = "mx"):
    """``(y [T, N], dx [T, K], dw [E, N, K])`` in fp32 (any device; reads ``offsets`` on the
    host): per expert, the products of the dequantised reference quantisations, each operand
    quantised along the axis its GEMM contracts; for the wgrad that is the group's rows, blocks
    starting at the group's first row and the tail zero-padded. Rows outside the groups and the
    ``dw`` of an expert without rows are zero."""
    from ddlb_amd.ops import mx
    from ddlb_amd.ops.gemm import clamp_offsets

    T, N, K, E = check_shapes(x, w, offsets, fmt, dy)
    mod = _mod(fmt)
    if fmt == "mxfp4":
        qref, deq = mx.quantize_mxfp4_reference, mx.dequantize_mxfp4
    else:
        qref, deq = mx.quantize_mx_reference, mx.dequantize_mx

    def rows(t):   # blocks along the rows of t
        return deq(*qref(t))

    def cols(t):   # blocks down the columns of t (rows a multiple of mod), stored transposed
        return deq(*mx.quantize_mx_t_reference(t, fmt))

    def pad(t):    # zero rows up to a multiple of mod
        n = -(-t.shape[0] // mod) * mod
        out = torch.zeros((n, t.shape[1]), dtype=t.dtype, device=t.device)
        out[:t.shape[0]] = t
        return out

    o = clamp_offsets(offsets, T)
    y = torch.zeros((T, N), dtype=torch.float32, device=x.device)
    dx = torch.zeros((T, K), dtype=torch.float32, device=x.device)
    dw = torch.zeros((E, N, K), dtype=torch.float32, device=x.device)
    xr, dyr = (rows(x), rows(dy)) if T else (x.float(), dy.float())
    for g in range(E):
        lo, hi = o[g], o[g + 1]
        if hi == lo:
            continue
        y[lo:hi] = xr[lo:hi] @ rows(w[g]).t()              # [n, K] x [N, K]
        dx[lo:hi] = dyr[lo:hi] @ cols(w[g]).t()            # [n, N] x [K, N]
        dw[g] = cols(pad(dy[lo:hi])) @ cols(pad(x[lo:hi])).t()  # [N, n'] x [K, n']
    return y, dx, dw
