"""A trainable routed (top-k mixture-of-experts) gated FFN on the block-scaled matrix pipe.

    offsets, row_token, slot_row = route(ids, E)          counting sort, no host sync
    xp  = gather(x, row_token)                            [T = S k, H]   the permuted 16-bit copy
    c1  = mx_grouped_linear(xp, w1, offsets)              [T, 2F]        w1 [E, 2F, H] packed
    h   = glu(c1, act)                                    [T, F]
    yp  = mx_grouped_linear(h, w2, offsets)               [T, H]         w2 [E, H, F]
    out = combine(yp, slot_row, gates)                    [S, H]

differentiable in ``x``, ``w1``, ``w2`` and ``gates``. The two linear layers bring their own
backward (grouped dgrad, K-grouped wgrad: ``ddlb_amd/models/mx_grouped_linear.py``); this module
adds three ``torch.autograd.Function`` s around the HIP ops of ``ddlb_amd.ops.moe`` and
``ddlb_amd.ops.glu``:

* the gather, whose backward is ``combine(dxp, slot_row, ones)``: the existing kernel, summing a
  token's ``k`` rows in ``j`` order with one rounding to ``x``'s dtype;
* the GLU, which saves ``c1`` and whose backward is ``glu_bwd``;
* the combine, whose backward is ``combine_bwd``; it saves ``yp`` only when the gates need a
  gradient. ``dgates`` is what a router (a linear layer, softmax and top-k in torch) trains on.

Nothing waits for the device in forward or backward. A graph capture of a step that is to run
autograd's backward is refused with an error (:func:`refuse_captured_backward`): such a capture
ends the process inside torch's ``capture_end``. A forward that needs no gradient is not refused.
``w1`` is kept in the packed layout of ``ops.gemm.pack_glu_grouped``. Unlike the
inference layer ``MxMoE`` (``quantize_mx_gather``, fused ``glu + out_quant`` epilogue) it writes the
permuted copy ``xp`` and the pre-activation ``c1``: both linear layers quantise their 16-bit input
twice, row-wise and grouped-transposed. No activation is recomputed.

:func:`mx_moe_ffn_reference` is the same chain in torch from the stages' own references.
"""

from __future__ import annotations

import torch

from ddlb_amd.models.mx_grouped_linear import (MxGroupedLinear, mx_grouped_linear,
                                               mx_grouped_linear_reference)
from ddlb_amd.models.mx_linear import FMTS, _mod


def check_shapes(x, w1, w2, ids, gates, fmt: str = "mx", act: str = "silu", dout=None):
    """The layer's host-side refusals (any device; no tensor's content is read). Returns
    ``(S, H, F, E, k)``."""
    from ddlb_amd.ops.gemm import ACTS, MAX_GROUPS

    if fmt not in FMTS:
        raise ValueError(f"fmt must be one of {FMTS}, not {fmt!r}")
    if act not in ACTS:
        raise ValueError(f"act must be one of {tuple(ACTS)}, not {act!r}")
    mod = _mod(fmt)
    for name, t, nd in (("x", x, 2), ("w1", w1, 3), ("w2", w2, 3)):
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.bfloat16, torch.float16):
            raise TypeError(f"mx_moe_ffn takes bfloat16 / float16 tensors, {name} is "
                            f"{getattr(t, 'dtype', type(t))}")
        if t.dim() != nd:
            raise ValueError(f"mx_moe_ffn expects x [S, H], w1 [E, 2F, H] and w2 [E, H, F]; "
                             f"{name} is {tuple(t.shape)}")
    if not (x.dtype == w1.dtype == w2.dtype):
        raise TypeError(f"x, w1 and w2 must share one dtype, not {x.dtype}, {w1.dtype}, "
                        f"{w2.dtype}")
    (S, H), (E, N1, H1), (E2, H2, F) = x.shape, w1.shape, w2.shape
    if E != E2 or N1 != 2 * F or H1 != H or H2 != H:
        raise ValueError(f"shape mismatch: x {tuple(x.shape)}, w1 {tuple(w1.shape)} (want "
                         f"[E, 2F, H]), w2 {tuple(w2.shape)} (want [E, H, F])")
    if not 1 <= E <= MAX_GROUPS:
        raise ValueError(f"experts must be in 1 .. {MAX_GROUPS}, not {E}")
    if H % mod or F % mod or 0 in (H, F):
        raise ValueError(f"mx_moe_ffn(fmt={fmt!r}) needs H and F to be positive multiples of "
                         f"{mod} (H, F = {H}, {F})")
    if not isinstance(ids, torch.Tensor) or ids.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"ids must be an int32 or int64 tensor, not "
                        f"{getattr(ids, 'dtype', type(ids))}")
    if ids.dim() != 2 or ids.shape[0] != S or ids.shape[1] < 1:
        raise ValueError(f"ids must be [S, k] with S = {S} and k >= 1, not {tuple(ids.shape)}")
    k = ids.shape[1]
    if not isinstance(gates, torch.Tensor) or gates.dtype != torch.float32:
        raise TypeError(f"gates must be a float32 tensor, not "
                        f"{getattr(gates, 'dtype', type(gates))}")
    if tuple(gates.shape) != (S, k):
        raise ValueError(f"gates must have ids' shape {(S, k)}, not {tuple(gates.shape)}")
    if dout is not None and tuple(dout.shape) != (S, H):
        raise ValueError(f"dout must have shape {(S, H)}, not {tuple(dout.shape)}")
    for name, t in (("w1", w1), ("w2", w2), ("ids", ids), ("gates", gates)):
        if t.device != x.device:
            raise ValueError(f"{name} is on {t.device}, x on {x.device}")
    return S, H, F, E, k


def refuse_captured_backward(tensors) -> None:
    """Raise when the current stream is capturing a graph and one of ``tensors`` would get a
    gradient: the backward's launches come from autograd's worker thread, and closing a capture
    that holds them ends the process with a segmentation fault inside torch's ``capture_end``
    instead of an error. A forward under ``torch.no_grad()`` or on tensors that need no gradient
    passes."""
    if (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
            and torch.is_grad_enabled() and any(t.requires_grad for t in tensors)):
        raise RuntimeError("mx_moe_ffn: a graph capture of a step with autograd's backward is not "
                           "supported (closing it crashes the process); capture the forward under "
                           "torch.no_grad(), or run the training step without a capture")


_ONES = {}


def _ones(shape, device):
    """``[S, k]`` float32 ones, the gates of the gather's backward; the last one made is kept, so
    a training loop fills it once and not once per step."""
    key = (tuple(shape), device)
    if key not in _ONES:
        _ONES.clear()
        _ONES[key] = torch.ones(tuple(shape), dtype=torch.float32, device=device)
    return _ONES[key]


class _GatherFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, row_token, slot_row):
        from ddlb_amd.ops.moe import gather

        ctx.save_for_backward(slot_row)
        return gather(x.detach(), row_token)

    @staticmethod
    def backward(ctx, dxp):
        from ddlb_amd.ops.moe import combine

        (slot_row,) = ctx.saved_tensors
        return combine(dxp.contiguous(), slot_row, _ones(slot_row.shape, dxp.device)), None, None


class _GluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, c, act):
        from ddlb_amd.ops.glu import glu

        c = c.detach()
        ctx.save_for_backward(c)
        ctx.act = act
        return glu(c, act)

    @staticmethod
    def backward(ctx, dh):
        from ddlb_amd.ops.glu import glu_bwd

        (c,) = ctx.saved_tensors
        return glu_bwd(dh.contiguous(), c, ctx.act), None


class _CombineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, slot_row, gates, row_token):
        from ddlb_amd.ops.moe import combine

        y, g = y.detach(), gates.detach().contiguous()
        ctx.need_gates = ctx.needs_input_grad[2]
        ctx.save_for_backward(slot_row, g, row_token, *((y,) if ctx.need_gates else ()))
        ctx.y_dtype = y.dtype
        return combine(y, slot_row, g)

    @staticmethod
    def backward(ctx, dout):
        from ddlb_amd.ops.moe import combine_bwd

        slot_row, g, row_token = ctx.saved_tensors[:3]
        y = ctx.saved_tensors[3] if ctx.need_gates else None
        dy, dgates = combine_bwd(dout.contiguous(), slot_row, g, row_token, y,
                                 dy_dtype=ctx.y_dtype)
        return dy, None, dgates, None


def mx_moe_ffn(x, w1, w2, ids, gates, *, act: str = "silu", fmt: str = "mx", tile: str = "auto",
               w1_quant=None, w2_quant=None):
    """The routed gated FFN of the module docstring: ``x [S, H]``, ``w1 [E, 2F, H]`` (packed),
    ``w2 [E, H, F]`` bf16 or f16, ``ids [S, k]`` int32 / int64, ``gates [S, k]`` float32 ->
    ``out [S, H]`` in ``x``'s dtype, differentiable in ``x``, ``w1``, ``w2`` and ``gates``; each
    gradient is computed only when it is needed. ``H`` and ``F`` are multiples of 128 (``mxfp4``:
    256). An id outside ``[0, E)`` drops its slot: it adds nothing to ``out`` and gets a zero
    ``dgate``. ``w1_quant`` / ``w2_quant``: ``mx_grouped_linear.quantize_weight``'s results when
    the caller keeps them (:class:`MxMoEFFN` does). :func:`check_shapes` holds the refusals."""
    from ddlb_amd.ops.moe import route

    S, H, F, E, k = check_shapes(x, w1, w2, ids, gates, fmt, act)
    refuse_captured_backward((x, w1, w2, gates))
    offsets, row_token, slot_row = route(ids.contiguous(), E)
    xp = _GatherFn.apply(x, row_token, slot_row)
    c1 = mx_grouped_linear(xp, w1, offsets, fmt, tile, w_quant=w1_quant)
    h = _GluFn.apply(c1, act)
    yp = mx_grouped_linear(h, w2, offsets, fmt, tile, w_quant=w2_quant)
    return _CombineFn.apply(yp, slot_row, gates, row_token)


class MxMoEFFN(torch.nn.Module):
    """:func:`mx_moe_ffn` with its weights: two :class:`MxGroupedLinear` s, ``fc1.weight
    [E, 2F, H]`` in the packed gate / up layout and ``fc2.weight [E, H, F]``. Each keeps its
    quantised copies until its parameter's ``_version`` moves; ``n_quant`` counts the weight
    quantisations of both. ``forward(x, ids, gates)``: the router is the caller's."""

    def __init__(self, experts: int, hidden: int, ffn: int, fmt: str = "mx", act: str = "silu",
                 tile: str = "auto", dtype=torch.bfloat16, device=None, seed: int = 0):
        from ddlb_amd.ops.gemm import ACTS

        super().__init__()
        if act not in ACTS:
            raise ValueError(f"act must be one of {tuple(ACTS)}, not {act!r}")
        self.experts, self.hidden, self.ffn = experts, hidden, ffn
        self.fmt, self.act, self.tile = fmt, act, tile
        self.fc1 = MxGroupedLinear(experts, hidden, 2 * ffn, fmt, tile, dtype, device, seed)
        self.fc2 = MxGroupedLinear(experts, ffn, hidden, fmt, tile, dtype, device, seed + 1)

    @property
    def n_quant(self) -> int:
        return self.fc1.n_quant + self.fc2.n_quant

    def forward(self, x, ids, gates):
        return mx_moe_ffn(x, self.fc1.weight, self.fc2.weight, ids, gates, act=self.act,
                          fmt=self.fmt, tile=self.tile, w1_quant=self.fc1._quantised_weight(),
                          w2_quant=self.fc2._quantised_weight())


def mx_moe_ffn_reference(x, w1, w2, ids, gates, dout, act: str = "silu", fmt: str = "mx"):
    """``(out [S, H], dx [S, H], dw1 [E, 2F, H], dw2 [E, H, F], dgates [S, k])`` in fp32, on any
    device (reads the offsets on the host): the chain of the module docstring and its backward
    with cotangent ``dout``, from ``mx_grouped_linear_reference``'s per-stage rules,
    ``glu_reference``, ``glu_bwd_reference``, ``combine_reference`` and
    ``combine_bwd_reference``. Every intermediate is rounded to the 16-bit dtype where the chain
    rounds it; the five results are not."""
    from ddlb_amd.ops.gemm import glu_reference
    from ddlb_amd.ops.glu import glu_bwd_reference
    from ddlb_amd.ops.moe import (combine_bwd_reference, combine_reference, gather_reference,
                                  route_reference)

    S, H, F, E, k = check_shapes(x, w1, w2, ids, gates, fmt, act, dout)
    dt, f32 = x.dtype, torch.float32
    T = S * k
    offsets, row_token, slot_row = route_reference(ids, E)
    xp = gather_reference(x, row_token)
    no_dy1 = torch.zeros((T, 2 * F), dtype=dt, device=x.device)
    no_dy2 = torch.zeros((T, H), dtype=dt, device=x.device)
    c1 = mx_grouped_linear_reference(xp, w1, no_dy1, offsets, fmt)[0].to(dt)
    h = glu_reference(c1.to(f32), act).to(dt)
    yp = mx_grouped_linear_reference(h, w2, no_dy2, offsets, fmt)[0].to(dt)
    out = combine_reference(yp, slot_row, gates, out_dtype=f32)
    dyp, dgates = combine_bwd_reference(dout, slot_row, gates, row_token, yp, dy_dtype=dt)
    _, dh, dw2 = mx_grouped_linear_reference(h, w2, dyp, offsets, fmt)
    dc1 = glu_bwd_reference(dh.to(dt), c1, act).to(dt)
    _, dxp, dw1 = mx_grouped_linear_reference(xp, w1, dc1, offsets, fmt)
    ones = torch.ones((S, k), dtype=f32, device=x.device)
    dx = combine_reference(dxp.to(dt), slot_row, ones, out_dtype=f32)
    return out, dx, dw1, dw2, dgates.to(f32)
