"""The gated activation as an op of its own, forward and backward (``csrc/gemm/glu_act.hip``).

The layout is the packed one of :func:`ddlb_amd.ops.gemm.pack_glu` (``GLU_GROUP = 32``): in
``c [T, 2F]`` columns ``64g .. 64g + 31`` are gate columns and ``64g + 32 .. 64g + 63`` the
matching up columns. :func:`glu` is what the gated GEMM epilogue does to its accumulators, with the
same ``act1``; it exists so that a training step can keep ``c`` and run :func:`glu_bwd` on it.

:func:`ddlb_amd.ops.gemm.glu_reference` is the forward's specification and
:func:`glu_bwd_reference` the backward's; both run on any device.
"""

from __future__ import annotations

from ddlb_amd.ops.gemm import ACTS, GLU_GROUP

C_DTYPES = ("bfloat16", "float16", "float32")


def _check_rows(name, t, rows, cols, what):
    """``t [rows, cols]`` row-major with unit inner stride and 16-byte-aligned rows."""
    if tuple(t.shape) != (rows, cols):
        raise ValueError(f"{name} must have shape {(rows, cols)}, not {tuple(t.shape)}")
    if rows == 0 or cols == 0:
        return
    if t.stride(1) != 1 or (rows > 1 and t.stride(0) < cols):
        raise ValueError(f"{what} needs row-major {name} with unit inner stride")
    if t.data_ptr() % 16 or (rows > 1 and (t.stride(0) * t.element_size()) % 16):
        raise ValueError(f"{what} needs 16-byte-aligned rows of {name}")


def _check_c(c, act, what):
    import torch

    dts = (torch.bfloat16, torch.float16, torch.float32)
    if act not in ACTS:
        raise ValueError(f"unknown activation {act!r}")
    if not isinstance(c, torch.Tensor) or c.dtype not in dts:
        raise TypeError(f"c must be one of {C_DTYPES}, not {getattr(c, 'dtype', type(c))}")
    if c.dim() != 2:
        raise ValueError(f"c must be [T, 2F] (2-D), not {tuple(c.shape)}")
    T, N = c.shape
    if N % (2 * GLU_GROUP):
        raise ValueError(f"{what} needs 2F % {2 * GLU_GROUP} == 0: whole groups of {GLU_GROUP} "
                         f"gate and {GLU_GROUP} up columns (c is {T} x {N})")
    if T >= 2 ** 31 or N >= 2 ** 30:
        raise ValueError("dimensions must fit in 32 bits")
    _check_rows("c", c, T, N, what)
    return T, N // 2


def _check_glu(c, act="none", out=None, out_dtype=None):
    """Every refusal of :func:`glu`, on the host and before the extension is loaded (CPU tensors
    reach the device refusal, which comes last). Returns ``(T, F, output dtype)``."""
    import torch

    T, F = _check_c(c, act, "glu")
    if out is not None and not isinstance(out, torch.Tensor):
        raise TypeError(f"out must be a tensor, not {type(out)}")
    if out is not None and out_dtype is not None and out_dtype != out.dtype:
        raise TypeError(f"out is {out.dtype}, out_dtype={out_dtype}")
    odt = out.dtype if out is not None else (out_dtype or c.dtype)
    if odt not in (c.dtype, torch.float32):
        raise TypeError(f"glu of a {c.dtype} c writes {c.dtype} or torch.float32, not {odt}")
    if out is not None:
        if out.device != c.device:
            raise ValueError(f"out is on {out.device}, c on {c.device}")
        _check_rows("out", out, T, F, "glu")
    if c.device.type != "cuda":  # last, so that CPU tensors reach every refusal above
        raise ValueError("glu needs ROCm device tensors (ops.gemm.glu_reference runs anywhere)")
    return T, F, odt


def _ld(t, cols):
    return max(t.stride(0), cols) if t.shape[0] > 1 else cols


def glu(c, act: str = "none", *, out=None, out_dtype=None, stream=None):
    """``h [T, F] = act(gate) * up`` of the packed ``c [T, 2F]`` (bf16 / f16 / f32, row-major,
    ``ld >= 2F``, rows 16-byte aligned, ``2F % 64 == 0``) in ``c``'s dtype (default) or float32.
    The arithmetic is the fused epilogue's: ``h = rne(act1(float(g)) * float(u))``, one fp32
    multiply and one rounding, ``act1`` the GEMM's own. ``T == 0`` launches nothing.
    :func:`_check_glu` holds every refusal."""
    import torch

    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import dtype_code

    T, F, odt = _check_glu(c, act, out, out_dtype)
    if out is None:
        out = torch.empty((T, F), dtype=odt, device=c.device)
    C = load()
    if T == 0 or F == 0:
        return out
    strm = stream if stream is not None else torch.cuda.current_stream(c.device).cuda_stream
    with torch.cuda.device(c.device):
        C.glu_fwd(c=c.data_ptr(), out=out.data_ptr(), ldc=_ld(c, 2 * F), ldo=_ld(out, F), T=T,
                  F=F, act=ACTS[act], din=dtype_code(c.dtype), dout=dtype_code(odt), stream=strm)
    if stream is not None:  # the output stays allocated until that stream reaches it
        out.record_stream(torch.cuda.ExternalStream(strm))
    return out


def _check_glu_bwd(dh, c, act="none", out=None):
    """Every refusal of :func:`glu_bwd` (as :func:`_check_glu`). Returns ``(T, F)``."""
    import torch

    T, F = _check_c(c, act, "glu_bwd")
    if not isinstance(dh, torch.Tensor) or dh.dtype != c.dtype:
        raise TypeError(f"dh must be a tensor of c's dtype {c.dtype}, not "
                        f"{getattr(dh, 'dtype', type(dh))}")
    if dh.device != c.device:
        raise ValueError(f"dh is on {dh.device}, c on {c.device}")
    _check_rows("dh", dh, T, F, "glu_bwd")
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != c.dtype:
            raise TypeError(f"out must be a tensor of c's dtype {c.dtype}, not "
                            f"{getattr(out, 'dtype', type(out))}")
        if out.device != c.device:
            raise ValueError(f"out is on {out.device}, c on {c.device}")
        _check_rows("out", out, T, 2 * F, "glu_bwd")
    if c.device.type != "cuda":  # last, so that CPU tensors reach every refusal above
        raise ValueError("glu_bwd needs ROCm device tensors (glu_bwd_reference runs anywhere)")
    return T, F


def glu_bwd(dh, c, act: str = "none", *, out=None, stream=None):
    """The backward of :func:`glu`: ``dh [T, F]`` and the saved ``c [T, 2F]`` (one dtype) ->
    ``dc [T, 2F]`` in that dtype and the packed layout. In fp32, with one rounding each::

        dc[., 64g + j]      = (dh * u) * act'(g)
        dc[., 64g + 32 + j] = dh * act1(g)

    ``act'`` is 1 (``none``), ``g <= 0 ? 0 : 1`` (``relu``), ``s (1 + g (1 - s))`` with
    ``s = sigmoid(g)`` (``silu``) and ``s + g s (1 - s) 2u'(g)`` with ``s = sigmoid(2u)`` (``gelu``,
    the tanh form), evaluated so that every finite ``g`` gives a finite value (the limit, 1 or 0,
    where ``g^3`` overflows). A NaN ``g`` makes both of its outputs NaN; a NaN or Inf anywhere
    else touches only its own element pair. :func:`_check_glu_bwd` holds every refusal."""
    import torch

    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import dtype_code

    T, F = _check_glu_bwd(dh, c, act, out)
    if out is None:
        out = torch.empty((T, 2 * F), dtype=c.dtype, device=c.device)
    C = load()
    if T == 0 or F == 0:
        return out
    strm = stream if stream is not None else torch.cuda.current_stream(c.device).cuda_stream
    with torch.cuda.device(c.device):
        C.glu_bwd(dh=dh.data_ptr(), c=c.data_ptr(), out=out.data_ptr(), ldh=_ld(dh, F),
                  ldc=_ld(c, 2 * F), ldo=_ld(out, 2 * F), T=T, F=F, act=ACTS[act],
                  din=dtype_code(c.dtype), stream=strm)
    if stream is not None:
        out.record_stream(torch.cuda.ExternalStream(strm))
    return out


def glu_bwd_reference(dh, c, act: str = "none"):
    """The specification of :func:`glu_bwd` on any device, independent of the hand-written
    derivatives: fp64 autograd through ``apply_act(g) * u`` on the upcast inputs with cotangent
    ``dh``, re-packed; float64 ``[T, 2F]``. Both outputs of a NaN ``g`` are NaN."""
    import torch

    from ddlb_amd.parallel.sim import apply_act

    if act not in ACTS:
        raise ValueError(f"unknown activation {act!r}")
    if c.dim() != 2 or c.shape[1] % (2 * GLU_GROUP) or tuple(dh.shape) != (c.shape[0],
                                                                          c.shape[1] // 2):
        raise ValueError(f"glu_bwd_reference takes dh [T, F] and c [T, 2F] with 2F % "
                         f"{2 * GLU_GROUP} == 0, not {tuple(dh.shape)} and {tuple(c.shape)}")
    T, N = c.shape
    v = c.detach().to(torch.float64).reshape(T, N // (2 * GLU_GROUP), 2, GLU_GROUP)
    g = v[:, :, 0].clone().requires_grad_()
    u = v[:, :, 1].clone().requires_grad_()
    with torch.enable_grad():
        h = apply_act(g, ACTS[act]) * u
        dg, du = torch.autograd.grad(h, (g, u), dh.detach().to(torch.float64).reshape(h.shape))
    nan = torch.isnan(g.detach())
    dg = torch.where(nan, g.detach(), dg)
    du = torch.where(nan, g.detach(), du)
    return torch.stack((dg, du), dim=2).reshape(T, N)
