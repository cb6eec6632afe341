"""MoE dispatch: the routing sort and the weighted un-permute of a routed (top-k) layer.

``route`` sorts the ``S * k`` (token, choice) slots ``p = t * k + j`` of ``ids [S, k]`` by expert,
stably, on the device (``csrc/moe/moe_route.hip``: a counting sort in three launches, no host sync,
no workgroup that waits for another). ``combine`` sums a token's ``k`` expert outputs with its
gate weights through the inverted index ``slot_row`` in a fixed order
(``csrc/moe/moe_combine.hip``), so the result is bitwise reproducible. Between the two,
:func:`ddlb_amd.ops.mx.quantize_mx_gather` quantises ``x[row_token]`` without writing the
permuted copy and ``ops.gemm.gemm_grouped`` runs the experts.

For training (``ddlb_amd.models.mx_moe_ffn``): ``gather`` writes the permuted 16-bit copy
``x[row_token]`` (``csrc/moe/moe_gather.hip``; its backward is ``combine`` with gates of 1) and
``combine_bwd`` is the backward of ``combine`` (``csrc/moe/moe_combine_bwd.hip``): the rows'
gradient and, reduced in a fixed order without atomics, the gate weights'.

:func:`route_reference`, :func:`combine_reference`, :func:`gather_reference` and
:func:`combine_bwd_reference` are pure torch, run on any device and are the specification; on the
GPU the kernels agree with them bit for bit (``dgate``: to fp32 summation accuracy).
"""

from __future__ import annotations

from ddlb_amd.ops.gemm import MAX_GROUPS

ROUTE_CHUNK = 1024  # csrc/moe/moe_route_map.h kRouteChunk: slots per workgroup of the sort
Y_DTYPES = ("bfloat16", "float16", "float32")


def route_workspace_words(n: int, experts: int) -> int:
    """int32 words of the sort's workspace (moe_route_map.h ``route_workspace_words``): one count
    per (chunk, expert) and the experts' totals."""
    return (-(-n // ROUTE_CHUNK) + 1) * experts


def _check_route(ids, experts, out=None):
    """Every refusal of :func:`route`, on the host and before the extension is loaded (CPU tensors
    reach the device refusal; the ids' content is never read). Returns ``(S, k)``."""
    import torch

    if not isinstance(ids, torch.Tensor) or ids.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"ids must be an int32 or int64 tensor, not "
                        f"{getattr(ids, 'dtype', type(ids))}")
    if ids.dim() != 2:
        raise ValueError(f"ids must be [S, k] (2-D), not {tuple(ids.shape)}")
    if isinstance(experts, bool) or not isinstance(experts, int):
        raise TypeError(f"experts must be an int, not {type(experts)}")
    if not 1 <= experts <= MAX_GROUPS:
        raise ValueError(f"experts must be in 1 .. {MAX_GROUPS}, not {experts}")
    S, k = ids.shape
    if k < 1:
        raise ValueError(f"ids needs at least one choice per token (k >= 1), not {tuple(ids.shape)}")
    if S * k >= 2 ** 31:
        raise ValueError(f"S * k must be below 2^31 (ids is {S} x {k})")
    if not ids.is_contiguous():
        raise ValueError(f"ids must be contiguous (strides {tuple(ids.stride())})")
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 3:
            raise TypeError("out must be a triple (offsets, row_token, slot_row)")
        shapes = ((experts + 1,), (S * k,), (S, k))
        for name, t, shape in zip(("out[0] (offsets)", "out[1] (row_token)",
                                   "out[2] (slot_row)"), out, shapes):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
                raise TypeError(f"{name} must be an int32 tensor, not "
                                f"{getattr(t, 'dtype', type(t))}")
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} must have shape {shape}, not {tuple(t.shape)}")
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous (strides {tuple(t.stride())})")
            if t.device != ids.device:
                raise ValueError(f"{name} is on {t.device}, ids on {ids.device}")
    if ids.device.type != "cuda":  # last, so that CPU tensors reach every refusal above
        raise ValueError("route needs a ROCm device tensor (route_reference runs anywhere)")
    return S, k


def route(ids, experts: int, *, out=None, stream=None):
    """The HIP routing sort: ``ids [S, k]`` int32 / int64, contiguous, on a ROCm device ->
    ``(offsets, row_token, slot_row)``, all int32 and every element written:

    * ``offsets [experts + 1]``: ``offsets[0] = 0``, ``offsets[e + 1] - offsets[e]`` the number of
      slots whose id is ``e`` (what ``gemm_grouped`` takes);
    * ``row_token [S * k]``: the token of the slot sorted to row ``r < offsets[experts]``, ``-1``
      for the rows behind (what :func:`ddlb_amd.ops.mx.quantize_mx_gather` takes as ``src``);
    * ``slot_row [S, k]``: the row of slot ``(t, j)``, ``-1`` when ``ids[t, j]`` is outside
      ``[0, experts)``: such slots are dropped, not counted (what :func:`combine` takes).

    Rows are ordered by expert and, inside an expert, by ascending slot ``t * k + j``: for ``k = 1``
    and valid ids ``row_token`` is ``torch.argsort(ids, stable=True)``. Nothing waits on the host
    (the workspace comes from torch's caching allocator), so the call can be captured in a graph.
    ``out`` may hold the three preallocated outputs. :func:`_check_route` holds every refusal."""
    import torch

    from ddlb_amd.ops import load

    S, k = _check_route(ids, experts, out)
    n = S * k
    dev = ids.device
    if out is None:
        offsets = torch.empty(experts + 1, dtype=torch.int32, device=dev)
        row_token = torch.empty(n, dtype=torch.int32, device=dev)
        slot_row = torch.empty((S, k), dtype=torch.int32, device=dev)
    else:
        offsets, row_token, slot_row = out
    C = load()
    if n == 0:
        offsets.zero_()
        return offsets, row_token, slot_row
    strm = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    ws = torch.empty(route_workspace_words(n, experts), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        C.moe_route(ids=ids.data_ptr(), offsets=offsets.data_ptr(),
                    row_token=row_token.data_ptr(), slot_row=slot_row.data_ptr(),
                    ws=ws.data_ptr(), n=n, k=k, E=experts, ids64=ids.dtype == torch.int64,
                    stream=strm)
    if stream is not None:  # the buffers stay allocated until that stream reaches them
        for t in (ws, offsets, row_token, slot_row):
            t.record_stream(torch.cuda.ExternalStream(strm))
    return offsets, row_token, slot_row


def route_reference(ids, experts: int):
    """The specification of :func:`route` in torch ops, on any device."""
    import torch

    if ids.dim() != 2:
        raise ValueError(f"ids must be [S, k] (2-D), not {tuple(ids.shape)}")
    S, k = ids.shape
    n = S * k
    dev = ids.device
    flat = ids.reshape(n).to(torch.int64)
    valid = (flat >= 0) & (flat < experts)
    key = torch.where(valid, flat, torch.full_like(flat, experts))  # dropped slots sort last
    order = torch.argsort(key, stable=True)
    counts = torch.zeros(experts + 1, dtype=torch.int64, device=dev)
    counts.scatter_add_(0, key, torch.ones_like(key))
    offsets = torch.zeros(experts + 1, dtype=torch.int32, device=dev)
    offsets[1:] = torch.cumsum(counts[:experts], 0).to(torch.int32)
    rows = torch.arange(n, device=dev)
    kept = valid[order]                                  # the first offsets[E] rows
    row_token = torch.where(kept, torch.div(order, k, rounding_mode="floor"),
                            torch.full_like(order, -1)).to(torch.int32)
    slot_row = torch.empty(n, dtype=torch.int64, device=dev)
    slot_row[order] = torch.where(kept, rows, torch.full_like(rows, -1))
    return offsets, row_token, slot_row.to(torch.int32).reshape(S, k)


def _check_combine(y, slot_row, gate, out=None, out_dtype=None):
    """Every refusal of :func:`combine`, on the host and before the extension is loaded (CPU
    tensors reach the device refusal). Returns ``(S, k, T, H, output dtype)``."""
    import torch

    dts = (torch.bfloat16, torch.float16, torch.float32)
    if not isinstance(y, torch.Tensor) or y.dtype not in dts:
        raise TypeError(f"y must be one of {Y_DTYPES}, not {getattr(y, 'dtype', type(y))}")
    if y.dim() != 2:
        raise ValueError(f"y must be [T, H] (2-D), not {tuple(y.shape)}")
    if not isinstance(slot_row, torch.Tensor) or slot_row.dtype != torch.int32:
        raise TypeError(f"slot_row must be an int32 tensor, not "
                        f"{getattr(slot_row, 'dtype', type(slot_row))}")
    if not isinstance(gate, torch.Tensor) or gate.dtype != torch.float32:
        raise TypeError(f"gate must be a float32 tensor, not "
                        f"{getattr(gate, 'dtype', type(gate))}")
    if slot_row.dim() != 2 or slot_row.shape[1] < 1:
        raise ValueError(f"slot_row must be [S, k] with k >= 1, not {tuple(slot_row.shape)}")
    if tuple(gate.shape) != tuple(slot_row.shape):
        raise ValueError(f"gate must have slot_row's shape {tuple(slot_row.shape)}, not "
                         f"{tuple(gate.shape)}")
    if not slot_row.is_contiguous() or not gate.is_contiguous():
        raise ValueError("slot_row and gate must be contiguous")
    if slot_row.device != y.device or gate.device != y.device:
        raise ValueError(f"slot_row is on {slot_row.device}, gate on {gate.device}, y on "
                         f"{y.device}")
    S, k = slot_row.shape
    T, H = y.shape
    if T >= 2 ** 31 or H >= 2 ** 31 or S * k >= 2 ** 31:
        raise ValueError("dimensions must fit in 32 bits")
    if (H * y.element_size()) % 16:
        raise ValueError(f"combine needs rows of whole 16-byte vectors (y is {T} x {H} {y.dtype})")
    empty = T == 0 or H == 0
    if not empty and (y.stride(1) != 1 or (T > 1 and y.stride(0) < H)):
        raise ValueError("combine needs row-major y with unit inner stride")
    if not empty and (y.data_ptr() % 16 or (y.stride(0) * y.element_size()) % 16):
        raise ValueError("combine needs 16-byte-aligned rows of y")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype not in dts):
        raise TypeError(f"out must be one of {Y_DTYPES}, not {getattr(out, 'dtype', type(out))}")
    if out is not None and out_dtype is not None and out_dtype != out.dtype:
        raise TypeError(f"out is {out.dtype}, out_dtype={out_dtype}")
    odt = out.dtype if out is not None else (out_dtype or y.dtype)
    if odt not in (y.dtype, torch.float32):
        raise TypeError(f"combine of {y.dtype} rows writes {y.dtype} or torch.float32, not {odt}")
    if out is not None:
        if out.device != y.device:
            raise ValueError(f"out is on {out.device}, y on {y.device}")
        if tuple(out.shape) != (S, H):
            raise ValueError(f"out must have shape {(S, H)}, not {tuple(out.shape)}")
        if S and H and (out.stride(1) != 1 or (S > 1 and out.stride(0) < H)):
            raise ValueError("combine needs row-major out with unit inner stride")
        if S and H and (out.data_ptr() % 16 or (out.stride(0) * out.element_size()) % 16):
            raise ValueError("combine needs 16-byte-aligned rows of out")
    if y.device.type != "cuda":  # last, so that CPU tensors reach every refusal above
        raise ValueError("combine needs ROCm device tensors (combine_reference runs anywhere)")
    return S, k, T, H, odt


def combine(y, slot_row, gate, *, out=None, out_dtype=None, stream=None):
    """The HIP weighted un-permute: ``out[t, :] = sum_j gate[t, j] * y[slot_row[t, j], :]`` with
    ``y [T, H]`` bf16 / f16 / f32, ``slot_row [S, k]`` int32 (:func:`route`), ``gate [S, k]``
    float32 and ``out [S, H]`` in ``y``'s dtype (default) or float32.

    The arithmetic is fixed: per element ``acc = +0.0`` in fp32; for ``j = 0 .. k - 1`` in order,
    if ``0 <= slot_row[t, j] < T``, ``acc = acc + gate * float(y)`` with the product and the sum
    each rounded (no fma); one round-to-nearest-even to the output dtype. A dropped or
    out-of-range slot contributes nothing and its row is not read. :func:`combine_reference` is
    the same steps in torch ops and agrees bit for bit on the GPU. ``H * element size`` is a
    multiple of 16 and rows are 16-byte aligned; :func:`_check_combine` holds every refusal."""
    import torch

    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import dtype_code

    S, k, T, H, odt = _check_combine(y, slot_row, gate, out, out_dtype)
    if out is None:
        out = torch.empty((S, H), dtype=odt, device=y.device)
    C = load()
    if S == 0 or H == 0:
        return out
    strm = stream if stream is not None else torch.cuda.current_stream(y.device).cuda_stream
    with torch.cuda.device(y.device):
        C.moe_combine(y=y.data_ptr(), slot_row=slot_row.data_ptr(), gate=gate.data_ptr(),
                      out=out.data_ptr(), ldy=max(y.stride(0), H), ldo=max(out.stride(0), H),
                      S=S, k=k, T=T, H=H, din=dtype_code(y.dtype), dout=dtype_code(odt),
                      stream=strm)
    if stream is not None:  # the output stays allocated until that stream reaches it
        out.record_stream(torch.cuda.ExternalStream(strm))
    return out


def combine_reference(y, slot_row, gate, out_dtype=None):
    """The specification of :func:`combine` on any device: the same fp32 steps as separate torch
    multiplies and adds (so nothing is contracted), one rounding to the output dtype."""
    import torch

    S, k = slot_row.shape
    T, H = y.shape
    acc = torch.zeros((S, H), dtype=torch.float32, device=y.device)
    for j in range(k):
        r = slot_row[:, j].to(torch.int64)
        valid = (r >= 0) & (r < T)
        if T == 0:
            continue
        rows = y.index_select(0, torch.where(valid, r, torch.zeros_like(r))).to(torch.float32)
        prod = gate[:, j:j + 1] * rows
        acc = torch.where(valid.unsqueeze(1), acc + prod, acc)
    return acc.to(out_dtype or y.dtype)


def _check_rows(what, name, t, rows, cols):
    """``t [rows, cols]`` row-major with unit inner stride and 16-byte-aligned rows of whole
    16-byte vectors (:func:`combine`'s layout rules)."""
    if tuple(t.shape) != (rows, cols):
        raise ValueError(f"{name} must have shape {(rows, cols)}, not {tuple(t.shape)}")
    if (cols * t.element_size()) % 16:
        raise ValueError(f"{what} needs rows of whole 16-byte vectors ({name} is {rows} x {cols} "
                         f"{t.dtype})")
    if rows == 0 or cols == 0:
        return
    if t.stride(1) != 1 or (rows > 1 and t.stride(0) < cols):
        raise ValueError(f"{what} needs row-major {name} with unit inner stride")
    if t.data_ptr() % 16 or (rows > 1 and (t.stride(0) * t.element_size()) % 16):
        raise ValueError(f"{what} needs 16-byte-aligned rows of {name}")


def _ld(t):
    return max(t.stride(0), t.shape[1]) if t.shape[0] > 1 else t.shape[1]


def _check_index(name, t, like, shape=None):
    import torch

    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
        raise TypeError(f"{name} must be an int32 tensor, not {getattr(t, 'dtype', type(t))}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, not {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous (strides {tuple(t.stride())})")
    if t.device != like.device:
        raise ValueError(f"{name} is on {t.device}, the rows on {like.device}")


def _check_gather(x, row_token, out=None):
    """Every refusal of :func:`gather`, on the host and before the extension is loaded (CPU
    tensors reach the device refusal). Returns ``(S, T, H)``."""
    import torch

    dts = (torch.bfloat16, torch.float16, torch.float32)
    if not isinstance(x, torch.Tensor) or x.dtype not in dts:
        raise TypeError(f"x must be one of {Y_DTYPES}, not {getattr(x, 'dtype', type(x))}")
    if x.dim() != 2:
        raise ValueError(f"x must be [S, H] (2-D), not {tuple(x.shape)}")
    _check_index("row_token", row_token, x)
    if row_token.dim() != 1:
        raise ValueError(f"row_token must be [T] (1-D), not {tuple(row_token.shape)}")
    S, H = x.shape
    T = row_token.shape[0]
    if S >= 2 ** 31 or H >= 2 ** 31 or T >= 2 ** 31:
        raise ValueError("dimensions must fit in 32 bits")
    _check_rows("gather", "x", x, S, H)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != x.dtype:
            raise TypeError(f"out must be a tensor of x's dtype {x.dtype}, not "
                            f"{getattr(out, 'dtype', type(out))}")
        if out.device != x.device:
            raise ValueError(f"out is on {out.device}, x on {x.device}")
        _check_rows("gather", "out", out, T, H)
    if x.device.type != "cuda":  # last, so that CPU tensors reach every refusal above
        raise ValueError("gather needs ROCm device tensors (gather_reference runs anywhere)")
    return S, T, H


def gather(x, row_token, *, out=None, stream=None):
    """The HIP dense gather of the routed rows (``csrc/moe/moe_gather.hip``):
    ``xp[r, :] = x[row_token[r], :]`` with ``x [S, H]`` bf16 / f16 / f32 and ``row_token [T]``
    int32 (:func:`route`); a row whose index is outside ``[0, S)`` is ``+0.0`` and nothing is read
    for it. Byte for byte ``index_select`` with zero rows (:func:`gather_reference`). The layout
    and alignment rules are :func:`combine`'s; :func:`_check_gather` holds every refusal.

    The training path's permuted copy: ``mx_grouped_linear`` quantises the 16-bit rows twice. The
    inference path (:func:`ddlb_amd.ops.mx.quantize_mx_gather`) writes no such copy. Its backward
    is :func:`combine` with gates of 1."""
    import torch

    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import dtype_code

    S, T, H = _check_gather(x, row_token, out)
    if out is None:
        out = torch.empty((T, H), dtype=x.dtype, device=x.device)
    C = load()
    if T == 0 or H == 0:
        return out
    strm = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
    with torch.cuda.device(x.device):
        C.moe_gather(x=x.data_ptr(), row_token=row_token.data_ptr(), out=out.data_ptr(),
                     ldx=_ld(x), ldo=_ld(out), S=S, T=T, H=H, dt=dtype_code(x.dtype),
                     stream=strm)
    if stream is not None:  # the output stays allocated until that stream reaches it
        out.record_stream(torch.cuda.ExternalStream(strm))
    return out


def gather_reference(x, row_token):
    """The specification of :func:`gather` in torch ops, on any device."""
    import torch

    S, H = x.shape
    r = row_token.to(torch.int64)
    valid = (r >= 0) & (r < S)
    out = torch.zeros((r.shape[0], H), dtype=x.dtype, device=x.device)
    if S:
        rows = x.index_select(0, torch.where(valid, r, torch.zeros_like(r)))
        out = torch.where(valid.unsqueeze(1), rows, out)
    return out


def _check_combine_bwd(dout, slot_row, gate, row_token, y=None, dy_dtype=None, out=None):
    """Every refusal of :func:`combine_bwd`, on the host and before the extension is loaded (CPU
    tensors reach the device refusal). Returns ``(S, k, T, H, dy's dtype)``."""
    import torch

    dts = (torch.bfloat16, torch.float16, torch.float32)
    if not isinstance(dout, torch.Tensor) or dout.dtype not in dts:
        raise TypeError(f"dout must be one of {Y_DTYPES}, not "
                        f"{getattr(dout, 'dtype', type(dout))}")
    if dout.dim() != 2:
        raise ValueError(f"dout must be [S, H] (2-D), not {tuple(dout.shape)}")
    S, H = dout.shape
    _check_index("slot_row", slot_row, dout)
    if slot_row.dim() != 2 or slot_row.shape[1] < 1 or slot_row.shape[0] != S:
        raise ValueError(f"slot_row must be [S, k] with S = {S} and k >= 1, not "
                         f"{tuple(slot_row.shape)}")
    k = slot_row.shape[1]
    if not isinstance(gate, torch.Tensor) or gate.dtype != torch.float32:
        raise TypeError(f"gate must be a float32 tensor, not "
                        f"{getattr(gate, 'dtype', type(gate))}")
    if tuple(gate.shape) != (S, k):
        raise ValueError(f"gate must have slot_row's shape {(S, k)}, not {tuple(gate.shape)}")
    if not gate.is_contiguous():
        raise ValueError("slot_row and gate must be contiguous")
    if gate.device != dout.device:
        raise ValueError(f"gate is on {gate.device}, dout on {dout.device}")
    _check_index("row_token", row_token, dout)
    if row_token.dim() != 1:
        raise ValueError(f"row_token must be [T] (1-D), not {tuple(row_token.shape)}")
    T = row_token.shape[0]
    if T >= 2 ** 31 or H >= 2 ** 31 or S * k >= 2 ** 31:
        raise ValueError("dimensions must fit in 32 bits")
    if y is not None and (not isinstance(y, torch.Tensor) or y.dtype not in dts):
        raise TypeError(f"y must be one of {Y_DTYPES}, not {getattr(y, 'dtype', type(y))}")
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise TypeError("out must be a pair (dy, dgate); dgate is None without y")
        if not isinstance(out[0], torch.Tensor) or out[0].dtype not in dts:
            raise TypeError(f"out[0] (dy) must be one of {Y_DTYPES}, not "
                            f"{getattr(out[0], 'dtype', type(out[0]))}")
    given = [t.dtype for t in (y, out[0] if out is not None else None) if t is not None]
    if dy_dtype is not None:
        given.append(dy_dtype)
    ddt = given[0] if given else dout.dtype
    if any(d != ddt for d in given):
        raise TypeError(f"y, out[0] and dy_dtype must agree on dy's dtype, not {given}")
    if ddt not in dts or (ddt != dout.dtype and dout.dtype != torch.float32):
        raise TypeError(f"combine_bwd of a {dout.dtype} dout writes {dout.dtype} rows (a float32 "
                        f"dout: any of {Y_DTYPES}), not {ddt}")
    _check_rows("combine_bwd", "dout", dout, S, H)
    if (H * torch.empty((), dtype=ddt).element_size()) % 16:
        raise ValueError(f"combine_bwd needs rows of whole 16-byte vectors (dy is {T} x {H} "
                         f"{ddt})")
    if y is not None:
        if y.device != dout.device:
            raise ValueError(f"y is on {y.device}, dout on {dout.device}")
        _check_rows("combine_bwd", "y", y, T, H)
    if out is not None:
        dy, dgate = out
        if dy.device != dout.device:
            raise ValueError(f"out[0] (dy) is on {dy.device}, dout on {dout.device}")
        _check_rows("combine_bwd", "out[0] (dy)", dy, T, H)
        if (dgate is None) != (y is None):
            raise ValueError("out[1] (dgate) goes with y: both or neither")
        if dgate is not None:
            if not isinstance(dgate, torch.Tensor) or dgate.dtype != torch.float32:
                raise TypeError(f"out[1] (dgate) must be a float32 tensor, not "
                                f"{getattr(dgate, 'dtype', type(dgate))}")
            if tuple(dgate.shape) != (S, k) or not dgate.is_contiguous():
                raise ValueError(f"out[1] (dgate) must be contiguous with shape {(S, k)}, not "
                                 f"{tuple(dgate.shape)}")
            if dgate.device != dout.device:
                raise ValueError(f"out[1] (dgate) is on {dgate.device}, dout on {dout.device}")
    if dout.device.type != "cuda":  # last, so that CPU tensors reach every refusal above
        raise ValueError("combine_bwd needs ROCm device tensors (combine_bwd_reference runs "
                         "anywhere)")
    return S, k, T, H, ddt


def combine_bwd(dout, slot_row, gate, row_token, y=None, *, dy_dtype=None, out=None,
                stream=None):
    """The backward of :func:`combine` (``csrc/moe/moe_combine_bwd.hip``): ``dout [S, H]`` bf16 /
    f16 / f32 -> ``(dy [T, H], dgate [S, k] | None)``. ``dy`` has ``dy_dtype``: ``dout``'s dtype
    (default) or, for a float32 ``dout``, any of the three (the mirror of :func:`combine`'s
    pairs); ``y [T, H]``, the forward's input, has ``dy``'s dtype.

    Precondition: ``(row_token, slot_row)`` are mutually inverse, as :func:`route` writes them.
    Then every element of ``dy`` and ``dgate`` is written: for ``t = row_token[r]`` in ``[0, S)``
    and the ``j`` with ``slot_row[t, j] == r``, ``dy[r, c] = rne(gate[t, j] * float(dout[t, c]))``,
    one fp32 multiply and one rounding, bit for bit ``(gate[t, j] * dout[t].float()).to(dtype)``;
    the other rows (the padding behind ``offsets[E]``) are ``+0.0``. ``dgate[t, j]`` is the fp32
    sum over ``c`` of ``float(dout[t, c]) * float(y[slot_row[t, j], c])`` in a fixed order (bitwise
    reproducible, no atomics) and ``+0.0`` for a dropped or out-of-range slot, whose row is not
    read; it is what trains a router. ``y=None``: the gates need no gradient, the dot products are
    skipped and ``dgate`` is ``None``. Without the precondition every index is still
    range-checked before use; the values are then unspecified. :func:`_check_combine_bwd` holds
    every refusal."""
    import torch

    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import dtype_code

    S, k, T, H, ddt = _check_combine_bwd(dout, slot_row, gate, row_token, y, dy_dtype, out)
    dev = dout.device
    if out is None:
        dy = torch.empty((T, H), dtype=ddt, device=dev)
        dgate = None if y is None else torch.empty((S, k), dtype=torch.float32, device=dev)
    else:
        dy, dgate = out
    C = load()
    if dgate is not None and (T == 0 or H == 0):
        dgate.zero_()  # no row to read
    if H == 0 or T == 0:
        return dy, dgate
    strm = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        C.moe_combine_bwd(dout=dout.data_ptr(), slot_row=slot_row.data_ptr(),
                          gate=gate.data_ptr(), row_token=row_token.data_ptr(),
                          y=0 if y is None else y.data_ptr(), dy=dy.data_ptr(),
                          dgate=0 if dgate is None else dgate.data_ptr(), lddo=_ld(dout),
                          ldy=H if y is None else _ld(y), lddy=_ld(dy), S=S, k=k, T=T, H=H,
                          din=dtype_code(dout.dtype), dout_dt=dtype_code(ddt), stream=strm)
    if stream is not None:  # the outputs stay allocated until that stream reaches them
        for t in (dy, dgate):
            if t is not None:
                t.record_stream(torch.cuda.ExternalStream(strm))
    return dy, dgate


def combine_bwd_reference(dout, slot_row, gate, row_token, y=None, dy_dtype=None):
    """The specification of :func:`combine_bwd` in torch ops, on any device: ``dy`` with the same
    fp32 multiply and one rounding, ``dgate`` in fp64 (``None`` without ``y``)."""
    import torch

    S, k = slot_row.shape
    T = row_token.shape[0]
    H = dout.shape[1]
    ddt = dy_dtype or (y.dtype if y is not None else dout.dtype)
    dy = torch.zeros((T, H), dtype=ddt, device=dout.device)
    dgate = None if y is None else torch.zeros((S, k), dtype=torch.float64, device=dout.device)
    if T == 0 or S == 0:
        return dy, dgate
    d32 = dout.to(torch.float32)
    for j in range(k):
        r = slot_row[:, j].to(torch.int64)
        valid = ((r >= 0) & (r < T)).nonzero().flatten()
        rows = r[valid]
        dy[rows] = (gate[valid, j:j + 1] * d32[valid]).to(ddt)
        if y is not None:
            dgate[valid, j] = (d32[valid].double() * y[rows].double()).sum(dim=1)
    return dy, dgate
