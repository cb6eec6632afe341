"""MX block scaling for the fp8 GEMM: the quantiser and its specification.

The format. A block is 32 consecutive K elements of one row of ``A [M, K]`` or ``W [N, K]``. Each
block carries one E8M0 byte ``s`` (value ``2^(s - 127)``); the scales of a tensor are a ``uint8``
``[rows, K / 32]`` row-major array. ``K % 128 == 0`` (the MFMA fast path's own rule for fp8), so a
row's four scales of one 128-byte K-tile are one aligned 32-bit word.

The quantisation rule rounds the scale UP, so nothing saturates. Per block, in fp32:
``amax = max|x|``; ``amax == 0`` gives ``s = 127`` and ``q = 0``; otherwise ``amax = m 2^ex`` with
``m`` in [0.5, 1) and ``e = ex - 9`` if ``m <= 0.875`` else ``ex - 8`` (the smallest ``e`` with
``amax / 2^e <= 448``, the largest e4m3 value), clamped to [-127, 127]; ``s = e + 127`` and
``q = e4m3_rne(clamp(x 2^-e, -448, 448))``. ``s = 255`` is never produced. The sign of a zero is
kept: -0, and a negative value that rounds to zero, give the byte 0x80 (kernel and reference
agree byte for byte, ``tests/test_mx_extremes_gpu.py``). (The OCP "floor" rule,
``e = floor(log2 amax) - 8``, would clamp every element above 448 2^e: 11 % of the elements of
U[-1, 1) data.)

Non-finite input (all seven producers: the three row quantisers, the transposing, two-way and
grouped transposing ones, and the GEMM's quantising epilogue; ``tests/test_nonfinite_gpu.py``).
``amax`` is taken over the finite elements only: a NaN or +-Inf element counts as 0, and a block
with no finite non-zero element gets ``s = 127``. The finite elements are quantised exactly as
without it; no byte of an all-finite block depends on this paragraph. A NaN or +-Inf element
becomes the e4m3fn NaN byte with the input's sign, ``0x7F | sign << 7`` (e4m3fn has no Inf; it is
what torch's own cast gives). The reference builds these bytes itself (``torch.where`` on
``~isfinite``) and relies on no device's cast. An upstream overflow or NaN therefore stays visible:
the scaled GEMM that reads the block returns NaN for that row (or column).

:func:`quantize_mx_reference` and :func:`dequantize_mx` are pure torch, run on any device, and are
the specification; :func:`quantize_mx` is the HIP kernel (``csrc/gemm/mx_quant.hip``).

MXFP4 is the same block format with OCP E2M1 elements. A nibble is ``sign << 3 | code``; codes
0..7 stand for 0, 0.5, 1, 1.5, 2, 3, 4, 6. Two elements share a byte, element ``2j`` in the low
nibble of byte ``j`` (torch's ``float4_e2m1fn_x2``), so a quantised tensor is ``float4_e2m1fn_x2
[rows, K / 2]`` beside the same ``uint8 [rows, K / 32]`` scales. ``K % 256 == 0``: a 128-byte
K-tile row of the kernel holds 256 elements and eight scales, one aligned 64-bit word. The rule is
the fp8 one with 6 in place of 448: ``e = ex - 3`` if ``m <= 0.75`` else ``ex - 2`` (the smallest
``e`` with ``amax / 2^e <= 6``), clamped to [-127, 127]; ``q = e2m1_rne(clamp(x 2^-e, -6, 6))``
with ties to the even code (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4,
5 -> 4). The input's sign bit is kept (-0 and a negative value that rounds to zero give 0x8).
:func:`quantize_mxfp4_reference` / :func:`dequantize_mxfp4` are the specification,
:func:`quantize_mxfp4` the HIP kernel.

Non-finite input in MXFP4. E2M1 has no NaN; the format's only NaN is the scale byte 255, and in
the OCP rule every element of such a block is NaN. The block-scaled MFMA of gfx950 follows it:
with one ``a_scale`` byte set to 255 the output row is NaN in every column, zero-valued elements
and an all-zero block included, for every tile code, MX-fp8 and MXFP4 alike (measured,
``test_scale_byte_255``; docs/RESULTS.md). So a block that holds any NaN or +-Inf element gets
``s = 255``; its finite elements are quantised by the finite-amax rule above and each non-finite
element gets the nibble ``0x7 | sign << 3``. :func:`dequantize_mx` and :func:`dequantize_mxfp4`
return NaN for every element of a block with ``s = 255``. MX-fp8 never produces ``s = 255``; an
all-finite MXFP4 block never does either.
"""

from __future__ import annotations

BLOCK = 32
E4M3_MAX = 448.0
IN_DTYPES = ("bfloat16", "float16", "float32")
E2M1_MAX = 6.0
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)  # magnitude of codes 0..7


def _check_2d(x) -> None:
    if x.dim() != 2:
        raise ValueError(f"MX quantisation expects a 2-D tensor, not {tuple(x.shape)}")
    if x.shape[1] % 128:
        raise ValueError(f"MX quantisation needs K % 128 == 0 (K = {x.shape[1]})")


def ldexp_exact(x, n):
    """``x * 2^n`` (float32 ``x``, integer tensor ``n`` in [-252, 254]) with every power of two
    built from its bit pattern. ``torch.ldexp`` multiplies by ``pow(2, n)``, which a GPU's
    ``powf`` does not return exactly: a value on an e4m3 rounding tie then lands on the wrong
    side. Two normal factors cover 2^-127 and keep each product exact short of underflow."""
    import torch

    n = n.to(torch.int32)
    h = torch.div(n, 2, rounding_mode="floor")

    def pow2(k):  # k in [-126, 127]: a normal, finite factor
        return ((k + 127) << 23).view(torch.float32)

    return x * pow2(h) * pow2(n - h)


def quantize_mx_reference(x):
    """``x [R, K]`` (any float dtype, any device) -> ``(q [R, K] float8_e4m3fn, s [R, K/32]
    uint8)`` by the rule in the module docstring."""
    import torch

    _check_2d(x)
    R, K = x.shape
    xb = x.to(torch.float32).reshape(R, K // BLOCK, BLOCK)
    finite = torch.isfinite(xb)
    xf = torch.where(finite, xb, torch.zeros_like(xb))  # a non-finite element counts as 0
    amax = xf.abs().amax(dim=2)
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.875, ex - 9, ex - 8).clamp(-127, 127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    # the clamp stays: torch's own e4m3 cast turns values above 464 into NaN
    y = ldexp_exact(xf, (-e).unsqueeze(2)).clamp(-E4M3_MAX, E4M3_MAX)
    # NaN and +-Inf: the e4m3fn NaN byte with the input's sign, built here (no device's cast)
    sign = (xb.view(torch.int32) >> 31) & 1
    q = torch.where(finite, y.to(torch.float8_e4m3fn).view(torch.uint8),
                    (0x7F | (sign << 7)).to(torch.uint8))
    return q.view(torch.float8_e4m3fn).reshape(R, K), (e + 127).to(torch.uint8)


def _nan_blocks(v, s):
    """``v [R, K / 32, 32]`` with every element of a block whose scale byte is 255 (the E8M0 NaN)
    set to NaN, zeros included, as the block-scaled MFMA treats it."""
    import torch

    return torch.where((s == 255).unsqueeze(2), torch.full_like(v, float("nan")), v)


def dequantize_mx(q, s):
    """``q [R, K]`` e4m3 and ``s [R, K/32]`` E8M0 bytes -> the float32 values they stand for.
    fp32 cannot hold every one of them: at ``s = 254`` an element with ``|q| >= 2`` is ``inf``
    here (``2 * 2^127``), while the block-scaled MFMA, which adds the two scale exponents before
    it rounds, returns the finite product it has with a small partner scale. The scaled GEMM is
    exact over the whole byte range 0..254 (measured against an fp64 dequantisation,
    ``tests/test_mx_extremes_gpu.py``)."""
    import torch

    R, K = q.shape
    if tuple(s.shape) != (R, K // BLOCK):
        raise ValueError(f"scales must have shape {(R, K // BLOCK)}, not {tuple(s.shape)}")
    e = s.to(torch.int32) - 127
    v = ldexp_exact(q.to(torch.float32).reshape(R, K // BLOCK, BLOCK), e.unsqueeze(2))
    return _nan_blocks(v, s).reshape(R, K)


def _quantize_rows(x, fp4: bool, stream):
    """The body of :func:`quantize_mx` / :func:`quantize_mxfp4`: every check, then the launch."""
    import torch

    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import dtype_code

    name = "quantize_mxfp4" if fp4 else "quantize_mx"
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} expects a tensor")
    if x.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise TypeError(f"{name} takes {IN_DTYPES}, not {x.dtype}")
    if x.device.type != "cuda":
        raise ValueError(f"{name} needs a ROCm device tensor ({name}_reference runs anywhere)")
    (_check_2d_fp4 if fp4 else _check_2d)(x)
    R, K = x.shape
    if R >= 2 ** 31 or K >= 2 ** 31:
        raise ValueError("dimensions must fit in 32 bits")
    if x.stride(1) != 1 or (R > 1 and x.stride(0) < K):
        raise ValueError(f"{name} needs row-major input with unit inner stride")
    if x.data_ptr() % 16 or (x.stride(0) * x.element_size()) % 16:
        raise ValueError(f"{name} needs 16-byte-aligned rows")
    C = load()
    q, s = _alloc_quant(R, K, fp4, x.device)
    if R > 0:
        st = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
        with torch.cuda.device(x.device):
            (C.mxfp4_quantize if fp4 else C.mx_quantize)(
                x.data_ptr(), q.data_ptr(), s.data_ptr(), max(x.stride(0), K), q.shape[1],
                K // BLOCK, R, K, dtype_code(x.dtype), st)
        if stream is not None:  # the outputs stay allocated until that stream reaches them
            q.record_stream(torch.cuda.ExternalStream(st))
            s.record_stream(torch.cuda.ExternalStream(st))
    return q.view(torch.float4_e2m1fn_x2 if fp4 else torch.float8_e4m3fn), s


def quantize_mx(x, *, stream=None):
    """The HIP quantiser: ``x [R, K]`` bf16 / f16 / f32 on a ROCm device -> ``(q, s)`` as
    :func:`quantize_mx_reference` computes them, on ``stream`` (default: the current one). Every
    shape / dtype / stride / alignment check happens here, before the launch."""
    return _quantize_rows(x, False, stream)


# ---------------------------------------------------------------- MXFP4 (E2M1 elements)
def _check_2d_fp4(x) -> None:
    if x.dim() != 2:
        raise ValueError(f"MXFP4 quantisation expects a 2-D tensor, not {tuple(x.shape)}")
    if x.shape[1] % 256:
        raise ValueError(f"MXFP4 quantisation needs K % 256 == 0 (K = {x.shape[1]})")


def _e2m1_code(y):
    """E2M1 code 0..7 (int32) of float32 ``y`` in [0, 6]: round to nearest, ties to the even
    code. The step is 0.5 below 2, 1 below 4 and 2 up to 6, each a power of two, so rounding the
    value divided by its step to an integer (``torch.round``: half to even) is exact."""
    import torch

    lo = torch.round(y * 2.0)
    mid = torch.round(y) + 2.0
    hi = torch.round(y * 0.5) + 4.0
    return torch.where(y < 2.0, lo, torch.where(y < 4.0, mid, hi)).to(torch.int32)


def quantize_mxfp4_reference(x):
    """``x [R, K]`` (any float dtype, any device) -> ``(q [R, K/2] float4_e2m1fn_x2, s [R, K/32]
    uint8)`` by the MXFP4 rule in the module docstring."""
    import torch

    _check_2d_fp4(x)
    R, K = x.shape
    xb = x.to(torch.float32).reshape(R, K // BLOCK, BLOCK)
    finite = torch.isfinite(xb)
    xf = torch.where(finite, xb, torch.zeros_like(xb))  # a non-finite element counts as 0
    amax = xf.abs().amax(dim=2)
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.75, ex - 3, ex - 2).clamp(-127, 127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    y = ldexp_exact(xf, (-e).unsqueeze(2))
    code = _e2m1_code(y.abs().clamp(max=E2M1_MAX))
    code = torch.where(finite, code, torch.full_like(code, 7))  # NaN, +-Inf: the nibble 0x7 | sign
    sign = (xb.view(torch.int32) >> 31) & 1  # the input's sign bit: -0 stays negative
    # a block that holds a non-finite element: the E8M0 NaN byte
    s = torch.where(finite.all(dim=2), e + 127, torch.full_like(e, 255))
    return pack_e2m1(((sign << 3) | code).reshape(R, K)), s.to(torch.uint8)


def pack_e2m1(nib):
    """``nib [R, K]`` integer nibbles (``sign << 3 | code``, K even) -> ``[R, K/2]``
    float4_e2m1fn_x2, element ``2j`` in the low nibble of byte ``j``."""
    import torch

    R, K = nib.shape
    if K % 2:
        raise ValueError(f"an odd number of fp4 elements per row ({K}) does not pack")
    n = (nib.to(torch.int32) & 0xF).reshape(R, K // 2, 2)
    return (n[..., 0] | (n[..., 1] << 4)).to(torch.uint8).view(torch.float4_e2m1fn_x2)


def unpack_e2m1(q):
    """``q [R, K/2]`` float4_e2m1fn_x2 (or its uint8 bytes) -> float32 ``[R, K]`` element values,
    decoded by table (-0 decodes to -0)."""
    import torch

    b = q.view(torch.uint8) if q.dtype != torch.uint8 else q
    R, KB = b.shape
    nib = torch.stack((b & 0xF, b >> 4), dim=2).reshape(R, 2 * KB).to(torch.int64)
    mag = torch.tensor(E2M1_VALUES, dtype=torch.float32, device=b.device)[nib & 7]
    return torch.where((nib & 8) != 0, -mag, mag)


def dequantize_mxfp4(q, s):
    """``q [R, K/2]`` float4_e2m1fn_x2 and ``s [R, K/32]`` E8M0 bytes -> the float32 values they
    stand for (``s = 254`` with ``|q| >= 2`` is ``inf`` in fp32, as for :func:`dequantize_mx`)."""
    import torch

    if q.dim() != 2:
        raise ValueError(f"MXFP4 data must be 2-D, not {tuple(q.shape)}")
    R, K = q.shape[0], 2 * q.shape[1]
    if K % BLOCK or tuple(s.shape) != (R, K // BLOCK):
        raise ValueError(f"scales must have shape {(R, K // BLOCK)}, not {tuple(s.shape)}")
    e = s.to(torch.int32) - 127
    v = ldexp_exact(unpack_e2m1(q).reshape(R, K // BLOCK, BLOCK), e.unsqueeze(2))
    return _nan_blocks(v, s).reshape(R, K)


def quantize_mxfp4(x, *, stream=None):
    """The HIP quantiser: ``x [R, K]`` bf16 / f16 / f32 on a ROCm device -> ``(q, s)`` as
    :func:`quantize_mxfp4_reference` computes them, on ``stream`` (default: the current one).
    Every shape / dtype / stride / alignment check happens here, before the launch."""
    return _quantize_rows(x, True, stream)


# ---------------------------------------------------------------- gathering quantisation
# A routed layer quantises its tokens in the order of its sorted (token, choice) rows. The row
# quantiser has to read x anyway, so it reads x[src[r]] and the permuted 16-bit copy of x is never
# written. An index outside x makes a zero row, which gives padding rows a defined content.
def quantize_mx_gather_reference(x, src, fmt: str = "mx"):
    """``x [X, K]`` (any float dtype, any device), ``src [R]`` integer -> ``(q, s)``: the reference
    row quantisation of ``x[src]``, a zero row (zero data, scale byte 127) where ``src[r]`` is
    outside ``[0, X)``. The specification of :func:`quantize_mx_gather`."""
    import torch

    fp4 = _t_fmt(fmt)
    if x.dim() != 2:
        raise ValueError(f"MX quantisation expects a 2-D tensor, not {tuple(x.shape)}")
    r = src.to(torch.int64)
    valid = (r >= 0) & (r < x.shape[0])
    if x.shape[0]:
        rows = x.index_select(0, torch.where(valid, r, torch.zeros_like(r)))
        rows = torch.where(valid.unsqueeze(1), rows, torch.zeros_like(rows))
    else:
        rows = torch.zeros((r.shape[0], x.shape[1]), dtype=x.dtype, device=x.device)
    return quantize_mxfp4_reference(rows) if fp4 else quantize_mx_reference(rows)


def _check_quant_gather(x, src, fmt: str):
    """Every refusal of :func:`quantize_mx_gather`, on the host and before the extension is loaded
    (CPU tensors reach the device refusal; the indices are never read). Returns
    ``(X, K, R, fp4)``."""
    import torch

    name = "quantize_mx_gather"
    fp4 = _t_fmt(fmt)
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} expects a tensor")
    if x.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise TypeError(f"{name} takes {IN_DTYPES}, not {x.dtype}")
    if fp4 and not hasattr(torch, "float4_e2m1fn_x2"):
        raise TypeError("fmt='mxfp4' needs torch.float4_e2m1fn_x2")
    (_check_2d_fp4 if fp4 else _check_2d)(x)
    if not isinstance(src, torch.Tensor) or src.dtype != torch.int32:
        raise TypeError(f"src must be an int32 tensor, not {getattr(src, 'dtype', type(src))}")
    if src.dim() != 1 or not src.is_contiguous():
        raise ValueError(f"src must be contiguous and 1-D, not {tuple(src.shape)}")
    if src.device != x.device:
        raise ValueError(f"src is on {src.device}, x on {x.device}")
    X, K = x.shape
    R = src.shape[0]
    if X >= 2 ** 31 or K >= 2 ** 31 or R >= 2 ** 31:
        raise ValueError("dimensions must fit in 32 bits")
    if X and (x.stride(1) != 1 or (X > 1 and x.stride(0) < K)):
        raise ValueError(f"{name} needs row-major input with unit inner stride")
    if X and (x.data_ptr() % 16 or (x.stride(0) * x.element_size()) % 16):
        raise ValueError(f"{name} needs 16-byte-aligned rows")
    if x.device.type != "cuda":  # last, so that CPU tensors reach every refusal above
        raise ValueError(f"{name} needs a ROCm device tensor ({name}_reference runs anywhere)")
    return X, K, R, fp4


def quantize_mx_gather(x, src, *, fmt: str = "mx", stream=None):
    """The HIP gathering row quantiser (``csrc/gemm/mx_quant.hip``): ``x [X, K]`` bf16 / f16 / f32
    and ``src [R]`` int32 on one ROCm device -> ``(q [R, K], s [R, K / 32])`` (``fmt="mxfp4"``:
    ``q [R, K / 2]`` float4_e2m1fn_x2) with row ``r`` byte for byte what :func:`quantize_mx` /
    :func:`quantize_mxfp4` write for ``x[src[r]]``. ``src[r]`` outside ``[0, X)`` gives a zero
    row with scale byte 127: nothing in ``src`` (read by the kernel only, no host sync) can
    address outside ``x``. :func:`_check_quant_gather` holds every refusal."""
    import torch

    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import dtype_code

    X, K, R, fp4 = _check_quant_gather(x, src, fmt)
    C = load()
    q, s = _alloc_quant(R, K, fp4, x.device)
    if R > 0:
        st = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
        with torch.cuda.device(x.device):
            C.mx_quantize_gather(x=x.data_ptr(), src=src.data_ptr(), q=q.data_ptr(),
                                 s=s.data_ptr(), ldx=max(x.stride(0), K), ldq=q.shape[1],
                                 lds=K // BLOCK, R=R, K=K, X=X, din=dtype_code(x.dtype), fp4=fp4,
                                 stream=st)
        if stream is not None:  # the outputs stay allocated until that stream reaches them
            q.record_stream(torch.cuda.ExternalStream(st))
            s.record_stream(torch.cuda.ExternalStream(st))
    return q.view(torch.float4_e2m1fn_x2 if fp4 else torch.float8_e4m3fn), s


# ---------------------------------------------------------------- transposed quantisation
# A GEMM that contracts over the ROWS of ``x [R, C]`` (a linear layer's dgrad contracts over N,
# its wgrad over M) needs the blocks down the columns of ``x`` and those blocks stored as
# K-contiguous rows: ``qt [C, R]`` (fp4: ``[C, R / 2]``) and ``st [C, R / 32]``, the row-wise
# quantisation of ``x.T``. It is another quantisation of the tensor, not a transpose of the
# row-wise one: a column block and a row block hold different elements and get different scales.
T_FMTS = ("mx", "mxfp4")


def _t_fmt(fmt: str) -> bool:
    if fmt not in T_FMTS:
        raise ValueError(f"fmt must be one of {T_FMTS}, not {fmt!r}")
    return fmt == "mxfp4"


def quantize_mx_t_reference(x, fmt: str = "mx"):
    """``x [R, C]`` (any float dtype, any device) -> ``(qt, st)``: the reference quantisation of
    ``x.t().contiguous()``. ``qt`` is ``[C, R]`` float8_e4m3fn (``fmt="mxfp4"``: ``[C, R / 2]``
    float4_e2m1fn_x2), ``st`` is ``[C, R / 32]`` uint8. The specification of
    :func:`quantize_mx_t`."""
    fp4 = _t_fmt(fmt)
    if x.dim() != 2:
        raise ValueError(f"MX quantisation expects a 2-D tensor, not {tuple(x.shape)}")
    xt = x.t().contiguous()
    return quantize_mxfp4_reference(xt) if fp4 else quantize_mx_reference(xt)


def check_quant_pair_types(names, data, scales, qdt, what):
    """A preallocated (data, scales) pair, either of them optional: ``qdt`` data, uint8 scales.
    ``names`` are the caller's argument names, ``what`` the format argument it was given."""
    import torch

    if data is not None and (not isinstance(data, torch.Tensor) or data.dtype != qdt):
        raise TypeError(f"{names[0]} must be a {qdt} tensor for {what}, not "
                        f"{getattr(data, 'dtype', type(data))}")
    if scales is not None and (not isinstance(scales, torch.Tensor)
                               or scales.dtype != torch.uint8):
        raise TypeError(f"{names[1]} must be a uint8 tensor of E8M0 bytes")


def check_quant_pair_layout(names, data, scales, ncol, nblk, sal):
    """The rows of such a pair as the GEMM that reads them asks: unit inner stride, data rows of
    ``ncol`` bytes 16-byte aligned, scale rows of ``nblk`` bytes aligned to ``sal`` (4; 8 beside
    fp4 data), bases included."""
    for name, t, cols, mod, unit in ((names[0], data, ncol, 16, " bytes"),
                                     (names[1], scales, nblk, sal, "")):
        if t is None:
            continue
        if t.stride(1) != 1 or t.stride(0) < cols or t.stride(0) % mod:
            raise ValueError(f"{name} needs unit inner stride and a row stride that is a "
                             f"multiple of {mod}{unit} (strides {tuple(t.stride())})")
        if t.data_ptr() % mod:
            raise ValueError(f"{name} must start at a {mod}-byte-aligned address")


def _check_quant_t(x, fmt: str, out=None, *, two_way: bool = False):
    """Every refusal of :func:`quantize_mx_t` / :func:`quantize_mx_2way`, on the host and before
    the extension is loaded (CPU tensors reach the device refusal). Returns ``(R, C, fp4)``."""
    import torch

    name = "quantize_mx_2way" if two_way else "quantize_mx_t"
    fp4 = _t_fmt(fmt)
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} expects a tensor")
    if x.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise TypeError(f"{name} takes {IN_DTYPES}, not {x.dtype}")
    if fp4 and not hasattr(torch, "float4_e2m1fn_x2"):
        raise TypeError("fmt='mxfp4' needs torch.float4_e2m1fn_x2")
    if x.dim() != 2:
        raise ValueError(f"{name} expects a 2-D tensor, not {tuple(x.shape)}")
    R, C = x.shape
    mod = 256 if fp4 else 128
    if R % mod:
        raise ValueError(f"{name}(fmt={fmt!r}) needs R % {mod} == 0 (x is {R} x {C}): R is the K "
                         "of the GEMM that reads the transposed result")
    if (C * x.element_size()) % 16:
        raise ValueError(f"{name} needs rows of whole 16-byte vectors (x is {R} x {C} {x.dtype})")
    if two_way and C % mod:
        raise ValueError(f"{name}(fmt={fmt!r}) needs C % {mod} == 0 as well (x is {R} x {C})")
    if R >= 2 ** 31 or C >= 2 ** 31:
        raise ValueError("dimensions must fit in 32 bits")
    empty = R == 0 or C == 0  # nothing is read: torch gives such a tensor any strides
    if not empty and (x.stride(1) != 1 or (R > 1 and x.stride(0) < C)):
        raise ValueError(f"{name} needs row-major input with unit inner stride")
    if not empty and (x.data_ptr() % 16 or (x.stride(0) * x.element_size()) % 16):
        raise ValueError(f"{name} needs 16-byte-aligned rows")
    if R * max(x.stride(0), C) * x.element_size() >= 2 ** 31:
        raise ValueError(f"{name}: x spans 2 GiB or more")
    ncol, sal = (R // 2 if fp4 else R), (8 if fp4 else 4)
    if out is not None:
        if two_way:
            raise ValueError(f"{name} allocates its outputs")
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise TypeError("out must be a pair (qt, st)")
        qt, st = out
        qdt = torch.float4_e2m1fn_x2 if fp4 else torch.float8_e4m3fn
        check_quant_pair_types(("out[0]", "out[1]"), qt, st, qdt, f"fmt={fmt!r}")
        if qt.device != x.device or st.device != x.device:
            raise ValueError(f"out is on {qt.device} / {st.device}, x on {x.device}")
        if tuple(qt.shape) != (C, ncol):
            raise ValueError(f"out[0] must have shape {(C, ncol)}, not {tuple(qt.shape)}")
        if tuple(st.shape) != (C, R // BLOCK):
            raise ValueError(f"out[1] must have shape {(C, R // BLOCK)}, not {tuple(st.shape)}")
        check_quant_pair_layout(("out[0]", "out[1]"), qt, st, ncol, R // BLOCK, sal)
        if C * qt.stride(0) >= 2 ** 31 or C * st.stride(0) >= 2 ** 31:
            raise ValueError("out spans 2 GiB or more")
    if C * ncol >= 2 ** 31:
        raise ValueError(f"{name}: the quantised tensor spans 2 GiB or more")
    if x.device.type != "cuda":  # last, so that CPU tensors reach every refusal above
        raise ValueError(f"{name} needs a ROCm device tensor (quantize_mx_t_reference runs "
                         "anywhere)")
    return R, C, fp4


def _launch_quant_t(x, R, C, fp4, qt, st, q, s, stream):
    import torch

    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import dtype_code

    C_ = load()
    if R == 0 or C == 0:
        return
    strm = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
    two = q is not None
    with torch.cuda.device(x.device):
        C_.mx_quantize_t(x.data_ptr(), qt.data_ptr(), st.data_ptr(), max(x.stride(0), C),
                         qt.stride(0), st.stride(0), R, C, dtype_code(x.dtype), fp4, strm, two,
                         q.data_ptr() if two else 0, s.data_ptr() if two else 0,
                         q.stride(0) if two else 0, s.stride(0) if two else 0)
    if stream is not None:  # the outputs stay allocated until that stream reaches them
        for t in (qt, st, q, s):
            if t is not None:
                t.record_stream(torch.cuda.ExternalStream(strm))


def _alloc_quant(rows, cols, fp4, device):
    """Dense quantised data (as bytes) and scales of a ``[rows, cols]``-element tensor."""
    import torch

    q = torch.empty((rows, cols // 2 if fp4 else cols), dtype=torch.uint8, device=device)
    return q, torch.empty((rows, cols // BLOCK), dtype=torch.uint8, device=device)


def quantize_mx_t(x, *, fmt: str = "mx", out=None, stream=None):
    """The HIP transposing quantiser (``csrc/gemm/mx_quant_t.hip``): ``x [R, C]`` bf16 / f16 /
    f32 on a ROCm device -> ``(qt, st)`` as :func:`quantize_mx_t_reference` computes them, byte
    for byte, in one pass over ``x`` on ``stream`` (default: the current one). ``R % 128 == 0``
    (``fmt="mxfp4"``: 256): ``R`` is the K of the GEMM that takes ``qt`` / ``st`` as ``a`` /
    ``a_scale`` or ``w`` / ``w_scale``. ``C`` needs whole 16-byte vectors and nothing more.

    ``out = (qt, st)`` may be preallocated, for instance views into a buffer saved for a backward
    pass: ``qt`` ``[C, R]`` float8_e4m3fn (fp4: ``[C, R / 2]`` float4_e2m1fn_x2) with a 16-byte
    aligned base and a row stride that is a multiple of 16; ``st`` ``[C, R / 32]`` uint8 with base
    and row stride multiples of 4 (fp4: 8). Every refusal is raised here, before the launch."""
    import torch

    R, C, fp4 = _check_quant_t(x, fmt, out)
    if out is None:
        qt, st = _alloc_quant(C, R, fp4, x.device)
        if fp4:
            qt = qt.view(torch.float4_e2m1fn_x2)
        else:
            qt = qt.view(torch.float8_e4m3fn)
    else:
        qt, st = out
    _launch_quant_t(x, R, C, fp4, qt, st, None, None, stream)
    return qt, st


def quantize_mx_2way(x, *, fmt: str = "mx", stream=None):
    """Both quantisations of ``x [R, C]`` in one launch that reads ``x`` once: ``(q, s, qt, st)``
    with ``q, s`` byte-identical to :func:`quantize_mx` (:func:`quantize_mxfp4`) and ``qt, st`` to
    :func:`quantize_mx_t`. ``R`` and ``C`` are both multiples of 128 (``fmt="mxfp4"``: 256)."""
    import torch

    R, C, fp4 = _check_quant_t(x, fmt, two_way=True)
    qdt = torch.float4_e2m1fn_x2 if fp4 else torch.float8_e4m3fn
    q, s = _alloc_quant(R, C, fp4, x.device)
    qt, st = _alloc_quant(C, R, fp4, x.device)
    _launch_quant_t(x, R, C, fp4, qt, st, q, s, stream)
    return q.view(qdt), s, qt.view(qdt), st


# ---------------------------------------------------------------- grouped transposing quantiser
# The operands of a K-grouped GEMM (ddlb_amd.ops.gemm.gemm_kgrouped): the rows of x are sorted into
# groups and every group is quantised down its own rows, its blocks starting at the group's first
# row and its tail padded with zeros to a whole K-tile (ops.gemm.padded_offsets has the layout).
def quantize_mx_t_grouped_reference(x, offsets, fmt: str = "mx", stacked_rows: int = 0):
    """The specification of :func:`quantize_mx_t_grouped` on any device (reads ``offsets`` on the
    host): per group, :func:`quantize_mx_t_reference` of the group's rows padded with zero rows to
    a multiple of 128 (``fmt="mxfp4"``: 256). Returns ``(qt, st, written)`` as uint8 tensors:
    ``qt [C, cap]`` (fp4 ``[C, cap / 2]``), ``st [C, cap / 32]`` and a bool ``[cap]`` that marks
    the columns some group owns (the others hold zeros here and are not written by the kernel).
    ``stacked_rows = R``: ``qt [E, C, R]`` (fp4 ``R / 2``), ``st [E, C, R / 32]``, ``written
    [E, R]``; a group's tiles at or past row ``R`` are dropped."""
    import torch

    from ddlb_amd.ops.gemm import clamp_offsets, kgrouped_capacity, padded_offsets

    fp4 = _t_fmt(fmt)
    mod = 256 if fp4 else 128
    T, C = x.shape
    E = offsets.shape[0] - 1
    o = clamp_offsets(offsets, T)
    R = int(stacked_rows)
    cap = R if R else kgrouped_capacity(T, E, mod)
    lead = (E,) if R else ()
    qt = torch.zeros(lead + (C, cap // 2 if fp4 else cap), dtype=torch.uint8, device=x.device)
    st = torch.zeros(lead + (C, cap // BLOCK), dtype=torch.uint8, device=x.device)
    written = torch.zeros(lead + (cap,), dtype=torch.bool, device=x.device)
    k0s = padded_offsets(offsets, T, mod)
    for g in range(E):
        n = o[g + 1] - o[g]
        kl = k0s[g + 1] - k0s[g]
        if kl == 0:
            continue
        pad = torch.zeros((kl, C), dtype=x.dtype, device=x.device)
        pad[:n] = x[o[g]:o[g + 1]]
        q, s = quantize_mx_t_reference(pad, fmt)
        q = q.view(torch.uint8)
        if R:
            kl = min(kl, R)
            qt[g, :, :kl // (2 if fp4 else 1)] = q[:, :kl // (2 if fp4 else 1)]
            st[g, :, :kl // BLOCK] = s[:, :kl // BLOCK]
            written[g, :kl] = True
        else:
            k0 = k0s[g]
            d = 2 if fp4 else 1
            qt[:, k0 // d:(k0 + kl) // d] = q
            st[:, k0 // BLOCK:(k0 + kl) // BLOCK] = s
            written[k0:k0 + kl] = True
    return qt, st, written


def _check_quant_t_grouped(x, offsets, fmt: str, out=None, stacked_rows: int = 0):
    """Every refusal of :func:`quantize_mx_t_grouped`, on the host and before the extension is
    loaded (CPU tensors reach the device refusal; the offsets' content is never read). Returns
    ``(T, C, E, fp4, cap)``: ``cap`` the column capacity of the outputs (stacked: ``R``)."""
    import torch

    from ddlb_amd.ops.gemm import MAX_GROUPS, kgrouped_capacity

    name = "quantize_mx_t_grouped"
    fp4 = _t_fmt(fmt)
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{name} expects a tensor")
    if x.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise TypeError(f"{name} takes {IN_DTYPES}, not {x.dtype}")
    if fp4 and not hasattr(torch, "float4_e2m1fn_x2"):
        raise TypeError("fmt='mxfp4' needs torch.float4_e2m1fn_x2")
    if x.dim() != 2:
        raise ValueError(f"{name} expects a 2-D tensor, not {tuple(x.shape)}")
    if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int32:
        raise TypeError(f"offsets must be an int32 tensor, not "
                        f"{getattr(offsets, 'dtype', type(offsets))}")
    if offsets.dim() != 1 or not offsets.is_contiguous():
        raise ValueError(f"offsets must be contiguous and 1-D, not {tuple(offsets.shape)}")
    E = offsets.shape[0] - 1
    if E < 1 or E > MAX_GROUPS:
        raise ValueError(f"{name} takes 1 .. {MAX_GROUPS} groups (offsets of 2 .. "
                         f"{MAX_GROUPS + 1} entries), not {E}")
    if offsets.device != x.device:
        raise ValueError(f"offsets is on {offsets.device}, x on {x.device}")
    T, C = x.shape
    mod = 256 if fp4 else 128
    R = int(stacked_rows)
    if R < 0 or R % mod:
        raise ValueError(f"{name}(fmt={fmt!r}) needs stacked_rows % {mod} == 0 and >= 0, not {R}")
    if (C * x.element_size()) % 16:
        raise ValueError(f"{name} needs rows of whole 16-byte vectors (x is {T} x {C} {x.dtype})")
    if T >= 2 ** 31 or C >= 2 ** 31:
        raise ValueError("dimensions must fit in 32 bits")
    empty = T == 0 or C == 0
    if not empty and (x.stride(1) != 1 or (T > 1 and x.stride(0) < C)):
        raise ValueError(f"{name} needs row-major input with unit inner stride")
    if not empty and (x.data_ptr() % 16 or (x.stride(0) * x.element_size()) % 16):
        raise ValueError(f"{name} needs 16-byte-aligned rows")
    cap = R if R else kgrouped_capacity(T, E, mod)
    ctiles = (C + 63) // 64
    if min(T // mod + E, -(-T // mod) * E) * ctiles > 2 ** 31 - 1:
        raise ValueError(f"{name}: the grid bound does not fit a launch")
    ncol, sal = (cap // 2 if fp4 else cap), (8 if fp4 else 4)
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise TypeError("out must be a pair (qt, st)")
        qt, st = out
        qdt = torch.float4_e2m1fn_x2 if fp4 else torch.float8_e4m3fn
        check_quant_pair_types(("out[0]", "out[1]"), qt, st, qdt, f"fmt={fmt!r}")
        if qt.device != x.device or st.device != x.device:
            raise ValueError(f"out is on {qt.device} / {st.device}, x on {x.device}")
        lead = (E,) if R else ()
        if tuple(qt.shape) != lead + (C, ncol):
            raise ValueError(f"out[0] must have shape {lead + (C, ncol)}, not {tuple(qt.shape)}")
        if tuple(st.shape) != lead + (C, cap // BLOCK):
            raise ValueError(f"out[1] must have shape {lead + (C, cap // BLOCK)}, not "
                             f"{tuple(st.shape)}")
        if R:
            for nm, t, m in (("out[0]", qt, 16), ("out[1]", st, sal)):
                if t.stride(0) % m or (E > 1 and t.stride(0) < C * t.stride(1)):
                    raise ValueError(f"{nm} needs slabs a multiple of {m} bytes and at least C "
                                     f"rows apart (strides {tuple(t.stride())})")
            check_quant_pair_layout(("out[0]", "out[1]"), qt[0], st[0], ncol, cap // BLOCK, sal)
        else:
            check_quant_pair_layout(("out[0]", "out[1]"), qt, st, ncol, cap // BLOCK, sal)
    if x.device.type != "cuda":  # last, so that CPU tensors reach every refusal above
        raise ValueError(f"{name} needs a ROCm device tensor (quantize_mx_t_grouped_reference "
                         "runs anywhere)")
    return T, C, E, fp4, cap


def quantize_mx_t_grouped(x, offsets, *, fmt: str = "mx", out=None, stacked_rows: int = 0,
                          stream=None):
    """The HIP transposing quantiser's grouped form (``csrc/gemm/mx_quant_t.hip``): ``x [T, C]``
    bf16 / f16 / f32 with its rows sorted into ``E`` groups by ``offsets`` (int32 ``[E + 1]`` on
    ``x``'s device, read by the kernel only and clamped as a grouped GEMM clamps them: no host
    sync) -> ``(qt, st)`` in the padded K layout of :func:`ddlb_amd.ops.gemm.gemm_kgrouped`:
    ``qt [C, cap]`` float8_e4m3fn (``fmt="mxfp4"``: ``[C, cap / 2]`` float4_e2m1fn_x2) and
    ``st [C, cap / 32]`` uint8, ``cap = kgrouped_capacity(T, E, 128 | 256)``. Group ``g``'s columns
    ``[k0_g, k0_g + kl_g)`` (:func:`ddlb_amd.ops.gemm.padded_offsets`) hold, byte for byte,
    :func:`quantize_mx_t_reference` of the group's rows padded with zero rows; columns at or past
    ``k0_E`` are not written (and unspecified in outputs allocated here).

    ``stacked_rows = R > 0`` (a multiple of 128 | 256): group ``g`` is written to ``qt[g]`` of
    ``qt [E, C, R]`` / ``st [E, C, R / 32]`` from column 0 and its tiles at or past row ``R`` are
    dropped. With ``x = w.reshape(E * N, K)``, ``offsets = arange(E + 1) * N`` and ``R = N`` one
    launch gives the column-wise quantisation ``[E, K, N]`` of every expert's weight, the ``w`` /
    ``w_scale`` a grouped dgrad takes.

    ``out = (qt, st)`` may be preallocated (aligned as for :func:`quantize_mx_t`).
    :func:`_check_quant_t_grouped` holds every refusal."""
    import torch

    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import dtype_code

    T, C, E, fp4, cap = _check_quant_t_grouped(x, offsets, fmt, out, stacked_rows)
    R = int(stacked_rows)
    qdt = torch.float4_e2m1fn_x2 if fp4 else torch.float8_e4m3fn
    if out is None:
        lead = (E,) if R else ()
        qt = torch.empty(lead + (C, cap // 2 if fp4 else cap), dtype=torch.uint8,
                         device=x.device).view(qdt)
        st = torch.empty(lead + (C, cap // BLOCK), dtype=torch.uint8, device=x.device)
    else:
        qt, st = out
    C_ = load()
    if T == 0 or C == 0:
        return qt, st
    strm = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
    with torch.cuda.device(x.device):
        C_.mx_quantize_t_grouped(
            x=x.data_ptr(), qt=qt.data_ptr(), st=st.data_ptr(), offs=offsets.data_ptr(),
            ngroups=E, ldx=max(x.stride(0), C), ldqt=qt.stride(-2), ldst=st.stride(-2), T=T, C=C,
            din=dtype_code(x.dtype), fp4=fp4, stacked_rows=R,
            qt_gstride=qt.stride(0) if R else 0, st_gstride=st.stride(0) if R else 0,
            stream=strm)
    if stream is not None:  # the outputs stay allocated until that stream reaches them
        for t in (qt, st):
            t.record_stream(torch.cuda.ExternalStream(strm))
    return qt, st
