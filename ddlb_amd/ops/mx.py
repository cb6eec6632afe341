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
agree byte for byte, ``tests/test_mx_extremes_gpu.py``). Non-finite input is unspecified. (The
OCP "floor" rule, ``e = floor(log2 amax) - 8``, would clamp every element above 448 2^e: 11 % of
the elements of U[-1, 1) data.)

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
    amax = xb.abs().amax(dim=2)
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.875, ex - 9, ex - 8).clamp(-127, 127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    # the clamp stays: torch's own e4m3 cast turns values above 464 into NaN
    y = ldexp_exact(xb, (-e).unsqueeze(2)).clamp(-E4M3_MAX, E4M3_MAX)
    return y.to(torch.float8_e4m3fn).reshape(R, K), (e + 127).to(torch.uint8)


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
    return ldexp_exact(q.to(torch.float32).reshape(R, K // BLOCK, BLOCK),
                       e.unsqueeze(2)).reshape(R, K)


def quantize_mx(x, *, stream=None):
    """The HIP quantiser: ``x [R, K]`` bf16 / f16 / f32 on a ROCm device -> ``(q, s)`` as
    :func:`quantize_mx_reference` computes them, on ``stream`` (default: the current one). Every
    shape / dtype / stride / alignment check happens here, before the launch."""
    import torch

    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import dtype_code

    if not isinstance(x, torch.Tensor):
        raise TypeError("quantize_mx expects a tensor")
    if x.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise TypeError(f"quantize_mx takes {IN_DTYPES}, not {x.dtype}")
    if x.device.type != "cuda":
        raise ValueError("quantize_mx needs a ROCm device tensor (quantize_mx_reference runs "
                         "anywhere)")
    _check_2d(x)
    R, K = x.shape
    if R >= 2 ** 31 or K >= 2 ** 31:
        raise ValueError("dimensions must fit in 32 bits")
    if x.stride(1) != 1 or (R > 1 and x.stride(0) < K):
        raise ValueError("quantize_mx needs row-major input with unit inner stride")
    if x.data_ptr() % 16 or (x.stride(0) * x.element_size()) % 16:
        raise ValueError("quantize_mx needs 16-byte-aligned rows")
    C = load()
    q = torch.empty((R, K), dtype=torch.float8_e4m3fn, device=x.device)
    s = torch.empty((R, K // BLOCK), dtype=torch.uint8, device=x.device)
    if R == 0:
        return q, s
    st = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
    with torch.cuda.device(x.device):
        C.mx_quantize(x.data_ptr(), q.data_ptr(), s.data_ptr(), max(x.stride(0), K), K,
                      K // BLOCK, R, K, dtype_code(x.dtype), st)
    if stream is not None:  # the outputs stay allocated until that stream reaches them
        q.record_stream(torch.cuda.ExternalStream(st))
        s.record_stream(torch.cuda.ExternalStream(st))
    return q, s


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
    amax = xb.abs().amax(dim=2)
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.75, ex - 3, ex - 2).clamp(-127, 127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    y = ldexp_exact(xb, (-e).unsqueeze(2))
    code = _e2m1_code(y.abs().clamp(max=E2M1_MAX))
    sign = (xb.view(torch.int32) >> 31) & 1  # the input's sign bit: -0 stays negative
    return pack_e2m1(((sign << 3) | code).reshape(R, K)), (e + 127).to(torch.uint8)


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
    return ldexp_exact(unpack_e2m1(q).reshape(R, K // BLOCK, BLOCK), e.unsqueeze(2)).reshape(R, K)


def quantize_mxfp4(x, *, stream=None):
    """The HIP quantiser: ``x [R, K]`` bf16 / f16 / f32 on a ROCm device -> ``(q, s)`` as
    :func:`quantize_mxfp4_reference` computes them, on ``stream`` (default: the current one).
    Every shape / dtype / stride / alignment check happens here, before the launch."""
    import torch

    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import dtype_code

    if not isinstance(x, torch.Tensor):
        raise TypeError("quantize_mxfp4 expects a tensor")
    if x.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise TypeError(f"quantize_mxfp4 takes {IN_DTYPES}, not {x.dtype}")
    if x.device.type != "cuda":
        raise ValueError("quantize_mxfp4 needs a ROCm device tensor (quantize_mxfp4_reference "
                         "runs anywhere)")
    _check_2d_fp4(x)
    R, K = x.shape
    if R >= 2 ** 31 or K >= 2 ** 31:
        raise ValueError("dimensions must fit in 32 bits")
    if x.stride(1) != 1 or (R > 1 and x.stride(0) < K):
        raise ValueError("quantize_mxfp4 needs row-major input with unit inner stride")
    if x.data_ptr() % 16 or (x.stride(0) * x.element_size()) % 16:
        raise ValueError("quantize_mxfp4 needs 16-byte-aligned rows")
    C = load()
    q = torch.empty((R, K // 2), dtype=torch.uint8, device=x.device)
    s = torch.empty((R, K // BLOCK), dtype=torch.uint8, device=x.device)
    if R > 0:
        st = stream if stream is not None else torch.cuda.current_stream(x.device).cuda_stream
        with torch.cuda.device(x.device):
            C.mxfp4_quantize(x.data_ptr(), q.data_ptr(), s.data_ptr(), max(x.stride(0), K),
                             K // 2, K // BLOCK, R, K, dtype_code(x.dtype), st)
        if stream is not None:  # the outputs stay allocated until that stream reaches them
            q.record_stream(torch.cuda.ExternalStream(st))
            s.record_stream(torch.cuda.ExternalStream(st))
    return q.view(torch.float4_e2m1fn_x2), s
