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
"""

from __future__ import annotations

BLOCK = 32
E4M3_MAX = 448.0
IN_DTYPES = ("bfloat16", "float16", "float32")


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
