"""Shared helpers of the exact-arithmetic tests (a plain module: no fixtures, no test).

The operands are integers in -3..3, exact in bf16, f16, f32, f64 and e4m3. With K <= 1024 every
product and every partial sum of ``a @ w.T`` is an integer below 2^24, so an f32 accumulator holds
it exactly whatever the order of the additions: the specification of a GEMM on such operands is
"the exact product, rounded once to the output dtype", and it is compared with ``torch.equal``.

Operands come as views of larger buffers whose padding holds ``POISON`` (a read outside the view
changes the result) and outputs as views of buffers filled with ``SENTINEL`` (a write outside the
view is seen by :func:`untouched`)."""

import torch

POISON = 5.0
SENTINEL = -7.0
FP8 = torch.float8_e4m3fn
BLOCK = 32


def _filled(shape, value, dtype, device):
    # (torch.full has no e4m3 fill; every value used here is exact in every dtype)
    return torch.full(shape, float(value), dtype=torch.float32, device=device).to(dtype)


def ints(shape, dtype, gen):
    """Integers in -3..3 as ``dtype``, drawn from ``gen`` on its device."""
    x = torch.randint(-3, 4, shape, generator=gen, device=gen.device)
    return x.to(torch.float32).to(dtype)


def padded(x, pad_elems=None, extra_rows=3, poison=POISON, align=16):
    """``x [R, C]`` as the view ``[:R, :C]`` of a ``[R + extra_rows, C + pad_elems]`` buffer
    whose other elements hold ``poison``. The rows stay ``align``-byte aligned: ``pad_elems``
    must keep them so (default: the smallest padding of at least 4 elements that does)."""
    R, C = x.shape
    esz = x.element_size()
    if pad_elems is None:
        pad_elems = next(p for p in range(4, 4 + align + 1) if ((C + p) * esz) % align == 0)
    assert pad_elems > 0 and ((C + pad_elems) * esz) % align == 0, "rows must stay aligned"
    buf = _filled((R + extra_rows, C + pad_elems), poison, x.dtype, x.device)
    buf[:R, :C] = x
    view = buf[:R, :C]
    assert view.data_ptr() % align == 0 and (view.stride(0) * esz) % align == 0
    return view


def sentinel_out(M, N, dtype, pad_cols=4, extra_rows=3, device="cuda"):
    """``(buf, view)``: ``buf [M + extra_rows, N + pad_cols]`` filled with ``SENTINEL`` and
    ``view = buf[:M, :N]``."""
    buf = _filled((M + extra_rows, N + pad_cols), SENTINEL, dtype, device)
    return buf, buf[:M, :N]


def untouched(buf, M, N, rows=None):
    """Assert that every element of ``buf`` outside ``[:M, :N]`` (outside rows ``rows`` and
    columns ``:N`` when the physical rows written are given) still holds ``SENTINEL``."""
    written = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    if rows is None:
        written[:M, :N] = True
    else:
        written[rows, :N] = True
    outside = buf.to(torch.float32)[~written]
    bad = int((outside != SENTINEL).sum())
    assert bad == 0, f"{bad} elements outside the [{M}, {N}] view were written"


def pow2_f64(e):
    """``2^e`` as float64 for an integer tensor ``e`` in [-1022, 1023], built from its bit
    pattern (the fp64 twin of ``ddlb_amd.ops.mx.ldexp_exact``)."""
    return ((e.to(torch.int64) + 1023) << 52).view(torch.float64)


def exact64(a, w):
    """``a @ w.T`` in fp64 (exact for the operands above)."""
    return a.to(torch.float32).double() @ w.to(torch.float32).double().t()


def exact(a, w, out_dtype):
    """The exact product rounded once to f32 (no rounding at all for the operands above with
    K <= 1024) and then to ``out_dtype``."""
    return exact64(a, w).to(torch.float32).to(out_dtype)


def dequant64(q, s):
    """e4m3 ``q [R, K]`` with E8M0 bytes ``s [R, K / 32]`` as float64, never through fp32
    (``3 * 2^127`` is no fp32 number; every such value is an exact fp64 one)."""
    R, K = q.shape
    assert tuple(s.shape) == (R, K // BLOCK)
    v = q.to(torch.float32).double().reshape(R, K // BLOCK, BLOCK)
    return (v * pow2_f64(s.to(torch.int64) - 127).unsqueeze(2)).reshape(R, K)


def exact_scaled(a8, w8, s_a, s_w):
    """The product of the dequantised MX operands, in fp64."""
    return dequant64(a8, s_a) @ dequant64(w8, s_w).t()


def extreme_scales(M, N, K, gen):
    """Scale bytes over the whole E8M0 range the quantiser can emit (0..254) whose products stay
    small: ``s_a = 127 + D[b] + u[r, b]`` and ``s_w = 127 - D[b] + v[n, b]`` with ``D`` spread over
    -125..125 along the K blocks (both ends present) and ``u``, ``v`` in -2..2, so every block's
    net exponent ``u + v`` lies in -4..4 while the bytes themselves reach 0 and 254. Returns
    ``(s_a, s_w, e_a, e_w)``: the uint8 bytes and the int64 exponents ``s - 127``."""
    nb = K // BLOCK
    dev = gen.device
    D = torch.round(torch.linspace(-125, 125, nb, device=dev, dtype=torch.float64)).to(torch.int64)
    u = torch.randint(-2, 3, (M, nb), generator=gen, device=dev)
    v = torch.randint(-2, 3, (N, nb), generator=gen, device=dev)
    e_a = (D.unsqueeze(0) + u).clamp(-127, 127)
    e_w = (-D.unsqueeze(0) + v).clamp(-127, 127)
    return (e_a + 127).to(torch.uint8), (e_w + 127).to(torch.uint8), e_a, e_w
