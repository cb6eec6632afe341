"""The transposed MX quantisation and the MX linear backward chain, host side (no GPU): the torch
specification, every refusal of ``quantize_mx_t`` / ``quantize_mx_2way`` on CPU tensors (raised
before the extension is loaded) and the chain's transposes on exact integer data."""

import pytest
import torch

from ddlb_amd.models.mx_linear import MxLinear, check_shapes, mx_linear_reference
from ddlb_amd.ops import mx

FP8 = torch.float8_e4m3fn
FP4 = torch.float4_e2m1fn_x2
FMTS = ("mx", "mxfp4")


def _wide(rows, k, seed):
    """randn * 2^U{-20..20}, one exponent per 32-element block."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, k // 32, 32, generator=g)
    ex = torch.randint(-20, 21, (rows, k // 32, 1), generator=g)
    return torch.ldexp(x, ex).reshape(rows, k)


def _deq(fmt, q, s):
    return mx.dequantize_mxfp4(q, s) if fmt == "mxfp4" else mx.dequantize_mx(q, s)


def _qref(fmt, x):
    return mx.quantize_mxfp4_reference(x) if fmt == "mxfp4" else mx.quantize_mx_reference(x)


@pytest.fixture
def no_extension(monkeypatch):
    """Any attempt to load the native extension fails the test."""
    import ddlb_amd.ops

    def boom():
        raise AssertionError("the extension was loaded before the refusal")

    monkeypatch.setattr(ddlb_amd.ops, "load", boom)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_reference_shapes_and_dtypes(fmt, dtype):
    R, C = 512, 72
    x = _wide(R, 96, 1)[:, :C].clamp(-60000, 60000).to(dtype)
    qt, st = mx.quantize_mx_t_reference(x, fmt)
    assert st.dtype == torch.uint8 and tuple(st.shape) == (C, R // 32)
    if fmt == "mx":
        assert qt.dtype == FP8 and tuple(qt.shape) == (C, R)
    else:
        assert qt.dtype == FP4 and tuple(qt.shape) == (C, R // 2)
    want_q, want_s = _qref(fmt, x.t().contiguous())
    assert torch.equal(qt.view(torch.uint8), want_q.view(torch.uint8))
    assert torch.equal(st, want_s)
    with pytest.raises(ValueError):
        mx.quantize_mx_t_reference(x, "fp8")
    with pytest.raises(ValueError):
        mx.quantize_mx_t_reference(x[0], fmt)
    with pytest.raises(ValueError):  # R is the block axis
        mx.quantize_mx_t_reference(x[:96], fmt)


@pytest.mark.parametrize("fmt", FMTS)
def test_transposed_is_another_quantisation(fmt):
    """Blocks down the columns are not the row blocks transposed: on wide data most dequantised
    elements differ between the two, and so do the scale arrays."""
    x = _wide(256, 256, 7)
    qt, st = mx.quantize_mx_t_reference(x, fmt)
    q, s = _qref(fmt, x)
    a = _deq(fmt, qt, st)            # [C, R]: x.T quantised along R
    b = _deq(fmt, q, s).t()          # [C, R]: x quantised along C, then transposed
    assert tuple(a.shape) == tuple(b.shape) == (256, 256)
    differ = float((a != b).float().mean())
    assert differ > 0.5, differ
    # each is a quantisation of x.T all the same: within the format's half step of the block max
    step = 2.0 ** -4 if fmt == "mx" else 2.0 ** -2
    xt = x.t()
    amax = xt.reshape(256, 8, 32).abs().amax(dim=2, keepdim=True)
    assert bool(((a - xt).reshape(256, 8, 32).abs() <= step * amax).all())


def _good(fmt, dtype=torch.bfloat16):
    return torch.zeros(256, 512 if fmt == "mxfp4" else 384, dtype=dtype)


@pytest.mark.parametrize("fmt", FMTS)
def test_refusals_on_cpu_tensors(fmt, no_extension):
    fp4 = fmt == "mxfp4"
    mod = 256 if fp4 else 128
    x = _good(fmt)
    R, C = x.shape
    for fn in (mx.quantize_mx_t, mx.quantize_mx_2way):
        with pytest.raises(ValueError, match="ROCm device"):  # all else is right: the device
            fn(x, fmt=fmt)
        with pytest.raises(ValueError, match="fmt"):
            fn(x, fmt="fp8")
        with pytest.raises(TypeError):
            fn(x.double(), fmt=fmt)
        with pytest.raises(TypeError):
            fn([[1.0]], fmt=fmt)
        with pytest.raises(ValueError, match="2-D"):
            fn(x[0], fmt=fmt)
        with pytest.raises(ValueError, match=f"R % {mod}"):
            fn(x[:mod - 32], fmt=fmt)
        with pytest.raises(ValueError, match="16-byte vectors"):
            fn(x[:, :C - 4], fmt=fmt)
        with pytest.raises(ValueError, match="unit inner stride"):
            fn(torch.zeros(R, 2 * C, dtype=torch.bfloat16)[:, ::2], fmt=fmt)
        with pytest.raises(ValueError, match="unit inner stride"):
            fn(torch.zeros(C, R, dtype=torch.bfloat16).t(), fmt=fmt)
        with pytest.raises(ValueError, match="16-byte-aligned"):  # rows start 2 bytes off
            fn(torch.zeros(R, C + 8, dtype=torch.bfloat16)[:, 1:C + 1], fmt=fmt)
        with pytest.raises(ValueError, match="16-byte-aligned"):  # a row pitch of 2 mod 16 bytes
            fn(torch.zeros(R, C + 1, dtype=torch.bfloat16)[:, :C], fmt=fmt)
        with pytest.raises(ValueError, match="2 GiB"):
            fn(torch.zeros(mod, 2 ** 30, dtype=torch.bfloat16, device="meta"), fmt=fmt)
    # C: whole vectors are enough one way, the two-way launch wants whole K-tiles of columns
    with pytest.raises(ValueError, match="ROCm device"):
        mx.quantize_mx_t(x[:, :72], fmt=fmt)
    with pytest.raises(ValueError, match=f"C % {mod}"):
        mx.quantize_mx_2way(x[:, :72], fmt=fmt)
    with pytest.raises(ValueError, match="ROCm device"):  # ldx > C is fine
        mx.quantize_mx_t(torch.zeros(R, C + 64, dtype=torch.float32)[:, 8:C], fmt=fmt)
    with pytest.raises(TypeError):
        mx.quantize_mx_2way(x, fmt=fmt, out=(None, None))


@pytest.mark.parametrize("fmt", FMTS)
def test_out_refusals_on_cpu_tensors(fmt, no_extension):
    fp4 = fmt == "mxfp4"
    x = _good(fmt)
    R, C = x.shape
    ncol, nb, sal = (R // 2 if fp4 else R), R // 32, (8 if fp4 else 4)
    qdt = FP4 if fp4 else FP8

    def q(rows=C, cols=ncol, pitch=None):
        return torch.zeros(rows, pitch or cols, dtype=torch.uint8)[:, :cols].view(qdt)

    def s(rows=C, cols=nb, pitch=None):
        return torch.zeros(rows, pitch or cols, dtype=torch.uint8)[:, :cols]

    def call(qt, st):
        return mx.quantize_mx_t(x, fmt=fmt, out=(qt, st))

    with pytest.raises(ValueError, match="ROCm device"):  # a good pair, dense or pitched
        call(q(), s())
    with pytest.raises(ValueError, match="ROCm device"):
        call(q(C + 3, pitch=ncol + 32)[:C], s(C + 3, pitch=nb + 2 * sal)[:C])
    with pytest.raises(TypeError):
        mx.quantize_mx_t(x, fmt=fmt, out=q())
    with pytest.raises(TypeError):
        mx.quantize_mx_t(x, fmt=fmt, out=(q(), s(), s()))
    with pytest.raises(TypeError):
        call(q().view(torch.uint8), s())
    with pytest.raises(TypeError):
        call(q().view(torch.uint8).view(FP8 if fp4 else FP4), s())
    with pytest.raises(TypeError):
        call(q(), s().view(torch.int8))
    with pytest.raises(ValueError, match=r"out\[0\] must have shape"):
        call(q(C - 1), s())
    with pytest.raises(ValueError, match=r"out\[0\] must have shape"):
        call(q(cols=ncol + 16), s())
    with pytest.raises(ValueError, match=r"out\[1\] must have shape"):
        call(q(), s(C + 1))
    with pytest.raises(ValueError, match=r"out\[1\] must have shape"):
        call(q(), s(cols=nb + sal))
    with pytest.raises(ValueError, match="multiple of 16"):
        call(q(pitch=ncol + 8), s())
    with pytest.raises(ValueError, match="unit inner stride"):
        call(torch.zeros(C, 2 * ncol, dtype=torch.uint8)[:, ::2].view(qdt), s())
    buf = torch.zeros(C * ncol + 64, dtype=torch.uint8)
    off = (-buf.data_ptr()) % 16 + 8
    with pytest.raises(ValueError, match="16-byte-aligned address"):
        call(buf[off:off + C * ncol].view(C, ncol).view(qdt), s())
    with pytest.raises(ValueError, match=f"multiple of {sal}"):
        call(q(), s(pitch=nb + sal // 2))
    sbuf = torch.zeros(C * nb + 64, dtype=torch.uint8)
    soff = (-sbuf.data_ptr()) % sal + sal // 2
    with pytest.raises(ValueError, match=f"{sal}-byte-aligned address"):
        call(q(), sbuf[soff:soff + C * nb].view(C, nb))
    with pytest.raises(ValueError, match="is on"):
        call(torch.zeros(C, ncol, dtype=torch.uint8, device="meta").view(qdt), s())


def _ints(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, shape, generator=g).float()


@pytest.mark.parametrize("fmt", FMTS)
def test_reference_chain_is_exact_on_integers(fmt):
    """Integers in -3..3 quantise exactly along either axis, so the reference chain must return
    the exact products: a wrong axis or a missing transpose anywhere in it would not."""
    M, N, K = (256, 512, 256) if fmt == "mxfp4" else (256, 384, 128)
    x, w, dy = _ints((M, K), 1), _ints((N, K), 2), _ints((M, N), 3)
    for t in (x, w, dy):  # 0 differences, along the rows and down the columns
        assert torch.equal(_deq(fmt, *_qref(fmt, t)), t)
        assert torch.equal(_deq(fmt, *mx.quantize_mx_t_reference(t, fmt)), t.t())
    y, dx, dw = mx_linear_reference(x.bfloat16(), w.bfloat16(), dy.bfloat16(), fmt)
    assert y.dtype == dx.dtype == dw.dtype == torch.float32
    assert torch.equal(y.double(), x.double() @ w.double().t())
    assert torch.equal(dx.double(), dy.double() @ w.double())
    assert torch.equal(dw.double(), dy.double().t() @ x.double())


def test_linear_shape_refusals():
    x, w = torch.zeros(256, 128, dtype=torch.bfloat16), torch.zeros(384, 128, dtype=torch.bfloat16)
    assert check_shapes(x, w, "mx") == (256, 384, 128)
    with pytest.raises(ValueError, match="256, 384, 128"):  # the shape is named
        check_shapes(x, w, "mxfp4")
    with pytest.raises(ValueError, match="200, 384, 128"):
        check_shapes(x[:200], w, "mx")
    with pytest.raises(ValueError, match="K mismatch"):
        check_shapes(x, torch.zeros(384, 256, dtype=torch.bfloat16), "mx")
    with pytest.raises(TypeError):
        check_shapes(x.float(), w, "mx")
    with pytest.raises(ValueError, match="fmt"):
        check_shapes(x, w, "fp8")
    with pytest.raises(ValueError, match="dy must have shape"):
        mx_linear_reference(x, w, torch.zeros(256, 128), "mx")
    with pytest.raises(ValueError, match="100"):
        MxLinear(100, 128)
    with pytest.raises(TypeError):
        MxLinear(128, 128, dtype=torch.float32)
    lin = MxLinear(128, 256, fmt="mx")
    assert tuple(lin.weight.shape) == (256, 128) and lin.weight.dtype == torch.bfloat16
    assert lin.n_quant == 0
    with pytest.raises(ValueError, match="200"):  # refused before anything is quantised
        lin(torch.zeros(200, 128, dtype=torch.bfloat16))
    assert lin.n_quant == 0
