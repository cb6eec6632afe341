"""The references of the exact-arithmetic GPU tests (``tests/_exact.py``) hold the conditions
those tests rely on. Everything here runs on the CPU."""

import torch

from _exact import (FP8, POISON, SENTINEL, dequant64, exact, exact64, exact_scaled,
                    extreme_scales, ints, padded, pow2_f64, sentinel_out, untouched)

import pytest


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def test_ints_are_exact_in_every_dtype():
    x = ints((64, 64), torch.float64, _gen(1))
    assert set(x.unique().tolist()) == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0}
    for dt in (torch.bfloat16, torch.float16, torch.float32, FP8):
        assert torch.equal(x.to(torch.float32).to(dt).to(torch.float64), x)


def test_pow2_f64_is_the_power_of_two():
    e = torch.arange(-1022, 1024)
    p = pow2_f64(e)
    assert torch.equal(p, torch.tensor([2.0 ** int(k) for k in e], dtype=torch.float64))


def test_exact_scaled_equals_the_integer_model():
    """The extreme-scale case of the GPU test: bytes 0..254, net exponents -4..4, and the fp64
    product equal to per-block int64 dot products shifted by e_a + e_w; an exact f32."""
    M, N, K = 300, 202, 512
    g = _gen(2)
    a8, w8 = ints((M, K), FP8, g), ints((N, K), FP8, g)
    s_a, s_w, e_a, e_w = extreme_scales(M, N, K, g)
    for s in (s_a, s_w):
        assert int(s.min()) == 0 and int(s.max()) == 254
    net = e_a.unsqueeze(1) + e_w.unsqueeze(0)                       # [M, N, nb]
    assert int(net.min()) >= -4 and int(net.max()) <= 4
    ai = a8.float().to(torch.int64).reshape(M, K // 32, 32)
    wi = w8.float().to(torch.int64).reshape(N, K // 32, 32)
    dots = torch.einsum("mbk,nbk->mnb", ai, wi)                     # int64, exact
    model16 = (dots << (net + 4)).sum(dim=2)                        # 16 x the product
    got = exact_scaled(a8, w8, s_a, s_w)
    assert torch.equal(got * 16.0, model16.double())
    assert torch.equal(got.float().double(), got)                   # an exact f32
    assert float(got.abs().max()) < 2.0 ** 24 / 16


def test_dequant64_against_dequantize_mx():
    """Equal wherever the fp32 specification is finite; it overflows exactly at s = 254 with
    |q| >= 2, where the fp64 value (and a product with a small partner scale) is finite."""
    from ddlb_amd.ops.mx import dequantize_mx

    g = _gen(3)
    q = ints((64, 256), FP8, g)
    q[0, :8] = torch.tensor([1.0, 1.5, 1.75, 2.0, -2.0, 448.0, -1.0, 0.0]).to(FP8)
    s = torch.randint(0, 255, (64, 8), generator=g).to(torch.uint8)
    s[0, 0], s[1, 0], s[2, 0] = 254, 0, 254
    d32, d64 = dequantize_mx(q, s), dequant64(q, s)
    finite = torch.isfinite(d32)
    assert torch.equal(d32[finite].double(), d64[finite])
    over = (s.repeat_interleave(32, dim=1) == 254) & (q.float().abs() >= 2)
    assert torch.equal(~finite, over) and int(over.sum()) > 3
    assert bool(torch.isfinite(d64).all())


def _decode_e4m3(code):
    s, e, m = code >> 7, (code >> 3) & 0xF, code & 7
    if e == 0xF and m == 7:
        return float("nan")
    v = (m / 8.0) * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
    return -v if s else v


def test_every_e4m3_code():
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    vals = codes.view(FP8).float()
    assert int(torch.isfinite(vals).sum()) == 254
    assert bool(torch.isnan(vals[0x7F])) and bool(torch.isnan(vals[0xFF]))
    assert float(vals[0x80]) == 0.0 and bool(torch.signbit(vals[0x80]))
    assert float(vals[0x00]) == 0.0 and not bool(torch.signbit(vals[0x00]))
    assert float(vals[0x01]) == 2.0 ** -9 and float(vals[0x7E]) == 448.0
    model = torch.tensor([_decode_e4m3(c) for c in range(256)], dtype=torch.float32)
    keep = torch.isfinite(vals)
    assert torch.equal(vals[keep].view(torch.int32), model[keep].view(torch.int32))


def test_exact_rounds_to_the_output_dtype():
    """bf16 holds integers up to 256: at K = 1024 (sums of some hundreds) the rounding to the
    output dtype is really exercised; at the sweep's K of one to four K-tiles it rarely is, and
    what the sweep pins down there is the placement of every element."""
    g = _gen(4)
    a, w = ints((64, 1024), torch.bfloat16, g), ints((48, 1024), torch.bfloat16, g)
    f32 = exact(a, w, torch.float32)
    assert torch.equal(f32.double(), exact64(a, w))                 # nothing lost in f32
    bf = exact(a, w, torch.bfloat16)
    assert bf.dtype == torch.bfloat16
    assert int((bf.float() != f32).sum()) > 0                       # the rounding is exercised
    assert bool(((bf.float() - f32).abs() <= f32.abs() * 2.0 ** -8).all())
    assert torch.equal(exact(a, w, torch.float16).float(), f32)     # |sum| <= 2048: exact in f16


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32, FP8,
                                   torch.float64])
def test_padded_views(dtype):
    g = _gen(5)
    for cols in (128, 100, 256):
        x = ints((7, cols), dtype, g)
        v = padded(x)
        assert tuple(v.shape) == (7, cols) and v.stride(1) == 1 and v.stride(0) > cols
        assert v.data_ptr() % 16 == 0 and (v.stride(0) * v.element_size()) % 16 == 0
        assert torch.equal(v.float(), x.float())
        whole = torch.as_strided(v, (10, v.stride(0)), (v.stride(0), 1)).to(torch.float64)
        assert bool((whole[:7, cols:] == POISON).all()) and bool((whole[7:] == POISON).all())


def test_untouched_sees_a_planted_write():
    for dtype in (torch.bfloat16, torch.float32):
        buf, view = sentinel_out(5, 6, dtype, device="cpu")
        assert tuple(buf.shape) == (8, 10) and tuple(view.shape) == (5, 6)
        assert bool((buf.float() == SENTINEL).all())
        view.fill_(1.0)
        untouched(buf, 5, 6)
        for r, c in ((0, 6), (4, 9), (5, 0), (7, 9)):
            buf2 = buf.clone()
            buf2[r, c] = 1.0
            with pytest.raises(AssertionError):
                untouched(buf2, 5, 6)
    buf, _ = sentinel_out(8, 4, torch.float32, extra_rows=0, device="cpu")
    rows = torch.tensor([0, 1, 4, 5])
    buf[rows, :4] = 2.0
    untouched(buf, 8, 4, rows=rows)
    buf[2, 1] = 2.0
    with pytest.raises(AssertionError):
        untouched(buf, 8, 4, rows=rows)
