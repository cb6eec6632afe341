"""MX block scaling at its limits: scale bytes over the whole E8M0 range the quantiser can emit
(0..254), the f16 output of the block-scaled GEMM, operands whose blocks span 2^-100..2^100 end
to end, and the quantiser's output compared byte for byte (sign of zero included).

The references dequantise in fp64 (``tests/_exact.py``): the fp32 specification
``dequantize_mx`` overflows at s = 254 with |q| >= 2, where the product with a small partner
scale is an ordinary number."""

import pytest
import torch

from _exact import FP8, dequant64, exact_scaled, extreme_scales, ints, padded

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _tiles():
    from ddlb_amd.ops.gemm import SCALED_TILES

    return ("auto",) + tuple(SCALED_TILES)


def _scaled(a8, w8, s_a, s_w, out_dtype=torch.float32, **kw):
    from ddlb_amd.ops.gemm import gemm

    out = gemm(a8, w8, out_dtype=out_dtype, a_scale=s_a, w_scale=s_w, **kw)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------ the whole scale-byte range
@pytest.fixture(scope="module")
def extreme():
    M, N, K = 300, 202, 512
    g = _gen(21)
    a8, w8 = ints((M, K), FP8, g), ints((N, K), FP8, g)
    s_a, s_w, _, _ = extreme_scales(M, N, K, g)
    for s in (s_a, s_w):
        assert int(s.min()) == 0 and int(s.max()) == 254
    ref = exact_scaled(a8, w8, s_a, s_w)
    assert torch.equal(ref.float().double(), ref)      # an exact f32
    # padded operand rows and scale rows (row stride 20 bytes: a multiple of 4)
    return padded(a8), padded(w8), padded(s_a, align=4), padded(s_w, align=4), ref.float()


@pytest.mark.parametrize("tile", _tiles())
def test_full_scale_byte_range_exact(extreme, tile):
    """s_a = 127 + D[b] + u, s_w = 127 - D[b] + v with D over -125..125 along the 16 K blocks:
    both byte ranges are 0..254 while every block's net exponent stays in -4..4, so the result
    is an exact f32 that only a scaled MFMA exact over the whole byte range reproduces."""
    a8, w8, s_a, s_w, ref = extreme
    got = _scaled(a8, w8, s_a, s_w, tile=tile)
    bad = (got != ref)
    if bool(bad.any()):  # name the K blocks' bytes a failure involves
        r, n = [int(v) for v in bad.nonzero()[0]]
        print(f"tile {tile}: {int(bad.sum())} wrong; first ({r}, {n}) got {float(got[r, n])} "
              f"want {float(ref[r, n])}; s_a row {s_a[r].tolist()} s_w row {s_w[n].tolist()}")
    assert not bool(bad.any()), tile


# ------------------------------------------------------------------ f16 output
def test_single_block_rows_f16_output():
    """test_mx_scaled_gpu's single-block-row case (every (row, block) its own scale) into f16,
    the one output dtype of the block-scaled kernel that file does not run."""
    from test_mx_scaled_gpu import _single_block_case

    a8, w8, s_a, s_w = _single_block_case(300, 202, 256, 31)
    want = exact_scaled(a8, w8, s_a, s_w)
    want = want.float().to(torch.float16)          # (2^-12..2^12 scale products: some overflow
    finite = torch.isfinite(want)                  # f16, and round to inf on both sides)
    assert int((finite & (want != 0)).sum()) > want.numel() // 2 and not bool(finite.all())
    for tile in _tiles():
        out = torch.full((300, 204), -7.0, device=DEV, dtype=torch.float16)  # 8-byte rows
        got = _scaled(a8, w8, s_a, s_w, out=out[:, :202], tile=tile)
        assert got.dtype == torch.float16 and torch.equal(got, want), tile
        assert bool((out[:, 202:] == -7.0).all())


# ------------------------------------------------------------------ wide exponents end to end
def _very_wide(rows, k, g, sign):
    """randn * 2^(sign * E[b]) in f32, E spread over -100..100 along the row's blocks."""
    from ddlb_amd.ops.mx import ldexp_exact

    nb = k // 32
    x = torch.randn(rows, nb, 32, generator=g, device=DEV)
    E = torch.round(torch.linspace(-100, 100, nb, device=DEV)).to(torch.int32) * sign
    return ldexp_exact(x, E.view(1, nb, 1).expand(rows, nb, 32)).reshape(rows, k)


@pytest.fixture(scope="module")
def wide():
    g = _gen(22)
    return _very_wide(512, 512, g, 1), _very_wide(256, 512, g, -1)


def test_wide_exponent_quantiser_bit_exact(wide):
    from ddlb_amd.ops.mx import quantize_mx, quantize_mx_reference

    lo, hi = 255, 0
    for x in wide:
        q, s = quantize_mx(x)
        torch.cuda.synchronize()
        q_ref, s_ref = quantize_mx_reference(x)
        assert torch.equal(s, s_ref)
        assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8))
        lo, hi = min(lo, int(s.min())), max(hi, int(s.max()))
    print(f"wide exponents: scale bytes {lo}..{hi}")
    assert lo < 30 and hi > 215


def test_wide_exponent_end_to_end(wide):
    """quantize_mx -> block-scaled GEMM -> f32 against the fp64 product of the REFERENCE
    quantiser's output, with test_mx_scaled_gpu's end-to-end bound."""
    from ddlb_amd.ops.mx import quantize_mx, quantize_mx_reference

    a, w = wide
    (aq, a_s), (wq, w_s) = quantize_mx(a), quantize_mx(w)
    out = _scaled(aq, wq, a_s, w_s)
    a_dq, w_dq = dequant64(*quantize_mx_reference(a)), dequant64(*quantize_mx_reference(w))
    ref, mag = a_dq @ w_dq.t(), a_dq.abs() @ w_dq.abs().t()
    assert bool(torch.isfinite(ref.float()).all()) and bool(torch.isfinite(out).all())
    err = (out.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -10 * mag
    print(f"wide end to end: max err/bound {float((err / bound.clamp(min=1e-300)).max()):.4g}")
    assert bool((err <= bound).all())


# ------------------------------------------------------------------ the quantiser, byte for byte
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_quantizer_bytes(dtype):
    """test_quantizer_matches_reference's data compared as bytes: ``q.float()`` cannot tell -0
    from +0. Negative zeros and negative values that round to zero are in the data."""
    from test_mx_scaled_gpu import _wide
    from ddlb_amd.ops.mx import quantize_mx, quantize_mx_reference

    x = _wide(300, 256, _gen(11), dtype)
    x[0] = 0
    x[1, 32:64] = 0
    x[2] = 0
    x[2, 77] = -1.5
    for i, j in enumerate((-9, -1, 0, 2, 6)):            # the 448 boundary, as in that test
        x[3 + i, 0:32] = 3.0 * 2.0 ** j
        x[3 + i, 7] = 448.0 * 2.0 ** j
        x[3 + i, 32:64] = -5.0 * 2.0 ** j
        x[3 + i, 40] = 480.0 * 2.0 ** j
    x[8, 0:32] = 2.0 ** (10 if dtype != torch.float16 else 3)
    x[9, 0:32] = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -130
    x[10, 0:32] = -0.0                                   # an all -0 block
    x[11, 0:16] = -0.0                                   # -0 beside ordinary values
    x[12, 0:32] = 1.0
    x[12, 3] = -(2.0 ** -19)                             # e = -8: -2^-11 rounds to zero
    x[12, 4] = -(2.0 ** -18)                             # -2^-10: the tie below 2^-9, to even
    q, s = quantize_mx(x)
    torch.cuda.synchronize()
    q_ref, s_ref = quantize_mx_reference(x)
    assert torch.equal(s, s_ref)
    qb, rb = q.view(torch.uint8), q_ref.view(torch.uint8)
    diff = (qb != rb).nonzero()
    first = [(int(r), int(c), int(qb[r, c]), int(rb[r, c])) for r, c in diff[:6]]
    assert diff.numel() == 0, (f"{diff.shape[0]} bytes differ; first (row, col, kernel, "
                               f"reference): {first}")
    assert int((rb == 0x80).sum()) >= 48                 # -0 is in the reference's output
