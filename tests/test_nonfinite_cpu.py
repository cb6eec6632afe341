"""Non-finite input in the MX specification (``ddlb_amd.ops.mx``, CPU tensors): the amended
``quantize_mx_reference`` against per-block Python loops, the references built on it, and byte
identity with the earlier formula on finite data. The activation specification on NaN and Inf."""

import math

import pytest
import torch

from ddlb_amd.ops.mx import (dequantize_mx, ldexp_exact, quantize_mx_gather_reference,
                             quantize_mx_reference, quantize_mx_t_grouped_reference,
                             quantize_mx_t_reference, quantize_mxfp4_reference)

NAN, INF = float("nan"), float("inf")
FP8, U8 = torch.float8_e4m3fn, torch.uint8
K = 256


def _wide(rows, k, seed):
    """randn * 2^U{-20..20}, one exponent per 32-element block (``tests/test_mx_cpu.py``)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, k // 32, 32, generator=g)
    ex = torch.randint(-20, 21, (rows, k // 32, 1), generator=g)
    return torch.ldexp(x, ex).reshape(rows, k)


def _neg_nan(dtype=torch.float32):
    """-NaN by its bits (a conversion may make the canonical, positive NaN of it)."""
    word, bits = {torch.bfloat16: (torch.int16, -64), torch.float16: (torch.int16, -512),
                  torch.float32: (torch.int32, -(1 << 22))}[dtype]
    v = torch.tensor([bits], dtype=word).view(dtype)[0]
    assert math.isnan(float(v))
    return v


def _special(dtype=torch.float32):
    """Blocks holding NaN, -NaN, +-Inf, only non-finite elements, and one non-finite element among
    subnormals, among ordinary blocks."""
    x = _wide(8, K, 5)
    if dtype == torch.float16:
        x = x.clamp(-60000, 60000)
    x = x.to(dtype)
    x[0, 5] = NAN
    x[0, 37] = _neg_nan(dtype)
    x[1, 0:32] = 1.0
    x[1, 6] = 448.0
    x[1, 7] = INF
    x[1, 32:64] = 0
    x[1, 40] = -INF
    x[2, 0:32] = torch.tensor([NAN, INF, -INF, float(_neg_nan())] * 8).to(dtype)
    x[2, 3] = _neg_nan(dtype)
    tiny = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -130
    x[3, 0:32] = tiny
    x[3, 9] = -INF
    x[4, 0] = INF
    x[4, K - 1] = NAN
    return x


def _block_loop(x):
    """The MX-fp8 rule block by block on Python floats: ``(bytes [R, K], scale bytes [R, K/32])``
    as lists. Finite amax; a non-finite element the NaN byte with its sign; the finite ones
    e4m3_rne(clamp(x 2^-e, +-448)), each rounded by torch's cast of that one value."""
    x32 = x.to(torch.float32)
    bits = x32.view(torch.int32)
    R, Kx = x32.shape
    q = [[0] * Kx for _ in range(R)]
    s = [[0] * (Kx // 32) for _ in range(R)]
    for r in range(R):
        for b in range(Kx // 32):
            vals = [float(v) for v in x32[r, 32 * b:32 * b + 32]]
            amax = max([abs(v) for v in vals if math.isfinite(v)], default=0.0)
            if amax == 0.0:
                e = 0
            else:
                m, ex = math.frexp(amax)
                e = min(max(ex - 9 if m <= 0.875 else ex - 8, -127), 127)
            s[r][b] = e + 127
            for i, v in enumerate(vals):
                k = 32 * b + i
                if not math.isfinite(v):
                    q[r][k] = 0x7F | (0x80 if int(bits[r, k]) < 0 else 0)
                else:
                    y = min(max(math.ldexp(v, -e), -448.0), 448.0)
                    q[r][k] = int(torch.tensor(y, dtype=torch.float32).to(FP8).view(U8))
    return q, s


def _old_quantize_mx_reference(x):
    """The formula before non-finite input was specified, kept to show that no byte of finite
    data changed."""
    R, Kx = x.shape
    xb = x.to(torch.float32).reshape(R, Kx // 32, 32)
    amax = xb.abs().amax(dim=2)
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.875, ex - 9, ex - 8).clamp(-127, 127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    y = ldexp_exact(xb, (-e).unsqueeze(2)).clamp(-448.0, 448.0)
    return y.to(FP8).reshape(R, Kx), (e + 127).to(U8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_reference_against_block_loops(dtype):
    x = _special(dtype)
    q, s = quantize_mx_reference(x)
    ql, sl = _block_loop(x)
    assert s.tolist() == sl
    assert q.view(U8).tolist() == ql
    b = q.view(U8)
    assert int(b[0, 5]) == 0x7F and int(b[0, 37]) == 0xFF
    assert int(b[1, 7]) == 0x7F and int(b[1, 6]) == 0x7E and int(s[1, 0]) == 127
    assert int(b[1, 40]) == 0xFF and int(s[1, 1]) == 127          # -Inf alone: s = 127
    assert int(s[2, 0]) == 127 and bool(((b[2, :32] & 0x7F) == 0x7F).all())
    assert int(b[3, 9]) == 0xFF
    # (2^-24, f16's smallest subnormal, is 0.5 x 2^-23 in fp32: e = -23 - 9)
    assert int(s[3, 0]) == (127 - 32 if dtype == torch.float16 else 0)
    assert int(b[4, 0]) == 0x7F and int(b[4, K - 1]) == 0x7F
    # the finite neighbours are what they are without the bad element
    clean = torch.where(torch.isfinite(x), x, torch.zeros_like(x))
    q0, s0 = quantize_mx_reference(clean)
    fin = torch.isfinite(x)
    assert torch.equal(s, s0) and torch.equal(b[fin], q0.view(U8)[fin])
    # and the dequantisation is NaN exactly where the input was not finite
    assert torch.equal(torch.isnan(dequantize_mx(q, s)), ~fin)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_finite_data_keeps_every_byte(dtype):
    for seed in (2, 3, 11):
        x = _wide(64, K, seed)
        if dtype == torch.float16:
            x = x.clamp(-60000, 60000)
        x = x.to(dtype)
        x[1, 64:96] = 0
        x[3] = 0
        x[5, 7] = -0.0
        q, s = quantize_mx_reference(x)
        q0, s0 = _old_quantize_mx_reference(x)
        assert torch.equal(s, s0) and torch.equal(q.view(U8), q0.view(U8))


def test_derived_references_follow():
    """The gather, transposed and grouped references are the row reference on other rows."""
    x = _special().repeat(16, 1)                      # [128, 256]
    x[127, 3] = INF                                   # the last row of a column block
    x[96, 3] = NAN                                    # ... and its first
    qt, st = quantize_mx_t_reference(x)
    q, s = quantize_mx_reference(x.t().contiguous())
    assert torch.equal(qt.view(U8), q.view(U8)) and torch.equal(st, s)
    assert int(qt.view(U8)[3, 127]) == 0x7F and int(qt.view(U8)[3, 96]) == 0x7F
    src = torch.tensor([2, -1, 0, 128, 3])
    qg, sg = quantize_mx_gather_reference(x, src)
    rows = torch.stack([x[2], torch.zeros(K), x[0], torch.zeros(K), x[3]])
    q, s = quantize_mx_reference(rows)
    assert torch.equal(qg.view(U8), q.view(U8)) and torch.equal(sg, s)
    offs = torch.tensor([0, 97, 97, 128], dtype=torch.int32)
    qt, st, written = quantize_mx_t_grouped_reference(x, offs)
    # group 0 owns columns 0..127 (97 rows, zero padded), group 2 columns 128..255 (31 rows)
    assert int(qt[3, 96]) == 0x7F and int(qt[3, 128 + 30]) == 0x7F
    assert int(written.sum()) == 256
    pad = torch.zeros((128, K))
    pad[:31] = x[97:128]
    q, s = quantize_mx_t_reference(pad)
    assert torch.equal(qt[:, 128:256], q.view(U8)) and torch.equal(st[:, 4:8], s)


def _old_quantize_mxfp4_reference(x):
    """The MXFP4 formula before non-finite input was specified."""
    from ddlb_amd.ops.mx import _e2m1_code, pack_e2m1

    R, Kx = x.shape
    xb = x.to(torch.float32).reshape(R, Kx // 32, 32)
    amax = xb.abs().amax(dim=2)
    m, ex = torch.frexp(amax)
    e = torch.where(m <= 0.75, ex - 3, ex - 2).clamp(-127, 127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    y = ldexp_exact(xb, (-e).unsqueeze(2))
    code = _e2m1_code(y.abs().clamp(max=6.0))
    sign = (xb.view(torch.int32) >> 31) & 1
    return pack_e2m1(((sign << 3) | code).reshape(R, Kx)), (e + 127).to(U8)


def _block_loop_fp4(x):
    """The MXFP4 rule block by block on Python floats: ``(nibbles [R, K], scale bytes)``. Finite
    amax; a block with a non-finite element gets 255 and that element 0x7 | sign << 3; a finite
    element the nearest E2M1 value of clamp(|x| 2^-e, 6), ties to the even code."""
    values = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
    x32 = x.to(torch.float32)
    bits = x32.view(torch.int32)
    R, Kx = x32.shape
    nib = [[0] * Kx for _ in range(R)]
    s = [[0] * (Kx // 32) for _ in range(R)]
    for r in range(R):
        for b in range(Kx // 32):
            vals = [float(v) for v in x32[r, 32 * b:32 * b + 32]]
            amax = max([abs(v) for v in vals if math.isfinite(v)], default=0.0)
            if amax == 0.0:
                e = 0
            else:
                m, ex = math.frexp(amax)
                e = min(max(ex - 3 if m <= 0.75 else ex - 2, -127), 127)
            s[r][b] = e + 127 if all(math.isfinite(v) for v in vals) else 255
            for i, v in enumerate(vals):
                k = 32 * b + i
                sign = 8 if int(bits[r, k]) < 0 else 0
                if not math.isfinite(v):
                    nib[r][k] = sign | 7
                    continue
                y = min(abs(math.ldexp(v, -e)), 6.0)
                best = min(range(8), key=lambda c: (abs(values[c] - y), c % 2))
                nib[r][k] = sign | best
    return nib, s


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_mxfp4_reference_against_block_loops(dtype):
    from ddlb_amd.ops.mx import dequantize_mxfp4

    x = _special(dtype)
    q, s = quantize_mxfp4_reference(x)
    b = q.view(U8)
    nib = torch.stack((b & 0xF, b >> 4), dim=2).reshape(x.shape)
    nl, sl = _block_loop_fp4(x)
    assert s.tolist() == sl and nib.tolist() == nl
    fin = torch.isfinite(x)
    bad_blocks = (~fin).reshape(8, K // 32, 32).any(dim=2)
    assert torch.equal(s == 255, bad_blocks) and int(bad_blocks.sum()) == 8
    assert int(nib[0, 5]) == 0x7 and int(nib[0, 37]) == 0xF and int(nib[1, 40]) == 0xF
    # the finite neighbours are what they are without the bad element
    clean = torch.where(fin, x, torch.zeros_like(x))
    q0, s0 = quantize_mxfp4_reference(clean)
    b0 = q0.view(U8)
    nib0 = torch.stack((b0 & 0xF, b0 >> 4), dim=2).reshape(x.shape)
    assert torch.equal(nib[fin], nib0[fin]) and torch.equal(s[~bad_blocks], s0[~bad_blocks])
    # the dequantisation is NaN in the whole block of a non-finite element
    want = bad_blocks.unsqueeze(2).expand(8, K // 32, 32).reshape(8, K)
    assert torch.equal(torch.isnan(dequantize_mxfp4(q, s)), want)


def test_mxfp4_finite_data_keeps_every_byte():
    for seed in (7, 8):
        x = _wide(16, 512, seed)
        x[1, 64:96] = 0
        x[2, 5] = -0.0
        q, s = quantize_mxfp4_reference(x)
        q0, s0 = _old_quantize_mxfp4_reference(x)
        assert int(s.max()) < 255
        assert torch.equal(s, s0) and torch.equal(q.view(U8), q0.view(U8))


def test_scale_byte_255_dequantises_to_nan():
    q = torch.zeros((2, 128), dtype=U8).view(FP8)
    s = torch.full((2, 4), 127, dtype=U8)
    s[1, 2] = 255
    d = dequantize_mx(q, s)
    assert bool(torch.isnan(d[1, 64:96]).all()) and int(torch.isnan(d).sum()) == 32


def test_activation_specification_on_nonfinite():
    """What the fused epilogue must equal: relu keeps NaN; silu and gelu (tanh) give NaN at -Inf
    and NaN, +Inf at +Inf."""
    from ddlb_amd.ops.gemm import ACTS
    from ddlb_amd.parallel.sim import apply_act

    x = torch.tensor([NAN, INF, -INF, -2.0, 0.0, 3.0])
    relu = apply_act(x, ACTS["relu"])
    assert math.isnan(float(relu[0])) and relu[1:].tolist() == [INF, 0.0, 0.0, 0.0, 3.0]
    for act in ("gelu", "silu"):
        y = apply_act(x, ACTS[act])
        assert math.isnan(float(y[0])) and float(y[1]) == INF and math.isnan(float(y[2]))
        assert bool(torch.isfinite(y[3:]).all())
