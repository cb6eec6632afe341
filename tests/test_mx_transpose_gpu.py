"""The transposing MX quantiser on the GPU (``csrc/gemm/mx_quant_t.hip``): ``qt, st`` byte for byte
against the torch specification (the row-wise reference applied to ``x.T``), for MX-fp8 and MXFP4,
one-way and two-way. The kernel's tile is 128 rows (fp4: 256) by 64 columns; it has no grid cap
(one workgroup per tile), so there is no grid-stride case to test."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
FP4 = torch.float4_e2m1fn_x2
FMTS = ("mx", "mxfp4")
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)
TILE_COLS = 64


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _wide(rows, k, g, dtype=torch.bfloat16):
    """randn * 2^U{-20..20}, one exponent per 32-element block."""
    x = torch.randn(rows, k // 32, 32, generator=g, device=DEV)
    ex = torch.randint(-20, 21, (rows, k // 32, 1), generator=g, device=DEV)
    x = torch.ldexp(x, ex).reshape(rows, k)
    if dtype == torch.float16:
        x = x.clamp(-60000, 60000)
    return x.to(dtype)


def _wide_t(R, C, seed, dtype=torch.bfloat16):
    """``[R, C]`` input whose exponent changes from one COLUMN block to the next."""
    return _wide(C, R, _gen(seed), dtype).t().contiguous()


def _ref(x0, fmt):
    from ddlb_amd.ops.mx import quantize_mx_reference, quantize_mxfp4_reference

    return quantize_mxfp4_reference(x0) if fmt == "mxfp4" else quantize_mx_reference(x0)


def _same(got, want):
    return (torch.equal(got[0].view(torch.uint8), want[0].view(torch.uint8))
            and torch.equal(got[1], want[1]))


def _check(x, fmt, **kw):
    """quantize_mx_t(x) against the row-wise reference of x.T; returns the outputs."""
    from ddlb_amd.ops.mx import quantize_mx_t, quantize_mx_t_reference

    qt, st = quantize_mx_t(x, fmt=fmt, **kw)
    torch.cuda.synchronize()
    R, C = x.shape
    assert qt.dtype == (FP4 if fmt == "mxfp4" else FP8) and st.dtype == torch.uint8
    assert tuple(qt.shape) == (C, R // 2 if fmt == "mxfp4" else R)
    assert tuple(st.shape) == (C, R // 32)
    want = quantize_mx_t_reference(x, fmt)
    bad = int((qt.view(torch.uint8) != want[0].view(torch.uint8)).sum())
    sbad = int((st != want[1]).sum())
    assert bad == 0 and sbad == 0, f"{bad} data bytes, {sbad} scale bytes differ ({R} x {C})"
    return qt, st


def _edge_matrix(fmt, dtype, rows=72, k=512):
    """The matrix of test_quantizer_matches_reference (tests/test_mx_scaled_gpu.py for fp8,
    tests/test_mxfp4_gpu.py for fp4), ``rows`` x ``k``: zero rows and blocks, a lone maximum, the
    448 / 6 boundary at five exponents, subnormal amax, all ties in both signs, -0, a negative
    value that rounds to zero, e = -127."""
    x = _wide(rows, k, _gen(11), dtype)
    x[0] = 0                                   # zero blocks (a whole row ...
    x[1, 32:64] = 0                            # ... and one inside a row)
    x[2] = 0
    x[2, 77] = -1.5                            # a lone maximum
    top, unit, other, above = ((6.0, 1.0, -2.0, 6.03125) if fmt == "mxfp4"
                               else (448.0, 3.0, -5.0, 480.0))
    for i, j in enumerate((-9, -1, 0, 2, 6)):  # the boundary: e = j, then e = j + 1
        x[3 + i, 0:32] = unit * 2.0 ** j
        x[3 + i, 7] = top * 2.0 ** j
        x[3 + i, 32:64] = other * 2.0 ** j
        x[3 + i, 40] = above * 2.0 ** j        # (representable in bf16, f16 and f32)
    x[8, 0:32] = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -130  # subnormal amax
    x[9] = 0                                   # every E2M1 tie, both signs, under e = 0 (fp8:
    x[9, 0] = top                              # exact values); signed zeros
    for i, v in enumerate(TIES):
        x[9, 1 + i] = v
        x[9, 9 + i] = -v
    x[9, 20] = -0.0
    x[9, 21] = -0.1 if fmt == "mxfp4" else -2.0 ** -11  # a negative value that rounds to zero
    x[9, 32:64] = 0                            # e4m3 ties under e = 0: 17 -> 16, 19 -> 20, ...
    x[9, 32] = top
    x[9, 33:37] = torch.tensor([17.0, -19.0, 2.0 ** -10, -3.0 * 2.0 ** -10]).to(dtype)
    x[11, 0:32] = 2.0 ** (10 if dtype != torch.float16 else 3)
    if dtype != torch.float16:                 # e = -127 (s = 0): subnormal inputs and scale
        x[10, 0:32] = 0
        x[10, 0:5] = torch.tensor([2.0 ** -125, 2.0 ** -126, -2.0 ** -127, 2.0 ** -128,
                                   1.5 * 2.0 ** -127]).to(dtype)
        x[10, 32:64] = 0                       # clamped to e = -127: 3 * 2^-127 stays 3
        x[10, 32:35] = torch.tensor([3.0 * 2.0 ** -127, -2.0 ** -127, 2.0 ** -129]).to(dtype)
    return x


# ------------------------------------------------------------------ 1. byte for byte, the edges
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_matches_reference_on_edge_matrix(fmt, dtype):
    C, R = TILE_COLS + 8, 512                  # one vector beyond a column tile (16-bit)
    x0 = _edge_matrix(fmt, dtype, C, R)
    x = x0.t().contiguous()                    # [R, C]: the edge rows are now columns
    qt, st = _check(x, fmt)
    q_ref, s_ref = _ref(x0, fmt)
    assert _same((qt, st), (q_ref, s_ref))
    # the reference itself sees the edges it was built for
    assert int(s_ref[0, 0]) == 127 and int(s_ref[1, 1]) == 127
    assert [int(v) - 127 for v in s_ref[3:8, 0]] == [-9, -1, 0, 2, 6]
    assert [int(v) - 127 for v in s_ref[3:8, 1]] == [-8, 0, 1, 3, 7]
    if dtype != torch.float16:
        assert s_ref[10, :2].tolist() == [0, 0] and int(s_ref[8, 0]) == 0
    byte = qt.view(torch.uint8)[9]
    if fmt == "mxfp4":
        assert int(byte[10]) == 0x88           # elements 20 (-0) and 21 (-0.1): 0x8 each
    else:
        assert int(byte[20]) == 0x80 and int(byte[21]) == 0x80


# ------------------------------------------------------------------ 2. shapes
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_shapes(fmt, dtype):
    """One and three row tiles; one 16-byte vector of columns, 200 columns (three full tiles and
    a part of one; 200 % 32 != 0), exactly one tile; an input that is a column slice."""
    tr = 256 if fmt == "mxfp4" else 128
    vec = 16 // torch.empty((), dtype=dtype).element_size()
    for R in (tr, 3 * tr):
        for C in (vec, 200, TILE_COLS):
            _check(_wide_t(R, C, R + C, dtype), fmt)
    wide = _wide_t(tr, 320, 5, dtype)
    view = wide[:, 64:64 + 136]                # ldx = 320 > C = 136, a 16-byte-aligned start
    assert view.stride(0) == 320 and not view.is_contiguous()
    _check(view, fmt)


def test_empty_launches_nothing():
    from ddlb_amd.ops.mx import quantize_mx_t

    for fmt in FMTS:
        qt, st = quantize_mx_t(torch.zeros(0, 64, device=DEV, dtype=torch.bfloat16), fmt=fmt)
        assert tuple(qt.shape) == (64, 0) and tuple(st.shape) == (64, 0)
        qt, st = quantize_mx_t(torch.zeros(256, 0, device=DEV, dtype=torch.bfloat16), fmt=fmt)
        assert qt.shape[0] == 0 and tuple(st.shape) == (0, 8)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 4. preallocated outputs
@pytest.mark.parametrize("fmt", FMTS)
def test_preallocated_outputs_and_nothing_outside(fmt):
    fp4 = fmt == "mxfp4"
    R, C = (512, 72)
    ncol, nb, sal = (R // 2 if fp4 else R), R // 32, (8 if fp4 else 4)
    qbuf = torch.full((C + 5, ncol + 48), 0xA5, dtype=torch.uint8, device=DEV)
    sbuf = torch.full((C + 5, nb + 3 * sal), 0xA5, dtype=torch.uint8, device=DEV)
    qv = qbuf[2:2 + C, 16:16 + ncol]           # a spare margin on every side
    sv = sbuf[3:3 + C, sal:sal + nb]
    x = _wide_t(R, C, 21)
    qt, st = _check(x, fmt, out=(qv.view(FP4 if fp4 else FP8), sv))
    assert qt.data_ptr() == qv.data_ptr() and st.data_ptr() == sv.data_ptr()
    qmask = torch.ones_like(qbuf, dtype=torch.bool)
    qmask[2:2 + C, 16:16 + ncol] = False
    smask = torch.ones_like(sbuf, dtype=torch.bool)
    smask[3:3 + C, sal:sal + nb] = False
    assert bool((qbuf[qmask] == 0xA5).all()) and bool((sbuf[smask] == 0xA5).all())


# ------------------------------------------------------------------ 5. two-way
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_way(fmt, dtype):
    from ddlb_amd.ops.mx import (quantize_mx, quantize_mx_2way, quantize_mx_t_reference,
                                 quantize_mxfp4)

    fp4 = fmt == "mxfp4"
    tr = 256 if fp4 else 128
    rowwise = quantize_mxfp4 if fp4 else quantize_mx
    # the two-way launch deals the tiles to its workgroups in whole groups of 16 (fp4: 32) and
    # the rest in order: fewer tiles than a group, whole groups only, a group and a rest
    for R, C in ((256, 512 if fp4 else 384), (3 * tr, tr), (512, 1024),
                 (768, 768) if fp4 else (384, 640)):
        # exponents that vary along both axes: per row block times per column block
        x = (_wide(R, C, _gen(R), torch.float32)
             * torch.ldexp(torch.ones(R // 32, 1, device=DEV),
                           torch.randint(-6, 7, (R // 32, 1), generator=_gen(C), device=DEV)
                           ).repeat_interleave(32, dim=0)).clamp(-60000, 60000).to(dtype)
        q, s, qt, st = quantize_mx_2way(x, fmt=fmt)
        torch.cuda.synchronize()
        assert q.dtype == qt.dtype == (FP4 if fp4 else FP8)
        assert _same((q, s), rowwise(x)), (R, C)
        assert _same((qt, st), quantize_mx_t_reference(x, fmt)), (R, C)
        assert tuple(q.shape) == (R, C // 2 if fp4 else C) and tuple(s.shape) == (R, C // 32)


# ------------------------------------------------------------------ 6. repeats
@pytest.mark.parametrize("fmt", FMTS)
def test_repeats_are_bit_identical(fmt):
    from ddlb_amd.ops.mx import quantize_mx_2way, quantize_mx_t

    x = _wide_t(768, 512, 3)
    a, b = quantize_mx_t(x, fmt=fmt), quantize_mx_t(x, fmt=fmt)
    c, d = quantize_mx_2way(x, fmt=fmt), quantize_mx_2way(x, fmt=fmt)
    torch.cuda.synchronize()
    assert _same(a, b) and _same(c[:2], d[:2]) and _same(c[2:], d[2:]) and _same(a, c[2:])


def test_side_stream():
    from ddlb_amd.ops.mx import quantize_mx_t, quantize_mx_t_reference

    x = _wide_t(256, 136, 9)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    qt, st = quantize_mx_t(x, stream=side.cuda_stream)
    side.synchronize()
    assert _same((qt, st), quantize_mx_t_reference(x))


# ------------------------------------------------------------------ 7. the native entry
@pytest.mark.parametrize("fmt", FMTS)
def test_native_entry_refuses_what_python_would(fmt):
    """The launch entry itself refuses (never something substituted) when called direct."""
    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import dtype_code
    from ddlb_amd.ops.mx import quantize_mx_t_reference

    C_ = load()
    fp4 = fmt == "mxfp4"
    mod, sal = (256, 8) if fp4 else (128, 4)
    R, C = 2 * mod, 2 * mod
    ncol, nb = (R // 2 if fp4 else R), R // 32
    x = _wide_t(R, C, 4)

    def big(*shape):
        return torch.full(shape, 0xA5, dtype=torch.uint8, device=DEV)

    qt, st = big(C, ncol + 32), big(C, nb + 16)
    q, s = big(R, (C // 2 if fp4 else C) + 32), big(R, C // 32 + 16)
    strm = torch.cuda.current_stream().cuda_stream
    good = dict(x=x.data_ptr(), qt=qt.data_ptr(), st=st.data_ptr(), ldx=C, ldqt=ncol + 32,
                ldst=nb + 16, R=R, C=C, din=dtype_code(x.dtype), fp4=fp4, stream=strm)
    good2 = dict(good, two=True, q=q.data_ptr(), s=s.data_ptr(), ldq=q.stride(0),
                 lds=s.stride(0))

    def refused(base, **bad):
        with pytest.raises(RuntimeError, match="invalid"):
            C_.mx_quantize_t(**dict(base, **bad))

    for base in (good, good2):
        for name in ("x", "qt", "st"):
            refused(base, **{name: 0})             # a null pointer
        refused(base, R=R - 32)                    # R no multiple of the row tile
        refused(base, R=mod // 2)
        refused(base, C=C - 4)                     # C bf16 elements: not whole vectors
        refused(base, R=-mod)
        refused(base, C=-8)
        refused(base, din=99)
        refused(base, ldx=C - 8)                   # ldx < C
        refused(base, ldx=C + 4)                   # rows no multiple of 16 bytes apart
        refused(base, x=x.data_ptr() + 2)
        refused(base, ldqt=ncol - 16)              # too short
        refused(base, ldqt=ncol + 8)               # not a multiple of 16
        refused(base, qt=qt.data_ptr() + 8)
        refused(base, ldst=nb - sal)
        refused(base, ldst=nb + sal // 2)
        refused(base, st=st.data_ptr() + sal // 2)
    refused(good2, q=0)
    refused(good2, s=0)
    refused(good2, C=C - 64)                       # whole vectors, but no whole K-tile
    refused(good2, ldq=(C // 2 if fp4 else C) - 8)
    refused(good2, ldq=q.stride(0) + 2)
    refused(good2, q=q.data_ptr() + 2)
    refused(good2, lds=C // 32 - 1)
    torch.cuda.synchronize()
    for t in (qt, st, q, s):
        assert bool((t == 0xA5).all())             # nothing was launched
    C_.mx_quantize_t(**dict(good, R=0))            # an empty problem is no error, and no launch
    C_.mx_quantize_t(**dict(good, C=0))
    torch.cuda.synchronize()
    assert bool((qt == 0xA5).all()) and bool((st == 0xA5).all())
    C_.mx_quantize_t(**good2)
    torch.cuda.synchronize()
    want = quantize_mx_t_reference(x, fmt)
    assert _same((qt[:, :ncol], st[:, :nb]), want)
    assert bool((qt[:, ncol:] == 0xA5).all()) and bool((st[:, nb:] == 0xA5).all())
    assert bool((q[:, -32:] == 0xA5).all()) and bool((s[:, -16:] == 0xA5).all())
