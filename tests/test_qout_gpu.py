"""Quantised GEMM output on the GPU: the tiled kernel's MX epilogue (``gemm(..., out_quant=)``).

The oracle everywhere is the SAME kernel and tile with f32 output and the same activation, then
the torch reference quantiser: the fused ``(q, s)`` must equal it byte for byte
(``torch.equal`` on the bytes of ``q`` and of ``s``)."""

import itertools

import pytest
import torch

from _exact import ints, pow2_f64

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
FP4 = torch.float4_e2m1fn_x2
TILES = ("256x128", "128x256", "128x128", "256x128w4")
FORMS = ("bf16", "f16", "mxfp8", "mxfp4")
FMTS = ("mx", "mxfp4")
SENT = 0xA5
INT_CODE = (0, 2, 4, 5)  # E2M1 codes of |v| = 0, 1, 2, 3


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _qref(fmt):
    from ddlb_amd.ops import mx

    return mx.quantize_mx_reference if fmt == "mx" else mx.quantize_mxfp4_reference


def _pack_ints(v):
    from ddlb_amd.ops.mx import pack_e2m1

    code = torch.tensor(INT_CODE, device=v.device)[v.abs().long()]
    return pack_e2m1(code | ((v < 0).long() << 3))


def _scale_bytes(rows, k, g, spread=2):
    return (127 + torch.randint(-spread, spread + 1, (rows, k // 32), generator=g,
                                device=DEV)).to(torch.uint8)


def _operands(form, M, N, K, g):
    """Integer operands in -3..3 in an input form -> (a, w, keyword arguments of gemm)."""
    if form in ("bf16", "f16"):
        dt = torch.bfloat16 if form == "bf16" else torch.float16
        return ints((M, K), dt, g), ints((N, K), dt, g), {}
    kw = dict(a_scale=_scale_bytes(M, K, g), w_scale=_scale_bytes(N, K, g))  # non-trivial bytes
    if form == "mxfp8":
        return ints((M, K), FP8, g), ints((N, K), FP8, g), kw
    return (_pack_ints(ints((M, K), torch.float32, g)),
            _pack_ints(ints((N, K), torch.float32, g)), kw)


def _oracle(a, w, fmt, **kw):
    """f32 output of the same kernel, tile and activation, then the reference quantiser."""
    from ddlb_amd.ops.gemm import gemm

    c = gemm(a, w, out_dtype=torch.float32, **kw)
    torch.cuda.synchronize()
    q, s = _qref(fmt)(c)
    return c, q, s


def _bytes(t):
    return t.view(torch.uint8)


def _same(q, s, q_ref, s_ref):
    assert q.dtype == q_ref.dtype and s.dtype == torch.uint8
    assert tuple(q.shape) == tuple(q_ref.shape) and tuple(s.shape) == tuple(s_ref.shape)
    assert torch.equal(s, s_ref), f"{int((s != s_ref).sum())} scale bytes differ"
    bad = int((_bytes(q) != _bytes(q_ref)).sum())
    assert bad == 0, f"{bad} data bytes differ"


def _views(fmt, M, N, pad=32, spad=8, extra=3):
    """Sentinel-filled buffers and the (out, out_scale) views into them: ldc > N, a scale pitch
    greater than N / 32, extra rows."""
    ncol = N if fmt == "mx" else N // 2
    qb = torch.full((M + extra, ncol + pad), SENT, dtype=torch.uint8, device=DEV)
    sb = torch.full((M + extra, N // 32 + spad), SENT, dtype=torch.uint8, device=DEV)
    return qb, sb, qb[:M, :ncol].view(FP8 if fmt == "mx" else FP4), sb[:M, :N // 32]


def _untouched(buf, M, ncol):
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    mask[:M, :ncol] = False
    bad = int((buf[mask] != SENT).sum())
    assert bad == 0, f"{bad} bytes outside the [{M}, {ncol}] view were written"


# ------------------------------------------------------------------ 1. exact sweep
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tile", TILES)
def test_exact_sweep(tile, form, fmt):
    """Every offered tile x input form x output form, ragged M, N with a half-empty tile under
    the 256-column tiles, two K-tile counts; outputs as views of sentinel-filled buffers."""
    from ddlb_amd.ops.gemm import gemm

    g = _gen(100 + TILES.index(tile) * 8 + FORMS.index(form) * 2 + FMTS.index(fmt))
    Ns = (128, 256, 384) if fmt == "mx" else (256, 512, 768)
    Ks = (256, 512) if form == "mxfp4" else (128, 384)
    for M, N, K in itertools.product((1, 130, 257, 300), Ns, Ks):
        a, w, kw = _operands(form, M, N, K, g)
        c, q_ref, s_ref = _oracle(a, w, fmt, tile=tile, **kw)
        assert bool(torch.isfinite(c).all())
        qb, sb, out, out_scale = _views(fmt, M, N)
        q, s = gemm(a, w, out, tile=tile, out_quant=fmt, out_scale=out_scale, **kw)
        torch.cuda.synchronize()
        assert q.data_ptr() == out.data_ptr() and s.data_ptr() == out_scale.data_ptr()
        _same(q, s, q_ref, s_ref)
        _untouched(qb, M, out.shape[1])
        _untouched(sb, M, N // 32)
    # allocated by gemm(): dense, and `auto` lands on an offered tile
    q, s = gemm(a, w, out_quant=fmt, **kw)
    torch.cuda.synchronize()
    assert q.is_contiguous() and s.is_contiguous()
    _, q_ref, s_ref = _oracle(a, w, fmt, **kw)
    _same(q, s, q_ref, s_ref)


def _padded(t, pad, poison):
    """``t`` (one-byte elements) as a view of a buffer whose rows are ``pad`` bytes longer, the
    padding filled with ``poison``."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), poison, dtype=torch.uint8, device=DEV)
    buf[:, :t.shape[1]] = _bytes(t)
    return buf[:, :t.shape[1]].view(t.dtype)


def test_padded_fp4_operand_rows_and_scale_pitch_exact():
    """fp4 -> mxfp4 with the operands and their scales as views of wider buffers (lda > K / 2
    bytes, a scale pitch greater than K / 32; 6.0 pairs and NaN bytes in the padding) and the
    outputs as views as well: two ragged row tiles, two K-tiles. The accumulator is the exact
    sum (integers times powers of two, 21 bits at the most), so the specification is the
    reference quantiser on it."""
    from ddlb_amd.ops.gemm import gemm

    g = _gen(900)
    M, N, K = 130, 256, 512
    nb = K // 32
    av, wv = ints((M, K), torch.float32, g), ints((N, K), torch.float32, g)
    s_a, s_w = _scale_bytes(M, K, g), _scale_bytes(N, K, g)
    c = torch.zeros(M, N, dtype=torch.float64, device=DEV)
    for b in range(nb):
        p = av[:, 32 * b:32 * b + 32].double() @ wv[:, 32 * b:32 * b + 32].double().t()
        c += p * pow2_f64(s_a[:, b].long().unsqueeze(1) + s_w[:, b].long().unsqueeze(0) - 254)
    q_ref, s_ref = _qref("mxfp4")(c.float())
    a4, w4 = _padded(_pack_ints(av), 32, 0x77), _padded(_pack_ints(wv), 48, 0x77)
    sa, sw = _padded(s_a, 8, 0xFF), _padded(s_w, 16, 0xFF)
    assert a4.stride(0) == K // 2 + 32 and sa.stride(0) == nb + 8
    for tile in ("auto", "128x128"):
        qb, sb, out, out_scale = _views("mxfp4", M, N)
        q, s = gemm(a4, w4, out, tile=tile, out_quant="mxfp4", out_scale=out_scale, a_scale=sa,
                    w_scale=sw)
        torch.cuda.synchronize()
        _same(q, s, q_ref, s_ref)
        _untouched(qb, M, N // 2)
        _untouched(sb, M, N // 32)


# ------------------------------------------------------------------ 2. all 32 block positions
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("form", ("bf16", "mxfp8"))
@pytest.mark.parametrize("tile", TILES)
def test_block_maximum_at_every_position(tile, form, fmt):
    """Row m's blocks hold 1 everywhere and 64 at position m % 32: a reduce that misses a lane or
    a fragment of the pair yields a too-small scale and saturated codes."""
    from ddlb_amd.ops.gemm import gemm
    from ddlb_amd.ops.mx import dequantize_mx

    M, N, K = 64, 256, 128
    m = torch.arange(M, device=DEV)
    n = torch.arange(N, device=DEV)
    a = torch.zeros(M, K, device=DEV)
    a[m, m % 32] = 1.0
    w = torch.zeros(N, K, device=DEV)
    w[:, :32] = 1.0
    w[n, n % 32] = 64.0
    kw = {}
    if form == "mxfp8":
        a, w = a.to(FP8), w.to(FP8)
        kw = dict(a_scale=torch.full((M, K // 32), 127, dtype=torch.uint8, device=DEV),
                  w_scale=torch.full((N, K // 32), 127, dtype=torch.uint8, device=DEV))
    else:
        a, w = a.to(torch.bfloat16), w.to(torch.bfloat16)
    c, q_ref, s_ref = _oracle(a, w, fmt, tile=tile, **kw)
    want = torch.where((n % 32).unsqueeze(0) == (m % 32).unsqueeze(1), 64.0, 1.0)
    assert torch.equal(c, want)
    q, s = gemm(a, w, tile=tile, out_quant=fmt, **kw)
    torch.cuda.synchronize()
    # 64 = 0.5 * 2^7: e = 7 - 9 (fp8: 64 -> 256, 1 -> 4) / 7 - 3 (fp4: 64 -> 4, 1 -> 0)
    assert bool((s == (125 if fmt == "mx" else 131)).all())
    _same(q, s, q_ref, s_ref)
    if fmt == "mx":
        assert torch.equal(dequantize_mx(q, s), want)


# ------------------------------------------------------------------ 3. activations
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("tile", TILES)
def test_relu_zero_blocks(tile, fmt):
    """Whole blocks non-positive before relu: s = 127 and q = +0 there."""
    from ddlb_amd.ops.gemm import gemm

    g = _gen(31)
    M, N, K = 130, 512, 128
    a = ints((M, K), torch.bfloat16, g).abs()
    w = ints((N, K), torch.bfloat16, g)
    neg = (torch.arange(N, device=DEV) // 32) % 2 == 1  # every other block: W rows <= 0
    w[neg] = -w[neg].abs()
    c, q_ref, s_ref = _oracle(a, w, fmt, tile=tile, act="relu")
    q, s = gemm(a, w, tile=tile, out_quant=fmt, act="relu")
    torch.cuda.synchronize()
    _same(q, s, q_ref, s_ref)
    zero_blocks = s.reshape(M, N // 32)[:, 1::2]
    assert bool((zero_blocks == 127).all())
    qz = _bytes(q).reshape(M, N // 32, -1)[:, 1::2]
    assert bool((qz == 0).all())                      # +0, never 0x80 / 0x8
    assert bool((s.reshape(M, N // 32)[:, 0::2] != 127).any())


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("act", ("gelu", "silu"))
@pytest.mark.parametrize("form", ("bf16", "mxfp8"))
def test_gelu_silu_random(form, act, fmt):
    """The same act4 text runs in the f32-output and the quantising epilogue: byte equality, no
    tolerance."""
    from ddlb_amd.ops.gemm import gemm
    from ddlb_amd.ops.mx import quantize_mx

    g = _gen(32)
    M, N, K = 300, 512, 256
    a = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g, device=DEV) / 8).to(torch.bfloat16)
    kw = {}
    if form == "mxfp8":
        (a, sa), (w, sw) = quantize_mx(a), quantize_mx(w)
        kw = dict(a_scale=sa, w_scale=sw)
    for tile in TILES:
        c, q_ref, s_ref = _oracle(a, w, fmt, tile=tile, act=act, **kw)
        assert float(c.min()) < 0 < float(c.max())
        q, s = gemm(a, w, tile=tile, out_quant=fmt, act=act, **kw)
        torch.cuda.synchronize()
        _same(q, s, q_ref, s_ref)


# ------------------------------------------------------------------ 4. wide range
@pytest.mark.parametrize("fmt", FMTS)
def test_wide_range_of_output_scales(fmt):
    """Scaled-fp8 inputs whose scale bytes spread C over about 2^-127 .. 2^127 across blocks.

    Both ends of the output scale are reached, asserted on the oracle's ``s``: the lower clamp
    (``s = 0``: a block whose amax lies below the smallest scale the format can express), and the
    largest byte a finite f32 block can have: amax = 1.875 * 2^127 gives ``e = 128 - 8`` (fp8,
    ``s = 247``) / ``128 - 2`` (fp4, ``s = 253``). The upper clamp ``e > 127`` itself would need
    amax >= 2^131, which is not a finite f32."""
    from ddlb_amd.ops.gemm import gemm

    g = _gen(41)
    M, N, K = 96, 512, 128
    nb = N // 32
    a = ints((M, K), torch.float32, g)
    w = ints((N, K), torch.float32, g)
    a[:, 0] = 1.0
    e_a = ((torch.arange(M, device=DEV) % 3) - 1) * 30                     # -30, 0, 30 by row
    D = torch.round(torch.linspace(-88, 88, nb, device=DEV)).to(torch.int64)
    # crafted blocks (W rows non-zero at k = 0 only, so C[m, n] = W[n, 0] 2^(e_a[m] + D)):
    # block 0: C = 2^-120 on the e_a = -30 rows (normal; fp8's e = -128 clamps)
    # block 1: C = 2^-127 there (subnormal; fp4's e = -129 clamps)
    # last block: one 15 among ones, C = 15 * 2^124 = 1.875 * 2^127 on the e_a = +30 rows
    for blk, d in ((0, -90), (1, -97), (nb - 1, 94)):
        w[blk * 32:(blk + 1) * 32] = 0
        w[blk * 32:(blk + 1) * 32, 0] = 1.0
        D[blk] = d
    w[(nb - 1) * 32 + 5, 0] = 15.0
    s_a = (127 + e_a).to(torch.uint8).unsqueeze(1).expand(M, K // 32).contiguous()
    s_w = (127 + D).to(torch.uint8).repeat_interleave(32).unsqueeze(1).expand(
        N, K // 32).contiguous()
    a8, w8 = a.to(FP8), w.to(FP8)
    for tile in TILES:
        c, q_ref, s_ref = _oracle(a8, w8, fmt, tile=tile, a_scale=s_a, w_scale=s_w)
        assert bool(torch.isfinite(c).all())
        nz = c[c != 0].abs()
        print(f"{fmt} {tile}: |C| in [2^{float(nz.min().log2()):.1f}, "
              f"2^{float(nz.max().log2()):.1f}], s in [{int(s_ref.min())}, {int(s_ref.max())}]")
        assert float(nz.min()) <= 2.0 ** -100 and float(nz.max()) >= 2.0 ** 100
        assert int(s_ref.min()) == 0
        assert int(s_ref.max()) == (247 if fmt == "mx" else 253)
        q, s = gemm(a8, w8, tile=tile, out_quant=fmt, a_scale=s_a, w_scale=s_w)
        torch.cuda.synchronize()
        _same(q, s, q_ref, s_ref)


# ------------------------------------------------------------------ 5. round trip
@pytest.mark.parametrize("fmt", FMTS)
def test_round_trip_into_the_next_gemm(fmt):
    """(q, s) go straight back in as a / a_scale: no copy, no re-layout."""
    from ddlb_amd.ops.gemm import gemm
    from ddlb_amd.ops.mx import quantize_mx, quantize_mxfp4

    g = _gen(51)
    M, H, F = 300, 256, 512
    x = torch.randn(M, H, generator=g, device=DEV).to(torch.bfloat16)
    w1 = (torch.randn(F, H, generator=g, device=DEV) / 16).to(torch.bfloat16)
    w2 = (torch.randn(H, F, generator=g, device=DEV) / 16).to(torch.bfloat16)
    w2q, w2s = (quantize_mx if fmt == "mx" else quantize_mxfp4)(w2)
    t = "128x128"
    _, q_ref, s_ref = _oracle(x, w1, fmt, act="gelu", tile=t)
    q, s = gemm(x, w1, out_quant=fmt, act="gelu", tile=t)
    y = gemm(q, w2q, a_scale=s, w_scale=w2s, out_dtype=torch.float32, tile=t)
    y_ref = gemm(q_ref, w2q, a_scale=s_ref, w_scale=w2s, out_dtype=torch.float32, tile=t)
    torch.cuda.synchronize()
    _same(q, s, q_ref, s_ref)
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    assert torch.equal(y, y_ref)


# ------------------------------------------------------------------ 6. refusals of the entry
def test_native_entry_refuses_what_python_would():
    """``gemm_launch`` itself refuses every unsupported combination (argument inspection only)
    and launches nothing: the sentinel bytes survive."""
    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import DT_BF16, DT_F32, DT_FP4, DT_FP8, TILES as CODES

    C = load()
    M, N, K = 256, 256, 256
    a = torch.ones(M, K, device=DEV, dtype=torch.bfloat16)
    w = torch.ones(N, K, device=DEV, dtype=torch.bfloat16)
    a8, w8, af = a.to(FP8), w.to(FP8), a.float()
    sc = torch.full((M, K // 32), 127, dtype=torch.uint8, device=DEV)
    q = torch.full((M, N), SENT, dtype=torch.uint8, device=DEV)
    s = torch.full((M, N // 32), SENT, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(x=a, y=w, din=DT_BF16, dout=DT_FP8, tile="auto", mode=0, ksplit=1, n=N, ldc=N,
             a_grp=0, c_grp=0, sa=0, sw=0, cs=None, cs_ld=N // 32, c=None):
        C.gemm(x.data_ptr(), y.data_ptr(), q.data_ptr() if c is None else c, K, K, ldc, M, n, K,
               din, dout, CODES[tile], mode, a_grp, a_grp, c_grp, c_grp, st, 0, ksplit, sa, sw,
               K // 32, K // 32, s.data_ptr() if cs is None else cs, cs_ld)

    bad = [
        dict(cs=0),                                   # quantised dout without output scales
        dict(dout=DT_BF16),                           # output scales without a quantised dout
        dict(dout=DT_F32),
        dict(n=N - 32), dict(n=64),                   # N % 128
        dict(dout=DT_FP4, n=128, ldc=2 * N),          # N % 256 for fp4
        dict(dout=DT_FP4, ldc=N + 1),                 # an odd fp4 ldc
        dict(x=af, y=af, din=DT_F32),                 # f32 inputs
        dict(x=a8, y=w8, din=DT_FP8),                 # fp8 without scales
        dict(x=a8, y=w8, din=DT_FP8, sa=sc.data_ptr()),
        dict(x=a8, y=w8, din=DT_FP4),                 # fp4 without scales
        dict(sa=sc.data_ptr(), sw=sc.data_ptr()),     # scales with 16-bit operands
        dict(mode=1), dict(mode=2),                   # generic; MX without fp8 / fp4 operands
        dict(tile="256x256"), dict(tile="256x256w4"), dict(tile="pt4"), dict(tile="t8"),
        dict(tile="i128"),
        dict(ksplit=2),
        dict(a_grp=64), dict(c_grp=64),               # grouped A / C rows
        dict(ldc=N + 8), dict(ldc=N - 16),            # rows off 16 bytes; ldc < N
        dict(c=q.data_ptr() + 8),                     # base off 16 bytes
        dict(cs=s.data_ptr() + 2), dict(cs_ld=N // 32 + 2), dict(cs_ld=N // 32 - 4),
        dict(dout=DT_FP4, ldc=2 * N, cs_ld=N // 32 + 4),  # fp4 scales: multiples of 8
    ]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((q == SENT).all()) and bool((s == SENT).all())
    call()                                            # and the supported call runs
    torch.cuda.synchronize()
    # C = K = 256 = 0.5 * 2^9: e = 0, the e4m3 byte of 256 is 0x78
    assert bool((s == 127).all()) and bool((q == 0x78).all())


# ------------------------------------------------------------------ 7. the MLP
@pytest.mark.parametrize("fmt", FMTS)
def test_mx_mlp(fmt):
    from ddlb_amd.models.mx_mlp import MxMLP
    from ddlb_amd.ops.gemm import gemm
    from ddlb_amd.ops.mx import quantize_mx, quantize_mxfp4

    S, H, F = 300, 256, (384 if fmt == "mx" else 512)
    tile = "128x128"
    mlp = MxMLP(H, F, S, "bfloat16", "gelu", fmt=fmt, fused=True, tile=tile)
    y = mlp.forward().clone()
    torch.cuda.synchronize()
    # the hand-chained forward: f32-out fc1 + reference quantiser + fc2, on the same tiles
    xq, xs = (quantize_mx if fmt == "mx" else quantize_mxfp4)(mlp.X)
    h = gemm(xq, mlp.w1q, a_scale=xs, w_scale=mlp.w1s, act="gelu", tile=tile,
             out_dtype=torch.float32)
    hq, hs = _qref(fmt)(h)
    want = gemm(hq, mlp.w2q, a_scale=hs, w_scale=mlp.w2s, tile=tile, out_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (S, H)
    assert torch.equal(y, want)
    mlp.validate(y)
    y2 = mlp.forward().clone()
    torch.cuda.synchronize()
    assert torch.equal(y, y2)                         # two forwards are bit-identical
    unfused = MxMLP(H, F, S, "bfloat16", "gelu", fmt=fmt, fused=False, tile=tile)
    assert torch.equal(unfused.X, mlp.X) and torch.equal(unfused.W1, mlp.W1)
    yu = unfused.forward()
    torch.cuda.synchronize()
    unfused.validate(yu)
