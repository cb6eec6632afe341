"""Gated (GLU) GEMM epilogue on the GPU: ``gemm(..., glu=True)``, dense and quantised.

The oracle of the exact tests is the existing ungated kernel on the same tile with f32 output
(``c``, exact for integer operands in -3..3 under power-of-two block scales), then
``act(c[gate]) * c[up]`` in torch f32 for ``act`` in (none, relu): one f32 multiply, correctly
rounded on both sides, then one rounding to the output dtype or the torch reference quantiser.
Everything is compared with ``torch.equal`` (bytes for quantised data and scales). ``c`` is
computed once per (tile, form, shape) and shared by the dense and the quantised test."""

import itertools

import pytest
import torch

from _exact import ints, sentinel_out, untouched

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
FP4 = torch.float4_e2m1fn_x2
TILES = ("256x128", "128x256", "128x128", "256x128w4")
FORMS = ("bf16", "f16", "mxfp8", "mxfp4")
FMTS = ("mx", "mxfp4")
DENSE = {"bf16": (torch.bfloat16, torch.float32), "f16": (torch.float16, torch.float32),
         "mxfp8": (torch.bfloat16, torch.float16, torch.float32),
         "mxfp4": (torch.bfloat16, torch.float16, torch.float32)}
MS = (1, 130, 257)
SENT = 0xA5
INT_CODE = (0, 2, 4, 5)  # E2M1 codes of |v| = 0, 1, 2, 3
ZERO_GATE_N = 512        # the N (in both tests) whose first 32 gate rows of W are zero


def _ks(form):
    return (256, 512) if form == "mxfp4" else (128, 384)  # two K-tile counts


def _qref(fmt):
    from ddlb_amd.ops import mx

    return mx.quantize_mx_reference if fmt == "mx" else mx.quantize_mxfp4_reference


def _bytes(t):
    return t.view(torch.uint8)


def _pack_ints(v):
    from ddlb_amd.ops.mx import pack_e2m1

    code = torch.tensor(INT_CODE, device=v.device)[v.abs().long()]
    return pack_e2m1(code | ((v < 0).long() << 3))


def _scale_bytes(rows, k, g, centre=127, spread=2):
    return (centre + torch.randint(-spread, spread + 1, (rows, k // 32), generator=g,
                                   device=DEV)).to(torch.uint8)


def _typed(v, form):
    """Integer-valued f32 ``v`` in an input form's data type."""
    if form == "mxfp4":
        return _pack_ints(v)
    return v.to({"bf16": torch.bfloat16, "f16": torch.float16, "mxfp8": FP8}[form])


_CASES = {}


def _case(tile, form, M, N, K):
    """``(a, w, kw, c)`` of a shape, made once: integer operands in -3..3 (non-trivial scale
    bytes for the block-scaled forms) and the ungated kernel's f32 product on ``tile``. For
    ``N == ZERO_GATE_N`` the first 32 gate rows of ``w`` are zero: that block of the result is
    ``+-0`` throughout, ``-0.0`` wherever ``up`` is negative."""
    from ddlb_amd.ops.gemm import gemm

    key = (tile, form, M, N, K)
    if key not in _CASES:
        g = torch.Generator(device=DEV).manual_seed(
            7000 + 1009 * FORMS.index(form) + 101 * M + 7 * N + K)
        av, wv = ints((M, K), torch.float32, g), ints((N, K), torch.float32, g)
        if N == ZERO_GATE_N:
            wv[:32] = 0
        kw = {}
        if form in ("mxfp8", "mxfp4"):
            kw = dict(a_scale=_scale_bytes(M, K, g), w_scale=_scale_bytes(N, K, g))
        a, w = _typed(av, form), _typed(wv, form)
        c = gemm(a, w, out_dtype=torch.float32, tile=tile, **kw)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(c).all())
        _CASES[key] = (a, w, kw, c)
    return _CASES[key]


def _expected(c, act):
    """``act(c[gate]) * c[up]`` in torch f32 for the two exact activations."""
    M, N = c.shape
    v = c.reshape(M, N // 64, 2, 32)
    gate = torch.relu(v[:, :, 0]) if act == "relu" else v[:, :, 0]
    return (gate * v[:, :, 1]).reshape(M, N // 2)


def _qviews(fmt, M, F, pad=32, spad=8, extra=3):
    """Sentinel-filled buffers and the (out, out_scale) views into them for ``F`` output columns:
    ldc > F, a scale pitch greater than F / 32, extra rows."""
    ncol = F if fmt == "mx" else F // 2
    qb = torch.full((M + extra, ncol + pad), SENT, dtype=torch.uint8, device=DEV)
    sb = torch.full((M + extra, F // 32 + spad), SENT, dtype=torch.uint8, device=DEV)
    return qb, sb, qb[:M, :ncol].view(FP8 if fmt == "mx" else FP4), sb[:M, :F // 32]


def _untouched_bytes(buf, M, ncol):
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    mask[:M, :ncol] = False
    bad = int((buf[mask] != SENT).sum())
    assert bad == 0, f"{bad} bytes outside the [{M}, {ncol}] view were written"


def _same(q, s, q_ref, s_ref, what=""):
    assert q.dtype == q_ref.dtype and s.dtype == torch.uint8
    assert tuple(q.shape) == tuple(q_ref.shape) and tuple(s.shape) == tuple(s_ref.shape)
    assert torch.equal(s, s_ref), f"{what}: {int((s != s_ref).sum())} scale bytes differ"
    bad = int((_bytes(q) != _bytes(q_ref)).sum())
    assert bad == 0, f"{what}: {bad} data bytes differ"


# ------------------------------------------------------------------ 1. exact, dense
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tile", TILES)
def test_exact_dense(tile, form):
    """act in (none, relu) x every dense output of the form, ragged M, N from one 64-row group
    to a half-empty 128-column and a quarter-filled 256-column tile (320), two K-tile counts;
    outputs as views of sentinel-filled buffers with ldc > N / 2 and extra rows."""
    from ddlb_amd.ops.gemm import gemm

    for M, N, K in itertools.product(MS, (64, 128, 320, 512), _ks(form)):
        a, w, kw, c = _case(tile, form, M, N, K)
        for act in ("none", "relu"):
            want32 = _expected(c, act)
            for odt in DENSE[form]:
                buf, out = sentinel_out(M, N // 2, odt, pad_cols=4)
                got = gemm(a, w, out, tile=tile, act=act, glu=True, **kw)
                torch.cuda.synchronize()
                assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (M, N // 2)
                assert torch.equal(got, want32.to(odt)), (M, N, K, act, odt)
                untouched(buf, M, N // 2)
    # allocated by gemm(): dense rows, the form's default output, `auto` lands on an offered tile
    got = gemm(a, w, act="relu", glu=True, **kw)
    torch.cuda.synchronize()
    assert got.is_contiguous() and got.dtype == DENSE[form][0]
    c_auto = gemm(a, w, out_dtype=torch.float32, **kw)
    assert torch.equal(got, _expected(c_auto, "relu").to(got.dtype))


# ------------------------------------------------------------------ 2. exact, quantised
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tile", TILES)
def test_exact_quantised(tile, form, fmt):
    """The reference quantiser on the expected f32 of test 1, data and scales byte for byte,
    outputs as views of sentinel-filled buffers (ldc > N / 2, a wider scale pitch, extra rows).
    The N = 512 cases hold a block of ``+-0`` (zero gate rows): ``-0.0`` elements in an all-zero
    block, whose bytes the reference quantiser specifies."""
    from ddlb_amd.ops.gemm import gemm

    Ns = (256, 512, 768) if fmt == "mx" else (512, 1024)
    seen_negative_zero = seen_zero_block = False
    for M, N, K in itertools.product(MS, Ns, _ks(form)):
        a, w, kw, c = _case(tile, form, M, N, K)
        F = N // 2
        for act in ("none", "relu"):
            want32 = _expected(c, act)
            if N == ZERO_GATE_N and act == "relu":
                blk = want32[:, :32]
                assert bool((blk == 0).all())
                seen_zero_block = True
                seen_negative_zero |= bool(torch.signbit(blk).any())
                # relu(g) = 0 against u < 0 elsewhere too
                assert bool((torch.signbit(want32) & (want32 == 0))[:, 32:].any())
            q_ref, s_ref = _qref(fmt)(want32)
            qb, sb, out, out_scale = _qviews(fmt, M, F)
            q, s = gemm(a, w, out, tile=tile, act=act, glu=True, out_quant=fmt,
                        out_scale=out_scale, **kw)
            torch.cuda.synchronize()
            assert q.data_ptr() == out.data_ptr() and s.data_ptr() == out_scale.data_ptr()
            _same(q, s, q_ref, s_ref, f"{(M, N, K, act)}")
            _untouched_bytes(qb, M, out.shape[1])
            _untouched_bytes(sb, M, F // 32)
    assert seen_negative_zero and seen_zero_block
    # allocated by gemm(): [M, N / 2] (fp4: N / 4 bytes) data, [M, N / 64] scales, tile auto
    q, s = gemm(a, w, act="relu", glu=True, out_quant=fmt, **kw)
    torch.cuda.synchronize()
    assert q.is_contiguous() and s.is_contiguous() and tuple(s.shape) == (M, N // 64)
    assert tuple(q.shape) == (M, N // 2 if fmt == "mx" else N // 4)
    c_auto = gemm(a, w, out_dtype=torch.float32, **kw)
    _same(q, s, *_qref(fmt)(_expected(c_auto, "relu")), "auto")


# ------------------------------------------------------------------ 3. silu / gelu
def _random_operands(form, M, N, K, g):
    """Random operands of a form -> (a, w, kw): bf16 / f16 values, or their MX quantisation."""
    from ddlb_amd.ops.mx import quantize_mx, quantize_mxfp4

    a = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g, device=DEV) / 8).to(torch.bfloat16)
    if form == "bf16":
        return a, w, {}
    if form == "f16":
        return a.to(torch.float16), w.to(torch.float16), {}
    (aq, sa), (wq, sw) = (quantize_mx if form == "mxfp8" else quantize_mxfp4)(a), \
        (quantize_mx if form == "mxfp8" else quantize_mxfp4)(w)
    return aq, wq, dict(a_scale=sa, w_scale=sw)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("act", ("silu", "gelu"))
@pytest.mark.parametrize("form", FORMS)
def test_silu_gelu_quantised_equals_quantised_dense(form, act, fmt):
    """The dense and the quantising gated epilogue run the same text up to the multiply: the
    fused (q, s) are the reference quantiser's bytes on the same tile's dense f32 GLU output."""
    from ddlb_amd.ops.gemm import gemm

    g = torch.Generator(device=DEV).manual_seed(32)
    M, N, K = 130, 512, 256
    a, w, kw = _random_operands(form, M, N, K, g)
    for tile in ("128x128", "256x128"):
        h = gemm(a, w, out_dtype=torch.float32, tile=tile, act=act, glu=True, **kw)
        torch.cuda.synchronize()
        assert tuple(h.shape) == (M, N // 2) and bool(torch.isfinite(h).all())
        assert float(h.min()) < 0 < float(h.max())
        q_ref, s_ref = _qref(fmt)(h)
        q, s = gemm(a, w, tile=tile, act=act, glu=True, out_quant=fmt, **kw)
        torch.cuda.synchronize()
        _same(q, s, q_ref, s_ref, tile)


@pytest.mark.parametrize("act", ("silu", "gelu"))
@pytest.mark.parametrize("form", FORMS)
def test_silu_gelu_dense_against_the_torch_specification(form, act):
    """Dense 16-bit GLU output against ``glu_reference`` on the ungated f32 product, with the
    bound of the existing activation test (tests/test_gemm_gpu.py). Integer operands scaled by
    2^-4 each (the block-scaled forms: through their scale bytes), so ``|gate|`` stays within a
    few units and the absolute part of the bound does not swallow the result."""
    from ddlb_amd.ops.gemm import gemm, glu_reference

    g = torch.Generator(device=DEV).manual_seed(33)
    M, N, K = 130, 320, 256
    av, wv = ints((M, K), torch.float32, g), ints((N, K), torch.float32, g)
    if form in ("mxfp8", "mxfp4"):
        a, w = _typed(av, form), _typed(wv, form)
        kw = dict(a_scale=_scale_bytes(M, K, g, centre=123, spread=1),
                  w_scale=_scale_bytes(N, K, g, centre=123, spread=1))
    else:
        a, w, kw = _typed(av / 16, form), _typed(wv / 16, form), {}
    odt = torch.float16 if form == "f16" else torch.bfloat16
    for tile in ("128x128", "128x256"):
        c = gemm(a, w, out_dtype=torch.float32, tile=tile, **kw)
        want = glu_reference(c, act)
        got = gemm(a, w, out_dtype=odt, tile=tile, act=act, glu=True, **kw)
        torch.cuda.synchronize()
        gate = c.reshape(M, N // 64, 2, 32)[:, :, 0]
        err = float((got.float() - want).abs().max())
        print(f"{form} {act} {tile}: max|gate| {float(gate.abs().max()):.3g}, max|want| "
              f"{float(want.abs().max()):.3g}, max|err| {err:.3g}")
        assert 0.5 < float(gate.abs().max()) < 8
        torch.testing.assert_close(got.float(), want, rtol=0.02, atol=0.05)


# ------------------------------------------------------------------ 4. the gated MLP
@pytest.mark.parametrize("fused", (True, False))
@pytest.mark.parametrize("fmt", FMTS)
def test_gated_mx_mlp(fmt, fused):
    from ddlb_amd.models.mx_mlp import MxMLP
    from ddlb_amd.ops.gemm import unpack_glu

    mlp = MxMLP(hidden=256, ffn=512, seq=130, act="silu", fmt=fmt, fused=fused, gated=True)
    assert tuple(mlp.W1.shape) == (1024, 256) and tuple(mlp.w1q.shape)[0] == 1024
    assert mlp.flops == 6.0 * 130 * 256 * 512
    gate, up = unpack_glu(mlp.W1)
    assert not torch.equal(gate, up)
    y = mlp.forward().clone()
    torch.cuda.synchronize()
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (130, 256)
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    mlp.validate(y)
    y2 = mlp.forward()
    torch.cuda.synchronize()
    assert torch.equal(y, y2)


# ------------------------------------------------------------------ 5. repeat screen
@pytest.mark.parametrize("fmt", FMTS)
def test_two_runs_write_identical_bytes(fmt):
    from ddlb_amd.ops.gemm import gemm

    a, w, kw, _ = _case("128x128", "mxfp8", 257, 512, 384)
    runs = []
    for _ in range(2):
        qb, sb, out, out_scale = _qviews(fmt, 257, 256)
        gemm(a, w, out, tile="128x128", act="relu", glu=True, out_quant=fmt,
             out_scale=out_scale, **kw)
        torch.cuda.synchronize()
        runs.append((qb, sb))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert bool((runs[0][0][:257, :8] != SENT).any())


# ------------------------------------------------------------------ 6. refusals of the entry
def test_native_entry_refuses_and_launches_nothing():
    """``gemm_launch`` itself refuses what Python would (argument inspection only): the sentinel
    bytes survive; the supported call then runs."""
    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import DT_BF16, DT_F32, DT_FP8, TILES as CODES

    C = load()
    M, N, K = 256, 512, 256
    a = torch.ones(M, K, device=DEV, dtype=torch.bfloat16)
    w = torch.ones(N, K, device=DEV, dtype=torch.bfloat16)
    a8, w8, af, wf = a.to(FP8), w.to(FP8), a.float(), w.float()
    q = torch.full((M, N // 2), SENT, dtype=torch.uint8, device=DEV)
    s = torch.full((M, N // 64), SENT, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(x=a, y=w, din=DT_BF16, dout=DT_FP8, tile="auto", mode=0, ksplit=1, n=N, ldc=N // 2,
             a_grp=0, c_grp=0, cs=None, cs_ld=N // 64):
        C.gemm(x.data_ptr(), y.data_ptr(), q.data_ptr(), K, K, ldc, M, n, K, din, dout,
               CODES[tile], mode, a_grp, a_grp, c_grp, c_grp, st, 0, ksplit, 0, 0, 0, 0,
               s.data_ptr() if cs is None else cs, cs_ld, 1)

    bad = [
        dict(n=N - 128), dict(n=N - 64),              # N % 256
        dict(ldc=N // 2 - 16),                        # ldc < N / 2
        dict(cs_ld=N // 64 - 4),                      # a short scale pitch
        dict(cs=0),                                   # quantised dout without output scales
        dict(dout=DT_BF16),                           # output scales with a dense dout
        dict(x=af, y=wf, din=DT_F32),                 # f32 operands
        dict(x=a8, y=w8, din=DT_FP8),                 # unit-scale fp8
        dict(tile="pt4"), dict(tile="t8"), dict(tile="256x256"), dict(tile="i128"),
        dict(mode=1), dict(ksplit=2), dict(a_grp=64), dict(c_grp=64),
    ]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((q == SENT).all()) and bool((s == SENT).all())
    call()
    torch.cuda.synchronize()
    # gate = up = K = 256, product 2^16 = 0.5 * 2^17: e = 17 - 9, 2^16 / 2^8 = 256 -> byte 0x78
    assert bool((s == 135).all()) and bool((q == 0x78).all())
