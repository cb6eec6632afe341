"""Skinny-M GEMM with the gated (``glu``) and MX-quantising (``out_quant``) epilogues on the GPU.
Integer operands in -3..3 under scale bytes 127 +- 2 make every f32 sum exact whatever the K-split:
fp64 arithmetic, ``glu_reference`` in torch f32, one rounding or the reference quantiser; bytes."""

import pytest
import torch

from _exact import FP8, classes64, dequant64, exact_scaled, ints, sentinel_out, untouched
from ddlb_amd.ops import gemm as G
from ddlb_amd.ops import mx

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32, U8 = torch.bfloat16, torch.float16, torch.float32, torch.uint8
FMTS = ("mx", "mxfp4")
KTILE = {"mx": 128, "mxfp4": 256}
QREF = {"mx": mx.quantize_mx_reference, "mxfp4": mx.quantize_mxfp4_reference}
STRIP = G.SKINNY_STRIP
SENT = 0xA5
BASE = dict(out=BF16, M=17, N=STRIP + 64, kt=5, ks=2)
AXES = dict(M=(1, 16, 64, 65), N=(64, 2 * STRIP), ks=(1, 5, "auto"), out=(F16, F32))
CASES = [BASE] + [dict(BASE, **{k: v}) for k, vs in AXES.items() for v in vs] + \
    [dict(BASE, M=64, ks=1)]
QUANT = [(True, "mx", 256), (True, "mx", 512), (True, "mxfp4", 512),
         (False, "mx", 128), (False, "mx", 384), (False, "mxfp4", 256)]
_MADE = {}


def _case(fmt, M, N, kt, centre=127, spread=2, zero_gate=False):
    """``(a, w, scales as keywords, a8, w8)``: operands in ``fmt``, scale bytes ``centre +-
    spread``, the same integers as e4m3; ``zero_gate``: the first 32 (gate) rows of ``w`` are 0."""
    key = (fmt, M, N, kt, centre, spread, zero_gate)
    if key not in _MADE:
        K = kt * KTILE[fmt]
        g = torch.Generator(device=DEV).manual_seed(23 + 1009 * M + 31 * N + K)
        vs = [ints((M, K), F32, g), ints((N, K), F32, g)]
        vs[1][:32 if zero_gate else 0] = 0
        kw = {n: (centre + torch.randint(-spread, spread + 1, (r, K // 32), generator=g,
                                         device=DEV)).to(U8) for n, r in (("a_scale", M),
                                                                          ("w_scale", N))}
        code = torch.tensor((0, 2, 4, 5), device=DEV)
        a, w = (v.to(FP8) if fmt == "mx" else
                mx.pack_e2m1(code[v.abs().long()] | ((v < 0).long() << 3)) for v in vs)
        _MADE[key] = (a, w, kw, vs[0].to(FP8), vs[1].to(FP8))
    return _MADE[key]


def _want(a8, w8, kw, glu, act):
    c = exact_scaled(a8, w8, kw["a_scale"], kw["w_scale"]).to(F32)
    return G.glu_reference(c, act) if glu else torch.relu(c) if act == "relu" else c


def _qviews(fmt, M, F):
    """Sentinel buffers and the (out, out_scale) views: larger pitches, extra rows."""
    ncol = F if fmt == "mx" else F // 2
    qb, sb = (torch.full((M + 3, c), SENT, dtype=U8, device=DEV) for c in (ncol + 32, F // 32 + 8))
    return (qb, sb), dict(out=qb[:M, :ncol].view(G.out_quant_dtype(fmt)),
                          out_scale=sb[:M, :F // 32])


def _holds(bufs, rows, ref, what=""):
    """Each sentinel buffer holds its reference's bytes in ``rows`` and the sentinel elsewhere."""
    for buf, r in zip(bufs, ref):
        want = torch.full_like(buf, SENT)
        want[rows, :r.shape[1]] = r.view(U8)[rows]
        assert torch.equal(buf, want), f"{what}: {int((buf != want).sum())} bytes differ"


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v).split(".")[-1]
                                                               for v in c.values()))
@pytest.mark.parametrize("fmt", FMTS)
def test_exact_dense_gated(fmt, case):
    M, N, odt = case["M"], case["N"], case["out"]
    a, w, kw, a8, w8 = _case(fmt, M, N, case["kt"])
    for act in ("none", "relu"):
        buf, out = sentinel_out(M, N // 2, odt)
        assert G.gemm_skinny(a, w, out, glu=True, act=act, ksplit=case["ks"], **kw) is out
        assert torch.equal(out, _want(a8, w8, kw, True, act).to(odt)), act
        untouched(buf, M, N // 2)


@pytest.mark.parametrize("ks", (1, 2))
@pytest.mark.parametrize("M", (1, 17, 64))
@pytest.mark.parametrize("glu,q,N", QUANT)
@pytest.mark.parametrize("fmt", FMTS)
def test_exact_quantised(fmt, glu, q, N, M, ks):
    a, w, kw, a8, w8 = _case(fmt, M, N, 5, zero_gate=glu and N == 512)
    for act in ("none", "relu"):
        want = _want(a8, w8, kw, glu, act)
        if glu and N == 512 and act == "relu":  # a block of +-0
            assert bool((want[:, :32] == 0).all())
        bufs, views = _qviews(q, M, want.shape[1])
        got = G.gemm_skinny(a, w, glu=glu, act=act, ksplit=ks, out_quant=q, **views, **kw)
        assert got[0].data_ptr() == bufs[0].data_ptr() and got[1].data_ptr() == bufs[1].data_ptr()
        _holds(bufs, slice(0, M), QREF[q](want), act)


@pytest.mark.parametrize("ks", (1, 2))
@pytest.mark.parametrize("raw", ([2, 2, 5, 22, 22, 23], [2, -7, 5, 22, 9, 999]),
                         ids=("sorted", "garbage"))
@pytest.mark.parametrize("fmt", FMTS)
def test_grouped_equals_dense_per_group(fmt, raw, ks):
    T, N, E = 24, 256 if fmt == "mx" else 512, 5  # (an MXFP4 output takes N / 2 % 256 == 0)
    a, a_s = _case(fmt, T, N, 5)[0], _case(fmt, T, N, 5)[2]["a_scale"]
    ws = [_case(fmt, T, N + 64 * e, 5) for e in range(E)]
    w = torch.stack([G._as_bytes(c[1][:N]) for c in ws]).view(a.dtype)
    s_w = torch.stack([c[2]["w_scale"][:N] for c in ws])
    offs = torch.tensor(raw, dtype=torch.int32, device=DEV)
    o = G.clamp_offsets(offs, T)
    bufs, views = _qviews(fmt, T, N // 2)
    kw = dict(ksplit=ks, glu=True, act="relu", out_quant=fmt)
    G.gemm_skinny_grouped(a, w, offs, a_scale=a_s, w_scale=s_w, **views, **kw)
    ref = [torch.zeros_like(v.view(U8)) for v in views.values()]
    for e in range(E):
        if o[e + 1] > o[e]:
            r = slice(o[e], o[e + 1])
            for t, d in zip(ref, G.gemm_skinny(a[r], w[e], a_scale=a_s[r], w_scale=s_w[e], **kw)):
                t[r] = d.view(U8)
    _holds(bufs, slice(o[0], o[-1]), ref)


@pytest.mark.parametrize("ks", (1, 2))
@pytest.mark.parametrize("act", ("silu", "gelu"))
@pytest.mark.parametrize("fmt", FMTS)
def test_silu_gelu(fmt, act, ks):
    """Random quantised operands: the fused (q, s) against the reference quantiser on the same
    call's f32 output. Integers under scale bytes around 123: the bf16 gated output within the
    tiled GLU test's bound of ``glu_reference`` on the ungated f32 product."""
    M, N, K = 40, 512, 1024
    g = torch.Generator(device=DEV).manual_seed(32)
    quant = mx.quantize_mx if fmt == "mx" else mx.quantize_mxfp4
    (a, s_a), (w, s_w) = (quant((torch.randn(r, K, generator=g, device=DEV) * sc).to(BF16))
                          for r, sc in ((M, 1.0), (N, 0.125)))
    kw = dict(a_scale=s_a, w_scale=s_w, ksplit=ks, glu=True, act=act)
    h = G.gemm_skinny(a, w, out_dtype=F32, **kw)
    assert bool(torch.isfinite(h).all()) and float(h.min()) < 0 < float(h.max())
    for got, ref in zip(G.gemm_skinny(a, w, out_quant=fmt, **kw), QREF[fmt](h)):
        assert torch.equal(got.view(U8), ref.view(U8))
    a, w, kw, _, _ = _case(fmt, M, N, K // KTILE[fmt], centre=123, spread=1)
    c = G.gemm_skinny(a, w, out_dtype=F32, ksplit=ks, **kw)
    got = G.gemm_skinny(a, w, out_dtype=BF16, ksplit=ks, glu=True, act=act, **kw)
    assert 0.5 < float(c.reshape(M, N // 64, 2, 32)[:, :, 0].abs().max()) < 8
    torch.testing.assert_close(got.float(), G.glu_reference(c, act), rtol=0.02, atol=0.05)


@pytest.mark.parametrize("ks", (1, 2))
@pytest.mark.parametrize("fmt", FMTS)
def test_non_finite_reach_the_quantised_output(fmt, ks):
    """A NaN byte in A row 1 (fp8) and the scale byte 255 on a block of W gate row 9: the
    affected elements are the format's NaN byte / nibble (either sign), their MXFP4 blocks carry
    the scale byte 255, every other byte is the reference quantiser's."""
    M, N = 17, 256 if fmt == "mx" else 512
    a, w, kw, a8, w8 = _case(fmt, M, N, 8)
    a, kw = a.clone(), {k: v.clone() for k, v in kw.items()}
    if fmt == "mx":
        a.view(U8)[1, 0] = 0x7F
        a8 = a
    kw["w_scale"][9, 0] = 255
    want = classes64(dequant64(a8, kw["a_scale"]), dequant64(w8, kw["w_scale"].clamp(max=129)))
    want[:, 9] = float("nan")
    h = G.glu_reference(want.float())
    nan = torch.isnan(h)
    assert bool(nan[:, 9].all()) and bool(nan[1].all()) == (fmt == "mx") and not bool(nan[2, 8])
    q, s = G.gemm_skinny(a, w, ksplit=ks, glu=True, out_quant=fmt, **kw)
    q_ref, s_ref = QREF[fmt](h)
    assert torch.equal(s, s_ref) and bool((s_ref == 255).any()) == (fmt == "mxfp4")
    b, b_ref = q.view(U8), q_ref.view(U8)
    if fmt == "mxfp4":  # nibbles, element 2j in the low one
        b, b_ref = (torch.stack((t & 15, t >> 4), dim=2).reshape(M, N // 2) for t in (b, b_ref))
    code = 0x7 if fmt == "mxfp4" else 0x7F
    assert bool(((b & code) == code)[nan].all()) and torch.equal(b[~nan], b_ref[~nan])


@pytest.mark.parametrize("fmt", FMTS)
def test_models_on_the_fused_fc1(fmt):
    from ddlb_amd.models.mx_mlp import MxMLP
    from ddlb_amd.models.mx_moe import MxMoE

    kw = dict(hidden=256, ffn=256, seq=12, experts=4, fmt=fmt, kernel="skinny",
              dispatch="native", top_k=2)
    y = MxMoE(fused=True, **kw).forward().clone()
    chain = MxMoE(fused=False, **kw)
    assert torch.equal(y, chain.forward())
    chain.validate(y)
    for gated in (True, False):
        mlp = MxMLP(hidden=256, ffn=512, seq=16, fmt=fmt, act="silu", gated=gated,
                    kernel="skinny")
        y = mlp.forward().clone()
        mlp.validate(y)
        assert torch.equal(y, mlp.forward())
