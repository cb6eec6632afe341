"""Skinny-M GEMM for bf16 / f16 activations (``gemm_skinny_a16``) on the GPU: MXFP4, MX-fp8 and
16-bit weights against fp64 arithmetic on the dequantised weights. Integers in -3..3 are exact in
every format here and the scale bytes are powers of two inside the activation dtype's normal
range, so every weight converts exactly and every sum is exact in f32: ``torch.equal``."""

import pytest
import torch

from _exact import FP8, classes64, dequant64, ints, nan_padded, same, sentinel_out, untouched
from ddlb_amd.models.mx_mlp import MxMLP
from ddlb_amd.models.mx_moe import MxMoE
from ddlb_amd.ops import gemm as G
from test_gemm_skinny_gpu import BF16, DEV, F16, F32, STRIP, _pack

pytestmark = pytest.mark.gpu
U8 = torch.uint8
KTILE = {"mxfp4": 256, "mx": 128, "same": 64}
forms = pytest.mark.parametrize("wfmt", tuple(KTILE))
dtypes = pytest.mark.parametrize("dt", (BF16, F16), ids=("bf16", "f16"))
BASE = dict(out=None, M=17, N=STRIP + 24, kt=5, ks=2)
AXES = dict(out=(F32,), M=(1, 16, 33, 65), N=(7, STRIP), ks=(1, 5, "auto"), kt=(9,))
CASES = [BASE] + [dict(BASE, **{k: v}) for k, vs in AXES.items() for v in vs]
_MADE = {}


def _case(wfmt, dt, M, N, kt):
    """``(a, w, s_w, wd)``: ``a`` in ``dt``, ``w`` in its form with scale bytes 125 .. 129 (none
    for ``"same"``) and ``wd``, the dequantised weight in fp64."""
    key = (wfmt, dt, M, N, kt)
    if key not in _MADE:
        K = kt * KTILE[wfmt]
        g = torch.Generator(device=DEV).manual_seed(7 + 1009 * M + 31 * N + K)
        av, wv = ints((M, K), F32, g), ints((N, K), F32, g)
        s = torch.randint(125, 130, (N, K // 32), generator=g, device=DEV).to(U8)
        if wfmt == "same":
            _MADE[key] = (av.to(dt), wv.to(dt), None, wv.double())
        else:
            _MADE[key] = (av.to(dt), _pack(wv, wfmt), s, dequant64(wv.to(FP8), s))
    return _MADE[key]


def _run(a, w, s_w, odt=None, **kw):
    cols = w.shape[0] // 2 if kw.get("glu") else w.shape[0]
    buf, out = sentinel_out(a.shape[0], cols, odt or a.dtype)
    assert G.gemm_skinny_a16(a, w, out, w_scale=s_w, **kw) is out
    untouched(buf, a.shape[0], cols)
    return out


@pytest.mark.parametrize("b", range(8))
@dtypes
@forms
def test_one_block_at_a_time(wfmt, dt, b):
    """The K map of the expansion: operands non-zero in eighth ``b`` of the one K-tile only (one
    fp4 block, half an fp8 block, one 16-bit chunk), every row's scale bytes all different and,
    for bf16, far apart. A wrong map or chunk / scale pairing is a wrong value."""
    K = KTILE[wfmt]
    g = torch.Generator(device=DEV).manual_seed(b)
    keep = torch.zeros(K, device=DEV)
    keep[K // 8 * b:K // 8 * (b + 1)] = 1
    a, wv = (ints((16, K), F32, g) * keep).to(dt), ints((16, K), F32, g) * keep
    if wfmt == "same":
        w, s, wd = wv.to(dt), None, wv.double()
    else:
        spread = torch.tensor((30, 60, 90, 118, 127, 150, 190, 220) if dt == BF16 else
                              tuple(range(122, 130)), device=DEV)
        s = torch.stack([spread[torch.randperm(8, generator=g, device=DEV)][:K // 32]
                         for _ in range(16)]).to(U8)
        w, wd = _pack(wv, wfmt), dequant64(wv.to(FP8), s)
    assert torch.equal(_run(a, w, s, F32, ksplit=1), (a.double() @ wd.t()).to(F32))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v).split(".")[-1]
                                                               for v in c.values()))
@dtypes
@forms
def test_exact_on_integers(wfmt, dt, case):
    a, w, s, wd = _case(wfmt, dt, case["M"], case["N"], case["kt"])
    out = _run(a, w, s, case["out"], ksplit=case["ks"])
    assert torch.equal(out, (a.double() @ wd.t()).to(F32).to(out.dtype))


@pytest.mark.parametrize("ks", (1, 3))
@pytest.mark.parametrize("glu", (False, True), ids=("dense", "glu"))
@dtypes
@forms
def test_six_strips(wfmt, dt, glu, ks):
    """Six workgroups along N: ``N = 5 STRIP + 1`` (the last strip one weight row), and gated at
    ``N = 6 STRIP`` against ``glu_reference`` of the exact f32 product."""
    a, w, s, wd = _case(wfmt, dt, 17, 6 * STRIP if glu else 5 * STRIP + 1, 5)
    want = (a.double() @ wd.t()).to(F32)
    out = _run(a, w, s, F32, ksplit=ks, glu=glu)
    assert torch.equal(out, G.glu_reference(want) if glu else want)


@pytest.mark.parametrize("ks", (1, 2))
@pytest.mark.parametrize("raw", ([2, 2, 5, 22, 22, 23], [2, -7, 5, 22, 9, 999]),
                         ids=("sorted", "garbage"))
@dtypes
@forms
def test_grouped_equals_dense_per_group(wfmt, dt, raw, ks):
    """E = 5, sizes (0, 3, 17, 0, 1) from row 2 of T = 24; garbage clamps to (0, 3, 17, 0, 2)."""
    T, N, E = 24, STRIP + 24, 5
    a = _case(wfmt, dt, T, N, 5)[0]
    ws = [_case(wfmt, dt, T, N + e, 5) for e in range(E)]
    w = torch.stack([G._as_bytes(c[1][:N]) for c in ws]).view(ws[0][1].dtype)
    s = None if wfmt == "same" else torch.stack([c[2][:N] for c in ws])
    offs = torch.tensor(raw, dtype=torch.int32, device=DEV)
    o = G.clamp_offsets(offs, T)
    buf, out = sentinel_out(T, N, dt)
    G.gemm_skinny_a16_grouped(a, w, offs, out, w_scale=s, ksplit=ks)
    untouched(buf, T, N, rows=slice(o[0], o[-1]))
    for e in (e for e in range(E) if o[e + 1] > o[e]):
        r = slice(o[e], o[e + 1])
        assert torch.equal(out[r], G.gemm_skinny_a16(a[r], w[e], ksplit=ks,
                                                     w_scale=None if s is None else s[e])), e


@pytest.mark.parametrize("ks", (1, 2))
@pytest.mark.parametrize("N", (64, 256))
@dtypes
@forms
def test_glu(wfmt, dt, N, ks):
    """Byte for byte ``glu_reference`` of the f32 output of the same operands."""
    a, w, s, _ = _case(wfmt, dt, 17, N, 5)
    c = _run(a, w, s, F32, ksplit=ks)
    assert torch.equal(_run(a, w, s, F32, ksplit=ks, glu=True, act="relu"),
                       G.glu_reference(c, "relu"))


@pytest.mark.parametrize("ks", (1, 2))
@dtypes
@forms
def test_padding_and_non_finite(wfmt, dt, ks):
    """NaN-poisoned padding around every tensor changes nothing; a scale byte 255, an e4m3 NaN
    byte and a NaN in ``a`` reach exactly their output column / row."""
    a, w, s, wd = _case(wfmt, dt, 17, STRIP + 24, 5)
    kind = {"mxfp4": "fp4", "mx": None, "same": None}[wfmt]
    out = _run(nan_padded(a), nan_padded(w, kind), None if s is None else nan_padded(s, "scale"),
               F32, ksplit=ks)
    assert torch.equal(out, (a.double() @ wd.t()).to(F32))
    a, w, wd = a.clone(), w.clone(), wd.clone()
    a[1, 0], cols = float("nan"), []
    if s is not None:
        s = s.clone()
        s[9, 0] = 255
        cols.append(9)
    if wfmt == "mx":
        w.view(U8)[2, a.shape[1] // 2] = 0xFF
        cols.append(2)
    if wfmt == "same":
        w[2, a.shape[1] // 2] = float("nan")
        cols.append(2)
    want = classes64(a.double(), wd)
    want[:, cols] = float("nan")
    assert int(torch.isnan(want).sum()) == want.shape[1] + len(cols) * 16
    same(_run(a, w, s, F32, ksplit=ks), want.float())


@pytest.mark.parametrize("model", ("mlp", "mlp-gated", "moe"))
@pytest.mark.parametrize("fmt", ("w4a16", "w8a16"))
def test_models(fmt, model):
    """The weight-only formats against ``reference_chain`` under ``validate``
    (``atol = 1e-3 ffn``); a second forward writes the same bytes."""
    kw = dict(hidden=256, ffn=256, seq=12, fmt=fmt, kernel="skinny")
    m = MxMoE(experts=4, dispatch="native", top_k=2, **kw) if model == "moe" else \
        MxMLP(act="silu", gated=model == "mlp-gated", **kw)
    assert m.w1q.shape[-1] == (128 if fmt == "w4a16" else 256) and m.X.dtype == BF16
    y = m.forward().clone()
    m.validate(y)
    assert torch.equal(y, m.forward())
