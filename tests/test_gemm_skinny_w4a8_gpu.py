"""Skinny-M GEMM, MX-fp8 ``a`` on MXFP4 ``w`` (W4A8), on the GPU. Integers in -3..3 are exact in
e4m3 and in E2M1, so under power-of-two scales every sum is exact in f32: ``torch.equal`` to fp64
arithmetic on the dequantised operands, whatever the K-split. A K-tile is W's: 256 elements."""

import pytest
import torch

from _exact import (FP8, classes64, dequant64, exact_scaled, nan_padded, same, sentinel_out,
                    untouched)
from ddlb_amd.models.mx_mlp import MxMLP
from ddlb_amd.models.mx_moe import MxMoE
from ddlb_amd.ops import gemm as G
from ddlb_amd.ops import mx
from test_gemm_skinny_fused_gpu import _holds, _qviews
from test_gemm_skinny_gpu import BF16, DEV, F16, F32, STRIP, _case as _fp8_case, _pack, _run

pytestmark = pytest.mark.gpu
U8 = torch.uint8
BASE = dict(out=BF16, M=17, N=STRIP + 24, kt=5, ks=2)
AXES = dict(out=(F16, F32), M=(1, 16, 33, 65), N=(7, STRIP), ks=(1, 5, "auto"), kt=(9,))
CASES = [BASE] + [dict(BASE, **{k: v}) for k, vs in AXES.items() for v in vs] + \
    [dict(BASE, M=33, kt=9, ks=1)]


def _case(M, N, kt, centre=None):
    """``(a, w, s_a, s_w, a8, w8)``: the fp8 case of ``2 kt`` fp8 K-tiles (``extreme_scales``, or
    ``centre`` +- 2) with ``w`` packed again as E2M1 pairs; ``a8``, ``w8`` for the reference."""
    a, _, s_a, s_w, a8, w8 = _fp8_case("mx", M, N, 2 * kt, centre)
    return a, _pack(w8.float(), "mxfp4"), s_a, s_w, a8, w8


@pytest.mark.parametrize("b", range(8))
def test_one_block_at_a_time(b):
    """The K map of the mixed MFMA: operands non-zero in block ``b`` of the one K-tile only, the
    eight scale bytes of every row all different. A wrong map is a wrong value in this block."""
    _, _, s_a, s_w, a8, w8 = _case(16, 16, 1)
    assert all(len(set(r)) == 8 for s in (s_a, s_w) for r in s.tolist())
    keep = torch.zeros(256, device=DEV)
    keep[32 * b:32 * b + 32] = 1
    a8, w8 = (a8.float() * keep).to(FP8), (w8.float() * keep).to(FP8)
    out = _run(a8, _pack(w8.float(), "mxfp4"), s_a, s_w, F32, ksplit=1)
    assert torch.equal(out, exact_scaled(a8, w8, s_a, s_w).to(F32))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v).split(".")[-1]
                                                               for v in c.values()))
def test_exact_on_integers(case):
    a, w, s_a, s_w, a8, w8 = _case(case["M"], case["N"], case["kt"])
    out = _run(a, w, s_a, s_w, case["out"], ksplit=case["ks"])
    assert torch.equal(out, exact_scaled(a8, w8, s_a, s_w).to(F32).to(case["out"]))


@pytest.mark.parametrize("ks", (1, 3))
@pytest.mark.parametrize("glu", (False, True), ids=("dense", "glu"))
def test_six_strips(glu, ks):
    """Six workgroups along N: ``N = 5 STRIP + 1`` (the last strip one weight row), and gated at
    ``N = 6 STRIP``."""
    N = 6 * STRIP if glu else 5 * STRIP + 1
    a, w, s_a, s_w, a8, w8 = _case(17, N, 3, centre=127)
    want = exact_scaled(a8, w8, s_a, s_w).to(F32)
    if not glu:
        assert torch.equal(_run(a, w, s_a, s_w, F32, ksplit=ks), want)
        return
    buf, out = sentinel_out(17, N // 2, F32)
    G.gemm_skinny(a, w, out, a_scale=s_a, w_scale=s_w, ksplit=ks, glu=True)
    assert torch.equal(out, G.glu_reference(want))
    untouched(buf, 17, N // 2)


@pytest.mark.parametrize("ks", (1, 2))
@pytest.mark.parametrize("raw", ([2, 2, 5, 22, 22, 23], [2, -7, 5, 22, 9, 999]),
                         ids=("sorted", "garbage"))
def test_grouped_equals_dense_per_group(raw, ks):
    """E = 5, sizes (0, 3, 17, 0, 1) from row 2 of T = 24; garbage clamps to (0, 3, 17, 0, 2)."""
    T, N, E = 24, STRIP + 24, 5
    a, s_a = _case(T, N, 5)[0], _case(T, N, 5)[2]
    ws = [_case(T, N + e, 5) for e in range(E)]
    w = torch.stack([G._as_bytes(c[1][:N]) for c in ws]).view(ws[0][1].dtype)
    s_w = torch.stack([c[3][:N] for c in ws])
    offs = torch.tensor(raw, dtype=torch.int32, device=DEV)
    o = G.clamp_offsets(offs, T)
    buf, out = sentinel_out(T, N, BF16)
    G.gemm_skinny_grouped(a, w, offs, out, a_scale=s_a, w_scale=s_w, ksplit=ks)
    untouched(buf, T, N, rows=slice(o[0], o[-1]))
    for e in (e for e in range(E) if o[e + 1] > o[e]):
        r = slice(o[e], o[e + 1])
        assert torch.equal(out[r], G.gemm_skinny(a[r], w[e], a_scale=s_a[r], w_scale=s_w[e],
                                                 ksplit=ks)), e


@pytest.mark.parametrize("ks", (1, 2))
@pytest.mark.parametrize("glu,q,N", [(True, None, 64), (False, "mx", 128), (False, "mxfp4", 256),
                                     (True, "mx", 256), (True, "mxfp4", 512)])
def test_fused_epilogues(glu, q, N, ks):
    """Byte for byte the chain: the f32 output of the same operands, ``glu_reference``, the row
    quantiser's specification."""
    a, w, s_a, s_w, _, _ = _case(17, N, 5)
    c = _run(a, w, s_a, s_w, F32, ksplit=ks)
    kw = dict(a_scale=s_a, w_scale=s_w, ksplit=ks, glu=glu, act="relu" if glu else "none")
    want = G.glu_reference(c, "relu") if glu else c
    if q is None:
        buf, out = sentinel_out(17, N // 2, F32)
        assert torch.equal(G.gemm_skinny(a, w, out, **kw), want)
        return untouched(buf, 17, N // 2)
    ref = getattr(mx, f"quantize_{q}_reference")(want)
    bufs, views = _qviews(q, 17, want.shape[1])  # sentinel buffers, larger pitches
    G.gemm_skinny(a, w, out_quant=q, **views, **kw)
    _holds(bufs, slice(0, 17), ref)


@pytest.mark.parametrize("ks", (1, 2))
def test_padding_and_non_finite(ks):
    """Poisoned padding around all four tensors changes nothing; a NaN byte in ``a`` reaches
    exactly its output row and a scale byte 255 in ``w_scale`` exactly its output column."""
    a, w, s_a, s_w, a8, w8 = _case(17, STRIP + 24, 5)
    out = _run(nan_padded(a), nan_padded(w, "fp4"), nan_padded(s_a, "scale"),
               nan_padded(s_w, "scale"), F32, ksplit=ks)
    assert torch.equal(out, exact_scaled(a8, w8, s_a, s_w).to(F32))
    a, w, s_a, s_w, _, w8 = (t.clone() for t in _case(17, STRIP + 24, 5, centre=127))
    a.view(U8)[1, 0] = 0x7F
    s_w[9, 0] = 255
    want = classes64(dequant64(a, s_a), dequant64(w8, s_w.clamp(max=129)))
    want[:, 9] = float("nan")
    assert int(torch.isnan(want).sum()) == 17 + want.shape[1] - 1  # row 1 and column 9 only
    same(_run(a, w, s_a, s_w, F32, ksplit=ks), want.float())


@pytest.mark.parametrize("model", ("mlp", "mlp-gated", "moe"))
def test_models(model):
    """``fmt="w4a8"`` against ``reference_chain`` under the skinny model tests' bound
    (``validate``: ``atol = 1e-3 ffn``); ``MxMoE`` is gated by construction."""
    kw = dict(hidden=256, ffn=256, seq=12, fmt="w4a8", kernel="skinny")
    m = MxMoE(experts=4, dispatch="native", top_k=2, **kw) if model == "moe" else \
        MxMLP(act="silu", gated=model == "mlp-gated", **kw)
    assert m.w1q.dtype == torch.float4_e2m1fn_x2 and m.w1q.shape[-1] == 128
    y = m.forward().clone()
    m.validate(y)
    assert torch.equal(y, m.forward())
