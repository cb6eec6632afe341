"""Tiled W4A8 GEMM (MX-fp8 ``a`` on MXFP4 ``w``, prefill shapes) on the GPU. Integers in -3..3 are
exact in e4m3 and in E2M1, so under power-of-two scales every sum is exact in f32: ``torch.equal``
to fp64 arithmetic on the dequantised operands. A K-tile is 128 elements; the skinny W4A8 tests'
case builder counts ``kt`` in 256."""

import pytest
import torch

from _exact import (FP8, classes64, dequant64, exact_scaled, nan_padded, same, sentinel_out,
                    untouched)
from ddlb_amd.models.mx_mlp import MxMLP
from ddlb_amd.models.mx_moe import MxMoE
from ddlb_amd.ops import gemm as G
from ddlb_amd.ops import mx
from test_gemm_skinny_fused_gpu import _holds, _qviews
from test_gemm_skinny_gpu import BF16, DEV, F16, F32, _pack
from test_gemm_skinny_w4a8_gpu import _case

pytestmark = pytest.mark.gpu
TILES = G.W4A8_TILES + ("auto",)
BASE = dict(tile="256x128", M=129, N=130, kt=3, out=BF16, pad=False)
AXES = dict(tile=TILES[1:], M=(1, 257), N=(7, 256), kt=(1, 5), out=(F16, F32), pad=(True,))
CASES = [BASE] + [dict(BASE, **{k: v}) for k, vs in AXES.items() for v in vs]


def _run(a, w, s_a, s_w, odt, **kw):
    cols = w.shape[0] // 2 if kw.get("glu") else w.shape[0]
    buf, out = sentinel_out(a.shape[0], cols, odt)
    assert G.gemm_w4a8(a, w, out, a_scale=s_a, w_scale=s_w, **kw) is out
    untouched(buf, a.shape[0], cols)
    return out


@pytest.mark.parametrize("b", range(8))
def test_one_block_at_a_time(b):
    """K map, lane / scale map, LDS permutations and the stage ring: ``K = 256`` is two K-tiles,
    the operands non-zero in block ``b`` of 8 only, all eight scale bytes of every row different."""
    _, _, s_a, s_w, a8, w8 = _case(16, 16, 1)
    assert all(len(set(r)) == 8 for s in (s_a, s_w) for r in s.tolist())
    keep = torch.zeros(256, device=DEV)
    keep[32 * b:32 * b + 32] = 1
    a8, w8 = (a8.float() * keep).to(FP8), (w8.float() * keep).to(FP8)
    out = _run(a8, _pack(w8.float(), "mxfp4"), s_a, s_w, F32, tile="128x128")
    assert torch.equal(out, exact_scaled(a8, w8, s_a, s_w).to(F32))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v).split(".")[-1]
                                                               for v in c.values()))
def test_exact_on_integers(case):
    a, w, s_a, s_w, a8, w8 = _case(case["M"], case["N"], case["kt"])
    want = exact_scaled(a8, w8, s_a, s_w).to(F32).to(case["out"])
    if case["pad"]:  # larger pitches, NaN bits in the padding of all four tensors
        a, w = nan_padded(a), nan_padded(w, "fp4")
        s_a, s_w = nan_padded(s_a, "scale"), nan_padded(s_w, "scale")
    assert torch.equal(_run(a, w, s_a, s_w, case["out"], tile=case["tile"]), want)


@pytest.mark.parametrize("tile", G.W4A8_TILES)
@pytest.mark.parametrize("glu,q,N", [(False, None, 64), (True, None, 64), (False, "mx", 128),
                                     (True, "mx", 256)])
def test_epilogues(glu, q, N, tile):
    """Byte for byte the chain built from the same operands' f32 output: ``act`` in f32,
    ``glu_reference``, the row quantiser's specification."""
    a, w, s_a, s_w, _, _ = _case(17, N, 3)
    c = _run(a, w, s_a, s_w, F32, tile=tile)
    want = G.glu_reference(c, "relu") if glu else torch.relu(c)
    kw = dict(tile=tile, glu=glu, act="relu")
    if q is None:
        assert torch.equal(_run(a, w, s_a, s_w, F32, **kw), want)
        return
    bufs, views = _qviews(q, 17, want.shape[1])  # sentinel buffers, larger pitches
    G.gemm_w4a8(a, w, a_scale=s_a, w_scale=s_w, out_quant=q, **views, **kw)
    _holds(bufs, slice(0, 17), mx.quantize_mx_reference(want))


@pytest.mark.parametrize("tile", G.W4A8_TILES)
@pytest.mark.parametrize("raw", ([2, 2, 5, 135, 135, 136], [2, -7, 5, 135, 9, 999]),
                         ids=("sorted", "garbage"))
@pytest.mark.parametrize("fused", (False, True), ids=("dense", "glu-mx"))
def test_grouped_equals_dense_per_group(fused, raw, tile):
    """E = 5, sizes (0, 3, 130, 0, 1) from row 2 of T = 140; garbage clamps to (0, 3, 130, 0, 5).
    ``fused``: the gated quantised form, data and scales."""
    T, E, N = 140, 5, 256 if fused else 130
    a, s_a = _case(T, N, 3)[0], _case(T, N, 3)[2]
    ws = [_case(T, N + e, 3) for e in range(E)]
    w = torch.stack([G._as_bytes(c[1][:N]) for c in ws]).view(ws[0][1].dtype)
    s_w = torch.stack([c[3][:N] for c in ws])
    offs = torch.tensor(raw, dtype=torch.int32, device=DEV)
    o = G.clamp_offsets(offs, T)
    live = [e for e in range(E) if o[e + 1] > o[e]]
    kw = dict(tile=tile, glu=True, act="relu", out_quant="mx") if fused else dict(tile=tile)
    if not fused:
        buf, out = sentinel_out(T, N, BF16)
        G.gemm_w4a8_grouped(a, w, offs, out, a_scale=s_a, w_scale=s_w, **kw)
        untouched(buf, T, N, rows=slice(o[0], o[-1]))
    else:
        bufs, views = _qviews("mx", T, N // 2)
        G.gemm_w4a8_grouped(a, w, offs, a_scale=s_a, w_scale=s_w, **views, **kw)
        ref = tuple(torch.zeros_like(v).view(torch.uint8) for v in views.values())
    for e in live:
        r = slice(o[e], o[e + 1])
        one = G.gemm_w4a8(a[r], w[e], a_scale=s_a[r], w_scale=s_w[e], **kw)
        if not fused:
            assert torch.equal(out[r], one), e
        else:
            for dst, src in zip(ref, one):
                dst[r] = src.view(torch.uint8)
    if fused:
        _holds(bufs, slice(o[0], o[-1]), ref)


@pytest.mark.parametrize("tile", G.W4A8_TILES)
@pytest.mark.parametrize("grouped", (False, True), ids=("dense", "grouped"))
def test_remapped_grid(grouped, tile):
    """``M = 513``, ``N = 258``: 15 tiles at 128x128 and 9 at 256x128, more than 8 and no multiple
    of 8, so ``xcd_remap`` is no identity (``q >= 1``, ``r != 0``). Grouped: E = 3, sizes
    (200, 57, 256), every group against the fp64 product with its expert's weights."""
    M, N, E = 513, 258, 3
    a, w, s_a, s_w, a8, w8 = _case(M, N, 1)
    if not grouped:
        want = exact_scaled(a8, w8, s_a, s_w).to(F32)
        assert torch.equal(_run(a, w, s_a, s_w, F32, tile=tile), want)
        return
    ws = [_case(M, N + e, 1) for e in range(E)]
    wg = torch.stack([G._as_bytes(c[1][:N]) for c in ws]).view(w.dtype)
    sg = torch.stack([c[3][:N] for c in ws])
    o = [0, 200, 257, 513]
    buf, out = sentinel_out(M, N, F32)
    G.gemm_w4a8_grouped(a, wg, torch.tensor(o, dtype=torch.int32, device=DEV), out, a_scale=s_a,
                        w_scale=sg, tile=tile)
    untouched(buf, M, N)
    for e in range(E):
        r = slice(o[e], o[e + 1])
        assert torch.equal(out[r], exact_scaled(a8[r], ws[e][5][:N], s_a[r], sg[e]).to(F32)), e


def test_non_finite():
    """A NaN byte in ``a`` reaches exactly its output row, a scale byte 255 in ``w_scale`` exactly
    its output column."""
    a, w, s_a, s_w, _, w8 = (t.clone() for t in _case(129, 130, 3, centre=127))
    a.view(torch.uint8)[1, 0] = 0x7F
    s_w[9, 0] = 255
    want = classes64(dequant64(a, s_a), dequant64(w8, s_w.clamp(max=129)))
    want[:, 9] = float("nan")
    assert int(torch.isnan(want).sum()) == 129 + 130 - 1  # row 1 and column 9 only
    same(_run(a, w, s_a, s_w, F32), want.float())


@pytest.mark.parametrize("model", ("mlp", "mlp-gated", "moe"))
def test_models(model):
    """``kernel="mixed"`` at 96 rows against ``reference_chain`` under the models' own bound
    (``validate``: ``atol = 1e-3 ffn``); at 16 rows against the ``kernel="skinny"`` model of the
    same seed under the same bound."""
    def make(seq, kernel):
        kw = dict(hidden=256, ffn=256, seq=seq, fmt="w4a8", kernel=kernel)
        return MxMoE(experts=4, dispatch="native", top_k=2, **kw) if model == "moe" else \
            MxMLP(act="silu", gated=model == "mlp-gated", **kw)

    m = make(96, "mixed")
    y = m.forward().clone()
    m.validate(y)
    assert torch.equal(y, m.forward())
    y16, ref16 = (make(16, k).forward().float() for k in ("mixed", "skinny"))
    torch.testing.assert_close(y16, ref16, rtol=0, atol=1e-3 * 256)
