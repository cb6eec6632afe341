"""Tiled A16 GEMM (bf16 / f16 ``a`` on MXFP4 / MX-fp8 ``w``, prefill shapes) on the GPU. Integers
in -3..3 under scale bytes 125..129: every weight is a normal number of both dtypes and every sum
is exact in f32, so the output is ``torch.equal`` to fp64 arithmetic on the dequantised weights,
rounded once. The case builder counts ``kt`` in the skinny kernel's K-tiles (256 fp4 / 128 fp8
elements); the kernel's own K-tile is 128 elements, so ``kt = 1`` is its one-K-tile loop for fp8."""

import pytest
import torch

from _exact import FP8, classes64, dequant64, ints, nan_padded, same, sentinel_out, untouched
from ddlb_amd.models.mx_mlp import MxMLP
from ddlb_amd.models.mx_moe import MxMoE
from ddlb_amd.ops import gemm as G
from test_gemm_skinny_a16_gpu import KTILE, U8, _case
from test_gemm_skinny_gpu import BF16, DEV, F16, F32, _pack

pytestmark = pytest.mark.gpu
forms = pytest.mark.parametrize("wfmt", ("mxfp4", "mx"))
dtypes = pytest.mark.parametrize("dt", (BF16, F16), ids=("bf16", "f16"))
tiles = pytest.mark.parametrize("tile", G.A16_TILES)
TILES = G.A16_TILES + ("auto",)
BASE = dict(tile=TILES[0], M=129, N=130, kt=3, out=None, pad=False)
AXES = dict(tile=TILES[1:], M=(1, 257), N=(7, 256), kt=(1, 5), out=(F32,), pad=(True,))
CASES = [BASE] + [dict(BASE, **{k: v}) for k, vs in AXES.items() for v in vs]


def _run(a, w, s_w, odt=None, **kw):
    cols = w.shape[0] // 2 if kw.get("glu") else w.shape[0]
    buf, out = sentinel_out(a.shape[0], cols, odt or a.dtype)
    assert G.gemm_a16(a, w, out, w_scale=s_w, **kw) is out
    untouched(buf, a.shape[0], cols)
    return out


def _stacked(wfmt, dt, T, N, kt, E):
    """``E`` experts' weights, scales and fp64 dequantised weights, ``N`` rows each."""
    ws = [_case(wfmt, dt, T, N + e, kt) for e in range(E)]
    w = torch.stack([G._as_bytes(c[1][:N]) for c in ws]).view(ws[0][1].dtype)
    return w, torch.stack([c[2][:N] for c in ws]), [c[3][:N] for c in ws]


@pytest.mark.parametrize("b", range(8))
@dtypes
@forms
def test_one_block_at_a_time(wfmt, dt, b):
    """K map, scale-byte pairing, LDS permutations and (fp8) the one-K-tile loop: operands non-zero
    in eighth ``b`` of ``K = 256 / 128`` only, every row's scale bytes all different and, for
    bf16, far apart. A wrong map or chunk / scale pairing is a wrong value."""
    K = KTILE[wfmt]
    g = torch.Generator(device=DEV).manual_seed(b)
    keep = torch.zeros(K, device=DEV)
    keep[K // 8 * b:K // 8 * (b + 1)] = 1
    a, wv = (ints((16, K), F32, g) * keep).to(dt), ints((16, K), F32, g) * keep
    spread = torch.tensor((30, 60, 90, 118, 127, 150, 190, 220) if dt == BF16 else
                          tuple(range(122, 130)), device=DEV)
    s = torch.stack([spread[torch.randperm(8, generator=g, device=DEV)][:K // 32]
                     for _ in range(16)]).to(U8)
    wd = dequant64(wv.to(FP8), s)
    assert torch.equal(_run(a, _pack(wv, wfmt), s, F32), (a.double() @ wd.t()).to(F32))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v).split(".")[-1]
                                                               for v in c.values()))
@dtypes
@forms
def test_exact_on_integers(wfmt, dt, case):
    a, w, s, wd = _case(wfmt, dt, case["M"], case["N"], case["kt"])
    want = (a.double() @ wd.t()).to(F32).to(case["out"] or dt)
    if case["pad"]:  # larger pitches, NaN bits in the padding of all three tensors
        a, w = nan_padded(a), nan_padded(w, "fp4" if wfmt == "mxfp4" else None)
        s = nan_padded(s, "scale")
    assert torch.equal(_run(a, w, s, case["out"], tile=case["tile"]), want)


@tiles
@pytest.mark.parametrize("glu", (False, True), ids=("act", "glu"))
@dtypes
@forms
def test_epilogues(wfmt, dt, glu, tile):
    """Byte for byte ``torch.relu`` / ``glu_reference`` of the same launch's f32 output."""
    a, w, s, _ = _case(wfmt, dt, 17, 64, 3)
    c = _run(a, w, s, F32, tile=tile)
    want = G.glu_reference(c, "relu") if glu else torch.relu(c)
    assert torch.equal(_run(a, w, s, F32, tile=tile, glu=glu, act="relu"), want)


@tiles
@pytest.mark.parametrize("raw", ([2, 2, 5, 135, 135, 136], [2, -7, 5, 135, 9, 999]),
                         ids=("sorted", "garbage"))
@pytest.mark.parametrize("glu", (False, True), ids=("dense", "glu"))
@dtypes
@forms
def test_grouped_equals_dense_per_group(wfmt, dt, glu, raw, tile):
    """E = 5, sizes (0, 3, 130, 0, 1) from row 2 of T = 140; garbage clamps to (0, 3, 130, 0, 5)."""
    T, E, N = 140, 5, 192 if glu else 130
    a = _case(wfmt, dt, T, N, 3)[0]
    w, s, _ = _stacked(wfmt, dt, T, N, 3, E)
    offs = torch.tensor(raw, dtype=torch.int32, device=DEV)
    o = G.clamp_offsets(offs, T)
    kw = dict(tile=tile, glu=True, act="relu") if glu else dict(tile=tile)
    cols = N // 2 if glu else N
    buf, out = sentinel_out(T, cols, dt)
    G.gemm_a16_grouped(a, w, offs, out, w_scale=s, **kw)
    untouched(buf, T, cols, rows=slice(o[0], o[-1]))
    for e in (e for e in range(E) if o[e + 1] > o[e]):
        r = slice(o[e], o[e + 1])
        assert torch.equal(out[r], G.gemm_a16(a[r], w[e], w_scale=s[e], **kw)), e


@tiles
@pytest.mark.parametrize("grouped", (False, True), ids=("dense", "grouped"))
@dtypes
@forms
def test_remapped_grid(wfmt, dt, grouped, tile):
    """``M = 513``, ``N = 258``: 15 tiles at 128x128 and 9 at 256x128, more than 8 and no multiple
    of 8, so ``xcd_remap`` is no identity. Grouped: E = 3, sizes (200, 57, 256), every group
    against the fp64 product with its expert's weights."""
    M, N, E = 513, 258, 3
    a, w, s, wd = _case(wfmt, dt, M, N, 1)
    if not grouped:
        assert torch.equal(_run(a, w, s, F32, tile=tile), (a.double() @ wd.t()).to(F32))
        return
    wg, sg, wds = _stacked(wfmt, dt, M, N, 1, E)
    o = [0, 200, 257, 513]
    buf, out = sentinel_out(M, N, F32)
    G.gemm_a16_grouped(a, wg, torch.tensor(o, dtype=torch.int32, device=DEV), out, w_scale=sg,
                       tile=tile)
    untouched(buf, M, N)
    for e in range(E):
        r = slice(o[e], o[e + 1])
        assert torch.equal(out[r], (a[r].double() @ wds[e].t()).to(F32)), e


@dtypes
@forms
def test_non_finite(wfmt, dt):
    """A NaN in ``a`` reaches exactly its output row; a scale byte 255 and (fp8) an e4m3 NaN byte
    in ``w`` exactly their output column."""
    a, w, s, wd = (t.clone() for t in _case(wfmt, dt, 129, 130, 3))
    a[1, 0], s[9, 0], cols = float("nan"), 255, [9]
    if wfmt == "mx":
        w.view(U8)[2, a.shape[1] // 2] = 0xFF
        cols.append(2)
    want = classes64(a.double(), wd)
    want[:, cols] = float("nan")
    assert int(torch.isnan(want).sum()) == 130 + len(cols) * 128  # row 1 and those columns only
    same(_run(a, w, s, F32), want.float())


@pytest.mark.parametrize("model", ("mlp", "mlp-gated", "moe"))
@pytest.mark.parametrize("fmt", ("w4a16", "w8a16"))
def test_models(fmt, model):
    """``kernel="a16"`` at 96 rows against ``reference_chain`` under the models' own bound
    (``validate``: ``atol = 1e-3 ffn``), a second forward writing the same bytes; at 16 rows
    against the ``kernel="skinny"`` model of the same seed under the same bound."""
    def make(seq, kernel):
        kw = dict(hidden=256, ffn=256, seq=seq, fmt=fmt, kernel=kernel)
        return MxMoE(experts=4, dispatch="native", top_k=2, **kw) if model == "moe" else \
            MxMLP(act="silu", gated=model == "mlp-gated", **kw)

    m = make(96, "a16")
    y = m.forward().clone()
    m.validate(y)
    assert torch.equal(y, m.forward())
    y16, ref16 = (make(16, k).forward().float() for k in ("a16", "skinny"))
    torch.testing.assert_close(y16, ref16, rtol=0, atol=1e-3 * 256)
