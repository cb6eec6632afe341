"""Skinny-M block-scaled GEMM on the GPU: ``gemm_skinny`` / ``gemm_skinny_grouped`` against fp64
arithmetic on the dequantised operands. Integer operands in -3..3 under power-of-two block scales
make every partial sum exact in f32, so the result is compared with ``torch.equal`` whatever the
K-split; a case (operands and fp64 product) is made once and shared.

e4m3fn has no Inf and E2M1 neither Inf nor NaN, so the non-finite plants are what the operand
formats can carry: NaN bytes (fp8) and the scale byte 255 (both formats)."""

import pytest
import torch

from _exact import (FP8, classes64, dequant64, exact_scaled, extreme_scales, ints, nan_padded,
                    same, sentinel_out, untouched)
from ddlb_amd.ops import gemm as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP4 = torch.float4_e2m1fn_x2
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
FMTS = ("mx", "mxfp4")
KTILE = {"mx": 128, "mxfp4": 256}
STRIP = G.SKINNY_STRIP
NAN = float("nan")
# one axis at a time around the base case; pairs where two axes meet in the kernel (the 16-row
# chunk count with the unsplit epilogue, several A panels with and without a split)
BASE = dict(out=BF16, M=17, N=STRIP + 24, kt=5, ks=2)
AXES = dict(out=(F16, F32), M=(1, 7, 16, 33, 65), N=(16, STRIP, 7), ks=(1, 5, "auto"), kt=(9,))
CASES = [BASE] + [dict(BASE, **{k: v}) for k, vs in AXES.items() for v in vs] + \
    [dict(BASE, M=7, ks=1), dict(BASE, M=33, kt=9, ks=1)]


def _pack(v, fmt):
    """Integer-valued f32 ``v`` as e4m3, or as E2M1 nibble pairs."""
    if fmt == "mx":
        return v.to(FP8)
    from ddlb_amd.ops.mx import pack_e2m1

    code = torch.tensor((0, 2, 4, 5), device=v.device)[v.abs().long()]
    return pack_e2m1(code | ((v < 0).long() << 3))


_MADE = {}


def _case(fmt, M, N, kt, centre=None):
    """``(a, w, s_a, s_w, a8, w8)``: the operands in ``fmt``, their scale bytes (the whole E8M0
    range, or ``centre`` +- 2) and the same integers as e4m3 for the fp64 reference."""
    key = (fmt, M, N, kt, centre)
    if key not in _MADE:
        K = kt * KTILE[fmt]
        g = torch.Generator(device=DEV).manual_seed(11 + 1009 * M + 31 * N + K)
        av, wv = ints((M, K), F32, g), ints((N, K), F32, g)
        if centre is None:
            s_a, s_w = extreme_scales(M, N, K, g)[:2]
        else:
            s_a, s_w = ((centre + torch.randint(-2, 3, (r, K // 32), generator=g, device=DEV))
                        .to(torch.uint8) for r in (M, N))
        _MADE[key] = (_pack(av, fmt), _pack(wv, fmt), s_a, s_w, av.to(FP8), wv.to(FP8))
    return _MADE[key]


def _run(a, w, s_a, s_w, odt, **kw):
    buf, out = sentinel_out(a.shape[0], w.shape[0], odt)
    assert G.gemm_skinny(a, w, out, a_scale=s_a, w_scale=s_w, **kw) is out
    torch.cuda.synchronize()
    untouched(buf, a.shape[0], w.shape[0])
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v).split(".")[-1]
                                                               for v in c.values()))
@pytest.mark.parametrize("fmt", FMTS)
def test_exact_on_integers(fmt, case):
    a, w, s_a, s_w, a8, w8 = _case(fmt, case["M"], case["N"], case["kt"])
    out = _run(a, w, s_a, s_w, case["out"], ksplit=case["ks"])
    assert torch.equal(out, exact_scaled(a8, w8, s_a, s_w).to(F32).to(case["out"]))


@pytest.mark.parametrize("ks", (1, 2))
@pytest.mark.parametrize("raw", ([2, 2, 5, 22, 22, 23], [2, -7, 5, 22, 9, 999]),
                         ids=("sorted", "garbage"))
@pytest.mark.parametrize("fmt", FMTS)
def test_grouped_equals_dense_per_group(fmt, raw, ks):
    """E = 5, group sizes (0, 3, 17, 0, 1) from row 2 of T = 24; the garbage offsets (negative,
    decreasing, > T) clamp to (0, 3, 17, 0, 2)."""
    T, N, E = 24, STRIP + 24, 5
    a, _, s_a, _, _, _ = _case(fmt, T, N, 5)
    ws = [_case(fmt, T, N + e, 5) for e in range(E)]
    w = torch.stack([G._as_bytes(c[1][:N]) for c in ws]).view(a.dtype)
    s_w = torch.stack([c[3][:N] for c in ws])
    offs = torch.tensor(raw, dtype=torch.int32, device=DEV)
    o = G.clamp_offsets(offs, T)
    buf, out = sentinel_out(T, N, BF16)
    G.gemm_skinny_grouped(a, w, offs, out, a_scale=s_a, w_scale=s_w, ksplit=ks)
    torch.cuda.synchronize()
    untouched(buf, T, N, rows=slice(o[0], o[-1]))
    for e in range(E):
        if o[e + 1] > o[e]:
            rows = slice(o[e], o[e + 1])
            assert torch.equal(out[rows], G.gemm_skinny(a[rows], w[e], a_scale=s_a[rows],
                                                        w_scale=s_w[e], ksplit=ks)), e


@pytest.mark.parametrize("ks", (1, 2))
@pytest.mark.parametrize("fmt", FMTS)
def test_poisoned_padding_changes_nothing(fmt, ks):
    """Operands and scales as views of buffers whose padding holds NaN bytes (fp4: 6.0 pairs) and
    the scale byte 255, on leading dimensions larger than K."""
    a, w, s_a, s_w, a8, w8 = _case(fmt, 17, STRIP + 24, 5)
    kind = "fp4" if fmt == "mxfp4" else None
    out = _run(nan_padded(a, kind), nan_padded(w, kind), nan_padded(s_a, "scale"),
               nan_padded(s_w, "scale"), F32, ksplit=ks)
    assert torch.equal(out, exact_scaled(a8, w8, s_a, s_w).to(F32))


@pytest.mark.parametrize("ks", (1, 2))
@pytest.mark.parametrize("fmt", FMTS)
def test_non_finite_reach_their_rows_and_columns(fmt, ks):
    M, N, kt = 17, STRIP + 24, 8
    a, w, s_a, s_w, a8, w8 = (t.clone() for t in _case(fmt, M, N, kt, centre=127))
    K = a8.shape[1]
    if fmt == "mx":  # a NaN byte in the first K-slice of A and in the second of W
        a.view(torch.uint8)[1, 0] = 0x7F
        w.view(torch.uint8)[2, K // 2] = 0xFF
        a8, w8 = a, w
    s_a[5, K // 32 - 1] = 255
    s_w[9, 0] = 255
    # (the two blocks under a byte 255 are set to NaN below: as numbers they count with scale 1)
    want = classes64(dequant64(a8, s_a.clamp(max=127 + 2)), dequant64(w8, s_w.clamp(max=127 + 2)))
    want[5] = NAN
    want[:, 9] = NAN
    same(_run(a, w, s_a, s_w, F32, ksplit=ks), want.float())


@pytest.mark.parametrize("fmt", FMTS)
def test_random_data_twice(fmt):
    """``rtol = 0, atol = 1e-3 K`` against the fp64 product of the dequantised operands; a second
    run writes the same bytes."""
    from ddlb_amd.models.mx_mlp import _fmt_ops

    quant, _, dequant = _fmt_ops(fmt)
    M, N, K = 40, STRIP + 24, 1024
    g = torch.Generator(device=DEV).manual_seed(5)
    (a, s_a), (w, s_w) = (quant(torch.randn((r, K), generator=g, device=DEV, dtype=BF16))
                          for r in (M, N))
    want = dequant(a, s_a).double() @ dequant(w, s_w).double().t()
    out = _run(a, w, s_a, s_w, F32, ksplit="auto")
    torch.testing.assert_close(out.double(), want, rtol=0, atol=1e-3 * K)
    assert torch.equal(out, _run(a, w, s_a, s_w, F32, ksplit="auto"))


@pytest.mark.parametrize("act", ("none", "relu", "silu", "gelu"))
def test_activation_within_one_ulp(act):
    """``act`` of the exact f32 sum (fp64 arithmetic), one ulp of the output dtype plus the GLU
    tests' absolute term; scales around 2^-4 keep the sums within a few units."""
    from ddlb_amd.parallel.sim import apply_act

    a, w, s_a, s_w, a8, w8 = _case("mx", 17, STRIP + 24, 5, centre=123)
    want = apply_act(exact_scaled(a8, w8, s_a, s_w), G.ACTS[act])
    assert 0.5 < float(want.abs().max()) < 64
    for odt, rtol in ((BF16, 2.0 ** -7), (F32, 2.0 ** -20)):
        out = _run(a, w, s_a, s_w, odt, ksplit=2, act=act)
        if act in ("none", "relu"):
            assert torch.equal(out, want.to(F32).to(odt))
        err = (out.double() - want).abs()
        assert bool((err <= 2.0 ** -14 + rtol * want.abs()).all()), float(err.max())


@pytest.mark.parametrize("ks", (1, 3))
@pytest.mark.parametrize("fmt", FMTS)
def test_six_strips(fmt, ks):
    """``N = 5 STRIP + 1``: six workgroups along N, the last one a single weight row."""
    a, w, s_a, s_w, a8, w8 = _case(fmt, 17, 5 * STRIP + 1, 5, centre=127)
    out = _run(a, w, s_a, s_w, F32, ksplit=ks)
    assert torch.equal(out, exact_scaled(a8, w8, s_a, s_w).to(F32))


@pytest.mark.parametrize("ks", (1, 3))
@pytest.mark.parametrize("fmt", FMTS)
def test_six_strips_gated(fmt, ks):
    """``N = 6 STRIP`` gated: ``glu_reference`` of the exact f32 product, 3 STRIP columns."""
    a, w, s_a, s_w, a8, w8 = _case(fmt, 17, 6 * STRIP, 5, centre=127)
    buf, out = sentinel_out(17, 3 * STRIP, F32)
    G.gemm_skinny(a, w, out, a_scale=s_a, w_scale=s_w, ksplit=ks, glu=True)
    assert torch.equal(out, G.glu_reference(exact_scaled(a8, w8, s_a, s_w).to(F32)))
    untouched(buf, 17, 3 * STRIP)


@pytest.mark.parametrize("dispatch,top_k", (("torch", 1), ("native", 2)))
@pytest.mark.parametrize("fmt", FMTS)
def test_moe_model_on_the_skinny_kernel(fmt, dispatch, top_k):
    from ddlb_amd.models.mx_moe import MxMoE

    moe = MxMoE(hidden=256, ffn=256, seq=12, experts=4, fmt=fmt, dispatch=dispatch, top_k=top_k,
                kernel="skinny")
    y = moe.forward().clone()
    torch.cuda.synchronize()
    moe.validate(y)
    assert torch.equal(y, moe.forward())
