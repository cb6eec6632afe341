"""The MoE training ops without a GPU: every host-side refusal of ``glu``, ``glu_bwd``, ``gather``,
``combine_bwd`` and of the layer's ``check_shapes`` (reached with CPU tensors, the device refusal
last), the torch references against plain Python loops on tiny inputs, and the two facts the GPU
bounds of ``tests/test_glu_act_gpu.py`` rest on: ``glu_bwd_reference`` is finite at huge gates, and
an fp32 evaluation of the documented derivative formulas, rounded to the dtype, meets the bound
with about 2x headroom."""

import math

import pytest
import torch

from ddlb_amd.models.mx_moe_ffn import check_shapes, mx_moe_ffn_reference
from ddlb_amd.ops.gemm import glu_reference
from ddlb_amd.ops.glu import _check_glu, _check_glu_bwd, glu, glu_bwd, glu_bwd_reference
from ddlb_amd.ops.moe import (_check_combine_bwd, _check_gather, combine_bwd,
                              combine_bwd_reference, combine_reference, gather,
                              gather_reference, route_reference)

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32)


# ---------------------------------------------------------------------------- refusals
def test_glu_refusals_and_the_device_refusal_last():
    c = torch.zeros(4, 128, dtype=BF)
    with pytest.raises(ValueError, match="unknown activation"):
        _check_glu(c, "tanh")
    with pytest.raises(TypeError, match="c must be"):
        _check_glu(c.to(torch.float64))
    with pytest.raises(TypeError, match="c must be"):
        _check_glu([1.0])
    with pytest.raises(ValueError, match="2-D"):
        _check_glu(c[0])
    with pytest.raises(ValueError, match="% 64"):
        _check_glu(torch.zeros(4, 96, dtype=BF))
    with pytest.raises(ValueError, match="unit inner stride"):
        _check_glu(torch.zeros(128, 4, dtype=BF).t())
    with pytest.raises(ValueError, match="16-byte-aligned"):
        _check_glu(torch.zeros(4, 132, dtype=BF)[:, 4:])
    with pytest.raises(ValueError, match="16-byte-aligned"):
        _check_glu(torch.zeros(4, 132, dtype=BF)[:, :128])
    with pytest.raises(TypeError, match="out is"):
        _check_glu(c, out=torch.zeros(4, 64, dtype=BF), out_dtype=F32)
    with pytest.raises(TypeError, match="writes"):
        _check_glu(c, out_dtype=F16)
    with pytest.raises(TypeError, match="writes"):
        _check_glu(c.float(), out=torch.zeros(4, 64, dtype=BF))
    with pytest.raises(ValueError, match="shape"):
        _check_glu(c, out=torch.zeros(4, 128, dtype=BF))
    with pytest.raises(ValueError, match="ROCm device"):
        _check_glu(c, "silu", out=torch.zeros(4, 64), out_dtype=F32)
    with pytest.raises(ValueError, match="ROCm device"):
        glu(c)
    assert tuple(_shape_only(_check_glu, torch.zeros(0, 64, dtype=F16))) == (0, 32)


def _shape_only(check, *a):
    """The check's dims for a CPU tensor: everything passes up to the device refusal."""
    with pytest.raises(ValueError, match="ROCm device"):
        check(*a)
    return a[-1].shape[0], a[-1].shape[1] // 2


def test_glu_bwd_refusals():
    c, dh = torch.zeros(4, 128, dtype=BF), torch.zeros(4, 64, dtype=BF)
    with pytest.raises(ValueError, match="unknown activation"):
        _check_glu_bwd(dh, c, "swish")
    with pytest.raises(TypeError, match="dh must be"):
        _check_glu_bwd(dh.float(), c)
    with pytest.raises(ValueError, match="dh must have shape"):
        _check_glu_bwd(c, c)
    with pytest.raises(ValueError, match="% 64"):
        _check_glu_bwd(dh, torch.zeros(4, 32, dtype=BF))
    with pytest.raises(ValueError, match="16-byte-aligned"):
        _check_glu_bwd(torch.zeros(4, 68, dtype=BF)[:, 4:], c)
    with pytest.raises(TypeError, match="out must be"):
        _check_glu_bwd(dh, c, out=torch.zeros(4, 128))
    with pytest.raises(ValueError, match="out must have shape"):
        _check_glu_bwd(dh, c, out=torch.zeros(4, 64, dtype=BF))
    with pytest.raises(ValueError, match="ROCm device"):
        _check_glu_bwd(dh, c, "gelu", out=torch.zeros(4, 128, dtype=BF))
    with pytest.raises(ValueError, match="ROCm device"):
        glu_bwd(dh, c)


def test_gather_refusals():
    x, rt = torch.zeros(5, 8, dtype=BF), _i32(0, 4, -1)
    with pytest.raises(TypeError, match="x must be"):
        _check_gather(x.to(torch.float64), rt)
    with pytest.raises(ValueError, match="2-D"):
        _check_gather(x[0], rt)
    with pytest.raises(TypeError, match="row_token must be an int32"):
        _check_gather(x, rt.long())
    with pytest.raises(ValueError, match="1-D"):
        _check_gather(x, rt.reshape(3, 1))
    with pytest.raises(ValueError, match="contiguous"):
        _check_gather(x, _i32(0, 1, 2, 3)[::2])
    with pytest.raises(ValueError, match="whole 16-byte vectors"):
        _check_gather(torch.zeros(5, 12, dtype=BF), rt)
    with pytest.raises(ValueError, match="unit inner stride"):
        _check_gather(torch.zeros(8, 5, dtype=BF).t(), rt)
    with pytest.raises(ValueError, match="16-byte-aligned"):
        _check_gather(torch.zeros(5, 12, dtype=BF)[:, :8], rt)
    with pytest.raises(TypeError, match="out must be"):
        _check_gather(x, rt, torch.zeros(3, 8))
    with pytest.raises(ValueError, match="out must have shape"):
        _check_gather(x, rt, torch.zeros(5, 8, dtype=BF))
    with pytest.raises(ValueError, match="ROCm device"):
        _check_gather(x, rt, torch.zeros(3, 8, dtype=BF))
    with pytest.raises(ValueError, match="ROCm device"):
        gather(x, rt)


def test_combine_bwd_refusals():
    S, k, T, H = 3, 2, 6, 8
    dout, y = torch.zeros(S, H, dtype=BF), torch.zeros(T, H, dtype=BF)
    sr = torch.zeros(S, k, dtype=torch.int32)
    gate, rt = torch.zeros(S, k), torch.zeros(T, dtype=torch.int32)
    bad = [
        (TypeError, "dout must be", (dout.to(torch.float64), sr, gate, rt)),
        (ValueError, "2-D", (dout[0], sr, gate, rt)),
        (TypeError, "slot_row must be an int32", (dout, sr.long(), gate, rt)),
        (ValueError, "slot_row must be", (dout, sr[:2], gate, rt)),
        (ValueError, "slot_row must be", (dout, sr[:, :0], gate, rt)),
        (TypeError, "gate must be a float32", (dout, sr, gate.double(), rt)),
        (ValueError, "gate must have", (dout, sr, gate[:, :1], rt)),
        (ValueError, "contiguous", (dout, sr, torch.zeros(k, S).t(), rt)),
        (TypeError, "row_token must be an int32", (dout, sr, gate, rt.long())),
        (ValueError, "1-D", (dout, sr, gate, rt.reshape(T, 1))),
        (TypeError, "y must be", (dout, sr, gate, rt, y.to(torch.float64))),
        (TypeError, "agree", (dout, sr, gate, rt, y, F32)),
        (TypeError, "writes", (dout, sr, gate, rt, y.to(F16))),
        (TypeError, "writes", (dout, sr, gate, rt, None, F32)),
        (ValueError, "whole 16-byte vectors", (dout.float()[:, :4], sr, gate, rt, None, BF)),
        (ValueError, "y must have shape", (dout, sr, gate, rt, y[:5])),
        (ValueError, "16-byte-aligned", (dout, sr, gate, rt, torch.zeros(T, 12, dtype=BF)[:, :8])),
        (TypeError, "pair", (dout, sr, gate, rt, y, None, y)),
        (TypeError, "dy", (dout, sr, gate, rt, y, None, (None, None))),
        (ValueError, "both or neither", (dout, sr, gate, rt, y, None, (y.clone(), None))),
        (ValueError, "both or neither", (dout, sr, gate, rt, None, None, (y, gate.clone()))),
        (TypeError, "dgate", (dout, sr, gate, rt, y, None, (y.clone(), gate.double()))),
        (ValueError, "dgate", (dout, sr, gate, rt, y, None, (y.clone(), gate[:2].clone()))),
        (ValueError, "must have shape", (dout, sr, gate, rt, y, None, (y[:5].clone(), gate))),
        (ValueError, "ROCm device", (dout, sr, gate, rt, y, None, (y.clone(), gate.clone()))),
        (ValueError, "ROCm device", (dout.float(), sr, gate, rt, y.to(F16))),
    ]
    for exc, match, args in bad:
        with pytest.raises(exc, match=match):
            _check_combine_bwd(*args)
    with pytest.raises(ValueError, match="ROCm device"):
        combine_bwd(dout, sr, gate, rt, y)


def test_layer_check_shapes():
    E, S, k, H, F = 3, 5, 2, 128, 256
    x, w1, w2 = (torch.zeros(S, H, dtype=BF), torch.zeros(E, 2 * F, H, dtype=BF),
                 torch.zeros(E, H, F, dtype=BF))
    ids, gates = torch.zeros(S, k, dtype=torch.int64), torch.zeros(S, k)
    assert check_shapes(x, w1, w2, ids, gates) == (S, H, F, E, k)
    assert check_shapes(x.half(), w1.half(), w2.half(), ids.int(), gates, "mx", "gelu",
                        torch.zeros(S, H)) == (S, H, F, E, k)
    bad = [
        (ValueError, "fmt", (x, w1, w2, ids, gates, "fp8")),
        (ValueError, "act", (x, w1, w2, ids, gates, "mx", "tanh")),
        (TypeError, "x is", (x.float(), w1, w2, ids, gates)),
        (TypeError, "share one dtype", (x, w1.half(), w2, ids, gates)),
        (ValueError, "w1 is", (x, w1[0], w2, ids, gates)),
        (ValueError, "shape mismatch", (x, w1[:, :F], w2, ids, gates)),
        (ValueError, "shape mismatch", (x, w1, w2[:2], ids, gates)),
        (ValueError, "multiples of 256", (x, w1, w2, ids, gates, "mxfp4")),
        (ValueError, "multiples of 128", (x[:, :64], w1[:, :, :64], w2[:, :64], ids, gates)),
        (TypeError, "ids must be", (x, w1, w2, ids.float(), gates)),
        (ValueError, "ids must be", (x, w1, w2, ids[:4], gates)),
        (TypeError, "gates must be", (x, w1, w2, ids, gates.double())),
        (ValueError, "gates must have", (x, w1, w2, ids, gates[:, :1])),
        (ValueError, "dout must have", (x, w1, w2, ids, gates, "mx", "silu", x[:2])),
    ]
    for exc, match, args in bad:
        with pytest.raises(exc, match=match):
            check_shapes(*args)
    from ddlb_amd.models.mx_moe_ffn import mx_moe_ffn

    with pytest.raises(ValueError, match="ROCm device"):     # route's refusal, after the layer's
        mx_moe_ffn(x, w1, w2, ids, gates)


def test_a_captured_backward_is_refused_with_an_error(monkeypatch):
    """A step that would run autograd's backward inside a graph capture raises before anything is
    launched; without a gradient to compute the call goes on (here to route's device refusal)."""
    from ddlb_amd.models.mx_moe_ffn import mx_moe_ffn, refuse_captured_backward

    x, w1, w2 = (torch.zeros(5, 128, dtype=BF), torch.zeros(3, 256, 128, dtype=BF),
                 torch.zeros(3, 128, 128, dtype=BF))
    ids, gates = torch.zeros(5, 2, dtype=torch.int64), torch.zeros(5, 2)
    refuse_captured_backward((x.clone().requires_grad_(),))      # no capture: nothing happens
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    for grads in ((x,), (w1,), (w2,), (gates,)):
        for t in grads:
            t.requires_grad_()
        with pytest.raises(RuntimeError, match="graph capture"):
            mx_moe_ffn(x, w1, w2, ids, gates)
        with torch.no_grad(), pytest.raises(ValueError, match="ROCm device"):
            mx_moe_ffn(x, w1, w2, ids, gates)
        for t in grads:
            t.requires_grad_(False)
    with pytest.raises(ValueError, match="ROCm device"):
        mx_moe_ffn(x, w1, w2, ids, gates)


# ---------------------------------------------------------------------------- references
def test_gather_and_combine_bwd_references_against_loops():
    g = torch.Generator().manual_seed(0)
    S, k, H, E = 5, 2, 8, 3
    ids = torch.randint(0, E, (S, k), generator=g)
    ids[1, 1] = E
    ids[3, 0] = -1
    offsets, row_token, slot_row = route_reference(ids, E)
    T = S * k
    x = torch.randn(S, H, generator=g).to(BF)
    xp = gather_reference(x, row_token)
    for r in range(T):
        t = int(row_token[r])
        want = x[t] if 0 <= t < S else torch.zeros(H, dtype=BF)
        assert torch.equal(xp[r], want)
    assert torch.equal(gather_reference(x, _i32(7, -3, 2)), torch.stack(
        (torch.zeros(H, dtype=BF), torch.zeros(H, dtype=BF), x[2])))

    dout = torch.randn(S, H, generator=g)
    y = torch.randn(T, H, generator=g).to(BF)
    gate = torch.rand(S, k, generator=g)
    dy, dgate = combine_bwd_reference(dout, slot_row, gate, row_token, y)
    assert dy.dtype == BF and dgate.dtype == torch.float64
    want_dy = torch.zeros(T, H, dtype=BF)
    for t in range(S):
        for j in range(k):
            r = int(slot_row[t, j])
            if r < 0:
                assert float(dgate[t, j]) == 0.0
                continue
            assert int(row_token[r]) == t
            for c in range(H):
                want_dy[r, c] = (gate[t, j] * dout[t, c]).to(BF)
            dot = sum(float(dout[t, c]) * float(y[r, c]) for c in range(H))
            assert abs(float(dgate[t, j]) - dot) <= 1e-12 * max(1.0, abs(dot))
    assert torch.equal(dy, want_dy)
    assert int((row_token < 0).sum()) == 2 and bool((dy[row_token < 0] == 0).all())
    dy2, none = combine_bwd_reference(dout, slot_row, gate, row_token, None, dy_dtype=F16)
    assert none is None and dy2.dtype == F16
    # combine_bwd is the adjoint of combine: <combine(y), dout> = <y, dy> and d/dgate of the same
    out = combine_reference(y.float(), slot_row, gate)
    dy32, dg = combine_bwd_reference(dout, slot_row, gate, row_token, y.float())
    lhs = float((out.double() * dout.double()).sum())
    assert abs(lhs - float((y.double() * dy32.double()).sum())) <= 1e-5 * abs(lhs)
    assert abs(lhs - float((gate.double() * dg).sum())) <= 1e-5 * abs(lhs)


def test_glu_bwd_reference_against_a_loop_and_autograd_of_the_forward():
    g = torch.Generator().manual_seed(1)
    c = torch.randn(2, 128, generator=g)
    dh = torch.randn(2, 64, generator=g)
    for act, fn, dfn in (("none", lambda v: v, lambda v: 1.0),
                         ("relu", lambda v: max(v, 0.0), lambda v: float(v > 0)),
                         ("silu", lambda v: v / (1 + math.exp(-v)),
                          lambda v: (1 + math.exp(-v) + v * math.exp(-v)) / (1 + math.exp(-v)) ** 2)):
        dc = glu_bwd_reference(dh, c, act)
        assert dc.dtype == torch.float64 and tuple(dc.shape) == (2, 128)
        for t in range(2):
            for e in range(64):
                gc, uc = 64 * (e // 32) + e % 32, 64 * (e // 32) + 32 + e % 32
                gv, uv, d = float(c[t, gc]), float(c[t, uc]), float(dh[t, e])
                assert abs(float(dc[t, gc]) - d * uv * dfn(gv)) <= 1e-12 * (1 + abs(d * uv))
                assert abs(float(dc[t, uc]) - d * fn(gv)) <= 1e-12 * (1 + abs(d * gv))
    cr = c.clone().requires_grad_()
    glu_reference(cr, "gelu").backward(dh)
    torch.testing.assert_close(glu_bwd_reference(dh, c, "gelu").float(), cr.grad,
                               rtol=1e-4, atol=1e-5)
    nan = c.clone()
    nan[0, 3] = float("nan")
    for act in ("none", "relu", "silu", "gelu"):
        dc = glu_bwd_reference(dh, nan, act)
        assert bool(torch.isnan(dc[0, 3])) and bool(torch.isnan(dc[0, 35]))
        assert int(torch.isnan(dc).sum()) == 2


LARGE = (30.0, 100.0, 1e4, 1e20, 3e38)


@pytest.mark.parametrize("act", ["silu", "gelu"])
def test_glu_bwd_reference_is_finite_at_huge_gates(act):
    big = torch.tensor([s * v for v in LARGE for s in (1.0, -1.0)])
    c = torch.zeros(1, 64)
    c[0, :10] = big
    c[0, 32:] = 1.0
    d = glu_bwd_reference(torch.ones(1, 32), c, act)[0, :10]
    assert bool(torch.isfinite(d).all())
    for v, dv in zip(big.tolist(), d.tolist()):
        assert (dv == 1.0 or abs(dv - 1.0) < 3e-12) if v > 0 else abs(dv) < 3e-12, (v, dv)


def _formulas_fp32(dh, c, act):
    """The documented derivative formulas evaluated with fp32 torch ops (the kernel's plan): s and
    1 - s from exp(-|z|), gelu's polynomial on the clamped gate."""
    T, N = c.shape
    v = c.float().reshape(T, N // 64, 2, 32)
    g, u = v[:, :, 0], v[:, :, 1]
    d = dh.float().reshape(T, N // 64, 32)

    def pair(z):
        t = torch.exp(-z.abs())
        hi = 1 / (1 + t)
        lo = t * hi
        return torch.where(z >= 0, hi, lo), torch.where(z >= 0, lo, hi)

    if act == "silu":
        s, one_s = pair(g)
        dact, a1 = s * (1 + g * one_s), g * s
    else:
        x = g.clamp(-32, 32)
        uu = 0.7978845608028654 * (x + 0.044715 * x * x * x)
        du = 0.7978845608028654 * (1 + 3 * 0.044715 * x * x)
        s, one_s = pair(2 * uu)
        dact = s + x * s * one_s * (2 * du)
        a1 = g * pair(2 * 0.7978845608028654 * (g + 0.044715 * g * g * g))[0]
    return torch.stack(((d * u) * dact, d * a1), dim=2).reshape(T, N)


@pytest.mark.parametrize("dtype,rtol", [(BF, 2.0 ** -8), (F16, 2.0 ** -10)])
@pytest.mark.parametrize("act", ["silu", "gelu"])
def test_fp32_formulas_meet_the_gpu_bound_with_headroom(act, dtype, rtol):
    """2^20 uniform values in +-4: the fp32 evaluation rounded to the dtype stays within
    ``atol = 2^-14`` plus HALF of bf16's GPU ``rtol`` (all of f16's) of the fp64 reference."""
    g = torch.Generator().manual_seed(2)
    c = (torch.rand(2 ** 14, 128, generator=g) * 8 - 4).to(dtype)
    dh = (torch.rand(2 ** 14, 64, generator=g) * 8 - 4).to(dtype)
    got = _formulas_fp32(dh, c, act).to(dtype).double()
    want = glu_bwd_reference(dh, c, act)
    ratio = float(((got - want).abs() / (2.0 ** -14 + rtol * want.abs())).max())
    print(f"{act} {dtype}: max err / bound = {ratio:.3f} at rtol = {rtol}")
    assert ratio <= 1.0
    big = torch.zeros(1, 64)
    big[0, :10] = torch.tensor([s * v for v in LARGE for s in (1.0, -1.0)])
    big[0, 32:] = 0.5
    d = _formulas_fp32(torch.full((1, 32), 0.5), big, act)
    assert bool(torch.isfinite(d).all())


def test_layer_reference_on_tiny_inputs():
    """The reference composes its stages: with one expert, one choice and a gate of 1 it is
    ``mx_grouped_linear_reference`` -> ``glu`` -> ``mx_grouped_linear_reference`` on the tokens in
    their own order, and the dropped token's row of ``out`` and ``dx`` is zero."""
    from ddlb_amd.models.mx_grouped_linear import mx_grouped_linear_reference

    g = torch.Generator().manual_seed(3)
    S, H, F = 6, 128, 128
    x = (torch.rand(S, H, generator=g) * 2 - 1).to(BF)
    w1 = ((torch.rand(1, 2 * F, H, generator=g) * 2 - 1) * H ** -0.5).to(BF)
    w2 = ((torch.rand(1, H, F, generator=g) * 2 - 1) * F ** -0.5).to(BF)
    dout = (torch.rand(S, H, generator=g) * 2 - 1).to(BF)
    ids = torch.zeros(S, 1, dtype=torch.int64)
    ids[4, 0] = 1
    gates = torch.ones(S, 1)
    out, dx, dw1, dw2, dgates = mx_moe_ffn_reference(x, w1, w2, ids, gates, dout, "silu", "mx")
    keep = [0, 1, 2, 3, 5]
    offs = _i32(0, 5)
    xk = x[keep]
    c1 = mx_grouped_linear_reference(xk, w1, torch.zeros(5, 2 * F, dtype=BF), offs)[0].to(BF)
    h = glu_reference(c1.float(), "silu").to(BF)
    yp = mx_grouped_linear_reference(h, w2, torch.zeros(5, H, dtype=BF), offs)[0].to(BF)
    assert torch.equal(out[keep], yp.float()) and bool((out[4] == 0).all())
    assert all(t.dtype == F32 for t in (out, dx, dw1, dw2, dgates))
    assert bool((dx[4] == 0).all()) and float(dgates[4, 0]) == 0.0
    assert float(dx[keep].abs().max()) > 0 and float(dw1.abs().max()) > 0
    _, _, want_dw2 = mx_grouped_linear_reference(h, w2, dout[keep], offs)
    assert torch.equal(dw2, want_dw2)
    want_dg = (dout[keep].double() * yp.double()).sum(dim=1)
    torch.testing.assert_close(dgates[keep, 0].double(), want_dg, rtol=1e-6, atol=1e-6)
