"""CPU-side checks of the routed MX backward: the padded K layout's Python twins
(``ops.gemm.padded_offsets`` / ``kgrouped_capacity``), the reference of the grouped transposing
quantiser, the layer's reference, and every Python refusal of ``quantize_mx_t_grouped``,
``gemm_kgrouped`` and the layer, all on CPU tensors (nothing is launched)."""

import pytest
import torch

FP8 = torch.float8_e4m3fn
FP4 = getattr(torch, "float4_e2m1fn_x2", None)
FMTS = ("mx", "mxfp4")


def _mod(fmt):
    return 256 if fmt == "mxfp4" else 128


def _i32(v):
    return torch.tensor(v, dtype=torch.int32)


# ------------------------------------------------------------------ the layout
def test_padded_offsets_and_capacity():
    from ddlb_amd.ops.gemm import kgrouped_capacity, padded_offsets

    assert kgrouped_capacity(644, 7, 128) == (5 + 7) * 128
    assert kgrouped_capacity(644, 7, 256) == (2 + 7) * 256
    assert kgrouped_capacity(0, 3, 128) == 384
    o = _i32([0, 0, 1, 131, 131, 387, 644, 644])
    assert padded_offsets(o, 644, 128) == [0, 0, 128, 384, 384, 640, 1024, 1024]
    assert padded_offsets(o, 644, 256) == [0, 0, 256, 512, 512, 768, 1280, 1280]
    # clamped as the kernels clamp: negative, decreasing, beyond T
    assert padded_offsets(_i32([-5, 200, 100, 10 ** 9]), 300, 128) == [0, 256, 256, 384]
    assert padded_offsets(_i32([7, 7, 7]), 5, 128) == [0, 0, 0]


def test_capacity_bounds_every_layout_and_is_attained():
    from ddlb_amd.ops.gemm import kgrouped_capacity, padded_offsets

    g = torch.Generator().manual_seed(3)
    attained = 0
    for mod in (128, 256):
        for _ in range(300):
            E = int(torch.randint(1, 10, (1,), generator=g))
            T = int(torch.randint(0, 6 * mod, (1,), generator=g))
            o = torch.randint(-mod, T + mod + 1, (E + 1,), generator=g).to(torch.int32)
            if int(torch.randint(0, 2, (1,), generator=g)):
                o = o.sort().values
            k0 = padded_offsets(o, T, mod)
            cap = kgrouped_capacity(T, E, mod)
            assert k0[0] == 0 and all(b >= a and b % mod == 0 for a, b in zip(k0, k0[1:]))
            assert k0[-1] <= cap
        for E, T in ((3, 2 * mod + 3), (1, mod + 1), (4, 4)):  # one row each, the rest at the end
            o = list(range(E)) + [T]
            k0 = padded_offsets(_i32(o), T, mod)
            attained += k0[-1] == kgrouped_capacity(T, E, mod)
    assert attained == 6


# ------------------------------------------------------------------ the quantiser's reference
@pytest.mark.parametrize("fmt", FMTS)
def test_grouped_transposer_reference(fmt):
    from ddlb_amd.ops.gemm import kgrouped_capacity, padded_offsets
    from ddlb_amd.ops.mx import quantize_mx_t_grouped_reference, quantize_mx_t_reference

    mod = _mod(fmt)
    T, C = 300, 8
    x = torch.randn((T, C), generator=torch.Generator().manual_seed(1)).bfloat16()
    o = _i32([3, 3, 133, 290])
    qt, st, written = quantize_mx_t_grouped_reference(x, o, fmt)
    cap = kgrouped_capacity(T, 3, mod)
    d = 2 if fmt == "mxfp4" else 1
    assert tuple(qt.shape) == (C, cap // d) and tuple(st.shape) == (C, cap // 32)
    k0 = padded_offsets(o, T, mod)
    assert int(written.sum()) == k0[-1] and bool(written[:k0[-1]].all())
    pad = torch.zeros((k0[3] - k0[2], C), dtype=x.dtype)
    pad[:157] = x[133:290]
    q1, s1 = quantize_mx_t_reference(pad, fmt)
    assert torch.equal(qt[:, k0[2] // d:k0[3] // d], q1.view(torch.uint8))
    assert torch.equal(st[:, k0[2] // 32:k0[3] // 32], s1)
    # the zero padding: scale byte 127, zero data
    tail = (k0[2] + 160) // 32
    assert bool((st[:, tail:k0[3] // 32] == 127).all())
    assert bool((qt[:, (k0[2] + 160) // d:k0[3] // d] == 0).all())
    # stacked: one slab per group, tiles past R dropped
    qs, ss, ws = quantize_mx_t_grouped_reference(x[:mod + 5], _i32([0, mod + 5, mod + 5]), fmt,
                                                 stacked_rows=mod)
    assert tuple(qs.shape) == (2, C, mod // d) and ws.sum(dim=1).tolist() == [mod, 0]
    q2, s2 = quantize_mx_t_reference(x[:mod], fmt)
    assert torch.equal(qs[0], q2.view(torch.uint8)) and torch.equal(ss[0], s2)


# ------------------------------------------------------------------ the layer's reference
@pytest.mark.parametrize("fmt", FMTS)
def test_layer_reference_is_exact_on_integers(fmt):
    from ddlb_amd.models.mx_grouped_linear import mx_grouped_linear_reference

    mod = _mod(fmt)
    E, K, N = 3, mod, mod
    g = torch.Generator().manual_seed(2)
    o = [2, 3, 3, 3 + 40]
    T = o[-1] + 1
    x = torch.randint(-3, 4, (T, K), generator=g).float()
    w = torch.randint(-3, 4, (E, N, K), generator=g).float()
    dy = torch.randint(-3, 4, (T, N), generator=g).float()
    y, dx, dw = mx_grouped_linear_reference(x.bfloat16(), w.bfloat16(), dy.bfloat16(), _i32(o), fmt)
    assert y.dtype == torch.float32 and tuple(dw.shape) == (E, N, K)
    for e in range(E):
        lo, hi = o[e], o[e + 1]
        assert torch.equal(y[lo:hi], x[lo:hi] @ w[e].t())
        assert torch.equal(dx[lo:hi], dy[lo:hi] @ w[e])
        assert torch.equal(dw[e], dy[lo:hi].t() @ x[lo:hi])
    assert bool((y[:2] == 0).all()) and bool((y[-1] == 0).all()) and bool((dx[:2] == 0).all())
    assert bool((dw[1] == 0).all())


# ------------------------------------------------------------------ refusals
def test_layer_refusals():
    from ddlb_amd.models.mx_grouped_linear import (MxGroupedLinear, check_shapes,
                                                   mx_grouped_linear_reference)

    x = torch.zeros((10, 128), dtype=torch.bfloat16)
    w = torch.zeros((2, 256, 128), dtype=torch.bfloat16)
    o = _i32([0, 4, 10])
    assert check_shapes(x, w, o, "mx") == (10, 256, 128, 2)
    for args, exc in (((x, w[0], o, "mx"), ValueError), ((x[0], w, o, "mx"), ValueError),
                      ((x.float(), w, o, "mx"), TypeError), ((x, w.float(), o, "mx"), TypeError),
                      ((x, w, o, "mxfp4"), ValueError), ((x, w, o, "fp8"), ValueError),
                      ((x[:, :64], w, o, "mx"), ValueError),
                      ((x, w[:, :200], o, "mx"), ValueError),
                      ((x, w, o.long(), "mx"), TypeError), ((x, w, o[:2], "mx"), ValueError),
                      ((x, w, [0, 4, 10], "mx"), TypeError)):
        with pytest.raises(exc):
            check_shapes(*args)
    with pytest.raises(ValueError):
        mx_grouped_linear_reference(x, w, torch.zeros((10, 128), dtype=torch.bfloat16), o)
    for kw in (dict(experts=0, in_features=128, out_features=128),
               dict(experts=2, in_features=100, out_features=128),
               dict(experts=2, in_features=128, out_features=128, fmt="mxfp4")):
        with pytest.raises(ValueError):
            MxGroupedLinear(**kw)
    with pytest.raises(TypeError):
        MxGroupedLinear(2, 128, 128, dtype=torch.float32)


def test_quantiser_refusals_before_the_device_check():
    from ddlb_amd.ops.mx import _check_quant_t_grouped

    x = torch.zeros((300, 72), dtype=torch.bfloat16)
    o = _i32([0, 100, 300])
    bad = [
        ((x.double(), o, "mx"), TypeError), ((x[0], o, "mx"), ValueError),
        ((x[:, :4], o, "mx"), ValueError), ((x[:, ::2], o, "mx"), ValueError),
        ((x, o.long(), "mx"), TypeError), ((x, o[:1], "mx"), ValueError),
        ((x, torch.zeros(1026, dtype=torch.int32), "mx"), ValueError),
        ((x, o, "fp8"), ValueError), ((x, o, "mx", None, 100), ValueError),
        ((x, o, "mxfp4", None, 128), ValueError),
        ((x, o, "mx", (torch.zeros((72, 384), dtype=FP8),
                       torch.zeros((72, 16), dtype=torch.uint8))), ValueError),
        ((x, o, "mx", (torch.zeros((72, 512), dtype=torch.uint8),
                       torch.zeros((72, 16), dtype=torch.uint8))), TypeError),
        ((x, o, "mx", (torch.zeros((2, 72, 128), dtype=FP8),
                       torch.zeros((2, 72, 4), dtype=torch.uint8)[:, :, :2]), 128), ValueError),
    ]
    for args, exc in bad:
        with pytest.raises(exc):
            _check_quant_t_grouped(*args)
    # everything in order but the device
    for args in ((x, o, "mx"), (x, o, "mx", None, 128),
                 (x, o, "mx", (torch.zeros((72, 512), dtype=FP8),
                               torch.zeros((72, 16), dtype=torch.uint8)))):
        with pytest.raises(ValueError, match="ROCm device"):
            _check_quant_t_grouped(*args)


@pytest.mark.parametrize("fmt", FMTS)
def test_kgrouped_refusals(fmt):
    from ddlb_amd.ops.gemm import _check_kgrouped, kgrouped_capacity

    if fmt == "mxfp4" and FP4 is None:
        pytest.skip("torch.float4_e2m1fn_x2 missing")
    mod, d = _mod(fmt), (2 if fmt == "mxfp4" else 1)
    M, N, T, E = 192, 320, 644, 7
    cap = kgrouped_capacity(T, E, mod)
    a = torch.zeros((M, cap // d), dtype=torch.uint8).view(FP4 if d == 2 else FP8)
    w = torch.zeros((N, cap // d), dtype=torch.uint8).view(a.dtype)
    sa = torch.zeros((M, cap // 32), dtype=torch.uint8)
    sw = torch.zeros((N, cap // 32), dtype=torch.uint8)
    o = torch.zeros(E + 1, dtype=torch.int32)
    out = torch.zeros((E, M, N), dtype=torch.bfloat16)
    ok = dict(a=a, w=w, offsets=o, rows=T, a_scale=sa, w_scale=sw)

    def check(**kw):
        args = dict(ok)
        args.update(kw)
        return _check_kgrouped(args.pop("a"), args.pop("w"), args.pop("offsets"),
                               args.pop("rows"), args.pop("out", None), **args)

    assert check() == (M, N, cap, E, torch.bfloat16)
    assert check(out=out, tile="128x256") == (M, N, cap, E, torch.bfloat16)
    assert check(out_dtype=torch.float32)[4] == torch.float32
    assert check(rows=T - 200)[2] == cap            # spare columns are fine
    u8 = lambda t: t.view(torch.uint8)
    bad = [
        (dict(a_scale=None), ValueError), (dict(w_scale=None), ValueError),
        (dict(a=u8(a).bfloat16(), w=u8(w).bfloat16()), TypeError),
        (dict(w=u8(w)), TypeError), (dict(a=a[0]), ValueError),
        (dict(offsets=o.long()), TypeError), (dict(offsets=o[:1]), ValueError),
        (dict(offsets=torch.zeros(1026, dtype=torch.int32)), ValueError),
        (dict(offsets=o.reshape(1, -1)), ValueError),
        (dict(rows=T + mod), ValueError), (dict(rows=-1), ValueError),
        (dict(rows=float(T)), ValueError), (dict(rows=True), ValueError),
        (dict(offsets=torch.zeros(E + 2, dtype=torch.int32)), ValueError),  # one more group
        (dict(a=u8(a)[:, :-mod // d].view(a.dtype), a_scale=sa[:, :-mod // 32]), ValueError),
        (dict(tile="pt4"), ValueError), (dict(tile="256x256"), ValueError),
        (dict(tile="i128"), ValueError),
        (dict(out_dtype=torch.float64), TypeError), (dict(out_dtype=FP8), TypeError),
        (dict(out=out[:, :, :N - 8]), ValueError), (dict(out=out[0]), ValueError),
        (dict(out=out, out_dtype=torch.float32), TypeError),
        (dict(out=torch.zeros((M, E, N), dtype=torch.bfloat16).transpose(0, 1)), ValueError),
        (dict(out=torch.zeros((E, M, 2 * N), dtype=torch.bfloat16)[:, :, ::2]), ValueError),
        (dict(a_scale=sa[:, :-4]), ValueError), (dict(a_scale=sa.to(torch.int8)), TypeError),
        (dict(w_scale=torch.zeros((N, cap // 32 + 2), dtype=torch.uint8)[:, :cap // 32]),
         ValueError),
    ]
    for kw, exc in bad:
        with pytest.raises(exc):
            check(**kw)
