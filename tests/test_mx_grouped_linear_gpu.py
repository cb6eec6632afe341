"""The routed (per-expert) MX linear layer on the GPU: forward and dgrad on the grouped GEMM, wgrad
on the K-grouped GEMM, operands from the row-wise and the grouped transposing quantisers
(``ddlb_amd/models/mx_grouped_linear.py``).

Three oracles. (1) With counts that are multiples of the K-tile, every expert's ``y``, ``dx`` and
``dw`` are bit for bit what ``mx_linear`` computes on that expert's rows with the same tile.
(2) With ragged counts and integer operands in -3..3, which quantise exactly along either axis
and whose products and partial sums are exact fp32 numbers, the results equal the fp64 integer
products rounded once to the output dtype. (3) On real-valued data the bound is the project's
own for 8-bit operands, ``rtol = 0, atol = 1e-3 k``, ``k`` the contraction length of the GEMM in
question; for the wgrad that is the largest padded group length."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMTS = ("mx", "mxfp4")
E = 4
TILE = "128x128"


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _mod(fmt):
    return 256 if fmt == "mxfp4" else 128


def _ints(shape, seed):
    return torch.randint(-3, 4, shape, generator=_gen(seed), device=DEV).float()


def _pm1(shape, seed, scale=1.0):
    return (torch.rand(shape, generator=_gen(seed), device=DEV) * 2 - 1) * scale


def _offs(counts, o0=0):
    o = [o0]
    for c in counts:
        o.append(o[-1] + c)
    return o, torch.tensor(o, dtype=torch.int32, device=DEV)


def _run(x, w, dy, offs, fmt, tile="auto"):
    from ddlb_amd.models.mx_grouped_linear import mx_grouped_linear

    x = x.detach().clone().requires_grad_()
    w = w.detach().clone().requires_grad_()
    y = mx_grouped_linear(x, w, offs, fmt, tile)
    y.backward(dy)
    torch.cuda.synchronize()
    return y.detach(), x.grad, w.grad


@pytest.mark.parametrize("fmt", FMTS)
def test_bit_for_bit_mx_linear_per_expert(fmt):
    from ddlb_amd.models.mx_linear import mx_linear

    mod = _mod(fmt)
    K = N = mod
    o, offs = _offs((mod, 0, 2 * mod, mod))
    T = o[-1]
    x = _pm1((T, K), 1).bfloat16()
    w = _pm1((E, N, K), 2, K ** -0.5).bfloat16()
    dy = _pm1((T, N), 3).bfloat16()
    y, dx, dw = _run(x, w, dy, offs, fmt, TILE)
    assert y.dtype == dx.dtype == dw.dtype == torch.bfloat16
    assert tuple(y.shape) == (T, N) and tuple(dx.shape) == (T, K) and tuple(dw.shape) == (E, N, K)
    for g in range(E):
        lo, hi = o[g], o[g + 1]
        if hi == lo:
            assert bool((dw[g].view(torch.int16) == 0).all()), "dw of the empty expert is +0.0"
            continue
        xg = x[lo:hi].clone().requires_grad_()
        wg = w[g].clone().requires_grad_()
        yg = mx_linear(xg, wg, fmt, TILE)
        yg.backward(dy[lo:hi])
        torch.cuda.synchronize()
        assert torch.equal(y[lo:hi], yg.detach()), (fmt, g, "y")
        assert torch.equal(dx[lo:hi], xg.grad), (fmt, g, "dx")
        assert torch.equal(dw[g], wg.grad), (fmt, g, "dw")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("fmt", FMTS)
def test_exact_on_integers_with_ragged_counts(fmt, dtype):
    """Counts (1, 0, 130, 70) behind 3 leading rows and before 2 trailing ones: rows outside the
    groups have zero ``y`` and ``dx``, the empty expert a zero ``dw``."""
    mod = _mod(fmt)
    K = N = mod
    o, offs = _offs((1, 0, 130, 70), o0=3)
    T = o[-1] + 2
    x, w, dy = _ints((T, K), 11), _ints((E, N, K), 12), _ints((T, N), 13)
    y, dx, dw = _run(x.to(dtype), w.to(dtype), dy.to(dtype), offs, fmt)
    y64 = torch.zeros((T, N), dtype=torch.float64, device=DEV)
    dx64 = torch.zeros((T, K), dtype=torch.float64, device=DEV)
    dw64 = torch.zeros((E, N, K), dtype=torch.float64, device=DEV)
    for g in range(E):
        lo, hi = o[g], o[g + 1]
        y64[lo:hi] = x[lo:hi].double() @ w[g].double().t()
        dx64[lo:hi] = dy[lo:hi].double() @ w[g].double()
        dw64[g] = dy[lo:hi].double().t() @ x[lo:hi].double()
    assert torch.equal(y, y64.float().to(dtype)), (fmt, "y")
    assert torch.equal(dx, dx64.float().to(dtype)), (fmt, "dx")
    assert torch.equal(dw, dw64.float().to(dtype)), (fmt, "dw")
    outside = [r for r in range(T) if r < o[0] or r >= o[-1]]
    assert outside and bool((y[outside] == 0).all()) and bool((dx[outside] == 0).all())
    assert bool((dw[1] == 0).all()) and float(dw64[0].abs().max()) > 0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("fmt", FMTS)
def test_project_bound_on_random_data(fmt, dtype):
    from ddlb_amd.models.mx_grouped_linear import mx_grouped_linear_reference
    from ddlb_amd.ops.gemm import padded_offsets

    mod = _mod(fmt)
    K = N = mod
    o, offs = _offs((1, 0, 130, 70), o0=3)
    T = o[-1] + 2
    x = _pm1((T, K), 21).to(dtype)
    w = _pm1((E, N, K), 22, K ** -0.5).to(dtype)
    dy = _pm1((T, N), 23).to(dtype)
    y, dx, dw = _run(x, w, dy, offs, fmt)
    y_ref, dx_ref, dw_ref = mx_grouped_linear_reference(x, w, dy, offs, fmt)
    k0 = padded_offsets(offs, T, mod)
    kw = max(k0[g + 1] - k0[g] for g in range(E))
    assert kw == mod * -(-130 // mod)
    for name, got, want, k in (("y", y, y_ref, K), ("dx", dx, dx_ref, N), ("dw", dw, dw_ref, kw)):
        err = float((got.float() - want).abs().max())
        print(f"{fmt} {dtype} {name}: max |err| = {err:.4g}, bound {1e-3 * k:.4g}, "
              f"max |ref| = {float(want.abs().max()):.4g}")
        torch.testing.assert_close(got.float(), want, rtol=0, atol=1e-3 * k)
    assert float(dx_ref.abs().max()) > 0 and float(dw_ref.abs().max()) > 0
    assert bool((dw[1] == 0).all()) and bool((dw_ref[1] == 0).all())


def test_only_the_needed_gradient_is_computed():
    from ddlb_amd.models.mx_grouped_linear import mx_grouped_linear

    o, offs = _offs((100, 0, 30, 70))
    x = _pm1((200, 128), 1).bfloat16()
    w = _pm1((E, 128, 128), 2, 128 ** -0.5).bfloat16()
    dy = _pm1((200, 128), 3).bfloat16()
    wr = w.clone().requires_grad_()
    mx_grouped_linear(x, wr, offs).backward(dy)
    assert x.grad is None and tuple(wr.grad.shape) == (E, 128, 128)
    xr = x.clone().requires_grad_()
    y = mx_grouped_linear(xr, w, offs)
    assert len(y.grad_fn.saved_tensors) == 3, "no transposed x is kept when w needs no gradient"
    y.backward(dy)
    assert w.grad is None and tuple(xr.grad.shape) == (200, 128)


def test_shape_the_gemms_cannot_take_is_named():
    from ddlb_amd.models.mx_grouped_linear import mx_grouped_linear

    x = torch.zeros(200, 128, device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(E, 384, 128, device=DEV, dtype=torch.bfloat16)
    _, offs = _offs((100, 0, 30, 70))
    with pytest.raises(ValueError, match="384, 128"):
        mx_grouped_linear(x, w, offs, "mxfp4")
    with pytest.raises(TypeError):
        mx_grouped_linear(x.float(), w.float(), offs)
    with pytest.raises(ValueError):
        mx_grouped_linear(x, w, offs[:-1])


@pytest.mark.parametrize("fmt", FMTS)
def test_module_requantises_after_a_weight_update_and_not_before(fmt):
    from ddlb_amd.models.mx_grouped_linear import MxGroupedLinear, mx_grouped_linear

    mod = _mod(fmt)
    K = N = mod
    o, offs = _offs((100, 0, 30, 70))
    T = o[-1]
    lin = MxGroupedLinear(E, K, N, fmt=fmt, device=DEV)
    x = _pm1((T, K), 5).bfloat16()
    assert lin.n_quant == 0
    y0 = lin(x, offs)
    y1 = lin(x, offs)
    assert lin.n_quant == 1 and torch.equal(y0, y1)
    y1.backward(_pm1((T, N), 6).bfloat16())          # a gradient is no weight update
    assert tuple(lin.weight.grad.shape) == (E, N, K)
    lin(x, offs)
    assert lin.n_quant == 1
    with torch.no_grad():                            # an optimiser step, in place
        lin.weight.add_(lin.weight.grad, alpha=-0.25)
    y2 = lin(x, offs)
    assert lin.n_quant == 2
    assert not torch.equal(y2, y0)
    assert torch.equal(y2, mx_grouped_linear(x, lin.weight.detach(), offs, fmt))
    lin(x, offs)
    assert lin.n_quant == 2
