"""The MX linear layer's backward pass on the GPU: dgrad and wgrad through the block-scaled GEMMs
on operands quantised along each GEMM's own contraction axis (``ddlb_amd/models/mx_linear.py``).

Exactness is claimed on integer operands in -3..3: they quantise exactly along either axis, every
product and partial sum is an exact fp32 number, so the results are compared bit for bit with the
fp64 integer products. On real-valued data the bound is the project's own for 8-bit operands,
``rtol = 0, atol = 1e-3 k`` with ``k`` the contraction length of the GEMM in question."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMTS = ("mx", "mxfp4")


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _shape(fmt):
    return (256, 512, 256) if fmt == "mxfp4" else (256, 384, 128)


def _ints(shape, seed):
    return torch.randint(-3, 4, shape, generator=_gen(seed), device=DEV).float()


def _pm1(shape, seed, scale=1.0):
    return (torch.rand(shape, generator=_gen(seed), device=DEV) * 2 - 1) * scale


# ------------------------------------------------------------------ 8. exact backward
@pytest.mark.parametrize("fmt", FMTS)
def test_exact_dgrad_and_wgrad_on_integers(fmt):
    from ddlb_amd.ops.gemm import gemm
    from ddlb_amd.ops.mx import quantize_mx_2way

    M, N, K = _shape(fmt)
    x, w, dy = _ints((M, K), 1), _ints((N, K), 2), _ints((M, N), 3)
    xq, xs, xtq, xts = quantize_mx_2way(x.bfloat16(), fmt=fmt)
    wq, ws, wtq, wts = quantize_mx_2way(w.bfloat16(), fmt=fmt)
    dyq, dys, dytq, dyts = quantize_mx_2way(dy.bfloat16(), fmt=fmt)
    y = gemm(xq, wq, out_dtype=torch.float32, a_scale=xs, w_scale=ws)
    dx = gemm(dyq, wtq, out_dtype=torch.float32, a_scale=dys, w_scale=wts)      # contracts N
    dw = gemm(dytq, xtq, out_dtype=torch.float32, a_scale=dyts, w_scale=xts)    # contracts M
    torch.cuda.synchronize()
    assert tuple(dx.shape) == (M, K) and tuple(dw.shape) == (N, K)
    assert torch.equal(y.double(), x.double() @ w.double().t())
    assert torch.equal(dx.double(), dy.double() @ w.double())
    assert torch.equal(dw.double(), dy.double().t() @ x.double())


# ------------------------------------------------------------------ 9. through autograd
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mx_linear_through_autograd(fmt, dtype):
    from ddlb_amd.models.mx_linear import mx_linear, mx_linear_reference

    M, N, K = _shape(fmt)
    x = _pm1((M, K), 1).to(dtype).requires_grad_()                 # scaled as in MxMLP
    w = _pm1((N, K), 2, K ** -0.5).to(dtype).requires_grad_()
    dy = _pm1((M, N), 3).to(dtype)
    y = mx_linear(x, w, fmt)
    assert y.dtype == dtype and tuple(y.shape) == (M, N) and y.requires_grad
    y.backward(dy, retain_graph=True)
    torch.cuda.synchronize()
    dx, dw = x.grad.clone(), w.grad.clone()
    assert dx.dtype == dtype and dw.dtype == dtype
    assert tuple(dx.shape) == (M, K) and tuple(dw.shape) == (N, K)
    y_ref, dx_ref, dw_ref = mx_linear_reference(x.detach(), w.detach(), dy, fmt)
    for name, got, want, k in (("y", y.detach(), y_ref, K), ("dx", dx, dx_ref, N),
                               ("dw", dw, dw_ref, M)):
        err = float((got.float() - want).abs().max())
        print(f"{fmt} {dtype} {name}: max |err| = {err:.4g}, bound {1e-3 * k:.4g}, "
              f"max |ref| = {float(want.abs().max()):.4g}")
        torch.testing.assert_close(got.float(), want, rtol=0, atol=1e-3 * k)
    assert float(dx_ref.abs().max()) > 0 and float(dw_ref.abs().max()) > 0
    # a second backward over the same graph: bit-identical gradients
    x.grad = w.grad = None
    y.backward(dy)
    torch.cuda.synchronize()
    assert torch.equal(x.grad, dx) and torch.equal(w.grad, dw)


def test_only_the_needed_gradient_is_computed():
    from ddlb_amd.models.mx_linear import mx_linear

    M, N, K = _shape("mx")
    x = _pm1((M, K), 1).bfloat16()
    w = _pm1((N, K), 2, K ** -0.5).bfloat16().requires_grad_()
    mx_linear(x, w).backward(_pm1((M, N), 3).bfloat16())
    assert x.grad is None and tuple(w.grad.shape) == (N, K)


def test_shape_the_gemms_cannot_take_is_named():
    from ddlb_amd.models.mx_linear import mx_linear

    x = torch.zeros(256, 128, device=DEV, dtype=torch.bfloat16)
    w = torch.zeros(384, 128, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="256, 384, 128"):
        mx_linear(x, w, "mxfp4")
    with pytest.raises(ValueError, match="192, 384, 128"):
        mx_linear(x[:192], w, "mx")
    with pytest.raises(TypeError):
        mx_linear(x.float(), w.float())


@pytest.mark.parametrize("fmt", FMTS)
def test_module_requantises_after_a_weight_update_and_not_before(fmt):
    from ddlb_amd.models.mx_linear import MxLinear, mx_linear

    M, N, K = _shape(fmt)
    lin = MxLinear(K, N, fmt=fmt, device=DEV)
    x = _pm1((M, K), 5).bfloat16()
    assert lin.n_quant == 0
    y0 = lin(x)
    y1 = lin(x)
    assert lin.n_quant == 1 and torch.equal(y0, y1)
    y1.backward(_pm1((M, N), 6).bfloat16())          # a gradient is no weight update
    assert tuple(lin.weight.grad.shape) == (N, K)
    lin(x)
    assert lin.n_quant == 1
    with torch.no_grad():                            # an optimiser step, in place
        lin.weight.add_(lin.weight.grad, alpha=-0.25)
    y2 = lin(x)
    assert lin.n_quant == 2
    assert not torch.equal(y2, y0)
    assert torch.equal(y2, mx_linear(x, lin.weight.detach(), fmt))  # the new weight's result
    lin(x)
    assert lin.n_quant == 2
