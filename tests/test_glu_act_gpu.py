"""The gated activation as an op on the GPU (``ddlb_amd/ops/glu.py``, ``csrc/gemm/glu_act.hip``).

Exact where the arithmetic is exact (``none`` and ``relu`` on integers in -3..3: the fp64 result
rounded once), the epilogue's own result where the GEMM can produce it (``glu(gemm(a, w))`` against
``gemm(a, w, glu=True)``), and for ``silu`` / ``gelu`` the fp64 references within one unit in the
last place of the output dtype: ``rtol = 2^-7`` (bf16), ``2^-10`` (f16), ``2^-20`` (f32), half of
it the final rounding and half margin for the fp32 evaluation, and ``atol = 2^-14``: the fp32
``act'`` carries an absolute error of at most about ``2^-19`` where it cancels, and
``|dh u| <= 16``. Outputs sit in sentinel-surrounded buffers and ``c`` has ``ld > 2F``."""

import pytest
import torch

from _exact import ints, padded, same, sentinel_out, untouched

from ddlb_amd.ops.gemm import ACTS, gemm, glu_reference
from ddlb_amd.ops.glu import glu, glu_bwd, glu_bwd_reference
from ddlb_amd.parallel.sim import apply_act

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
TS = (1, 3, 300)
FS = (32, 96, 32 * 65)   # one group; groups that are no power of two; more vectors than threads
RTOL = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 2.0 ** -20}
ATOL = 2.0 ** -14
LARGE = (30.0, 100.0, 1e4, 1e20, 3e38)
MANY_ROWS = 2509       # long rows go one per pass and the grid is capped at 8 workgroups per CU
#                        (2048 on 256 CUs): this many rows need a second grid-stride trip


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _run(c, dh, act, out_dtype=None):
    """``(h, dc)`` in sentinel-surrounded buffers, the guards checked."""
    T, F = dh.shape
    hbuf, h = sentinel_out(T, F, out_dtype or c.dtype, pad_cols=8)
    dbuf, dc = sentinel_out(T, 2 * F, c.dtype, pad_cols=8)
    assert glu(c, act, out=h) is h
    assert glu_bwd(dh, c, act, out=dc) is dc
    torch.cuda.synchronize()
    untouched(hbuf, T, F)
    untouched(dbuf, T, 2 * F)
    return h, dc


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["none", "relu"])
def test_exact_on_integers(act, dtype):
    for T in TS:
        for F in FS:
            g = _gen(1000 * T + F)
            c = padded(ints((T, 2 * F), dtype, g))
            dh = padded(ints((T, F), dtype, g))
            assert c.stride(0) > 2 * F
            h, dc = _run(c, dh, act)
            h64 = glu_reference(c.float(), act).double()
            dc64 = glu_bwd_reference(dh, c, act)
            assert torch.equal(h, h64.float().to(dtype)), (T, F, "h")
            assert torch.equal(dc, dc64.float().to(dtype)), (T, F, "dc")
            assert float(dc64.abs().max()) > 0
            if dtype != torch.float32:  # the float32 output of 16-bit rows
                h32, _ = _run(c, dh, act, torch.float32)
                assert torch.equal(h32, h64.float())
    assert glu(c, act).dtype == dtype and torch.equal(glu(c, act), h)


@pytest.mark.parametrize("act", ["none", "relu"])
def test_exact_with_more_rows_than_one_pass_of_the_grid(act):
    """``F = 32 * 65`` takes one row per workgroup pass and the grid is capped at 8 workgroups per
    CU: ``T = MANY_ROWS`` makes the grid-stride loops of both kernels take a second trip."""
    g = _gen(3)
    T, F = MANY_ROWS, FS[2]
    c, dh = ints((T, 2 * F), torch.bfloat16, g), ints((T, F), torch.bfloat16, g)
    h, dc = _run(c, dh, act)
    assert torch.equal(h, glu_reference(c.float(), act).bfloat16())
    assert torch.equal(dc, glu_bwd_reference(dh, c, act).float().bfloat16())
    assert torch.equal(glu_bwd(dh, c, act), dc)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("act", ["none", "relu"])
def test_packed_indexing_is_the_epilogues(act, dtype):
    g = _gen(7)
    a = ints((70, 128), dtype, g)
    w = ints((192, 128), dtype, g)
    c = gemm(a, w, out_dtype=torch.float32)
    fused = gemm(a, w, glu=True, act=act, out_dtype=torch.float32)
    torch.cuda.synchronize()
    assert tuple(fused.shape) == (70, 96)
    assert torch.equal(glu(c, act), fused)
    assert float(fused.abs().max()) > 0


def _h64(c, act):
    """``glu_reference``'s rule evaluated in fp64 on the upcast ``c``."""
    T, N = c.shape
    v = c.double().reshape(T, N // 64, 2, 32)
    return (apply_act(v[:, :, 0], ACTS[act]) * v[:, :, 1]).reshape(T, N // 2)


def _real_inputs(T, F, dtype, seed):
    """Uniform values in +-4 and, in row 0 (and the last row), the large gates of either sign that
    ``dtype`` holds, next to ``u = dh = 0.5`` so that ``h`` and ``dc`` stay finite."""
    g = _gen(seed)
    c = (torch.rand((T, 2 * F), generator=g, device=DEV) * 8 - 4).to(dtype)
    dh = (torch.rand((T, F), generator=g, device=DEV) * 8 - 4).to(dtype)
    big = torch.tensor([s * v for v in LARGE for s in (1.0, -1.0)], device=DEV).to(dtype)
    big = big[torch.isfinite(big)]
    n = big.numel()
    assert n >= 6 and n <= 32
    for row in {0, T - 1}:
        c[row, :n] = big
        c[row, 32:32 + n] = 0.5
        dh[row, :n] = 0.5
    return padded(c), padded(dh)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["silu", "gelu"])
def test_silu_and_gelu_within_one_ulp_of_fp64(act, dtype):
    rtol = RTOL[dtype]
    for T, F in [(T, F) for T in TS for F in FS] + [(MANY_ROWS, FS[2])]:
        c, dh = _real_inputs(T, F, dtype, 31 * T + F)
        h, dc = _run(c, dh, act)
        h64 = _h64(c, act)
        dc64 = glu_bwd_reference(dh, c, act)
        for name, got, want in (("h", h, h64), ("dc", dc, dc64)):
            assert bool(torch.isfinite(got).all()), (act, dtype, T, F, name)
            err = (got.double() - want).abs()
            bound = ATOL + rtol * want.abs()
            ratio = float((err / bound).max())
            print(f"{act} {dtype} T={T} F={F} {name}: max err / bound = {ratio:.3f}, "
                  f"max |err| = {float(err.max()):.3g}")
            assert ratio <= 1.0, (act, dtype, T, F, name, ratio)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["none", "relu", "silu", "gelu"])
def test_planted_non_finite_values_stay_in_their_pair(act, dtype):
    T, F = 5, 96
    c, dh = _real_inputs(T, F, dtype, 77)
    h0, dc0 = (t.clone() for t in _run(c, dh, act))
    nan, inf = float("nan"), float("inf")
    c[1, 64 + 3] = nan          # a NaN gate: group 1, element 3
    c[2, 32 + 5] = nan          # a NaN up: group 0, element 5
    dh[3, 70] = inf             # an Inf dh: group 2, element 6
    h, dc = _run(c, dh, act)
    # what changes: h[1, 35], h[2, 5]; dc pairs (1, 67 / 99), (2, 5 / 37), (3, 134 / 166)
    hw, dw = h0.clone(), dc0.clone()
    hw[1, 35] = nan
    hw[2, 5] = nan
    dw[1, 67], dw[1, 99] = nan, nan                        # both outputs of the NaN gate
    dw[2, 5] = nan                                         # dh u act': u is NaN
    for col in (134, 166):                                 # the pair of the Inf dh: by class
        dw[3, col] = dc[3, col]
        assert not bool(torch.isfinite(dc[3, col])), (act, col)
    same(h, hw)
    same(dc, dw)
    assert bool(torch.isnan(dc[1, 67])) and bool(torch.isnan(dc[1, 99]))


def test_empty_and_refusals_on_the_device():
    c = torch.zeros((0, 64), device=DEV, dtype=torch.bfloat16)
    assert tuple(glu(c, "silu").shape) == (0, 32)
    assert tuple(glu_bwd(torch.zeros((0, 32), device=DEV, dtype=torch.bfloat16), c).shape) \
        == (0, 64)
    with pytest.raises(ValueError, match="64"):
        glu(torch.zeros((4, 96), device=DEV), "silu")
    with pytest.raises(TypeError):
        glu_bwd(torch.zeros((4, 32), device=DEV), torch.zeros((4, 64), device=DEV).half())
