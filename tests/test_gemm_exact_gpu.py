"""Exact-arithmetic sweep of the GEMM: every tile code, every (input, output) dtype pair, ragged
edges, padded operand and output rows, and the memory around the output.

Operands are integers in -3..3 (``tests/_exact.py``): every partial sum is an exact f32, so the
specification is "the exact product, rounded once to the output dtype" and every comparison is
``torch.equal`` — one misplaced, dropped or duplicated element fails it. A and W are views of
larger buffers whose padding holds 5 (a read past a row end or past the last row changes the
result); C is a view of a buffer filled with -7 that must stay -7 everywhere outside the view."""

import functools

import pytest
import torch

from _exact import (FP8, POISON, exact, ints, padded, sentinel_out, untouched)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64

# (input, output, mode): test_gemm_gpu's _ALL_DT, fp8 -> f16, and the unit-scale MX kernels
FORMS = [(BF16, BF16, "auto"), (BF16, F32, "auto"), (F16, F16, "auto"), (F16, F32, "auto"),
         (F32, F32, "auto"), (FP8, BF16, "auto"), (FP8, F32, "auto"), (FP8, F16, "auto"),
         (FP8, BF16, "mx"), (FP8, F16, "mx"), (FP8, F32, "mx")]
PING = ["t8", "pt8", "t4", "pt4"]


def _name(dt):
    return str(dt).replace("torch.", "").replace("float8_e4m3fn", "fp8").replace("float", "f")


def _form_id(form):
    return f"{_name(form[0])}-{_name(form[1])}-{form[2]}"


def _tiles():
    from ddlb_amd.ops.gemm import TILES

    return list(TILES)


def _k(din, ktiles):
    """K of ``ktiles`` 128-byte K-tiles."""
    return ktiles * 128 // torch.empty((), dtype=din).element_size()


def _make_case(din, M, N, K):
    g = torch.Generator(device=DEV).manual_seed(1000003 * M + 1009 * N + K)
    a, w = ints((M, K), din, g), ints((N, K), din, g)
    return padded(a), padded(w), exact(a, w, F32)


_case = functools.lru_cache(maxsize=None)(_make_case)  # (the large cases call _make_case)


def _out_pad(N, dout):
    """Padding columns that keep the output rows 8-byte aligned (the fast path's rule)."""
    osz = torch.empty((), dtype=dout).element_size()
    return next(p for p in range(4, 12) if ((N + p) * osz) % 8 == 0)


def _check(form, tile, M, N, K, case=None, fast=True, **kw):
    """One GEMM into a sentinel buffer: exact result, nothing written around it."""
    from ddlb_amd.ops.gemm import fast_path_ok, gemm

    din, dout, mode = form
    a, w, ref = case if case is not None else _case(din, M, N, K)
    buf, view = sentinel_out(M, N, dout, pad_cols=_out_pad(N, dout))
    if fast:
        assert fast_path_ok(a, w, view), (form, M, N, K)
    gemm(a, w, view, tile=tile, mode=mode, **kw)
    torch.cuda.synchronize()
    want = ref.to(dout)
    if kw.get("act") == "relu":
        want = want.clamp(min=0)
    bad = int((view != want).sum())
    assert bad == 0, f"{_form_id(form)} {tile} {(M, N, K)}: {bad} wrong elements"
    untouched(buf, M, N)


# ------------------------------------------------------------------ a. ragged, tiled kernels
@pytest.mark.parametrize("form", FORMS, ids=_form_id)
@pytest.mark.parametrize("tile", _tiles())
def test_ragged_tiled(form, tile):
    """Off whole tiles every code runs gemm_tn_kernel (the ping-pong codes the interleaved
    256x256 one): clamped row loads, the scalar column tail, one live row / one live 4-column
    vector in the last tile, a single row; 1 K-tile (no main loop), 2, and 3 (odd parity).
    N = 203 ends in a three-column scalar tail: the one N % 4 at which `col + 3 < N` and
    `col + 3 <= N` differ (the padded output rows keep such an N on the fast path)."""
    din, dout, _ = form
    small = (1, 2) if dout == F32 else (1, 4)
    for M, N, kt in ((300, 202, 2), (257, 260, 2), small + (2,), (300, 202, 1), (300, 202, 3),
                     (130, 203, 2)):
        _check(form, tile, M, N, _k(din, kt))


# ------------------------------------------------------------------ b. whole tiles, ping-pong
@pytest.mark.parametrize("form", FORMS, ids=_form_id)
@pytest.mark.parametrize("tile", PING)
def test_whole_tiles_ping_pong(form, tile):
    """One tile with 1 - 4 K-tiles (pt4 hands single and odd counts to t4) and a 2 x 3 grid."""
    din = form[0]
    for M, N, kt in ((256, 256, 1), (256, 256, 2), (256, 256, 3), (256, 256, 4), (512, 768, 2)):
        _check(form, tile, M, N, _k(din, kt))


@pytest.mark.parametrize("form", [(BF16, BF16, "auto"), (FP8, F32, "mx")], ids=_form_id)
@pytest.mark.parametrize("tile", ["pt4", "pt8"])
def test_persistent_second_tile(form, tile):
    """17 x 17 = 289 tiles, more than the CUs: some persistent blocks take a second tile."""
    M = N = 4352
    K = _k(form[0], 2)
    assert (M // 256) * (N // 256) > torch.cuda.get_device_properties(0).multi_processor_count
    _check(form, tile, M, N, K, case=_make_case(form[0], M, N, K))


# ------------------------------------------------------------------ c. grouped rows
@pytest.mark.parametrize("form", [(BF16, BF16, "auto"), (FP8, F32, "mx")], ids=_form_id)
@pytest.mark.parametrize("tile", ["pt4", "t4"])
def test_grouped_rows_whole_tiles(form, tile):
    """A read from and C written to groups of 256 rows 512 apart: the skipped A rows hold
    poison, the skipped C rows keep the sentinel."""
    from ddlb_amd.ops.gemm import gemm

    din, dout, mode = form
    M, N, K, grp, gs = 1024, 512, _k(din, 2), 256, 512
    a, w, ref = _case(din, M, N, K)
    rows = torch.cat([torch.arange(g * gs, g * gs + grp) for g in range(M // grp)]).to(DEV)
    phys = (M // grp) * gs
    A = torch.full((phys, K), POISON, device=DEV)
    A[rows] = a.float()
    A = padded(A.to(din))
    buf, view = sentinel_out(phys, N, dout, pad_cols=_out_pad(N, dout))
    gemm(A, w, view, M=M, a_grp=grp, a_gstride=gs, c_grp=grp, c_gstride=gs, tile=tile, mode=mode)
    torch.cuda.synchronize()
    assert torch.equal(view[rows], ref.to(dout))
    untouched(buf, M, N, rows=rows)


# ------------------------------------------------------------------ d. every answer of choose_tile
@pytest.mark.parametrize("shape,tile", [((4100, 5888), "i256"), ((4100, 2900), "256x128"),
                                        ((3000, 3900), "128x256"), ((300, 202), "128x128"),
                                        ((8192, 1024), "pt4")])
def test_auto_reaches_each_choice(shape, tile):
    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import DT_BF16, TILES

    (M, N), K = shape, _k(BF16, 1)
    assert load().choose_tile(M, N, K, DT_BF16) == TILES[tile]
    _check((BF16, BF16, "auto"), "auto", M, N, K, case=_make_case(BF16, M, N, K))


# ------------------------------------------------------------------ e. the generic kernel
GENERIC = [(BF16, BF16), (BF16, F32), (F16, F16), (F16, F32), (F32, F32), (FP8, BF16), (FP8, F16),
           (FP8, F32), (F64, F64)]


@pytest.mark.parametrize("dt", GENERIC, ids=lambda d: f"{_name(d[0])}-{_name(d[1])}")
def test_generic_kernel(dt):
    """mode="generic" at a K the fast path would take, and mode="auto" at K = 100, which it
    refuses: two row tiles with a ragged second one, a single output column."""
    from ddlb_amd.ops.gemm import fast_path_ok

    din, dout = dt
    for M, N in ((130, 70), (65, 1)):
        _check((din, dout, "generic"), "auto", M, N, 128, fast=False)
        a, w, _ = _case(din, M, N, 100)
        assert not fast_path_ok(a, w, sentinel_out(M, N, dout, pad_cols=_out_pad(N, dout))[1])
        _check((din, dout, "auto"), "auto", M, N, 100, fast=False)


def test_generic_kernel_grouped_rows_relu():
    from ddlb_amd.ops.gemm import gemm

    M, N, K = 130, 70, 100
    a, w, ref = _case(BF16, M, N, K)
    ar = torch.arange(M, device=DEV)
    a_rows, c_rows = ar // 50 * 64 + ar % 50, ar // 26 * 40 + ar % 26
    A = torch.full((int(a_rows.max()) + 1, K), POISON, device=DEV)
    A[a_rows] = a.float()
    A = padded(A.to(BF16))
    phys = int(c_rows.max()) + 1
    buf, view = sentinel_out(phys, N, F32, pad_cols=_out_pad(N, F32))
    gemm(A, w, view, M=M, a_grp=50, a_gstride=64, c_grp=26, c_gstride=40, act="relu")
    torch.cuda.synchronize()
    assert int((ref < 0).sum()) > 100
    assert torch.equal(view[c_rows], ref.clamp(min=0))
    untouched(buf, M, N, rows=c_rows)


# ------------------------------------------------------------------ f. every e4m3 code
@functools.lru_cache(maxsize=None)
def _codes_case():
    codes = torch.arange(256, dtype=torch.int32, device=DEV).to(torch.uint8)
    codes[0x7F] = 0
    codes[0xFF] = 0                                   # the two NaN codes
    ab = torch.zeros((256, 256), dtype=torch.uint8, device=DEV)
    ab[torch.arange(256), torch.arange(256)] = codes
    a = ab.view(FP8)
    w = torch.eye(256, device=DEV).to(FP8)
    return padded(a), padded(w), a.float()


def _check_codes(tile, mode):
    """``a @ I`` returns ``a``: byte ``i`` on the diagonal, decoded bit for bit (compared as
    int32). One element is compared by value: code 0x80 is -0, and its product -0 x 1 is ADDED
    to a +0 accumulator (and to the +0 products of the row's other elements), which IEEE 754
    makes +0 in every kernel (docs/ARCHITECTURE.md); no kernel can show the decoded sign."""
    from ddlb_amd.ops.gemm import gemm

    a, w, want = _codes_case()
    buf, view = sentinel_out(256, 256, F32)
    gemm(a, w, view, tile=tile, mode=mode)
    torch.cuda.synchronize()
    got = view.contiguous().view(torch.int32)
    ref = want.view(torch.int32).clone()
    assert int(ref[0x80, 0x80]) == -2 ** 31 and float(view[0x80, 0x80]) == 0.0
    ref[0x80, 0x80] = got[0x80, 0x80]
    bad = (got != ref).nonzero()
    assert bad.numel() == 0, f"{tile} {mode}: wrong at (row, col) {bad[:8].tolist()}"
    assert float(view[0x01, 0x01]) == 2.0 ** -9 and float(view[0xFE, 0xFE]) == -448.0
    untouched(buf, 256, 256)


@pytest.mark.parametrize("mode", ["auto", "mx"])
@pytest.mark.parametrize("tile", _tiles())
def test_every_e4m3_code_mfma(tile, mode):
    _check_codes(tile, mode)


def test_every_e4m3_code_generic():
    """The generic kernel's hand-written decoder (load_elem<DT_FP8>), subnormals included."""
    _check_codes("auto", "generic")


# ------------------------------------------------------------------ g. fused activations, f32 out
FLT_MIN = 2.0 ** -126


def _act64(x, act):
    """act1's formula (csrc/gemm/gemm_kernels.h) in fp64: x sigmoid(z), z = 2u for gelu (tanh
    form) and z = x for silu. (The algebraically equal 0.5 x (1 + tanh(u)) cancels in fp64 too:
    it is -0 from x = -8 and off by 4e-6 at x = -6, so it cannot be the reference in the tail.
    exp(-z) overflows fp64 only where the result is below every f32, and x / inf = -0 is then
    the right limit.)"""
    z = x if act == "silu" else 2.0 * 0.7978845608028654 * (x + 0.044715 * x * x * x)
    return x / (1.0 + torch.exp(-z))


def act_rel_err(got, x, act):
    """Largest relative error of ``got`` (f32) against the fp64 formula on the exact product
    ``x``. The denominator is floored at the smallest normal f32: below it the output format has
    no relative precision to keep (and the reference is 0 at x = 0)."""
    ref = _act64(x, act)
    rel = (got.double() - ref).abs() / ref.abs().clamp(min=FLT_MIN)
    return float(rel.max()), float(x.flatten()[int(rel.argmax())])


ACT_FORMS = [(BF16, F32, "auto"), (FP8, F32, "mx")]
ACT_TILES = ["128x128", "i256", "t4", "t8"]


@pytest.mark.parametrize("form", ACT_FORMS, ids=_form_id)
@pytest.mark.parametrize("tile", ACT_TILES)
def test_fused_relu_exact(form, tile):
    _check(form, tile, 300, 202, _k(form[0], 2), act="relu")


# measured on an MI355X (largest relative error over the cases below); asserted with 4x slack
# for other library versions, which stays below 2^-12 as required
ACT_MEASURED = {"gelu": 3.29e-6, "silu": 6.361e-6}


@pytest.mark.parametrize("act", ["gelu", "silu"])
@pytest.mark.parametrize("form", ACT_FORMS, ids=_form_id)
@pytest.mark.parametrize("tile", ACT_TILES)
def test_fused_gelu_silu_relative_error(form, tile, act):
    """gelu (tanh form) and silu fused into the f32 store, against act1's formula in fp64 on the
    exact product (integers in -187..202 for bf16, -259..293 for MX): the largest relative error,
    denominators floored at FLT_MIN (``act_rel_err``). Measured on an MI355X, the same for all
    four tiles and both forms: gelu 3.29e-6 (at x = -10, result -1.2e-37), silu 6.361e-6 (at
    x = -90, result -7.4e-38); 2e-7 and 3.5e-6 where the result is above 1e-30. Asserted at 4x
    (1.3e-5, 2.5e-5), which is below 2^-12 = 2.4e-4, 16x finer than a bf16 rounding.
    Before act1 took the x sigmoid(z) form this measured 1.0 for both: 0.5 x (1 + tanhf(u)) gave
    0.30 at x = -4 and -0 from x = -6, x / (1 + __expf(-x)) gave -0 at x = -89..-91."""
    from ddlb_amd.ops.gemm import gemm

    din, _, mode = form
    M, N, K = 300, 202, _k(din, 2)
    a, w, ref = _case(din, M, N, K)
    buf, view = sentinel_out(M, N, F32, pad_cols=_out_pad(N, F32))
    gemm(a, w, view, tile=tile, mode=mode, act=act)
    torch.cuda.synchronize()
    x = ref.double()
    assert float(x.min()) < -100 and float(x.max()) > 100  # both tails, past exp's f32 range
    rel, at = act_rel_err(view, x, act)
    bound = 4 * ACT_MEASURED[act]
    print(f"{act} {_form_id(form)} {tile}: max rel err {rel:.4g} at x = {at} (bound {bound:.4g})")
    assert bound < 2.0 ** -12
    assert rel <= bound, (rel, at)
    untouched(buf, M, N)


def test_generic_f64_keeps_fp64():
    """Products beyond 2^24: an f64 GEMM that passes through f32 anywhere cannot be exact."""
    from ddlb_amd.ops.gemm import gemm

    M, N, K = 70, 66, 100
    g = torch.Generator(device=DEV).manual_seed(64)
    a, w = ints((M, K), F64, g) * 4097.0, ints((N, K), F64, g) * 4099.0
    want = a @ w.t()
    assert int((want.float().double() != want).sum()) > want.numel() // 2
    buf, view = sentinel_out(M, N, F64)
    gemm(padded(a), padded(w), view)
    torch.cuda.synchronize()
    assert torch.equal(view, want)
    untouched(buf, M, N)
