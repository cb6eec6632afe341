"""Non-finite values through every GEMM, epilogue and quantiser, compared exactly.

a. NaN poison: the operands' padding holds NaN (``_exact.NONFINITE_POISON``), so a kernel that
   loads an element outside its view and multiplies it by a masked zero no longer passes.
b. Propagation: ``_exact.planted`` puts NaN and +-Inf into integer operands; every output
   element's class (NaN / +Inf / -Inf / the exact sum) is fixed by ``_exact.classes64`` whatever
   the order of the additions, and compared with ``_exact.same``.
c. Grouped launches: a plant reaches its own group only.
d. Epilogues: relu exactly (NaN stays NaN), gelu / silu by class, the gated forms against
   ``glu_reference``, the quantising epilogue byte for byte against the reference quantiser.
e. The MX-fp8 quantisers byte for byte against ``quantize_mx_reference``: a non-finite element
   becomes the e4m3 NaN byte with its sign and counts as 0 in its block's amax.
f. ``test_scale_byte_255``: what the block-scaled MFMA makes of the E8M0 NaN byte.
g. ``combine`` and the reduce kernel propagate by plain IEEE arithmetic.

Every comparison is ``torch.equal`` (by class, then by value) except the finite part of gelu and
silu, which keeps the bound of ``test_gemm_exact_gpu.test_fused_gelu_silu_relative_error``."""

import functools

import pytest
import torch

import test_gemm_exact_gpu as G
from _exact import (FP8, SENTINEL, classes64, exact, ints, nan_padded, padded, planted, pow2_f64,
                    same, sentinel_out, untouched)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
FP4 = torch.float4_e2m1fn_x2
NAN, INF = float("nan"), float("inf")
U8 = torch.uint8


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _ints_case(din, M, N, K):
    g = _gen(77 + 1000003 * M + 1009 * N + K)
    return ints((M, K), din, g), ints((N, K), din, g)


# ============================================================================ a. NaN poison
@functools.lru_cache(maxsize=None)
def _nan_case(din, M, N, K):
    a, w = _ints_case(din, M, N, K)
    return nan_padded(a), nan_padded(w), exact(a, w, F32)


@pytest.mark.parametrize("form", G.FORMS, ids=G._form_id)
@pytest.mark.parametrize("tile", G._tiles())
def test_nan_poison_ragged(form, tile):
    din = form[0]
    for M, N, kt in ((300, 202, 2), (130, 203, 3), (1, 4, 1)):
        K = G._k(din, kt)
        G._check(form, tile, M, N, K, case=_nan_case(din, M, N, K))


@pytest.mark.parametrize("form", G.FORMS, ids=G._form_id)
@pytest.mark.parametrize("tile", G.PING)
def test_nan_poison_whole_tiles(form, tile):
    din = form[0]
    for M, N, kt in ((256, 256, 1), (256, 256, 2), (512, 768, 3)):
        K = G._k(din, kt)
        G._check(form, tile, M, N, K, case=_nan_case(din, M, N, K))


@pytest.mark.parametrize("form", [(BF16, BF16, "auto"), (FP8, F32, "mx")], ids=G._form_id)
@pytest.mark.parametrize("tile", ["pt4", "t4"])
def test_nan_poison_grouped_rows(form, tile):
    """``test_grouped_rows_whole_tiles`` with NaN in the skipped A rows and the padding."""
    from ddlb_amd.ops.gemm import gemm

    din, dout, mode = form
    M, N, K, grp, gs = 512, 256, G._k(din, 2), 256, 512
    a, w = _ints_case(din, M, N, K)
    rows = torch.cat([torch.arange(g * gs, g * gs + grp) for g in range(M // grp)]).to(DEV)
    phys = (M // grp) * gs
    A = torch.full((phys, K), NAN, device=DEV)
    A[rows] = a.float()
    A = nan_padded(A.to(din))
    buf, view = sentinel_out(phys, N, dout, pad_cols=G._out_pad(N, dout))
    gemm(A, nan_padded(w), view, M=M, a_grp=grp, a_gstride=gs, c_grp=grp, c_gstride=gs, tile=tile,
         mode=mode)
    torch.cuda.synchronize()
    assert torch.equal(view[rows], exact(a, w, dout))
    untouched(buf, M, N, rows=rows)


@pytest.mark.parametrize("dt", G.GENERIC, ids=lambda d: f"{G._name(d[0])}-{G._name(d[1])}")
def test_nan_poison_generic(dt):
    din, dout = dt
    for M, N in ((130, 70), (65, 1)):
        G._check((din, dout, "auto"), "auto", M, N, 100, fast=False,
                 case=_nan_case(din, M, N, 100))


def _pack_ints(v):
    from ddlb_amd.ops.mx import pack_e2m1

    code = torch.tensor((0, 2, 4, 5), device=v.device)[v.abs().long()]
    return pack_e2m1(code | ((v < 0).long() << 3))


def _scaled_case(fmt, M, N, K, seed, R=None):
    """Integer operands as MX-fp8 / MXFP4 data with random scale bytes 125..129:
    ``(a, w, s_a, s_w, want)``, ``want`` the exact fp64 product as f32."""
    g = _gen(seed)
    av, wv = ints((M, K), F32, g), ints((N, K), F32, g)
    s_a = (127 + torch.randint(-2, 3, (M, K // 32), generator=g, device=DEV)).to(U8)
    s_w = (127 + torch.randint(-2, 3, (N, K // 32), generator=g, device=DEV)).to(U8)

    def deq(v, s):
        return (v.double().reshape(-1, K // 32, 32)
                * pow2_f64(s.to(torch.int64) - 127).unsqueeze(2)).reshape(-1, K)

    want = (deq(av, s_a) @ deq(wv, s_w).t()).float()
    if fmt == "mxfp4":
        return _pack_ints(av), _pack_ints(wv), s_a, s_w, want
    return av.to(FP8), wv.to(FP8), s_a, s_w, want


def _scaled_tiles(fmt):
    from ddlb_amd.ops.gemm import SCALED_FP4_TILES, SCALED_TILES

    return ("auto",) + tuple(SCALED_FP4_TILES if fmt == "mxfp4" else SCALED_TILES)


@pytest.mark.parametrize("fmt", ["mx", "mxfp4"])
def test_nan_poison_scaled(fmt):
    """The block-scaled GEMMs: data rows padded with the NaN byte (fp4: 6.0 pairs), scale rows
    padded with the NaN scale byte 255."""
    from ddlb_amd.ops.gemm import gemm

    kind = "fp4" if fmt == "mxfp4" else None
    for M, N, K in ((300, 202, 512), (130, 203, 256), (256, 256, 768)):
        a, w, s_a, s_w, want = _scaled_case(fmt, M, N, K, 31 + M)
        a, w = nan_padded(a, kind), nan_padded(w, kind)
        s_a, s_w = nan_padded(s_a, "scale"), nan_padded(s_w, "scale")
        for tile in _scaled_tiles(fmt):
            buf, view = sentinel_out(M, N, F32, pad_cols=G._out_pad(N, F32))
            gemm(a, w, view, a_scale=s_a, w_scale=s_w, tile=tile)
            torch.cuda.synchronize()
            assert torch.equal(view, want), (fmt, tile, M, N, K)
            untouched(buf, M, N)


def _grouped_case(form, counts, N, K, seed, poison_nan=True):
    """Per-expert integer weights with NaN (fp4: 6.0, scales: 255) between the experts, rows of
    ``a`` for the groups: ``(a, w, offsets, o, kw, av, wv, sa, sv)``."""
    g = _gen(seed)
    E, T = len(counts), sum(counts)
    o = [0]
    for c in counts:
        o.append(o[-1] + c)
    av, wv = ints((T, K), F32, g), ints((E, N, K), F32, g)
    pad = 4
    scaled = form in ("mx", "mxfp4")
    if form == "mxfp4":
        wb = torch.full((E, N + pad, K // 2), 0x77, dtype=U8, device=DEV)
        wb[:, :N] = _pack_ints(wv.reshape(E * N, K)).view(U8).reshape(E, N, K // 2)
        w, a = wb.view(FP4)[:, :N], _pack_ints(av)
    elif form == "mx":
        wb = torch.full((E, N + pad, K), 0x7F, dtype=U8, device=DEV)
        wb[:, :N] = wv.to(FP8).view(U8)
        w, a = wb.view(FP8)[:, :N], av.to(FP8)
    else:
        wb = torch.full((E, N + pad, K), NAN, dtype=form, device=DEV)
        wb[:, :N] = wv.to(form)
        w, a = wb[:, :N], av.to(form)
    kw, sa, sv = {}, None, None
    if scaled:
        sa = (127 + torch.randint(-2, 3, (T, K // 32), generator=g, device=DEV)).to(U8)
        sv = (127 + torch.randint(-2, 3, (E, N, K // 32), generator=g, device=DEV)).to(U8)
        sb = torch.full((E, N + pad, K // 32), 255, dtype=U8, device=DEV)
        sb[:, :N] = sv
        kw = dict(a_scale=nan_padded(sa, "scale"), w_scale=sb[:, :N])
    kind = "fp4" if form == "mxfp4" else None
    offs = torch.tensor(o, dtype=torch.int32, device=DEV)
    return nan_padded(a, kind), w, offs, o, kw, av, wv, sa, sv


def _deq(v, s):
    v = v.double()
    if s is None:
        return v
    K = v.shape[-1]
    return (v.reshape(-1, K // 32, 32) * pow2_f64(s.reshape(-1, K // 32).to(torch.int64) - 127)
            .unsqueeze(2)).reshape(v.shape)


@pytest.mark.parametrize("form", [BF16, "mx"], ids=["bf16", "mxfp8"])
def test_nan_poison_gemm_grouped(form):
    from ddlb_amd.ops.gemm import gemm_grouped

    counts, N, K = (130, 0, 1, 257), 128, 256
    a, w, offs, o, kw, av, wv, sa, sv = _grouped_case(form, counts, N, K, 5)
    buf, out = sentinel_out(o[-1], N, F32, pad_cols=4)
    gemm_grouped(a, w, offs, out, tile="128x128", **kw)
    torch.cuda.synchronize()
    for g in range(len(counts)):
        lo, hi = o[g], o[g + 1]
        want = (_deq(av[lo:hi], None if sa is None else sa[lo:hi])
                @ _deq(wv[g], None if sv is None else sv[g]).t()).float()
        assert torch.equal(out[lo:hi], want), (form, g)
    untouched(buf, o[-1], N)


def _kgrouped_case(counts, M, N, seed):
    """MX-fp8 operands of a K-grouped GEMM in the padded K layout: integer data, scale bytes
    125..129, the padding columns of every group zero data with scale 127, and everything past
    the last group's columns poisoned (NaN bytes, scale 255)."""
    from ddlb_amd.ops.gemm import kgrouped_capacity, padded_offsets

    g = _gen(seed)
    E, T = len(counts), sum(counts)
    o = [0]
    for c in counts:
        o.append(o[-1] + c)
    offs = torch.tensor(o, dtype=torch.int32, device=DEV)
    cap = kgrouped_capacity(T, E, 128)
    k0 = padded_offsets(offs, T, 128)
    av, wv = torch.zeros((M, cap), device=DEV), torch.zeros((N, cap), device=DEV)
    sa = torch.full((M, cap // 32), 127, dtype=U8, device=DEV)
    sw = torch.full((N, cap // 32), 127, dtype=U8, device=DEV)
    for e in range(E):
        n = counts[e]
        av[:, k0[e]:k0[e] + n] = ints((M, n), F32, g)
        wv[:, k0[e]:k0[e] + n] = ints((N, n), F32, g)
    sa[:, :k0[-1] // 32] = (127 + torch.randint(-2, 3, (M, k0[-1] // 32), generator=g,
                                                device=DEV)).to(U8)
    sw[:, :k0[-1] // 32] = (127 + torch.randint(-2, 3, (N, k0[-1] // 32), generator=g,
                                                device=DEV)).to(U8)
    return av, wv, sa, sw, offs, k0, cap, T


def test_nan_poison_gemm_kgrouped():
    """Columns past the last group (never owned by a group) hold NaN bytes and scale 255, and so
    do the paddings of the operand and scale rows."""
    from ddlb_amd.ops.gemm import gemm_kgrouped

    counts, M, N = (130, 0, 1, 128), 130, 203
    av, wv, sa, sw, offs, k0, cap, T = _kgrouped_case(counts, M, N, 9)
    assert k0[-1] < cap
    a8, w8 = av.to(FP8), wv.to(FP8)
    for q, s in ((a8, sa), (w8, sw)):
        q.view(U8)[:, k0[-1]:] = 0x7F
        s[:, k0[-1] // 32:] = 255
    E = len(counts)
    buf = torch.full((E, M + 3, N + 5), SENTINEL, dtype=F32, device=DEV)
    out = buf[:, :M, :N]
    gemm_kgrouped(nan_padded(a8), nan_padded(w8), offs, T, out, a_scale=nan_padded(sa, "scale"),
                  w_scale=nan_padded(sw, "scale"), tile="128x128")
    torch.cuda.synchronize()
    for e in range(E):
        sl = slice(k0[e], k0[e + 1])
        want = (_deq(av[:, sl], sa[:, k0[e] // 32:k0[e + 1] // 32])
                @ _deq(wv[:, sl], sw[:, k0[e] // 32:k0[e + 1] // 32]).t()).float() \
            if k0[e + 1] > k0[e] else torch.zeros((M, N), device=DEV)
        assert torch.equal(out[e], want), e
        untouched(buf[e], M, N)


def _side_nan(x, left=8, right=8):
    """``x`` as the middle columns of a buffer whose side columns and extra rows hold NaN."""
    R, C = x.shape
    buf = torch.full((R + 2, left + C + right), NAN, dtype=x.dtype, device=x.device)
    buf[:R, left:left + C] = x
    return buf[:R, left:left + C]


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=G._name)
@pytest.mark.parametrize("fmt", ["mx", "mxfp4"])
def test_nan_poison_quantisers(dtype, fmt):
    """The three row quantisers and the transposer on a strided ``x`` whose neighbours are NaN:
    byte for byte what they write for a contiguous copy."""
    from ddlb_amd.ops.mx import (quantize_mx, quantize_mx_2way, quantize_mx_gather, quantize_mx_t,
                                 quantize_mxfp4)

    g = _gen(3)
    R, C = 256, 512
    x = (torch.randn((R, C), generator=g, device=DEV) * 4).to(dtype)
    v = _side_nan(x)
    assert v.data_ptr() % 16 == 0 and (v.stride(0) * v.element_size()) % 16 == 0
    row = quantize_mxfp4 if fmt == "mxfp4" else quantize_mx
    src = torch.tensor([5, -1, 0, R - 1, R, 17], dtype=torch.int32, device=DEV)
    pairs = [(row(v), row(x)),
             (quantize_mx_gather(v, src, fmt=fmt), quantize_mx_gather(x, src, fmt=fmt)),
             (quantize_mx_t(v, fmt=fmt), quantize_mx_t(x, fmt=fmt)),
             (quantize_mx_2way(v, fmt=fmt), quantize_mx_2way(x, fmt=fmt))]
    torch.cuda.synchronize()
    for i, (got, want) in enumerate(pairs):
        for gt, wt in zip(got, want):
            assert torch.equal(gt.view(U8), wt.view(U8)), (i, fmt, dtype)


# ============================================================================ b. propagation
def _planted_case(din, M, N, K):
    a, w = _ints_case(din, M, N, K)
    a, w, p = planted(a, w)
    return a, w, classes64(a, w), p


_pcase = functools.lru_cache(maxsize=None)(_planted_case)


def _check_planted(form, tile, M, N, K, **kw):
    from ddlb_amd.ops.gemm import gemm

    din, dout, mode = form
    a, w, ref, p = _pcase(din, M, N, K)
    if din != FP8:  # every class occurs (fp8 has no Inf: NaN rows and columns only)
        assert bool(torch.isnan(ref).any()) and bool((ref == INF).any()) \
            and bool((ref == -INF).any())
        row = ref[p["r1"]]
        assert bool(torch.isnan(row).any()) and bool((row == INF).any()) \
            and bool((row == -INF).any())
    assert bool(torch.isnan(ref[p["r0"]]).all()) and bool(torch.isnan(ref[:, p["n0"]]).all())
    assert int(torch.isfinite(ref).sum()) > ref.numel() // 2
    buf, view = sentinel_out(M, N, dout, pad_cols=G._out_pad(N, dout))
    gemm(padded(a), padded(w), view, tile=tile, mode=mode, **kw)
    torch.cuda.synchronize()
    same(view, ref.to(F32).to(dout))
    untouched(buf, M, N)


@pytest.mark.parametrize("form", G.FORMS, ids=G._form_id)
@pytest.mark.parametrize("tile", G._tiles())
def test_propagation_ragged(form, tile):
    din = form[0]
    for M, N, kt in ((300, 202, 2), (130, 203, 3), (300, 202, 1)):
        _check_planted(form, tile, M, N, G._k(din, kt))


@pytest.mark.parametrize("form", G.FORMS, ids=G._form_id)
@pytest.mark.parametrize("tile", G.PING)
def test_propagation_whole_tiles(form, tile):
    din = form[0]
    for M, N, kt in ((256, 256, 1), (256, 256, 2), (512, 768, 3)):
        _check_planted(form, tile, M, N, G._k(din, kt))


@pytest.mark.parametrize("dt", G.GENERIC, ids=lambda d: f"{G._name(d[0])}-{G._name(d[1])}")
def test_propagation_generic(dt):
    """The generic kernel (f64 included), with its own e4m3 decoder's NaN branch."""
    din, dout = dt
    _check_planted((din, dout, "generic"), "auto", 130, 70, 128, )
    _check_planted((din, dout, "auto"), "auto", 130, 70, 100)


@pytest.mark.parametrize("tile", ["pt4", "t4", "256x256"])
@pytest.mark.parametrize("S", [2, 4])
def test_propagation_ksplit(tile, S):
    """The public K-split: pt4's one launch over (slice, tile) pairs and the slice-by-slice
    fallback. The +Inf and -Inf of row r2 lie in the first and the last slice, so that row's NaN
    arises only in the reduce kernel."""
    from ddlb_amd.ops.gemm import gemm

    M, N, K = 256, 512, 512
    a, w, ref, p = _pcase(BF16, M, N, K)
    assert p["k2p"] < K // S and p["k2m"] >= K - K // S
    buf = torch.full((M + 3, N), SENTINEL, dtype=F32, device=DEV)
    gemm(padded(a), padded(w), buf[:M], tile=tile, ksplit=S)
    torch.cuda.synchronize()
    same(buf[:M], ref.to(F32))
    untouched(buf, M, N)


@pytest.fixture(scope="module")
def comm():
    import os

    from conftest import free_port
    from ddlb_amd.communicator import Communicator

    os.environ["DDLB_CHILD_INIT_METHOD"] = f"tcp://127.0.0.1:{free_port()}"
    c = Communicator()
    c.ensure_process_group()
    yield c
    Communicator.reset()
    os.environ.pop("DDLB_CHILD_INIT_METHOD", None)


@pytest.mark.parametrize("tile", ["pt4", "t4"])
def test_propagation_plan_ksplit_partials(comm, tile):
    """``Plan.gemm`` with ``ksplit=2`` writes the slices' partials (``tests/_exact_plan.py``):
    partial j has the classes of the product over K-slice j. Row r2 is +-Inf in partial 0 (its
    +Inf plant) and in partial 1 (its -Inf plant), and NaN in neither except where Inf meets 0."""
    import _exact_plan as P
    from ddlb_amd.ops.gemm import TILES
    from ddlb_amd.parallel.plan import Plan

    M, N, K, S = 256, 256, 256, 2
    a, w, _, p = _pcase(BF16, M, N, S * K)
    plan = Plan(0, 1, nstreams=1, stream_priority=[0])
    wm, am = P.place(plan, "w", N, S * K, BF16), P.place(plan, "a", M, S * K, BF16)
    cm = P.place(plan, "c", S * M, N, F32, align=8, guard=2)
    plan.gemm(0, am.ref, wm.ref, cm.ref, M=M, N=N, K=K, lda=am.ld, ldb=wm.ld, ldc=cm.ld,
              din=P.plan_dt(BF16), dout=P.plan_dt(F32), tile=TILES[tile], mode=0, ksplit=S)
    with P.bound_plan(comm, plan) as bound:
        P.put_operand(bound, wm, w)
        P.put_operand(bound, am, a)
        P.put_sentinel(bound, cm)
        P.run(bound)
        for j in range(S):
            sl = slice(j * K, (j + 1) * K)
            want = classes64(a[:, sl], w[:, sl]).float()
            assert bool(torch.isinf(want[p["r2"]]).any())
            same(P.view(bound, cm)[j * M:(j + 1) * M], want)
        P.check_untouched(bound, [cm], [(cm, None, N)])


def _nan_codes_case():
    codes = torch.arange(256, dtype=torch.int32, device=DEV).to(U8)
    ab = torch.zeros((256, 256), dtype=U8, device=DEV)
    ab[torch.arange(256), torch.arange(256)] = codes
    a = ab.view(FP8)
    w = torch.eye(256, device=DEV).to(FP8)
    want = a.float()                     # NaN at [0x7F, 0x7F] and [0xFF, 0xFF] ...
    want[0x7F] = NAN                     # ... and NaN x 0 = NaN along the two rows
    want[0xFF] = NAN
    return padded(a), padded(w), want


def _check_nan_codes(tile, mode):
    """``_check_codes`` with the two NaN bytes left on the diagonal: ``a @ I`` is NaN in exactly
    rows 0x7F and 0xFF, every other row is the decoded byte."""
    from ddlb_amd.ops.gemm import gemm

    a, w, want = _nan_codes_case()
    buf, view = sentinel_out(256, 256, F32)
    gemm(a, w, view, tile=tile, mode=mode)
    torch.cuda.synchronize()
    same(view, want)
    untouched(buf, 256, 256)


@pytest.mark.parametrize("mode", ["auto", "mx"])
@pytest.mark.parametrize("tile", G._tiles())
def test_nan_codes_mfma(tile, mode):
    _check_nan_codes(tile, mode)


def test_nan_codes_generic():
    _check_nan_codes("auto", "generic")


# ============================================================================ c. grouped forms
@pytest.mark.parametrize("form", [BF16, "mx"], ids=["bf16", "mxfp8"])
def test_grouped_plants_stay_in_their_group(form):
    """A NaN in one row of group 0, a NaN in ``w[3]``: group 0 has one NaN row, group 3 one NaN
    column, the empty group 1 beside them writes nothing, group 2 (no plant) is bit for bit the
    ungrouped ``gemm``."""
    from ddlb_amd.ops.gemm import gemm, gemm_grouped

    counts, N, K = (130, 0, 64, 257), 128, 256
    a, w, offs, o, kw, av, wv, sa, sv = _grouped_case(form, counts, N, K, 6)
    a, w = a.clone(), w.clone()
    if form == BF16:
        a[7, 40] = NAN
        w[3, 5, K - 1] = NAN
    else:
        a.view(U8)[7, 40] = 0x7F
        w.view(U8)[3, 5, K - 1] = 0xFF
    buf, out = sentinel_out(o[-1], N, F32, pad_cols=4)
    gemm_grouped(a, w, offs, out, tile="128x128", **kw)
    torch.cuda.synchronize()
    want = torch.empty((o[-1], N), dtype=torch.float64, device=DEV)
    for g in range(len(counts)):
        lo, hi = o[g], o[g + 1]
        want[lo:hi] = (_deq(av[lo:hi], None if sa is None else sa[lo:hi])
                       @ _deq(wv[g], None if sv is None else sv[g]).t())
    want[7] = NAN
    want[o[3]:o[4], 5] = NAN
    same(out, want.float())
    lo, hi = o[2], o[3]
    sl = dict(a_scale=kw["a_scale"][lo:hi], w_scale=kw["w_scale"][2]) if kw else {}
    assert torch.equal(out[lo:hi], gemm(a[lo:hi], w[2], out_dtype=F32, tile="128x128", **sl))
    untouched(buf, o[-1], N)


def test_kgrouped_plant_stays_in_its_group():
    """A NaN byte inside group 2's column range reaches ``out[2]`` only (its row); the expert
    without tokens stays +0.0."""
    from ddlb_amd.ops.gemm import gemm_kgrouped

    counts, M, N = (130, 0, 70, 128), 130, 203
    av, wv, sa, sw, offs, k0, cap, T = _kgrouped_case(counts, M, N, 10)
    a8, w8 = av.to(FP8), wv.to(FP8)
    a8.view(U8)[9, k0[2] + 3] = 0x7F
    E = len(counts)
    buf = torch.full((E, M + 3, N + 5), SENTINEL, dtype=F32, device=DEV)
    out = buf[:, :M, :N]
    gemm_kgrouped(a8, w8, offs, T, out, a_scale=sa, w_scale=sw, tile="128x128")
    torch.cuda.synchronize()
    for e in range(E):
        sl, bl = slice(k0[e], k0[e + 1]), slice(k0[e] // 32, k0[e + 1] // 32)
        want = (_deq(av[:, sl], sa[:, bl]) @ _deq(wv[:, sl], sw[:, bl]).t()).float() \
            if k0[e + 1] > k0[e] else torch.zeros((M, N), device=DEV)
        if e == 2:
            want[9] = NAN
        same(out[e], want)
        untouched(buf[e], M, N)
    assert torch.equal(out[1].view(torch.int32), torch.zeros((M, N), dtype=torch.int32,
                                                             device=DEV))


# ============================================================================ d. epilogues
def _act_ref(x32, act):
    from ddlb_amd.ops.gemm import ACTS
    from ddlb_amd.parallel.sim import apply_act

    return apply_act(x32, ACTS[act])


def _class_of(x):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf."""
    return torch.isnan(x) * 1 + (x == INF) * 2 + (x == -INF) * 3


def _check_act(got, x64, act):
    """relu: exact. gelu / silu: the reference's class everywhere, and on its finite elements the
    relative bound of ``test_fused_gelu_silu_relative_error``."""
    want = _act_ref(x64.float(), act)
    if act == "relu":
        same(got, want)
        return
    assert torch.equal(_class_of(got), _class_of(want)), act
    fin = torch.isfinite(want)
    rel, at = G.act_rel_err(got[fin], x64[fin], act)
    assert rel <= 4 * G.ACT_MEASURED[act], (act, rel, at)


@pytest.mark.parametrize("act", ["relu", "gelu", "silu"])
@pytest.mark.parametrize("form", G.ACT_FORMS, ids=G._form_id)
@pytest.mark.parametrize("tile", G.ACT_TILES)
def test_activation_classes(form, tile, act):
    from ddlb_amd.ops.gemm import gemm

    din, _, mode = form
    M, N, K = 300, 202, G._k(din, 2)
    a, w, ref, p = _pcase(din, M, N, K)
    buf, view = sentinel_out(M, N, F32, pad_cols=G._out_pad(N, F32))
    gemm(padded(a), padded(w), view, tile=tile, mode=mode, act=act)
    torch.cuda.synchronize()
    _check_act(view, ref, act)
    untouched(buf, M, N)


@pytest.mark.parametrize("act", ["relu", "gelu", "silu"])
def test_activation_classes_generic(act):
    from ddlb_amd.ops.gemm import gemm

    M, N, K = 130, 70, 100
    a, w, ref, p = _pcase(BF16, M, N, K)
    buf, view = sentinel_out(M, N, F32, pad_cols=G._out_pad(N, F32))
    gemm(padded(a), padded(w), view, act=act)
    torch.cuda.synchronize()
    _check_act(view, ref, act)
    untouched(buf, M, N)


def _glu_case(M=130, F=128, K=128):
    """bf16 operands of a gated GEMM with plants: NaN in gate row 3 of W (a NaN gate column), NaN
    in up row 40 (a NaN up column), +Inf in up row 70 against a gate row 70 of zeros (its gate
    is exactly 0, after relu and before: 0 x Inf = NaN), and A untouched. Returns
    ``(a, w packed, c64 classes of the [M, 2F] product)``."""
    from ddlb_amd.ops.gemm import pack_glu

    g = _gen(21)
    a = ints((M, K), BF16, g)
    gate, up = ints((F, K), BF16, g), ints((F, K), BF16, g)
    gate[3, 9] = NAN
    up[40, K - 1] = NAN
    gate[70] = 0
    up[70, 0] = INF
    a[:4, 0] = torch.tensor([-1.0, 0.0, 2.0, 1.0], dtype=BF16, device=DEV)
    w = pack_glu(gate, up)
    return a, w, classes64(a, w)


@pytest.mark.parametrize("act", ["none", "relu", "gelu", "silu"])
@pytest.mark.parametrize("tile", ["128x128", "256x128"])
def test_glu_classes(act, tile):
    from ddlb_amd.ops.gemm import gemm, glu_reference

    a, w, c64 = _glu_case()
    M, F = a.shape[0], w.shape[0] // 2
    want = glu_reference(c64.float(), act)
    assert bool(torch.isnan(want[:, 3]).all()) and bool(torch.isnan(want[:, 40]).all())
    assert bool(torch.isnan(want[:, 70]).all())       # 0 x +-Inf, and 0 x NaN in row 1
    buf, view = sentinel_out(M, F, F32, pad_cols=4)
    gemm(padded(a), padded(w), view, tile=tile, act=act, glu=True)
    torch.cuda.synchronize()
    if act in ("none", "relu"):
        same(view, want)
    else:
        assert torch.equal(_class_of(view), _class_of(want)), act
        # the finite part against act1's formula in fp64 (torch's own f32 gelu is -0 from
        # x = -6): the activation within its bound, then one f32 multiply by an exact integer,
        # which adds one rounding (2^-24 relative)
        v = c64.reshape(M, F // 32, 2, 32)
        ref = (G._act64(v[:, :, 0], act) * v[:, :, 1]).reshape(M, F)
        fin = torch.isfinite(want)
        # (the activation's denominator floor FLT_MIN is multiplied by |up| like its error)
        floor = (G.FLT_MIN * v[:, :, 1].abs().clamp(min=1.0)).reshape(M, F)
        rel = ((view[fin].double() - ref[fin]).abs()
               / torch.maximum(ref[fin].abs(), floor[fin])).max()
        assert float(rel) <= 4 * G.ACT_MEASURED[act] + 2.0 ** -24, (act, float(rel))
    untouched(buf, M, F)


def _quant_bytes(got, want):
    for g, w in zip(got, want):
        bad = (g.view(U8) != w.view(U8)).nonzero()
        assert bad.numel() == 0, f"{bad.shape[0]} bytes differ, first at {bad[:4].tolist()}"


FMTS = ["mx", "mxfp4"]


def _row_ref(fmt):
    from ddlb_amd.ops.mx import quantize_mx_reference, quantize_mxfp4_reference

    return quantize_mxfp4_reference if fmt == "mxfp4" else quantize_mx_reference


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("glu", [False, True], ids=["plain", "glu"])
def test_quantising_epilogue_nonfinite(act, glu, fmt):
    """``out_quant``: ``(q, s)`` byte for byte the reference quantiser on the f32 result the
    dense launch writes (NaN rows and columns, +-Inf, and with relu the zeros of -Inf)."""
    from ddlb_amd.ops.gemm import gemm

    if glu:
        a, w, _ = _glu_case(M=130, F=256, K=128)
    else:
        a, w, _, _ = _pcase(BF16, 300, 256, 128)
    a, w = padded(a), padded(w)
    for tile in ("128x128", "256x128"):
        dense = gemm(a, w, out_dtype=F32, tile=tile, act=act, glu=glu)
        q, s = gemm(a, w, tile=tile, act=act, glu=glu, out_quant=fmt)
        torch.cuda.synchronize()
        assert bool(torch.isnan(dense).any()) and bool(torch.isfinite(dense).any())
        q_ref, s_ref = _row_ref(fmt)(dense)
        assert bool((s_ref == 255).any()) == (fmt == "mxfp4")
        _quant_bytes((q, s), (q_ref, s_ref))


@pytest.mark.parametrize("fmt", FMTS)
def test_quantising_epilogue_nonfinite_grouped(fmt):
    from ddlb_amd.ops.gemm import gemm_grouped

    counts, N, K = (130, 0, 64, 257), 256, 256
    a, w, offs, o, kw, *_ = _grouped_case(BF16, counts, N, K, 6)
    a, w = a.clone(), w.clone()
    a[7, 40] = NAN
    a[200, 0] = INF
    w[3, 5, K - 1] = NAN
    dense = gemm_grouped(a, w, offs, out_dtype=F32, tile="128x128", act="relu")
    q, s = gemm_grouped(a, w, offs, tile="128x128", act="relu", out_quant=fmt)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dense).any()) and bool((dense == INF).any())
    _quant_bytes((q, s), _row_ref(fmt)(dense))


# ============================================================================ e. quantisers
def _special_rows(dtype, R=256, C=512):
    """Ordinary data (randn x 2^-6..6 per block) with the quantisers' edge rows of
    ``test_mx_scaled_gpu`` and the non-finite blocks: one NaN among ordinary values, -NaN, +Inf
    beside the block's finite maximum, -Inf alone, all 32 elements non-finite, a non-finite first
    and last element of a row, one non-finite among subnormals; for the transposer, non-finite
    elements in the first and the last row of a column block."""
    g = _gen(12)
    x = torch.randn(R, C // 32, 32, generator=g, device=DEV)
    x = torch.ldexp(x, torch.randint(-6, 7, (R, C // 32, 1), generator=g, device=DEV))
    x = x.reshape(R, C).to(dtype)
    x[0] = 0
    x[1, 32:64] = 0
    x[2] = 0
    x[2, 77] = -1.5
    for i, j in enumerate((-9, -1, 0, 2, 6)):
        x[3 + i, 0:32] = 3.0 * 2.0 ** j
        x[3 + i, 7] = 448.0 * 2.0 ** j
        x[3 + i, 32:64] = -5.0 * 2.0 ** j
        x[3 + i, 40] = 480.0 * 2.0 ** j
    tiny = 2.0 ** -24 if dtype == F16 else 2.0 ** -130
    x[9, 0:32] = tiny
    # -NaN by its bits (a conversion makes the canonical, positive NaN of it)
    word, bits = {BF16: (torch.int16, -64), F16: (torch.int16, -512),
                  F32: (torch.int32, -(1 << 22))}[dtype]
    neg_nan = torch.tensor([bits], dtype=word, device=DEV).view(dtype)[0]
    x[10, 5] = NAN                         # one NaN among ordinary values
    x[11, 37] = neg_nan                    # -NaN
    x[12, 64:96] = 1.0
    x[12, 70] = 448.0                      # +Inf beside the block's finite maximum
    x[12, 71] = INF
    x[13, 96:128] = 0
    x[13, 100] = -INF                      # -Inf alone
    x[14, 0:32] = torch.tensor([NAN, INF, -INF, NAN] * 8, device=DEV).to(dtype)   # all 32
    x[14, 3] = neg_nan
    x[15, 0] = INF                         # the first and the last element of a row
    x[15, C - 1] = NAN
    x[16, 32:64] = tiny                    # one non-finite among subnormals
    x[16, 33] = -INF
    x[32, 300] = NAN                       # the first and the last row of a column block
    x[63, 300] = -INF
    x[127, 301] = INF                      # ... and on both sides of a 128-row boundary
    x[128, 301] = neg_nan
    return x


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=G._name)
def test_quantisers_nonfinite(dtype, fmt):
    """The row quantiser, quantize_mx_gather, quantize_mx_t and quantize_mx_2way byte for byte
    against their references on the special rows, MX-fp8 and MXFP4."""
    from ddlb_amd.ops.mx import (quantize_mx, quantize_mx_2way, quantize_mx_gather,
                                 quantize_mx_gather_reference, quantize_mx_t,
                                 quantize_mx_t_reference, quantize_mxfp4)

    x = _special_rows(dtype)
    R = x.shape[0]
    q_ref, s_ref = _row_ref(fmt)(x)
    qb = q_ref.view(U8)
    if fmt == "mx":
        assert int(qb[10, 5]) == 0x7F and int(qb[11, 37]) == 0xFF and int(qb[12, 71]) == 0x7F
        assert int(qb[12, 70]) == 0x7E and int(s_ref[12, 2]) == 127      # 448 at e = 0
        assert int(qb[13, 100]) == 0xFF and int(s_ref[13, 3]) == 127
        assert int(s_ref[14, 0]) == 127 and bool(((qb[14, :32] & 0x7F) == 0x7F).all())
        assert int(s_ref[16, 1]) == (127 - 32 if dtype == F16 else 0)  # 2^-24 = 0.5 x 2^-23
        assert not bool((s_ref == 255).any())
    else:                                  # nibbles 0x7 | sign << 3, the blocks' scale bytes 255
        assert int(qb[10, 2]) >> 4 == 0x7 and int(qb[11, 18]) >> 4 == 0xF
        # 448 / 2^7 = 3.5 ties to 4 (code 6) beside the +Inf's 0x7; -Inf alone: 0xF
        assert int(qb[12, 35]) == 0x76 and (int(qb[13, 50]) & 0xF) == 0xF
        assert bool(((qb[14, :16] & 0x77) == 0x77).all())
        bad = (~torch.isfinite(x)).reshape(R, -1, 32).any(dim=2)
        assert torch.equal(s_ref == 255, bad) and int(bad.sum()) >= 12
    _quant_bytes((quantize_mxfp4 if fmt == "mxfp4" else quantize_mx)(x), (q_ref, s_ref))
    src = torch.tensor([14, -1, 10, R, 16, 12, 11, 13, 15, 0], dtype=torch.int32, device=DEV)
    _quant_bytes(quantize_mx_gather(x, src, fmt=fmt), quantize_mx_gather_reference(x, src, fmt))
    t_ref = quantize_mx_t_reference(x, fmt)
    _quant_bytes(quantize_mx_t(x, fmt=fmt), t_ref)
    _quant_bytes(quantize_mx_2way(x, fmt=fmt), (q_ref, s_ref) + tuple(t_ref))
    torch.cuda.synchronize()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=G._name)
def test_quantiser_t_grouped_nonfinite(dtype, fmt):
    """quantize_mx_t_grouped: non-finite elements in the last row of one group and the first row
    of the next (one column), so each lands in its own group's block."""
    from ddlb_amd.ops.mx import quantize_mx_t_grouped, quantize_mx_t_grouped_reference

    x = _special_rows(dtype)
    o = [0, 130, 130, 131, 256]
    x[129, 8] = NAN
    x[130, 8] = -INF
    x[131, 8] = INF
    offs = torch.tensor(o, dtype=torch.int32, device=DEV)
    qt, st = quantize_mx_t_grouped(x, offs, fmt=fmt)
    torch.cuda.synchronize()
    q_ref, s_ref, written = quantize_mx_t_grouped_reference(x, offs, fmt)
    per = 2 if fmt == "mxfp4" else 1
    wq = written[::per].nonzero().flatten()             # owned data bytes; owned scale bytes
    wsc = written[::32].nonzero().flatten()
    assert torch.equal(qt.view(U8)[:, wq], q_ref[:, wq])
    assert torch.equal(st[:, wsc], s_ref[:, wsc])
    if fmt == "mx":
        assert int((q_ref[8] == 0x7F).sum()) >= 2 and int((q_ref[8] == 0xFF).sum()) >= 1
    else:
        assert int((s_ref[8] == 255).sum()) >= 3        # a block in each of the three groups


@pytest.mark.parametrize("fmt", FMTS)
def test_quantised_nan_rows_through_the_scaled_gemm(fmt):
    """End to end: ``gemm(q, wq, a_scale=s, ..)`` is NaN in exactly the rows the reference's
    dequantisation makes NaN (a NaN byte; for MXFP4 a scale byte 255), and elsewhere equal to the
    run on the same data with the bad elements replaced by 0."""
    from ddlb_amd.ops.gemm import gemm
    from ddlb_amd.ops.mx import dequantize_mx, dequantize_mxfp4, quantize_mx, quantize_mxfp4

    quant = quantize_mxfp4 if fmt == "mxfp4" else quantize_mx
    x = _special_rows(BF16)
    g = _gen(14)
    w = torch.randn((202, x.shape[1]), generator=g, device=DEV).to(BF16)
    q, s = quant(x)
    wq, ws = quant(w)
    clean = torch.where(torch.isfinite(x), x, torch.zeros_like(x))
    q0, s0 = quant(clean)
    assert torch.equal(s[s != 255], s0[s != 255]) and bool((s == 255).any()) == (fmt == "mxfp4")
    bad_rows = torch.isnan((dequantize_mxfp4 if fmt == "mxfp4" else dequantize_mx)(q, s)) \
        .any(dim=1)
    assert torch.equal(bad_rows, (~torch.isfinite(x)).any(dim=1)) and int(bad_rows.sum()) >= 10
    for tile in _scaled_tiles(fmt):
        got = gemm(q, wq, out_dtype=F32, a_scale=s, w_scale=ws, tile=tile)
        base = gemm(q0, wq, out_dtype=F32, a_scale=s0, w_scale=ws, tile=tile)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(base).all())
        assert torch.equal(torch.isnan(got), bad_rows.unsqueeze(1).expand_as(got)), tile
        assert torch.equal(got[~bad_rows], base[~bad_rows]), tile


# ============================================================================ f. scale byte 255
@pytest.mark.parametrize("fmt", ["mx", "mxfp4"])
def test_scale_byte_255(fmt):
    """An ``a_scale`` byte set to 255 (the E8M0 NaN), one scaled GEMM per tile code: over integer
    elements in row 70, over a block of zeros in row 3 (last K-tile), and one ``w_scale`` byte in
    row 9 of W. In the OCP MX rule every element of such a block is NaN, zero-valued ones
    included, and the block-scaled MFMA of gfx950 follows it (docs/RESULTS.md): those output rows
    and that column are NaN everywhere, for every tile and both formats. The MXFP4 contract of
    ``ddlb_amd/ops/mx.py`` (a block with a non-finite element gets ``s = 255``) rests on this.
    Every other element is exact and nothing outside the output is written."""
    from ddlb_amd.ops.gemm import gemm

    M, N, K = 130, 203, 512
    a, w, s_a, s_w, want = _scaled_case(fmt, M, N, K, 255)
    a, s_a, s_w, want = a.clone(), s_a.clone(), s_w.clone(), want.clone()
    per = 2 if fmt == "mxfp4" else 1
    zb = K // 32 - 1                                  # row 3: a block of zeros in the last K-tile
    a.view(U8)[3, 32 * zb // per:32 * (zb + 1) // per] = 0
    s_a[70, 5] = 255
    s_a[3, zb] = 255
    s_w[9, 0] = 255
    want[70] = NAN
    want[3] = NAN
    want[:, 9] = NAN
    for tile in _scaled_tiles(fmt):
        buf, view = sentinel_out(M, N, F32, pad_cols=G._out_pad(N, F32))
        gemm(a, w, view, a_scale=s_a, w_scale=s_w, tile=tile)
        torch.cuda.synchronize()
        for r in (70, 3):
            row = view[r]
            print(f"scale byte 255, {fmt} {tile}: row {r} has {int(torch.isnan(row).sum())} NaN, "
                  f"{int(torch.isinf(row).sum())} Inf, {int(torch.isfinite(row).sum())} finite "
                  f"of {N}")
        same(view, want)
        untouched(buf, M, N)


# ============================================================================ g. combine, reduce
@pytest.mark.parametrize("dtype,odt", [(BF16, BF16), (F16, F16), (F32, F32), (BF16, F32),
                                       (F16, F32)],
                         ids=lambda d: G._name(d))
def test_combine_nonfinite(dtype, odt):
    from ddlb_amd.ops.moe import combine, combine_reference

    g = _gen(15)
    T, H, S, k = 40, 136, 24, 2
    y = ints((T, H), dtype, g)
    y[3, 5] = NAN
    y[4, 6] = INF
    y[5, 7] = -INF
    y[6] = INF                                   # an Inf row met by gate 0: NaN
    y[7, :8] = torch.tensor([INF, -INF] * 4, device=DEV).to(dtype)
    slot = torch.randint(8, T, (S, k), generator=g, device=DEV).to(torch.int32)
    gate = torch.randint(1, 4, (S, k), generator=g, device=DEV).float() / 2
    slot[0] = torch.tensor([3, 9]); slot[1] = torch.tensor([10, 4])
    slot[2] = torch.tensor([5, 4])               # -Inf and +Inf in different columns
    slot[3] = torch.tensor([6, 11]); gate[3, 0] = 0.0
    slot[4] = torch.tensor([12, 13]); gate[4, 1] = NAN          # a NaN gate
    slot[5] = torch.tensor([7, 7]); gate[5] = torch.tensor([1.0, -1.0])   # Inf - Inf
    slot[6] = torch.tensor([-1, 3])              # a dropped slot beside the NaN row
    slot[7] = torch.tensor([T, 14])
    osz = torch.empty((), dtype=odt).element_size()
    buf, out = sentinel_out(S, H, odt, pad_cols=16 // osz)
    combine(y, slot.contiguous(), gate.contiguous(), out=out)
    torch.cuda.synchronize()
    want = combine_reference(y, slot, gate, odt)
    assert bool(torch.isnan(want[3]).all()) and bool(torch.isnan(want[4]).all())
    assert bool(torch.isnan(want[5, :8]).all()) and bool((want == INF).any())
    assert bool((want == -INF).any()) and bool(torch.isfinite(want[8:]).all())
    same(out, want)
    untouched(buf, S, H)


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=G._name)
@pytest.mark.parametrize("nsrc", [3, 9])
def test_reduce_nonfinite(dtype, nsrc):
    """NaN, +Inf and -Inf in different sources at one index give NaN; +Inf with finite values
    gives +Inf; one case each in the vector body and the scalar tail; the filler past ``count``
    stays."""
    from ddlb_amd.ops import load

    C = load()
    count = 1003
    pad = (count + 7) // 8 * 8 + 8
    slab = torch.randint(-3, 4, (nsrc, pad), generator=_gen(16), device=DEV).float().to(dtype)
    for i in (16, 1001):                  # the vector body; the scalar tail (1000..1002)
        slab[0, i], slab[1, i], slab[2, i] = INF, NAN, -INF
        slab[0, i + 1], slab[2, i + 1] = INF, -INF
    slab[1, 40] = INF
    slab[nsrc - 1, 1000] = INF
    slab[0, 41] = -INF
    out = torch.full((pad,), SENTINEL, device=DEV, dtype=dtype)
    s = torch.cuda.current_stream().cuda_stream
    C.reduce_sum(out.data_ptr(), [slab[i].data_ptr() for i in range(nsrc)], count,
                 G_DT[dtype], s)
    torch.cuda.synchronize()
    ref = slab[0, :count].float()
    for i in range(1, nsrc):
        ref = ref + slab[i, :count].float()
    assert bool(torch.isnan(ref[[16, 17, 1001, 1002]]).all())
    assert float(ref[40]) == INF and float(ref[1000]) == INF and float(ref[41]) == -INF
    same(out[:count], ref.to(dtype))
    assert bool((out[count:].float() == SENTINEL).all())
    if dtype != F32:                      # f32 sources into a 16-bit destination
        slab32 = slab.float()
        out = torch.full((pad,), SENTINEL, device=DEV, dtype=dtype)
        C.reduce_sum(out.data_ptr(), [slab32[i].data_ptr() for i in range(nsrc)], count,
                     G_DT[dtype], s, G_DT[F32])
        torch.cuda.synchronize()
        same(out[:count], ref.to(dtype))
        assert bool((out[count:].float() == SENTINEL).all())


G_DT = {F32: 0, F16: 1, BF16: 2}
