"""Grouped GEMM over per-expert weights on the GPU: ``ops.gemm.gemm_grouped``, every flavour of
the tiled kernel.

The oracle is exact and has no tolerance: for each group ``g`` the ungrouped
``gemm(a[o[g]:o[g+1]], w[g], tile=same, ...)`` writes, bit for bit, what the grouped launch writes
into those rows (``torch.equal`` on dense outputs, byte equality of ``q`` and ``s`` with
``out_quant``). Dense outputs without an activation also get the absolute anchor: the exact
product of the integer operands (-3..3, power-of-two block scales), rounded once.

Weights and scales differ per expert (seeded per ``g``) and sit in views with
``w.stride(0) > N * K`` and poison between the experts; outputs are views of sentinel-filled
buffers with ``ldc > N``, a padded scale pitch and extra rows, and every byte outside the groups'
rows must still hold the sentinel."""

import gc

import pytest
import torch

import _exact as X
from _exact import FAR_PITCH, POISON, SENTINEL, far_out, far_view, untouched, untouched_far

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
FP4 = torch.float4_e2m1fn_x2
TILES = ("256x128", "128x256", "128x128", "256x128w4")
FORMS = ("bf16", "f16", "mxfp8", "mxfp4")
DENSE = {"bf16": (torch.bfloat16, torch.float32), "f16": (torch.float16, torch.float32),
         "mxfp8": (torch.bfloat16, torch.float16, torch.float32),
         "mxfp4": (torch.bfloat16, torch.float16, torch.float32)}
SENT = 0xA5
POISON_SCALE = 200       # a scale byte no operand uses: 2^73
INT_CODE = (0, 2, 4, 5)  # E2M1 codes of |v| = 0, 1, 2, 3
COUNTS = (0, 1, 130, 0, 256, 257, 0)
# (counts, o[0], rows behind o[E]): the issue's set
OFFSET_SETS = {"counts": (COUNTS, 0, 0), "shifted": (COUNTS, 3, 0), "one_group": ((130,), 0, 0),
               "all_empty": ((0, 0, 0), 2, 3), "trailing": (COUNTS, 0, 5)}


def _ks(form):
    return (256, 512) if form == "mxfp4" else (128, 384)  # two K-tile counts


def _pack_ints(v):
    from ddlb_amd.ops.mx import pack_e2m1

    code = torch.tensor(INT_CODE, device=v.device)[v.abs().long()]
    return pack_e2m1(code | ((v < 0).long() << 3))


def _typed(v, form):
    """Integer-valued f32 ``v [R, K]`` in an input form's data type."""
    if form == "mxfp4":
        return _pack_ints(v)
    return v.to({"bf16": torch.bfloat16, "f16": torch.float16, "mxfp8": FP8}[form])


def _scale_bytes(rows, k, g):
    return (127 + torch.randint(-2, 3, (rows, k // 32), generator=g, device=DEV)).to(torch.uint8)


def _offsets(counts, o0):
    o = [o0]
    for c in counts:
        o.append(o[-1] + c)
    return o


def _experts(form, E, N, K, seed, pad_rows=4):
    """``(w, w_scale, wv, sv)``: per-expert weights seeded per ``g``, as the view ``[:, :N]`` of a
    ``[E, N + pad_rows, K]`` buffer of poison (``w.stride(0) > N * K``), the scales likewise
    (poison byte ``POISON_SCALE``); ``wv`` / ``sv`` the integer values and scale bytes."""
    scaled = form in ("mxfp8", "mxfp4")
    wv = torch.empty((E, N, K), dtype=torch.float32, device=DEV)
    sv = torch.empty((E, N, K // 32), dtype=torch.uint8, device=DEV) if scaled else None
    for g in range(E):
        gen = torch.Generator(device=DEV).manual_seed(seed + 7919 * g)
        wv[g] = X.ints((N, K), torch.float32, gen)
        if scaled:
            sv[g] = _scale_bytes(N, K, gen)
    rows = N + pad_rows
    wvb = torch.full((E, rows, K), 3.0 if form == "mxfp4" else POISON, device=DEV)
    wvb[:, :N] = wv
    wt = _typed(wvb.reshape(E * rows, K), form)
    one_byte = wt.element_size() == 1  # (reshaped as bytes: fp8, fp4 pairs)
    wbuf = (wt.view(torch.uint8) if one_byte else wt).reshape(E, rows, -1)
    wbuf = wbuf.view(wt.dtype) if one_byte else wbuf
    w = wbuf[:, :N]
    assert w.stride(0) > N * w.stride(1) and w.stride(2) == 1
    ws = None
    if scaled:
        sbuf = torch.full((E, N + pad_rows, K // 32), POISON_SCALE, dtype=torch.uint8, device=DEV)
        sbuf[:, :N] = sv
        ws = sbuf[:, :N]
    return w, ws, wv, sv


_CASES = {}


def _case(form, name, N, K, slack=0):
    """``(a, kw, w, offsets tensor, clamped offsets list, T, av, sa, wv, sv)`` of a form and an
    offsets set, made once and left unchanged. ``slack`` rows of allocation behind ``T``."""
    key = (form, name, N, K, slack)
    if key not in _CASES:
        counts, o0, tail = OFFSET_SETS[name] if isinstance(name, str) else name
        o = _offsets(counts, o0)
        T = o[-1] + tail
        E = len(counts)
        seed = 9000 + 1009 * FORMS.index(form) + 7 * N + K + 31 * E + o0
        gen = torch.Generator(device=DEV).manual_seed(seed)
        av = X.ints((T + slack, K), torch.float32, gen)
        a = _typed(av, form)[:T]
        kw, sa = {}, None
        w, ws, wv, sv = _experts(form, E, N, K, seed)
        if ws is not None:
            sa = _scale_bytes(T + slack, K, gen)
            kw = dict(a_scale=sa[:T], w_scale=ws)
        offs = torch.tensor(o, dtype=torch.int32, device=DEV)
        _CASES[key] = (a, kw, w, offs, o, T, av[:T], sa[:T] if sa is not None else None, wv, sv)
    return _CASES[key]


def _slice_kw(kw, lo, hi, g):
    return dict(a_scale=kw["a_scale"][lo:hi], w_scale=kw["w_scale"][g]) if kw else {}


def _anchor(av, sa, wv, sv, odt):
    """The exact product of the integer operands under their power-of-two block scales, in fp64,
    rounded once to f32 (exact here) and to ``odt``."""
    def scaled(v, s):
        v = v.double()
        if s is None:
            return v
        R, K = v.shape
        return (v.reshape(R, K // 32, 32) * X.pow2_f64(s.to(torch.int64) - 127).unsqueeze(2)) \
            .reshape(R, K)
    return (scaled(av, sa) @ scaled(wv, sv).t()).to(torch.float32).to(odt)


def _qviews(fmt, T, F, pad=32, spad=8, extra=3):
    """Sentinel-filled buffers and the (out, out_scale) views into them for ``F`` output columns:
    ldc > F, a scale pitch greater than F / 32, extra rows."""
    ncol = F if fmt == "mx" else F // 2
    qb = torch.full((T + extra, ncol + pad), SENT, dtype=torch.uint8, device=DEV)
    sb = torch.full((T + extra, F // 32 + spad), SENT, dtype=torch.uint8, device=DEV)
    return qb, sb, qb[:T, :ncol].view(FP8 if fmt == "mx" else FP4), sb[:T, :F // 32]


def _untouched_bytes(buf, lo, hi, ncol):
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    mask[lo:hi, :ncol] = False
    bad = int((buf[mask] != SENT).sum())
    assert bad == 0, f"{bad} bytes outside rows [{lo}, {hi}) x {ncol} columns were written"


def _check_dense(tile, form, case, odt, act, o=None, **extra):
    """One grouped launch with a dense output against the per-group oracle (and the anchor)."""
    from ddlb_amd.ops.gemm import gemm, gemm_grouped

    a, kw, w, offs, o_list, T, av, sa, wv, sv = case
    o = o_list if o is None else o
    glu = extra.get("glu", False)
    cols = w.shape[1] // 2 if glu else w.shape[1]
    buf, out = X.sentinel_out(T, cols, odt, pad_cols=4)
    got = gemm_grouped(a, w, offs, out, tile=tile, act=act, **kw, **extra)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (T, cols)
    for g in range(w.shape[0]):
        lo, hi = o[g], o[g + 1]
        if hi == lo:
            continue
        want = gemm(a[lo:hi], w[g], out_dtype=odt, tile=tile, act=act,
                    **_slice_kw(kw, lo, hi, g), **extra)
        assert torch.equal(got[lo:hi], want), (form, tile, odt, act, g, (lo, hi))
        if act == "none" and not glu:
            ref = _anchor(av[lo:hi], None if sa is None else sa[lo:hi], wv[g],
                          None if sv is None else sv[g], odt)
            assert torch.equal(want, ref), ("anchor", form, tile, odt, g)
    untouched(buf, T, cols, rows=slice(o[0], o[-1]))


def _check_quant(tile, form, case, fmt, act, glu, o=None):
    """One grouped launch with a quantised output: ``q`` and ``s`` byte for byte."""
    from ddlb_amd.ops.gemm import gemm, gemm_grouped

    a, kw, w, offs, o_list, T, *_ = case
    o = o_list if o is None else o
    F = w.shape[1] // 2 if glu else w.shape[1]
    qb, sb, out, out_scale = _qviews(fmt, T, F)
    q, s = gemm_grouped(a, w, offs, out, tile=tile, act=act, glu=glu, out_quant=fmt,
                        out_scale=out_scale, **kw)
    assert q.data_ptr() == out.data_ptr() and s.data_ptr() == out_scale.data_ptr()
    assert tuple(s.shape) == (T, F // 32) and q.dtype == (FP8 if fmt == "mx" else FP4)
    for g in range(w.shape[0]):
        lo, hi = o[g], o[g + 1]
        if hi == lo:
            continue
        q_ref, s_ref = gemm(a[lo:hi], w[g], tile=tile, act=act, glu=glu, out_quant=fmt,
                            **_slice_kw(kw, lo, hi, g))
        assert torch.equal(s[lo:hi], s_ref), (form, tile, fmt, act, glu, g, "scales")
        assert torch.equal(q[lo:hi].view(torch.uint8), q_ref.view(torch.uint8)), \
            (form, tile, fmt, act, glu, g, "data")
    _untouched_bytes(qb, o[0], o[-1], out.shape[1])
    _untouched_bytes(sb, o[0], o[-1], F // 32)


# ------------------------------------------------------------------ 1. dense
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tile", TILES)
def test_grouped_dense(tile, form):
    """Every offsets set x two K-tile counts x every dense output of the form x act in (none,
    relu); N = 192 is ragged for 128- and 256-column tiles. Rows of empty groups and every row
    outside ``[o[0], o[E])`` (leading, trailing, the buffers' extra rows) stay sentinel."""
    for name in OFFSET_SETS:
        for K in _ks(form):
            case = _case(form, name, 192, K)
            for odt in DENSE[form]:
                for act in ("none", "relu"):
                    _check_dense(tile, form, case, odt, act)


def test_one_group_equals_plain_gemm():
    from ddlb_amd.ops.gemm import gemm, gemm_grouped

    a, kw, w, offs, o, T, *_ = _case("bf16", "one_group", 192, 128)
    assert o == [0, 130] and T == 130
    assert torch.equal(gemm_grouped(a, w, offs, tile="128x128"), gemm(a, w[0], tile="128x128"))
    # allocated here: dense rows, the form's default output dtype, `auto` picks an offered tile
    got = gemm_grouped(a, w, offs)
    assert got.is_contiguous() and got.dtype == torch.bfloat16 and tuple(got.shape) == (130, 192)
    assert torch.equal(got, gemm(a, w[0], tile="128x128"))


# ------------------------------------------------------------------ 2. glu, out_quant, both
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tile", TILES)
def test_grouped_epilogues(tile, form):
    """``glu`` (N = 320), ``out_quant`` (N = 256) and both (N = 256 for MX-fp8, 512 for MXFP4)
    through the same per-group oracle, on the shifted and the trailing-rows offsets, both K-tile
    counts, act in (none, relu)."""
    for name in ("shifted", "trailing"):
        for K in _ks(form):
            for act in ("none", "relu"):
                _check_dense(tile, form, _case(form, name, 320, K), DENSE[form][0], act, glu=True)
                _check_dense(tile, form, _case(form, name, 320, K), torch.float32, act, glu=True)
                for fmt in ("mx", "mxfp4"):
                    _check_quant(tile, form, _case(form, name, 256, K), fmt, act, False)
                    _check_quant(tile, form, _case(form, name, 256 if fmt == "mx" else 512, K),
                                 fmt, act, True)


# ------------------------------------------------------------------ 3. clamping
@pytest.mark.parametrize("form", FORMS)
def test_offsets_are_clamped(form):
    """Offsets ``(0, 200, 100, T + 50)`` run as ``(0, 200, 200, T)``: a non-monotone entry and one
    beyond ``T``. ``a`` and the scales are views of allocations with 64 more rows than ``T`` and
    the outputs have 64 extra sentinel rows, so a kernel that followed the raw offsets would
    show as a wrong value or a written sentinel, inside the allocations."""
    from ddlb_amd.ops.gemm import clamp_offsets, gemm, gemm_grouped

    K, T = _ks(form)[1], 300
    raw = [0, 200, 100, T + 50]
    for N, glu, fmt in ((192, False, None), (512, True, "mx")):
        a, kw, w, _, _, T_, *_ = _case(form, ((200, 0, 100), 0, 0), N, K, slack=64)
        assert T_ == T and a.shape[0] == T
        offs = torch.tensor(raw, dtype=torch.int32, device=DEV)
        o = clamp_offsets(offs, T)
        assert o == [0, 200, 200, T]
        for tile in ("128x128", "256x128"):
            if fmt is None:
                buf = X._filled((T + 64, N + 4), SENTINEL, torch.float32, DEV)
                out = buf[:T, :N]
                got = gemm_grouped(a, w, offs, out, tile=tile, **kw)
                for g in (0, 2):
                    want = gemm(a[o[g]:o[g + 1]], w[g], out_dtype=torch.float32, tile=tile,
                                **_slice_kw(kw, o[g], o[g + 1], g))
                    assert torch.equal(got[o[g]:o[g + 1]], want), (form, tile, g)
                untouched(buf, T, N)
            else:
                F = N // 2
                qb, sb, out, out_scale = _qviews(fmt, T, F, extra=64)
                q, s = gemm_grouped(a, w, offs, out, tile=tile, glu=True, out_quant=fmt,
                                    out_scale=out_scale, act="relu", **kw)
                for g in (0, 2):
                    q_ref, s_ref = gemm(a[o[g]:o[g + 1]], w[g], tile=tile, glu=True,
                                        out_quant=fmt, act="relu",
                                        **_slice_kw(kw, o[g], o[g + 1], g))
                    assert torch.equal(s[o[g]:o[g + 1]], s_ref)
                    assert torch.equal(q[o[g]:o[g + 1]].view(torch.uint8), q_ref.view(torch.uint8))
                _untouched_bytes(qb, 0, T, out.shape[1])
                _untouched_bytes(sb, 0, T, F // 32)


# ------------------------------------------------------------------ 4. far offsets
FAR_T, FAR_OFFS = 300, (0, 100, 260, 300)


@pytest.fixture(scope="module")
def far_backing():
    gc.collect()
    torch.cuda.empty_cache()
    nbytes = X.far_span(FAR_T, 4096, FAR_PITCH)
    free, total = torch.cuda.mem_get_info()
    if free < X.FAR_GUARD + nbytes + (64 << 20):
        pytest.skip(f"the far backing needs {X.FAR_GUARD + nbytes} bytes; {free} of {total} free")
    hold = [X.far_backing(nbytes)]
    yield hold[0]
    hold.clear()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("form", ("bf16", "mxfp8"))
@pytest.mark.parametrize("which", ("a", "c"))
def test_far_rows(far_backing, form, which):
    """``a`` or ``c`` in a view whose rows lie ``FAR_PITCH`` bytes apart behind a 2 GiB guard: the
    last group starts at row 260, past byte 2^32 of the view, so the re-basing must be 64-bit.
    The backing (6.7 GiB) is smaller than the one of tests/test_far_offsets_gpu.py."""
    from ddlb_amd.ops.gemm import gemm, gemm_grouped

    assert FAR_OFFS[2] * FAR_PITCH > 2 ** 32 and FAR_OFFS[1] * FAR_PITCH < 2 ** 31
    K, N = 128, 192
    counts = tuple(FAR_OFFS[i + 1] - FAR_OFFS[i] for i in range(3))
    a, kw, w, offs, o, T, av, sa, wv, sv = _case(form, (counts, 0, 0), N, K)
    assert o == list(FAR_OFFS) and T == FAR_T
    if which == "a":
        A = far_view(far_backing, a, FAR_PITCH)
        buf, out = X.sentinel_out(T, N, torch.float32, pad_cols=4)
    else:
        A = a
        out = far_out(far_backing, T, N, torch.float32, FAR_PITCH)
    got = gemm_grouped(A, w, offs, out, tile="128x128", **kw)
    torch.cuda.synchronize()
    for g in range(3):
        lo, hi = o[g], o[g + 1]
        want = gemm(a[lo:hi], w[g], out_dtype=torch.float32, tile="128x128",
                    **_slice_kw(kw, lo, hi, g))
        assert torch.equal(got[lo:hi], want), (form, which, g)
        ref = _anchor(av[lo:hi], None if sa is None else sa[lo:hi], wv[g],
                      None if sv is None else sv[g], torch.float32)
        assert torch.equal(want, ref)
    if which == "a":
        untouched(buf, T, N)
    else:
        untouched_far(far_backing, out)


# ------------------------------------------------------------------ 5. repeat, stream
def test_two_runs_write_identical_bytes():
    from ddlb_amd.ops.gemm import gemm_grouped

    a, kw, w, offs, o, T, *_ = _case("mxfp8", "shifted", 512, 384)
    runs = []
    for _ in range(2):
        qb, sb, out, out_scale = _qviews("mxfp4", T, 256)
        gemm_grouped(a, w, offs, out, tile="128x128", act="relu", glu=True, out_quant="mxfp4",
                     out_scale=out_scale, **kw)
        torch.cuda.synchronize()
        runs.append((qb, sb))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert bool((runs[0][1][o[0]:o[-1], :8] != SENT).all())


def test_stream_argument():
    from ddlb_amd.ops.gemm import gemm_grouped

    a, kw, w, offs, o, T, *_ = _case("bf16", "trailing", 192, 384)
    want = gemm_grouped(a, w, offs, tile="128x256")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got = gemm_grouped(a, w, offs, tile="128x256", stream=side.cuda_stream)
    side.synchronize()
    assert torch.equal(got[o[0]:o[-1]], want[o[0]:o[-1]])


# ------------------------------------------------------------------ 6. the routed FFN
@pytest.mark.parametrize("fused", (True, False))
@pytest.mark.parametrize("fmt", ("mx", "mxfp4"))
def test_mx_moe(fmt, fused):
    from ddlb_amd.models.mx_moe import MxMoE

    moe = MxMoE(hidden=256, ffn=256, seq=300, experts=5, fmt=fmt, fused=fused)
    counts = torch.bincount(moe.ids.cpu(), minlength=5)
    assert int(counts.sum()) == 300 and int((counts == 0).sum()) >= 1
    assert len(set(counts.tolist())) > 2, "uneven counts"
    perm, offsets = moe.route()
    assert offsets.dtype == torch.int32 and offsets.tolist()[-1] == 300
    assert offsets.tolist() == [0] + torch.cumsum(counts, 0).tolist()
    y = moe.forward().clone()
    torch.cuda.synchronize()
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (300, 256)
    assert bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    moe.validate(y)
    y2 = moe.forward()
    torch.cuda.synchronize()
    assert torch.equal(y, y2)


# ------------------------------------------------------------------ 7. refusals of the entry
def test_native_entry_refuses_and_launches_nothing():
    """``gemm_launch`` itself refuses what Python would (argument inspection only): the sentinel
    bytes survive; the supported call then runs."""
    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import DT_BF16, DT_F16, DT_F32, DT_FP8, TILES as CODES

    C = load()
    T, N, K, E = 256, 256, 256, 2
    a = torch.ones(T, K, device=DEV, dtype=torch.bfloat16)
    w = torch.ones(E, N, K, device=DEV, dtype=torch.bfloat16)
    a8, w8, af, wf = a.to(FP8), w.to(FP8), a.float(), w.float()
    offs = torch.tensor([0, 100, 256], dtype=torch.int32, device=DEV)
    out = X._filled((T, N), SENTINEL, torch.bfloat16, DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(x=a, y=w, din=DT_BF16, dout=DT_BF16, tile="auto", ngroups=E, o=None,
             b_gstride=N * K, ldc=N, glu=0, cs=0):
        C.gemm_grouped(a=x.data_ptr(), b=y.data_ptr(), c=out.data_ptr(),
                       offs=offs.data_ptr() if o is None else o, ngroups=ngroups, lda=K, ldb=K,
                       ldc=ldc, b_gstride=b_gstride, M=T, N=N, K=K, din=din, dout=dout,
                       tile=CODES[tile], stream=st, c_scale=cs, c_scale_ld=N // 32, glu=glu)

    bad = [
        dict(ngroups=0), dict(ngroups=-1), dict(ngroups=1025), dict(o=0),
        dict(b_gstride=N * K - 64), dict(b_gstride=0), dict(b_gstride=N * K + 1),
        dict(ldc=N - 8),
        dict(x=af, y=wf, din=DT_F32, dout=DT_F32),    # f32 operands
        dict(x=a8, y=w8, din=DT_FP8),                 # unit-scale fp8
        dict(dout=DT_F16),                            # bf16 -> f16
        dict(cs=out.data_ptr()),                      # output scales with a dense dout
        dict(tile="pt4"), dict(tile="t8"), dict(tile="256x256"), dict(tile="i128"),
    ]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((out.float() == SENTINEL).all())
    call()
    torch.cuda.synchronize()
    assert bool((out.float() == K).all())
