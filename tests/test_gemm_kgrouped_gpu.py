"""K-grouped GEMM on the GPU: ``ops.gemm.gemm_kgrouped``, the wgrad form of the tiled kernel.

The oracle is exact and has no tolerance: for each group ``g`` the ungrouped
``gemm(a[:, cols g], w[:, cols g], tile=same)`` writes, bit for bit, what the K-grouped launch
writes into ``out[g]``, and both equal the exact product of the integer operands (-3..3,
power-of-two block scales 2^-2..2^2) in fp64, rounded once. A group without columns is ``+0.0``
in every bit.

Operands are views with a pitch beyond the capacity; every column no group owns (from ``k0_E``
on) holds poison data under the scale byte 200. Outputs are views of sentinel-filled buffers with
``ldc > N``, extra rows and a gap between the groups' matrices."""

import pytest
import torch

import _exact as X
from _exact import POISON, SENTINEL

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
FP4 = torch.float4_e2m1fn_x2
TILES = ("256x128", "128x256", "128x128", "256x128w4")
FORMS = ("mxfp8", "mxfp4")
OUTS = (torch.float32, torch.bfloat16, torch.float16)
POISON_SCALE = 200       # a scale byte no operand uses: 2^73
INT_CODE = (0, 2, 4, 5)  # E2M1 codes of |v| = 0, 1, 2, 3
COUNTS = (0, 1, 130, 0, 256, 257, 0)
OFFSET_SETS = {"counts": (COUNTS, 0, 0), "shifted": (COUNTS, 3, 0), "one_group": ((130,), 0, 0),
               "all_empty": ((0, 0, 0), 2, 3), "trailing": (COUNTS, 0, 5)}
M, N = 192, 320          # ragged against every offered tile


def _mod(form):
    return 256 if form == "mxfp4" else 128


def _offsets(counts, o0):
    o = [o0]
    for c in counts:
        o.append(o[-1] + c)
    return o


def _typed(v, form):
    """Integer-valued f32 ``v [R, K]`` as e4m3 or packed E2M1."""
    from ddlb_amd.ops.mx import pack_e2m1

    if form == "mxfp8":
        return v.to(FP8)
    code = torch.tensor(INT_CODE, device=v.device)[v.abs().long()]
    return pack_e2m1(code | ((v < 0).long() << 3))


def _operand(rows, cap, k_end, form, gen):
    """``(data view [rows, cap], scale view [rows, cap / 32], values f32, scale bytes)``: a pitch
    of ``cap + MOD`` columns, poison from column ``k_end`` on."""
    mod = _mod(form)
    full = cap + mod
    v = X.ints((rows, full), torch.float32, gen)
    s = (127 + torch.randint(-2, 3, (rows, full // 32), generator=gen, device=DEV)).to(torch.uint8)
    vp, sp = v.clone(), s.clone()
    vp[:, k_end:] = 3.0 if form == "mxfp4" else POISON
    sp[:, k_end // 32:] = POISON_SCALE
    t = _typed(vp, form)
    d = 2 if form == "mxfp4" else 1
    data = t.view(torch.uint8)[:, :cap // d].view(t.dtype)
    return data, sp[:, :cap // 32], v[:, :cap], s[:, :cap // 32]


def _dequant64(v, s):
    R, K = v.shape
    return (v.double().reshape(R, K // 32, 32)
            * X.pow2_f64(s.to(torch.int64) - 127).unsqueeze(2)).reshape(R, K)


_CASES = {}


def _case(form, name):
    """Operands, offsets and the fp64 anchors of a form and an offsets set, made once."""
    from ddlb_amd.ops.gemm import kgrouped_capacity, padded_offsets

    key = (form, name)
    if key not in _CASES:
        counts, o0, tail = OFFSET_SETS[name] if isinstance(name, str) else name
        o = _offsets(counts, o0)
        T, E, mod = o[-1] + tail, len(counts), _mod(form)
        offs = torch.tensor(o, dtype=torch.int32, device=DEV)
        cap = kgrouped_capacity(T, E, mod)
        k0 = padded_offsets(offs, T, mod)
        assert k0[-1] <= cap
        gen = torch.Generator(device=DEV).manual_seed(4000 + 17 * FORMS.index(form) + T + 31 * E)
        a, sa, av, sav = _operand(M, cap, k0[-1], form, gen)
        w, sw, wv, swv = _operand(N, cap, k0[-1], form, gen)
        anchors = []
        for g in range(E):
            lo, hi = k0[g], k0[g + 1]
            anchors.append(None if hi == lo else
                           (_dequant64(av[:, lo:hi], sav[:, lo // 32:hi // 32])
                            @ _dequant64(wv[:, lo:hi], swv[:, lo // 32:hi // 32]).t())
                           .to(torch.float32))
        _CASES[key] = (a, sa, w, sw, offs, T, E, k0, anchors)
    return _CASES[key]


def _out(E, odt):
    buf = X._filled((E, M + 3, N + 4), SENTINEL, odt, DEV)
    return buf, buf[:, :M, :N]


def _untouched(buf):
    mask = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
    mask[:, :M, :N] = False
    bad = int((buf.float()[mask] != SENTINEL).sum())
    assert bad == 0, f"{bad} elements around the groups' outputs were written"


def _slices(case, form, g):
    a, sa, w, sw, offs, T, E, k0, anchors = case
    d = 2 if form == "mxfp4" else 1
    lo, hi = k0[g], k0[g + 1]
    u8 = lambda t: t.view(torch.uint8)[:, lo // d:hi // d].contiguous().view(t.dtype)
    return (u8(a), u8(w), sa[:, lo // 32:hi // 32].contiguous(),
            sw[:, lo // 32:hi // 32].contiguous())


def _check(tile, form, case, odt, offs=None):
    from ddlb_amd.ops.gemm import gemm, gemm_kgrouped

    a, sa, w, sw, offs0, T, E, k0, anchors = case
    buf, out = _out(E, odt)
    got = gemm_kgrouped(a, w, offs0 if offs is None else offs, T, out, a_scale=sa, w_scale=sw,
                        tile=tile)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (E, M, N)
    bits = {4: torch.int32, 2: torch.int16}[out.element_size()]
    for g in range(E):
        if k0[g + 1] == k0[g]:
            assert bool((got[g].contiguous().view(bits) == 0).all()), (form, tile, odt, g, "+0.0")
            continue
        ag, wg, sag, swg = _slices(case, form, g)
        want = gemm(ag, wg, out_dtype=odt, tile=tile, a_scale=sag, w_scale=swg)
        assert torch.equal(got[g], want), (form, tile, odt, g, (k0[g], k0[g + 1]))
        assert torch.equal(want, anchors[g].to(odt)), ("anchor", form, tile, odt, g)
    _untouched(buf)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tile", TILES)
def test_kgrouped_matches_ungrouped_and_anchor(tile, form):
    """Every offsets set x every output dtype: ``out[g]`` bit for bit the ungrouped ``gemm`` of
    the same tile on the group's column slices and the fp64 anchor rounded once; empty groups
    ``+0.0``; the sentinel around and between the ``out[g]`` intact."""
    for name in OFFSET_SETS:
        case = _case(form, name)
        for odt in OUTS:
            _check(tile, form, case, odt)


@pytest.mark.parametrize("form", FORMS)
def test_auto_tile_and_allocated_output(form):
    from ddlb_amd.ops.gemm import gemm_kgrouped

    a, sa, w, sw, offs, T, E, k0, anchors = _case(form, "counts")
    got = gemm_kgrouped(a, w, offs, T, a_scale=sa, w_scale=sw)
    assert got.dtype == torch.bfloat16 and got.is_contiguous() and tuple(got.shape) == (E, M, N)
    for g in range(E):
        want = torch.zeros((M, N), device=DEV) if anchors[g] is None else anchors[g]
        assert torch.equal(got[g], want.to(torch.bfloat16)), (form, g)


@pytest.mark.parametrize("form", FORMS)
def test_garbage_offsets_are_clamped(form):
    """Negative, decreasing and huge offsets run as their clamped forms and touch nothing outside
    ``out``: ``(-5, 200, 100, 2^31 - 1)`` is ``(0, 200, 200, T)``."""
    from ddlb_amd.ops.gemm import clamp_offsets

    case = _case(form, ((200, 0, 100), 0, 0))
    T = case[5]
    raw = torch.tensor([-5, 200, 100, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    assert clamp_offsets(raw, T) == [0, 200, 200, 300] and T == 300
    for tile in ("128x128", "256x128"):
        _check(tile, form, case, torch.float32, offs=raw)
    # everything empty, whatever the array says: all +0.0
    from ddlb_amd.ops.gemm import gemm_kgrouped

    a, sa, w, sw = case[:4]
    for vals in ([2 ** 31 - 1, -2 ** 31, 7, 7], [-9, -9, -9, -1]):
        buf, out = _out(3, torch.float32)
        gemm_kgrouped(a, w, torch.tensor(vals, dtype=torch.int32, device=DEV), T, out,
                      a_scale=sa, w_scale=sw, tile="128x128")
        assert bool((out.contiguous().view(torch.int32) == 0).all())
        _untouched(buf)


def test_graph_capture_reads_offsets_at_replay():
    """One capture, one replay after the offsets' content changed: the new result."""
    from ddlb_amd.ops.gemm import gemm_kgrouped

    form = "mxfp8"
    c1 = _case(form, ((200, 0, 100), 0, 0))
    a, sa, w, sw, offs1, T, E, k0_1, anchors1 = c1
    offs = offs1.clone()
    out = torch.empty((E, M, N), dtype=torch.float32, device=DEV)
    gemm_kgrouped(a, w, offs, T, out, a_scale=sa, w_scale=sw, tile="128x128")  # warm up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gemm_kgrouped(a, w, offs, T, out, a_scale=sa, w_scale=sw, tile="128x128")
    # the same operand bytes under other offsets: (0, 128, 128, 300) moves every column range
    new = torch.tensor([0, 128, 128, 300], dtype=torch.int32, device=DEV)
    offs.copy_(new)
    out.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    want = gemm_kgrouped(a, w, new, T, a_scale=sa, w_scale=sw, tile="128x128",
                         out_dtype=torch.float32)
    assert torch.equal(out, want)
    assert bool((out[1] == 0).all()) and not torch.equal(out[0], anchors1[0])


def test_stream_argument():
    from ddlb_amd.ops.gemm import gemm_kgrouped

    a, sa, w, sw, offs, T, E, *_ = _case("mxfp4", "shifted")
    want = gemm_kgrouped(a, w, offs, T, a_scale=sa, w_scale=sw, tile="128x256")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got = gemm_kgrouped(a, w, offs, T, a_scale=sa, w_scale=sw, tile="128x256",
                        stream=side.cuda_stream)
    side.synchronize()
    assert torch.equal(got, want)


def test_refusals_from_python():
    from ddlb_amd.ops.gemm import gemm_kgrouped

    a, sa, w, sw, offs, T, E, *_ = _case("mxfp8", "counts")
    cap = a.shape[1]
    ok = dict(a=a, w=w, offsets=offs, rows=T, a_scale=sa, w_scale=sw)
    out = torch.empty((E, M, N), dtype=torch.bfloat16, device=DEV)
    bad = [
        (dict(a_scale=None), ValueError), (dict(w_scale=None), ValueError),
        (dict(a=a.view(torch.uint8).to(torch.bfloat16), w=w.view(torch.uint8).to(torch.bfloat16)),
         TypeError),
        (dict(w=w.view(torch.uint8)), TypeError),
        (dict(offsets=offs.long()), TypeError), (dict(offsets=offs[:1]), ValueError),
        (dict(offsets=offs.cpu()), ValueError),
        (dict(rows=T + 128), ValueError),          # capacity above the operands' columns
        (dict(rows=-1), ValueError), (dict(rows=float(T)), ValueError),
        (dict(a=a[:, :cap - 128], a_scale=sa[:, :(cap - 128) // 32]), ValueError),
        (dict(tile="pt4"), ValueError), (dict(tile="256x256"), ValueError),
        (dict(out_dtype=torch.float64), TypeError),
        (dict(out=out[:, :, :N - 8]), ValueError), (dict(out=out[0]), ValueError),
        (dict(out=out.float(), out_dtype=torch.bfloat16), TypeError),
        (dict(out=torch.empty((M, E, N), dtype=torch.bfloat16, device=DEV).transpose(0, 1)),
         ValueError),                              # groups closer than M rows
        (dict(a_scale=sa[:, :-4]), ValueError), (dict(a_scale=sa.to(torch.int8)), TypeError),
    ]
    for kw, exc in bad:
        args = dict(ok)
        args.update(kw)
        with pytest.raises(exc):
            gemm_kgrouped(args.pop("a"), args.pop("w"), args.pop("offsets"), args.pop("rows"),
                          **args)
    for kw in (dict(act="relu"), dict(glu=True), dict(out_quant="mx")):
        with pytest.raises(TypeError):
            gemm_kgrouped(a, w, offs, T, a_scale=sa, w_scale=sw, **kw)


def test_native_entry_refuses_and_launches_nothing():
    """``gemm_launch`` itself refuses what Python would (argument inspection only): the sentinel
    survives; the supported call then runs."""
    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import DT_BF16, DT_FP8, TILES as CODES

    C = load()
    a, sa, w, sw, offs, T, E, *_ = _case("mxfp8", "counts")
    cap = a.shape[1]
    out = X._filled((E, M, N), SENTINEL, torch.bfloat16, DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(K=cap, rows=T, ngroups=E, o=None, c_gstride=M * N, din=DT_FP8, dout=DT_BF16,
             tile="auto", a_scale=None, ldc=N):
        C.gemm_kgrouped(a=a.data_ptr(), b=w.data_ptr(), c=out.data_ptr(),
                        offs=offs.data_ptr() if o is None else o, ngroups=ngroups, rows=rows,
                        lda=a.stride(0), ldb=w.stride(0), ldc=ldc, c_gstride=c_gstride, M=M, N=N,
                        K=K, din=din, dout=dout, tile=CODES[tile], stream=st,
                        a_scale=sa.data_ptr() if a_scale is None else a_scale,
                        b_scale=sw.data_ptr(), a_scale_ld=sa.stride(0), b_scale_ld=sw.stride(0))

    bad = [dict(K=cap - 128), dict(K=cap + 32), dict(rows=T + 128), dict(rows=-1),
           dict(ngroups=0), dict(ngroups=1025), dict(ngroups=E + 1), dict(o=0),
           dict(c_gstride=M * N - 64), dict(c_gstride=M * N + 2), dict(c_gstride=0),
           dict(din=DT_BF16), dict(dout=DT_FP8), dict(a_scale=0), dict(ldc=N - 8),
           dict(tile="pt4"), dict(tile="256x256"), dict(tile="i128")]
    for kw in bad:
        with pytest.raises(RuntimeError):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((out.float() == SENTINEL).all())
    call()
    torch.cuda.synchronize()
    assert bool((out[0] == 0).all()) and not bool((out[2].float() == SENTINEL).all())
