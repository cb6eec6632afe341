"""The MoE dispatch layer on the GPU: the routing sort (``csrc/moe/moe_route.hip``), the gathering
row quantiser (``csrc/gemm/mx_quant.hip``), the weighted un-permute (``csrc/moe/moe_combine.hip``)
and ``MxMoE(dispatch="native")``. Every comparison is ``torch.equal`` against a torch-op
specification; outputs passed as ``out=`` lie inside sentinel-filled buffers whose sentinels are
checked afterwards."""

import pytest
import torch

from _exact import FAR_PITCH, far_backing, far_span, far_view, ints, sentinel_out, untouched
from test_mx_scaled_gpu import _wide as wide_fp8
from test_mxfp4_gpu import TIES
from test_mxfp4_gpu import _wide as wide_fp4

from ddlb_amd.ops.moe import ROUTE_CHUNK, combine, combine_reference, route, route_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"
ISENT = -7777
BAD_IDS = (-1, None, 2 ** 31 - 1)   # None stands for E


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


# ------------------------------------------------------------------ route
def _route_checked(ids, E):
    """``route`` into slices of one sentinel-filled int32 buffer; the sentinels between and around
    the three outputs must survive. Returns the outputs."""
    S, k = ids.shape
    n, pad = S * k, 37
    buf = torch.full((4 * pad + E + 1 + 2 * n,), ISENT, dtype=torch.int32, device=DEV)
    o0 = pad
    r0 = o0 + E + 1 + pad
    s0 = r0 + n + pad
    out = (buf[o0:o0 + E + 1], buf[r0:r0 + n], buf[s0:s0 + n].view(S, k))
    got = route(ids, E, out=out)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[o0:o0 + E + 1] = inside[r0:r0 + n] = inside[s0:s0 + n] = True
    assert bool((buf[~inside] == ISENT).all()), "route wrote outside its outputs"
    assert not bool((buf[inside] == ISENT).any()), "route left an output element unwritten"
    return got


def _same_route(got, want, what):
    for name, g, w in zip(("offsets", "row_token", "slot_row"), got, want):
        assert g.dtype == torch.int32 and g.shape == w.shape, (what, name)
        assert torch.equal(g, w), (what, name, int((g != w).sum()))


SIZES = (1, 63, 64, 65, ROUTE_CHUNK - 1, ROUTE_CHUNK, ROUTE_CHUNK + 1, 3 * ROUTE_CHUNK + 7)


@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("n", SIZES)
def test_route_equals_reference(n, k):
    """Random ids over every E and both id dtypes. ``S * k = n`` where ``k`` divides ``n``; where
    it does not, ``S = ceil(n / k)``: the next slot count that ``k`` allows."""
    S = -(-n // k)
    g = _gen(1000 * n + k)
    for E in (1, 5, 64, 257, 1024):
        ids = torch.randint(0, E, (S, k), generator=g, device=DEV)
        want = route_reference(ids, E)
        assert int(want[0][E]) == S * k
        for dt in (torch.int32, torch.int64):
            _same_route(_route_checked(ids.to(dt), E), want, (n, k, E, dt))
        got = route(ids, E)                       # outputs allocated by the call
        _same_route(got, want, (n, k, E, "alloc"))


@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("dt", [torch.int32, torch.int64])
def test_route_dropped_ids(k, dt):
    """-1, E and 2^31 - 1 mixed in: dropped (slot_row -1), not counted, the tail of row_token -1."""
    g = _gen(77 + k)
    for n in (65, ROUTE_CHUNK + 1, 3 * ROUTE_CHUNK + 7):
        S = -(-n // k)
        for E in (1, 5, 257, 1024):
            ids = torch.randint(0, E, (S, k), generator=g, device=DEV).to(dt)
            flat = ids.view(-1)
            where = torch.randperm(S * k, generator=g, device=DEV)[:max(3, S * k // 5)]
            bad = torch.tensor([E if b is None else b for b in BAD_IDS], device=DEV).to(dt)
            flat[where] = bad[torch.arange(where.numel(), device=DEV) % 3]
            got = _route_checked(ids, E)
            _same_route(got, route_reference(ids, E), (n, k, E))
            kept = S * k - where.numel()
            assert int(got[0][E]) == kept
            assert bool((got[1][kept:] == -1).all()) and bool((got[1][:kept] >= 0).all())
            assert bool((got[2].view(-1)[where] == -1).all())
    if dt == torch.int64:                         # ids that only 64 bits tell from valid ones
        ids = torch.tensor([[2 ** 32, 1], [2 ** 32 + 1, 0], [-2 ** 40, 1]], device=DEV)
        got = _route_checked(ids, 2)
        _same_route(got, route_reference(ids, 2), "64-bit ids")
        assert got[0].tolist() == [0, 1, 3] and got[2].tolist() == [[-1, 1], [-1, 0], [-1, 2]]
    every = torch.full((ROUTE_CHUNK + 3, 1), -1, dtype=dt, device=DEV)   # every id invalid
    got = _route_checked(every, 5)
    assert int(got[0].abs().sum()) == 0 and bool((got[1] == -1).all()) and bool((got[2] == -1).all())


def test_route_one_expert_takes_all_and_one_takes_none():
    for n, k in ((1, 1), (64, 2), (ROUTE_CHUNK + 1, 1), (3 * ROUTE_CHUNK + 8, 8)):
        S = n // k
        for E, e in ((1, 0), (5, 3), (1024, 1023), (257, 0)):
            ids = torch.full((S, k), e, dtype=torch.int32, device=DEV)
            got = _route_checked(ids, E)
            _same_route(got, route_reference(ids, E), (n, k, E))
            assert torch.equal(got[2].view(-1), torch.arange(n, dtype=torch.int32, device=DEV))
            assert got[0].tolist() == [0] * (e + 1) + [n] * (E - e)
        g = _gen(n)
        E = 6
        ids = torch.randint(0, E - 1, (S, k), generator=g, device=DEV)
        ids[ids >= 2] += 1                        # expert 2 gets no slot
        got = _route_checked(ids, E)
        _same_route(got, route_reference(ids, E), (n, k, "empty expert"))
        assert int(got[0][3]) == int(got[0][2])


@pytest.mark.parametrize("dt", [torch.int32, torch.int64])
def test_route_top1_is_stable_argsort(dt):
    from ddlb_amd.models.mx_moe import expert_ids

    for S, E in ((300, 5), (3 * ROUTE_CHUNK + 7, 64), (ROUTE_CHUNK, 1024)):
        ids = expert_ids(S, E, seed=S).to(DEV)
        offsets, row_token, slot_row = route(ids.reshape(S, 1).to(dt), E)
        perm = torch.argsort(ids, stable=True)
        assert torch.equal(row_token.long(), perm)
        counts = torch.zeros(E, dtype=torch.int32, device=DEV)
        counts.scatter_add_(0, ids, torch.ones_like(ids, dtype=torch.int32))
        want = torch.zeros(E + 1, dtype=torch.int32, device=DEV)
        want[1:] = torch.cumsum(counts, 0)
        assert torch.equal(offsets, want)
        assert torch.equal(perm[slot_row.view(-1).long()], torch.arange(S, device=DEV))


def test_route_empty_and_repeatable():
    from ddlb_amd.ops import load

    assert load().ROUTE_CHUNK == ROUTE_CHUNK      # the Python copy of moe_route_map.h's constant
    offsets, row_token, slot_row = route(torch.zeros((0, 2), dtype=torch.int64, device=DEV), 7)
    assert offsets.tolist() == [0] * 8 and row_token.numel() == 0 and slot_row.shape == (0, 2)
    ids = torch.randint(0, 64, (2 * ROUTE_CHUNK + 5, 2), generator=_gen(3), device=DEV)
    first = [t.clone() for t in route(ids, 64)]
    for _ in range(3):
        _same_route(route(ids, 64), first, "repeat")


# ------------------------------------------------------------------ quantize_mx_gather
def _edge_rows(x, dtype, fp4):
    """The quantisers' edge values, written over the first rows of ``x`` (the rows of
    test_mx_scaled_gpu / test_mxfp4_gpu ``test_quantizer_matches_reference``)."""
    top = 6.0 if fp4 else 448.0
    x[0] = 0                                       # a zero row
    x[1, 32:64] = 0                                # a zero block inside a row
    x[2] = 0
    x[2, 77] = -1.5                                # a lone maximum
    for i, j in enumerate((-9, -1, 0, 2, 6)):      # the boundary of the scale rule and above it
        x[3 + i, 0:32] = 1.0 * 2.0 ** j
        x[3 + i, 7] = top * 2.0 ** j
        x[3 + i, 32:64] = -2.0 * 2.0 ** j
        x[3 + i, 40] = (6.03125 if fp4 else 480.0) * 2.0 ** j
    x[8, 0:32] = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -130   # subnormal amax
    x[9] = 0                                       # every fp4 tie, both signs; signed zeros
    x[9, 0] = 6.0
    for i, v in enumerate(TIES):
        x[9, 1 + i] = v
        x[9, 9 + i] = -v
    x[9, 20] = -0.0
    x[9, 21] = -0.1
    x[9, 32:64] = 0                                # e4m3 ties under e = 0: odd multiples of 2^-10
    x[9, 32] = 448.0
    x[9, 33:37] = torch.tensor([2.0 ** -10, 3 * 2.0 ** -10, -5 * 2.0 ** -10, 17.0]).to(dtype)
    if dtype != torch.float16:                     # e = -127 (s = 0)
        x[10, 0:32] = 0
        x[10, 0:5] = torch.tensor([2.0 ** -125, 2.0 ** -126, -2.0 ** -127, 2.0 ** -128,
                                   1.5 * 2.0 ** -127]).to(dtype)
    return x


def _gather_case(x, src, fmt):
    from ddlb_amd.ops.mx import (quantize_mx, quantize_mx_gather, quantize_mx_gather_reference,
                                 quantize_mxfp4)

    q, s = quantize_mx_gather(x, src, fmt=fmt)
    X = x.shape[0]
    valid = (src >= 0) & (src < X)
    rows = x.index_select(0, torch.where(valid, src, torch.zeros_like(src)).long())
    qw, sw = (quantize_mxfp4 if fmt == "mxfp4" else quantize_mx)(rows)
    qw, sw = qw.view(torch.uint8).clone(), sw.clone()
    qw[~valid] = 0                                 # invalid indices: zero rows, scale byte 127
    sw[~valid] = 127
    assert q.dtype == (torch.float4_e2m1fn_x2 if fmt == "mxfp4" else torch.float8_e4m3fn)
    assert s.dtype == torch.uint8 and s.shape == sw.shape and q.shape == qw.shape
    assert torch.equal(s, sw), int((s != sw).sum())
    assert torch.equal(q.view(torch.uint8), qw), int((q.view(torch.uint8) != qw).sum())
    qr, sr = quantize_mx_gather_reference(x, src, fmt)   # and the torch specification
    assert torch.equal(s, sr) and torch.equal(q.view(torch.uint8), qr.view(torch.uint8))


@pytest.mark.parametrize("R", [1, 7, 300])
@pytest.mark.parametrize("fmt, K", [("mx", 128), ("mx", 384), ("mx", 4096), ("mxfp4", 256),
                                    ("mxfp4", 512), ("mxfp4", 4096)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_quantize_mx_gather_bytes(dtype, fmt, K, R):
    fp4 = fmt == "mxfp4"
    X = 41
    g = _gen(R + K)
    x = _edge_rows((wide_fp4 if fp4 else wide_fp8)(X, K, g, dtype), dtype, fp4)
    src = torch.randint(0, X, (R,), generator=g, device=DEV).to(torch.int32)   # repeats
    src[:min(R, 11)] = torch.arange(11, dtype=torch.int32, device=DEV)[:R]      # the edge rows
    _gather_case(x, src, fmt)
    if R > 1:                                      # invalid indices among them
        bad = torch.tensor([-1, X, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device=DEV)
        src[1::3] = bad[torch.arange(src[1::3].numel(), device=DEV) % 4]
        _gather_case(x, src, fmt)
    # a strided x: the middle columns of a wider tensor
    big = (wide_fp4 if fp4 else wide_fp8)(X, K + 512, g, dtype)
    _gather_case(big[:, 256:256 + K], src, fmt)


def test_quantize_mx_gather_all_invalid_and_empty():
    from ddlb_amd.ops.mx import quantize_mx_gather

    x = torch.full((4, 256), float("nan"), dtype=torch.bfloat16, device=DEV)
    src = torch.tensor([-1, 4, -5], dtype=torch.int32, device=DEV)
    for fmt in ("mx", "mxfp4"):
        q, s = quantize_mx_gather(x, src, fmt=fmt)
        assert int(q.view(torch.uint8).max()) == 0 and s.tolist() == [[127] * 8] * 3
        q, s = quantize_mx_gather(x[:0], src, fmt=fmt)       # no rows to gather from
        assert int(q.view(torch.uint8).max()) == 0 and s.tolist() == [[127] * 8] * 3
        q, s = quantize_mx_gather(x, src[:0], fmt=fmt)
        assert q.shape[0] == 0 and s.shape == (0, 8)


def test_quantize_mx_gather_more_rows_than_one_pass():
    """More output rows than the grid takes in one pass (one row of 512 vectors per workgroup)."""
    g = _gen(4)
    x = wide_fp8(600, 4096, g)
    src = torch.randint(-2, 602, (2500,), generator=g, device=DEV).to(torch.int32)
    _gather_case(x, src, "mx")
    _gather_case(x, src, "mxfp4")


def test_quantize_mx_gather_rows_past_2_and_4_gib():
    """Source rows whose byte offset needs more than 32 bits: ``x`` rows ``FAR_PITCH`` apart
    behind a 2 GiB guard, so a truncated or sign-extended offset reads another row or poison."""
    X, K = 260, 128
    g = torch.Generator(device="cpu").manual_seed(8)
    x = ints((X, K), torch.bfloat16, g)
    x[:, 0] = torch.arange(X, dtype=torch.float32).to(torch.bfloat16)   # the rows differ
    backing = far_backing(far_span(X, K * 2, FAR_PITCH))
    view = far_view(backing, x.to(DEV), FAR_PITCH)
    src = torch.tensor([259, 0, 127, 128, 255, 256, 129, 259], dtype=torch.int32, device=DEV)
    _gather_case(view, src, "mx")


# ------------------------------------------------------------------ combine
def _combine_case(dtype, H, k, g, *, integers=False, out_dtype=None, S=37):
    """Slots spread over distinct rows of ``y``; every row no slot points at holds NaN. A fifth of
    the slots is dropped (-1) or out of range (T, 2^31 - 1, a large negative)."""
    n = S * k
    T = n + 9
    if integers:
        y = ints((T, H), dtype, g)
        gate = torch.randint(0, 5, (S, k), generator=g, device=DEV).float()
    else:
        y = torch.randn((T, H), generator=g, device=DEV).to(dtype)
        gate = torch.rand((S, k), generator=g, device=DEV)
    rows = torch.randperm(T, generator=g, device=DEV)[:n].to(torch.int32)
    bad = torch.tensor([-1, T, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device=DEV)
    where = torch.randperm(n, generator=g, device=DEV)[:n // 5]
    rows[where] = bad[torch.arange(where.numel(), device=DEV) % 4]
    if S > 2:
        rows.view(S, k)[2] = -1                     # an all-dropped token
    slot_row = rows.view(S, k).contiguous()
    used = torch.zeros(T, dtype=torch.bool, device=DEV)
    ok = (rows >= 0) & (rows < T)
    used[rows[ok].long()] = True
    y[~used] = float("nan")
    odt = out_dtype or dtype
    buf, out = sentinel_out(S, H, odt, pad_cols=16 // y.element_size(), device=DEV)
    assert out.data_ptr() % 16 == 0 and (out.stride(0) * out.element_size()) % 16 == 0
    got = combine(y, slot_row, gate, out=out)
    assert got.data_ptr() == out.data_ptr()
    untouched(buf, S, H)
    assert not bool(torch.isnan(out.float()).any()), "a row no slot points at reached out"
    assert torch.equal(out, combine_reference(y, slot_row, gate, out_dtype=odt))
    if S > 2:
        assert torch.equal(out[2].float().view(torch.int32),
                           torch.zeros(H, dtype=torch.int32, device=DEV))      # +0.0
    fresh = combine(y, slot_row, gate, out_dtype=out_dtype)    # allocated by the call
    assert fresh.dtype == odt and torch.equal(fresh, out)
    return y, slot_row, gate, out, ok.view(S, k)


@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("H", [8, 256, 4104])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_combine_equals_reference(dtype, H, k):
    g = _gen(H + k)
    _combine_case(dtype, H, k, g)
    if dtype != torch.float32:
        _combine_case(dtype, H, k, g, out_dtype=torch.float32)


@pytest.mark.parametrize("k", [1, 2, 8])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_combine_exact_on_integers(dtype, k):
    """Rows in -3..3 and gates in 0..4: every product and partial sum is a small integer, so the
    result is the fp64 sum exactly, in every dtype."""
    for H in (8, 256, 4104):
        y, slot_row, gate, out, ok = _combine_case(dtype, H, k, _gen(k), integers=True)
        rows = torch.nan_to_num(y.double())[torch.where(ok, slot_row, 0).long()]   # [S, k, H]
        want = (rows * (gate.double() * ok).unsqueeze(2)).sum(dim=1)
        assert torch.equal(out.double(), want)


def test_combine_many_choices_many_tokens_and_strided_rows():
    """k above the register-cached count, more tokens than one pass of the grid takes, and ``y``
    rows with padding between them."""
    g = _gen(21)
    _combine_case(torch.bfloat16, 64, 11, g)
    _combine_case(torch.float32, 8, 16, g)
    _combine_case(torch.bfloat16, 4104, 1, g, S=2500)   # one token per workgroup and pass
    _combine_case(torch.bfloat16, 256, 2, g, S=17000)   # eight tokens per workgroup and pass
    S, k, H = 50, 3, 264
    wide = torch.randn((S * k, H + 24), generator=g, device=DEV).to(torch.bfloat16)
    y = wide[:, 8:8 + H]
    slot_row = torch.randperm(S * k, generator=g, device=DEV).to(torch.int32).view(S, k)
    gate = torch.rand((S, k), generator=g, device=DEV)
    assert torch.equal(combine(y, slot_row, gate), combine_reference(y, slot_row, gate))
    out = combine(y[:0], slot_row, gate)           # no rows at all: every slot is out of range
    assert int(out.float().abs().sum()) == 0


# ------------------------------------------------------------------ the model
def _forward_emulated(m):
    """The native pipeline with torch ops on the token side: ``index_select`` by ``row_token``,
    the existing quantiser, the same grouped GEMMs, ``combine_reference``."""
    from ddlb_amd.models.mx_mlp import _fmt_ops
    from ddlb_amd.ops.gemm import gemm_grouped

    quant, _, _ = _fmt_ops(m.fmt)
    offsets, row_token, slot_row = route_reference(m.ids, m.E)
    assert int(offsets[m.E]) == m.S * m.top_k
    xq, xs = quant(m.X.index_select(0, row_token.long()))
    if m.fused:
        hq, hs = gemm_grouped(xq, m.w1q, offsets, a_scale=xs, w_scale=m.w1s, act=m.act,
                              tile=m.tile, glu=True, out_quant=m.fmt)
    else:
        h = gemm_grouped(xq, m.w1q, offsets, a_scale=xs, w_scale=m.w1s, act=m.act, tile=m.tile,
                         glu=True, out_dtype=torch.bfloat16)
        hq, hs = quant(h)
    y = gemm_grouped(hq, m.w2q, offsets, a_scale=hs, w_scale=m.w2s, tile=m.tile,
                     out_dtype=torch.bfloat16)
    return combine_reference(y, slot_row, m.gates)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("fmt", ["mx", "mxfp4"])
def test_model_native_top1_equals_torch_dispatch(fmt, fused):
    from ddlb_amd.models.mx_moe import MxMoE

    old = MxMoE(256, 256, 300, 5, fmt, fused=fused)
    new = MxMoE(256, 256, 300, 5, fmt, fused=fused, dispatch="native")
    assert torch.equal(new.ids.view(-1), old.ids) and new.flops == old.flops
    want = old.forward().clone()
    got = new.forward()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    new.validate()
    assert torch.equal(got, _forward_emulated(new))


@pytest.mark.parametrize("top_k", [2, 4])
@pytest.mark.parametrize("fmt", ["mx", "mxfp4"])
def test_model_top_k(fmt, top_k):
    from ddlb_amd.models.mx_moe import MxMoE

    for fused in (True, False):
        m = MxMoE(256, 256, 300, 5, fmt, fused=fused, top_k=top_k, dispatch="native")
        assert tuple(m.ids.shape) == (300, top_k) and m.flops == 6.0 * 300 * top_k * 256 * 256
        out = m.forward()
        torch.cuda.synchronize()
        m.validate()
        assert torch.equal(out, _forward_emulated(m))


def test_model_native_forward_in_a_graph():
    """One linear capture on one stream; the routing is replaced in place and the graph replayed."""
    from ddlb_amd.models.mx_moe import MxMoE, expert_ids_topk

    m = MxMoE(256, 256, 300, 5, "mx", top_k=2, dispatch="native")
    first = m.forward().clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.forward()                                 # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = m.forward()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, first)
    ids, gates = expert_ids_topk(300, 5, 2, seed=9)
    m.ids.copy_(ids)
    m.gates.copy_(gates)
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    assert not torch.equal(replayed, first)
    eager = m.forward()
    torch.cuda.synchronize()
    assert torch.equal(replayed, eager)
    m.validate(replayed)

