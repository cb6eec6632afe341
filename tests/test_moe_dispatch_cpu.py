"""The MoE dispatch layer off the GPU: every refusal of ``route`` / ``combine`` /
``quantize_mx_gather`` (all raised before anything is loaded or launched, so CPU tensors reach
them), the torch references against hand-written loops, and the top-k model helpers."""

import pytest
import torch

from ddlb_amd.models.mx_moe import MxMoE, expert_ids, expert_ids_topk
from ddlb_amd.ops.gemm import MAX_GROUPS
from ddlb_amd.ops.moe import (ROUTE_CHUNK, _check_combine, _check_route, combine, combine_reference,
                              route, route_reference, route_workspace_words)
from ddlb_amd.ops.mx import (_check_quant_gather, quantize_mx_gather, quantize_mx_gather_reference,
                             quantize_mx_reference, quantize_mxfp4_reference)

DEVICE_REFUSAL = "needs a ROCm device tensor|needs ROCm device tensors"


# ------------------------------------------------------------------ refusals
def _ids(S=6, k=2, dtype=torch.int64):
    return torch.zeros((S, k), dtype=dtype)


def _route_out(S=6, k=2, E=4):
    return [torch.zeros(E + 1, dtype=torch.int32), torch.zeros(S * k, dtype=torch.int32),
            torch.zeros((S, k), dtype=torch.int32)]


def test_route_good_arguments_reach_the_device_refusal():
    for dt in (torch.int32, torch.int64):
        with pytest.raises(ValueError, match=DEVICE_REFUSAL):
            route(_ids(dtype=dt), 4)
        with pytest.raises(ValueError, match=DEVICE_REFUSAL):
            route(_ids(dtype=dt), 4, out=_route_out())
    with pytest.raises(ValueError, match=DEVICE_REFUSAL):
        route(_ids(0, 2), MAX_GROUPS)       # S == 0 and the largest E are legal


@pytest.mark.parametrize("make, exc, msg", [
    (lambda: (_ids().float(), 4, None), TypeError, "int32 or int64"),
    (lambda: ([[0, 1]], 4, None), TypeError, "int32 or int64"),
    (lambda: (_ids().reshape(-1), 4, None), ValueError, "2-D"),
    (lambda: (_ids(), 4.0, None), TypeError, "experts must be an int"),
    (lambda: (_ids(), 0, None), ValueError, "experts must be in 1"),
    (lambda: (_ids(), MAX_GROUPS + 1, None), ValueError, "experts must be in 1"),
    (lambda: (torch.zeros((6, 0), dtype=torch.int64), 4, None), ValueError, "k >= 1"),
    (lambda: (torch.zeros((6, 4), dtype=torch.int64)[:, ::2], 4, None), ValueError, "contiguous"),
    (lambda: (torch.zeros((1, 2), dtype=torch.int32).expand(2 ** 30, 2), 4, None), ValueError,
     "below 2\\^31"),
    (lambda: (_ids(), 4, _route_out()[:2]), TypeError, "triple"),
])
def test_route_refusals(make, exc, msg):
    ids, E, out = make()
    with pytest.raises(exc, match=msg):
        _check_route(ids, E, out)


@pytest.mark.parametrize("which, change, exc, msg", [
    (0, lambda t: t.long(), TypeError, "offsets.*int32"),
    (1, lambda t: t.float(), TypeError, "row_token.*int32"),
    (2, lambda t: t.long(), TypeError, "slot_row.*int32"),
    (0, lambda t: t[:-1], ValueError, "offsets.*shape"),
    (1, lambda t: torch.zeros(13, dtype=torch.int32), ValueError, "row_token.*shape"),
    (2, lambda t: t.reshape(-1), ValueError, "slot_row.*shape"),
    (1, lambda t: torch.zeros(24, dtype=torch.int32)[::2], ValueError, "row_token.*contiguous"),
    (2, lambda t: torch.zeros((6, 4), dtype=torch.int32)[:, :2], ValueError,
     "slot_row.*contiguous"),
])
def test_route_out_refusals(which, change, exc, msg):
    out = _route_out()
    out[which] = change(out[which])
    with pytest.raises(exc, match=msg):
        _check_route(_ids(), 4, out)


def _combine_args(T=5, H=8, S=3, k=2, dtype=torch.bfloat16):
    return dict(y=torch.zeros((T, H), dtype=dtype), slot_row=torch.zeros((S, k), dtype=torch.int32),
                gate=torch.zeros((S, k), dtype=torch.float32))


def test_combine_good_arguments_reach_the_device_refusal():
    for dt, H in ((torch.bfloat16, 8), (torch.float16, 24), (torch.float32, 4)):
        a = _combine_args(H=H, dtype=dt)
        with pytest.raises(ValueError, match=DEVICE_REFUSAL):
            combine(**a)
        with pytest.raises(ValueError, match=DEVICE_REFUSAL):
            combine(**a, out_dtype=torch.float32)
        with pytest.raises(ValueError, match=DEVICE_REFUSAL):
            combine(**a, out=torch.zeros((3, H), dtype=dt))


@pytest.mark.parametrize("change, exc, msg", [
    (dict(y=torch.zeros((5, 8), dtype=torch.float64)), TypeError, "y must be one of"),
    (dict(y=torch.zeros((5, 8), dtype=torch.int32)), TypeError, "y must be one of"),
    (dict(y=torch.zeros(40, dtype=torch.bfloat16)), ValueError, "2-D"),
    (dict(slot_row=torch.zeros((3, 2), dtype=torch.int64)), TypeError, "slot_row must be an int32"),
    (dict(gate=torch.zeros((3, 2), dtype=torch.bfloat16)), TypeError, "gate must be a float32"),
    (dict(slot_row=torch.zeros(6, dtype=torch.int32)), ValueError, r"\[S, k\]"),
    (dict(slot_row=torch.zeros((3, 0), dtype=torch.int32)), ValueError, "k >= 1"),
    (dict(gate=torch.zeros((3, 3), dtype=torch.float32)), ValueError, "slot_row's shape"),
    (dict(gate=torch.zeros((3, 4), dtype=torch.float32)[:, ::2]), ValueError, "contiguous"),
    (dict(slot_row=torch.zeros((2, 3), dtype=torch.int32).t()), ValueError, "contiguous"),
    (dict(y=torch.zeros((5, 12), dtype=torch.bfloat16)), ValueError, "whole 16-byte vectors"),
    (dict(y=torch.zeros((5, 6), dtype=torch.float32)), ValueError, "whole 16-byte vectors"),
    (dict(y=torch.zeros((5, 16), dtype=torch.bfloat16)[:, ::2]), ValueError, "unit inner stride"),
    (dict(y=torch.zeros((5, 24), dtype=torch.bfloat16)[:, 4:12]), ValueError, "16-byte-aligned"),
    (dict(y=torch.zeros((5, 12), dtype=torch.bfloat16)[:, :8]), ValueError, "16-byte-aligned"),
    (dict(out_dtype=torch.float16), TypeError, "writes torch.bfloat16 or torch.float32"),
    (dict(out=torch.zeros((3, 8), dtype=torch.float16)), TypeError, "writes torch.bfloat16 or"),
    (dict(out=torch.zeros((3, 8), dtype=torch.int32)), TypeError, "out must be one of"),
    (dict(out=torch.zeros((3, 8), dtype=torch.bfloat16), out_dtype=torch.float32), TypeError,
     "out is torch.bfloat16, out_dtype"),
    (dict(out=torch.zeros((4, 8), dtype=torch.bfloat16)), ValueError, "out must have shape"),
    (dict(out=torch.zeros((3, 16), dtype=torch.bfloat16)[:, ::2]), ValueError,
     "row-major out"),
    (dict(out=torch.zeros((3, 12), dtype=torch.bfloat16)[:, :8]), ValueError,
     "16-byte-aligned rows of out"),
])
def test_combine_refusals(change, exc, msg):
    a = _combine_args()
    a.update(change)
    with pytest.raises(exc, match=msg):
        _check_combine(**a)


def test_quantize_mx_gather_good_arguments_reach_the_device_refusal():
    src = torch.zeros(7, dtype=torch.int32)
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        with pytest.raises(ValueError, match=DEVICE_REFUSAL):
            quantize_mx_gather(torch.zeros((4, 128), dtype=dt), src)
        with pytest.raises(ValueError, match=DEVICE_REFUSAL):
            quantize_mx_gather(torch.zeros((4, 256), dtype=dt), src, fmt="mxfp4")
    with pytest.raises(ValueError, match=DEVICE_REFUSAL):   # no rows to gather from, none to write
        quantize_mx_gather(torch.zeros((0, 128)), src[:0])


@pytest.mark.parametrize("x, src, fmt, exc, msg", [
    (torch.zeros((4, 128), dtype=torch.float64), None, "mx", TypeError, "takes"),
    ([[0.0] * 128], None, "mx", TypeError, "expects a tensor"),
    (torch.zeros((4, 128)), None, "fp8", ValueError, "fmt must be one of"),
    (torch.zeros(128), None, "mx", ValueError, "2-D"),
    (torch.zeros((4, 96)), None, "mx", ValueError, "K % 128"),
    (torch.zeros((4, 128)), None, "mxfp4", ValueError, "K % 256"),
    (torch.zeros((4, 128)), torch.zeros(7, dtype=torch.int64), "mx", TypeError, "src must be an"),
    (torch.zeros((4, 128)), torch.zeros((7, 1), dtype=torch.int32), "mx", ValueError, "1-D"),
    (torch.zeros((4, 128)), torch.zeros(14, dtype=torch.int32)[::2], "mx", ValueError,
     "contiguous"),
    (torch.zeros((4, 256))[:, ::2], None, "mx", ValueError, "unit inner stride"),
    (torch.zeros((4, 264), dtype=torch.bfloat16)[:, 1:129], None, "mx", ValueError,
     "16-byte-aligned"),
    (torch.zeros((4, 132), dtype=torch.bfloat16)[:, :128], None, "mx", ValueError,
     "16-byte-aligned"),
])
def test_quantize_mx_gather_refusals(x, src, fmt, exc, msg):
    src = torch.zeros(7, dtype=torch.int32) if src is None else src
    with pytest.raises(exc, match=msg):
        _check_quant_gather(x, src, fmt)


# ------------------------------------------------------------------ references
def _route_loop(ids, E):
    """The specification, slot by slot in Python."""
    S, k = ids.shape
    flat = ids.reshape(-1).tolist()
    rows = [p for e in range(E) for p in range(S * k) if flat[p] == e]
    offsets = [0]
    for e in range(E):
        offsets.append(offsets[-1] + sum(1 for v in flat if v == e))
    row_token = [p // k for p in rows] + [-1] * (S * k - len(rows))
    slot_row = [-1] * (S * k)
    for r, p in enumerate(rows):
        slot_row[p] = r
    return offsets, row_token, slot_row


@pytest.mark.parametrize("S, k, E", [(1, 1, 1), (7, 1, 3), (9, 2, 5), (33, 4, 8), (16, 8, 2),
                                     (40, 3, 64)])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_route_reference_is_the_loop(S, k, E, dtype):
    g = torch.Generator().manual_seed(S * 100 + k * 10 + E)
    ids = torch.randint(0, E, (S, k), generator=g).to(dtype)
    for drop in (False, True):
        if drop:  # -1, E, the largest value of the dtype: dropped, not counted
            bad = torch.tensor([-1, E, torch.iinfo(dtype).max, -5, 2 ** 31 - 1]).to(dtype)
            where = torch.randperm(S * k, generator=g)[:min(5, S * k)]
            ids.view(-1)[where] = bad[:where.numel()]
        offsets, row_token, slot_row = route_reference(ids, E)
        want = _route_loop(ids, E)
        assert offsets.dtype == row_token.dtype == slot_row.dtype == torch.int32
        assert tuple(slot_row.shape) == (S, k)
        assert offsets.tolist() == want[0]
        assert row_token.tolist() == want[1]
        assert slot_row.reshape(-1).tolist() == want[2]
        if drop:
            assert int(offsets[E]) < S * k


def test_route_reference_top1_is_the_model_route():
    """``k = 1``: ``row_token`` is the stable argsort and ``offsets`` what ``MxMoE.route()``
    counts (the same torch ops, on the CPU)."""
    S, E = 300, 5
    ids = expert_ids(S, E, seed=3)
    offsets, row_token, slot_row = route_reference(ids.reshape(S, 1), E)
    perm = torch.argsort(ids, stable=True)
    counts = torch.zeros(E, dtype=torch.int32)
    counts.scatter_add_(0, ids, torch.ones_like(ids, dtype=torch.int32))
    want = torch.zeros(E + 1, dtype=torch.int32)
    want[1:] = torch.cumsum(counts, 0)
    assert torch.equal(row_token.long(), perm)
    assert torch.equal(offsets, want)
    assert int(counts[E // 2]) == 0                      # the empty expert
    inv = torch.empty(S, dtype=torch.long)
    inv[perm] = torch.arange(S)
    assert torch.equal(slot_row.reshape(-1).long(), inv)


def test_route_workspace_words():
    assert ROUTE_CHUNK == 1024
    assert route_workspace_words(1, 5) == 2 * 5
    assert route_workspace_words(ROUTE_CHUNK, 7) == 2 * 7
    assert route_workspace_words(ROUTE_CHUNK + 1, 7) == 3 * 7
    assert route_workspace_words(2 ** 31 - 1, 1024) == (2 ** 21 + 1) * 1024


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_combine_reference_exact_on_small_integers(dtype):
    g = torch.Generator().manual_seed(5)
    T, H, S, k = 11, 8, 6, 3
    y = torch.randint(-3, 4, (T, H), generator=g).float()
    y[7] = float("nan")                                  # a row no slot points at
    gate = torch.randint(0, 4, (S, k), generator=g).float()
    slot_row = torch.tensor([[0, 1, 2], [3, -1, 4], [-1, -1, -1], [5, T, 6], [8, 9, 10],
                             [2 ** 31 - 1, 0, -7]], dtype=torch.int32)
    want = torch.zeros((S, H), dtype=torch.float64)
    for t in range(S):
        for j in range(k):
            r = int(slot_row[t, j])
            if 0 <= r < T:
                want[t] += float(gate[t, j]) * y[r].double()
    for odt in (None, torch.float32):
        out = combine_reference(y.to(dtype), slot_row, gate, out_dtype=odt)
        assert out.dtype == (odt or dtype)
        assert torch.equal(out.double(), want)
    # the all-dropped token is +0.0, not -0.0 and not what y holds
    out = combine_reference(y.to(dtype), slot_row, gate)
    assert torch.equal(out[2].float().view(torch.int32), torch.zeros(H, dtype=torch.int32))
    # a negative zero product does not make the sum negative: +0 + -0 = +0
    neg = combine_reference(torch.zeros((1, H), dtype=dtype), torch.zeros((1, 1), dtype=torch.int32),
                            torch.full((1, 1), -1.0))
    assert torch.equal(neg.float().view(torch.int32), torch.zeros((1, H), dtype=torch.int32))


@pytest.mark.parametrize("fmt", ["mx", "mxfp4"])
def test_quantize_mx_gather_reference(fmt):
    g = torch.Generator().manual_seed(9)
    x = torch.randn((6, 256), generator=g).to(torch.bfloat16)
    src = torch.tensor([5, 0, 0, -1, 6, 3, 2 ** 31 - 1], dtype=torch.int32)
    q, s = quantize_mx_gather_reference(x, src, fmt)
    rows = torch.zeros((7, 256), dtype=torch.bfloat16)
    for r, i in enumerate(src.tolist()):
        if 0 <= i < 6:
            rows[r] = x[i]
    qr, sr = (quantize_mxfp4_reference if fmt == "mxfp4" else quantize_mx_reference)(rows)
    assert torch.equal(q.view(torch.uint8), qr.view(torch.uint8)) and torch.equal(s, sr)
    for r in (3, 4, 6):                                  # invalid: zero data, scale byte 127
        assert int(q.view(torch.uint8)[r].max()) == 0 and s[r].tolist() == [127] * 8
    q0, s0 = quantize_mx_gather_reference(x[:0], src, fmt)
    assert int(q0.view(torch.uint8).max()) == 0 and int(s0.min()) == 127


# ------------------------------------------------------------------ the model's helpers
@pytest.mark.parametrize("E, k", [(5, 2), (5, 4), (8, 7), (3, 3), (64, 8), (1, 1)])
def test_expert_ids_topk(E, k):
    S = 400
    ids, gates = expert_ids_topk(S, E, k, seed=2)
    assert ids.dtype == torch.int64 and tuple(ids.shape) == (S, k)
    assert gates.dtype == torch.float32 and tuple(gates.shape) == (S, k)
    assert int(ids.min()) >= 0 and int(ids.max()) < E
    srt = torch.sort(ids, dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all())       # distinct experts per token
    if E >= 4:
        assert int((ids == E // 2).sum()) == 0           # one expert is never drawn
    assert bool((gates >= 0).all())
    assert float((gates.sum(dim=1) - 1.0).abs().max()) <= 1e-6
    again = expert_ids_topk(S, E, k, seed=2)
    assert torch.equal(ids, again[0]) and torch.equal(gates, again[1])
    other = expert_ids_topk(S, E, k, seed=3)
    assert k == E or (E >= 4 and k == E - 1) or not torch.equal(ids, other[0])
    assert not torch.equal(gates, other[1]) or k == 1
    if E > 2 and k < E - 1:                              # uneven: the heaviest beats the lightest
        assert int((ids == E - 1).sum()) > int((ids == 0).sum())


def test_expert_ids_topk_refusals():
    with pytest.raises(ValueError, match="positive"):
        expert_ids_topk(4, 4, 0)
    with pytest.raises(ValueError, match="can be drawn"):
        expert_ids_topk(4, 5, 5)                         # expert 2 of 5 is never drawn
    with pytest.raises(ValueError, match="can be drawn"):
        expert_ids_topk(4, 2, 3)


@pytest.mark.parametrize("kw, msg", [
    (dict(dispatch="hip"), "dispatch must be one of"),
    (dict(top_k=0), "top_k must be a positive int"),
    (dict(top_k=2), "needs dispatch='native'"),
    (dict(top_k=6, dispatch="native"), "at least that many experts"),
])
def test_model_argument_refusals(kw, msg):
    with pytest.raises(ValueError, match=msg):
        MxMoE(128, 128, 16, 5, **kw)


@pytest.mark.parametrize("fmt, H", [("mx", 128), ("mxfp4", 256)])
def test_reference_chain_topk_at_k1_is_reference_chain(fmt, H):
    from ddlb_amd.ops.gemm import pack_glu_grouped

    g = torch.Generator().manual_seed(1)
    S, E, F = 40, 5, H
    X = (torch.rand((S, H), generator=g) * 2 - 1).to(torch.bfloat16)
    gate, up = ((torch.rand((E, F, H), generator=g) * 2 - 1).mul(H ** -0.5).to(torch.bfloat16)
                for _ in range(2))
    W1 = pack_glu_grouped(gate, up)
    W2 = ((torch.rand((E, H, F), generator=g) * 2 - 1) * F ** -0.5).to(torch.bfloat16)
    ids = expert_ids(S, E, seed=4)
    one = MxMoE.reference_chain(X, W1, W2, ids, "silu", fmt)
    topk = MxMoE.reference_chain_topk(X, W1, W2, ids.reshape(S, 1), torch.ones((S, 1)), "silu", fmt)
    assert torch.equal(one, topk)
    # two choices with gates (1, 0) and (0.5, 0.5) of the same expert: still the top-1 chain
    ids2 = torch.stack((ids, ids), dim=1)
    for gates in ((1.0, 0.0), (0.5, 0.5)):
        got = MxMoE.reference_chain_topk(X, W1, W2, ids2, torch.tensor([gates]).expand(S, 2),
                                         "silu", fmt)
        assert torch.equal(one, got)
