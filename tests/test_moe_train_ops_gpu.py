"""The training-side dispatch ops on the GPU (``ddlb_amd/ops/moe.py``): the dense ``gather``
(``csrc/moe/moe_gather.hip``) and ``combine_bwd`` (``csrc/moe/moe_combine_bwd.hip``).

``gather`` and ``dy`` are compared bit for bit with their torch specifications; ``dgate`` exactly
on integer data and, on uniform +-1 data, within the first-order summation bound that holds for
any order of the additions, ``H 2^-24 sum_c |dout y|`` computed elementwise in fp64 (twice that
for f32 operands, whose products round as well). Outputs sit in sentinel-surrounded buffers."""

import pytest
import torch

from _exact import ints, padded, sentinel_out, untouched

from ddlb_amd.ops.moe import (combine_bwd, combine_bwd_reference, gather, gather_reference,
                              route)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
PAIRS = [(torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16),
         (torch.float32, torch.float32), (torch.float32, torch.bfloat16),
         (torch.float32, torch.float16)]             # (dout, dy): combine's pairs, mirrored
HS = (8, 24, 8 * 257)   # one vector; no power of two; more vectors per row than threads
E = 5
MANY_ROWS = 2509       # long rows go one per pass and the grid is capped at 8 workgroups per CU
#                        (2048 on 256 CUs): this many rows need a second grid-stride trip


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _pm1(shape, dtype, g):
    return (torch.rand(shape, generator=g, device=DEV) * 2 - 1).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", HS)
def test_gather_equals_index_select_with_zero_rows(H, dtype):
    g = _gen(H)
    S, T = 37, 300
    x = padded(_pm1((S, H), dtype, g))
    assert x.stride(0) > H
    row_token = torch.randint(0, S, (T,), generator=g, device=DEV).to(torch.int32)
    row_token[::7] = -1
    row_token[3::11] = S
    row_token[5] = 2 ** 31 - 1
    buf, out = sentinel_out(T, H, dtype, pad_cols=16 // x.element_size())
    assert gather(x, row_token, out=out) is out
    torch.cuda.synchronize()
    untouched(buf, T, H)
    want = gather_reference(x, row_token)
    assert torch.equal(out.contiguous().view(torch.uint8), want.view(torch.uint8))
    zero = out[::7].contiguous().view(torch.uint8)
    assert bool((zero == 0).all()), "+0.0 rows by bit pattern"
    assert torch.equal(gather(x, row_token), want)
    assert tuple(gather(x, row_token[:0]).shape) == (0, H)


def test_gather_more_rows_than_one_pass_of_the_grid():
    """Long rows take one row per workgroup pass and the grid is capped at 8 workgroups per CU, so
    ``T = MANY_ROWS`` rows make the grid-stride loop take a second trip."""
    g = _gen(5)
    S, T, H = 37, MANY_ROWS, HS[2]
    x = _pm1((S, H), torch.bfloat16, g)
    row_token = torch.randint(-1, S + 1, (T,), generator=g, device=DEV).to(torch.int32)
    buf, out = sentinel_out(T, H, torch.bfloat16, pad_cols=8)
    gather(x, row_token, out=out)
    torch.cuda.synchronize()
    untouched(buf, T, H)
    assert torch.equal(out, gather_reference(x, row_token))


def _routing(S, k, seed):
    """ids with an expert without tokens (3) and, past the first tokens, ids outside [0, E)."""
    g = _gen(seed)
    ids = torch.randint(0, E - 1, (S, k), generator=g, device=DEV)
    ids[ids == 3] = 4
    if S > 2:
        ids[1, 0] = -1
        ids[S - 1, k - 1] = E
        ids[S // 2, k // 2] = 2 ** 31 - 1
    offsets, row_token, slot_row = route(ids, E)
    return ids, offsets, row_token, slot_row


def _case(S, k, H, ddt, ydt, integers, seed):
    g = _gen(seed)
    ids, offsets, row_token, slot_row = _routing(S, k, seed)
    T = S * k
    draw = (lambda shape, dt: ints(shape, dt, g)) if integers else \
        (lambda shape, dt: _pm1(shape, dt, g))
    dout = padded(draw((S, H), ddt))
    y = draw((T, H), ydt)
    gate = draw((S, k), torch.float32)
    # rows no slot points at hold NaN: they must not be read
    used = torch.zeros(T, dtype=torch.bool, device=DEV)
    used[slot_row[slot_row >= 0].long()] = True
    y[~used] = float("nan")
    return dout, padded(y), gate, row_token, slot_row, used


def _run(dout, y, gate, row_token, slot_row, ydt):
    S, k = slot_row.shape
    T, H = row_token.shape[0], dout.shape[1]
    ybuf, dy = sentinel_out(T, H, ydt, pad_cols=16 // torch.empty((), dtype=ydt).element_size())
    gbuf = torch.full((S + 2, k), -7.0, device=DEV)
    dgate = gbuf[1:S + 1] if y is not None else None
    got = combine_bwd(dout, slot_row, gate, row_token, y, dy_dtype=ydt, out=(dy, dgate))
    torch.cuda.synchronize()
    assert got[0] is dy and got[1] is dgate
    untouched(ybuf, T, H)
    assert bool((gbuf[0] == -7.0).all()) and bool((gbuf[S + 1] == -7.0).all())
    if y is None:
        assert bool((gbuf == -7.0).all())
    return dy, dgate


@pytest.mark.parametrize("ddt,ydt", PAIRS)
@pytest.mark.parametrize("k", [1, 2, 8, 9])
def test_combine_bwd(k, ddt, ydt):
    for S in (1, 3, 300):
        for H in HS:
            for integers in (True, False):
                dout, y, gate, row_token, slot_row, used = _case(S, k, H, ddt, ydt, integers,
                                                                 S + 7 * k + H)
                T = S * k
                dy, dgate = _run(dout, y, gate, row_token, slot_row, ydt)
                dy_ref, dg_ref = combine_bwd_reference(dout, slot_row, gate, row_token, y,
                                                       dy_dtype=ydt)
                what = (S, k, H, integers)
                assert torch.equal(dy, dy_ref), what
                word = torch.int32 if ydt == torch.float32 else torch.int16
                assert bool((dy.contiguous().view(word)[~used] == 0).all()), \
                    (what, "padding rows are +0.0")
                assert not bool(torch.isnan(dgate).any()), (what, "an unused y row was read")
                dropped = (slot_row < 0)
                assert bool((dgate.contiguous().view(torch.int32)[dropped] == 0).all()), what
                if integers:
                    assert torch.equal(dgate.double(), dg_ref), what
                else:
                    rows = slot_row.clamp(min=0).long()
                    mag = torch.zeros((S, k), dtype=torch.float64, device=DEV)
                    for j in range(k):
                        prod = (dout.double() * torch.nan_to_num(y.double()[rows[:, j]])).abs()
                        mag[:, j] = prod.sum(dim=1)
                    mag[dropped] = 0
                    bound = H * 2.0 ** -24 * mag * (2 if ydt == torch.float32 else 1)
                    err = (dgate.double() - dg_ref).abs()
                    print(f"S={S} k={k} H={H} {ddt} {ydt}: max dgate err = {float(err.max()):.3g}"
                          f", its bound {float(bound.max()):.3g}")
                    assert bool((err <= bound).all()), what
                again = _run(dout, y, gate, row_token, slot_row, ydt)
                assert torch.equal(again[0], dy) and torch.equal(again[1], dgate), what
                dy2, none = _run(dout, None, gate, row_token, slot_row, ydt)
                assert none is None and torch.equal(dy2, dy), what
                if k > 1 and S > 2:
                    assert int(dropped.sum()) >= 3 and int((~used).sum()) >= 3
                assert T == row_token.shape[0]


@pytest.mark.parametrize("k", [2, 9])
def test_combine_bwd_more_tokens_than_one_pass_of_the_grid(k):
    """``S = MANY_ROWS`` tokens of long rows: both phases of the kernel, barriers included, take a
    second grid-stride trip, on the register path and on the loop path."""
    S, H, dt = MANY_ROWS, HS[2], torch.bfloat16
    dout, y, gate, row_token, slot_row, used = _case(S, k, H, dt, dt, True, k)
    dy, dgate = _run(dout, y, gate, row_token, slot_row, dt)
    dy_ref, dg_ref = combine_bwd_reference(dout, slot_row, gate, row_token, y)
    assert torch.equal(dy, dy_ref) and torch.equal(dgate.double(), dg_ref)
    assert bool((dy.contiguous().view(torch.int16)[~used] == 0).all()) and int((~used).sum()) >= 3


def test_combine_bwd_allocates_and_takes_empty_inputs():
    dout, y, gate, row_token, slot_row, _ = _case(3, 2, 24, torch.float32, torch.bfloat16, True, 1)
    dy, dgate = combine_bwd(dout, slot_row, gate, row_token, y)
    assert dy.dtype == torch.bfloat16 and dgate.dtype == torch.float32
    ref = combine_bwd_reference(dout, slot_row, gate, row_token, y)
    assert torch.equal(dy, ref[0]) and torch.equal(dgate.double(), ref[1])
    dy, none = combine_bwd(dout, slot_row, gate, row_token, dy_dtype=torch.float16)
    assert dy.dtype == torch.float16 and none is None
    z = torch.zeros((0, 24), device=DEV)
    e = combine_bwd(z, slot_row[:0], gate[:0], row_token[:0], z)
    assert tuple(e[0].shape) == (0, 24) and tuple(e[1].shape) == (0, 2)


@pytest.mark.parametrize("k", [2, 9])
def test_indices_out_of_range_write_nothing_outside(k):
    """The range checks: with indices that are no routing at all (negative, ``>= S``, ``>= T``,
    ``2^31 - 1``) both ops complete and every guard region is untouched."""
    S, H = 40, 24
    T = S * k
    g = _gen(k)
    bad = torch.tensor([-1, -5, -2 ** 31, 2 ** 31 - 1, S, T, T + 1, 10 * T], device=DEV)
    slot_row = torch.randint(0, T, (S, k), generator=g, device=DEV)
    slot_row.view(-1)[::3] = bad[torch.arange(len(slot_row.view(-1)[::3]), device=DEV) % len(bad)]
    row_token = torch.randint(0, S, (T,), generator=g, device=DEV)
    row_token[::4] = bad[torch.arange(len(row_token[::4]), device=DEV) % len(bad)]
    slot_row, row_token = slot_row.to(torch.int32), row_token.to(torch.int32)
    for ddt, ydt in PAIRS:
        dout = padded(_pm1((S, H), ddt, g))
        y = padded(_pm1((T, H), ydt, g))
        gate = _pm1((S, k), torch.float32, g)
        dy, dgate = _run(dout, y, gate, row_token, slot_row, ydt)
        assert bool(torch.isfinite(dgate).all())
        x = padded(_pm1((S, H), ydt, g))
        buf, out = sentinel_out(T, H, ydt, pad_cols=16 // x.element_size())
        gather(x, row_token, out=out)
        torch.cuda.synchronize()
        untouched(buf, T, H)
        assert torch.equal(out, gather_reference(x, row_token))
