"""The grouped transposing MX quantiser on the GPU: ``ops.mx.quantize_mx_t_grouped``.

The oracle is exact: inside every group's column range the bytes of ``qt`` and ``st`` equal
``quantize_mx_t_reference`` of the group's rows padded with zero rows to a multiple of 128
(MXFP4: 256), and every other byte of the sentinel-filled buffers the outputs are views of (the
columns no group owns, the padded pitches, the extra rows) still holds the sentinel. ``x`` is a
view with a padded pitch and poison behind its columns and rows."""

import pytest
import torch

import _exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP8 = torch.float8_e4m3fn
FP4 = torch.float4_e2m1fn_x2
SENT = 0xA5
COUNTS = (0, 1, 130, 0, 256, 257, 0)
# (counts, o[0], rows behind o[E]): the sets of tests/test_gemm_grouped_gpu.py
OFFSET_SETS = {"counts": (COUNTS, 0, 0), "shifted": (COUNTS, 3, 0), "one_group": ((130,), 0, 0),
               "all_empty": ((0, 0, 0), 2, 3), "trailing": (COUNTS, 0, 5)}
DTYPES = (torch.bfloat16, torch.float16, torch.float32)
FMTS = ("mx", "mxfp4")


def _mod(fmt):
    return 256 if fmt == "mxfp4" else 128


def _offsets(counts, o0):
    o = [o0]
    for c in counts:
        o.append(o[-1] + c)
    return o


def _views(fmt, lead, C, cap, pad=32, spad=8, extra=3):
    """Sentinel-filled byte buffers and the (qt, st) views into them: pitches above the row
    length, extra rows, and (``lead``: stacked) a gap between the slabs."""
    ncol = cap // 2 if fmt == "mxfp4" else cap
    qb = torch.full(lead + (C + extra, ncol + pad), SENT, dtype=torch.uint8, device=DEV)
    sb = torch.full(lead + (C + extra, cap // 32 + spad), SENT, dtype=torch.uint8, device=DEV)
    qt = qb[..., :C, :ncol].view(FP4 if fmt == "mxfp4" else FP8)
    return qb, sb, qt, sb[..., :C, :cap // 32]


def _check(x, offs, fmt, stacked_rows=0):
    """One launch against the reference: bytes inside the written columns, sentinel elsewhere."""
    from ddlb_amd.ops.gemm import kgrouped_capacity
    from ddlb_amd.ops.mx import quantize_mx_t_grouped, quantize_mx_t_grouped_reference

    T, C = x.shape
    E = offs.shape[0] - 1
    R = stacked_rows
    cap = R if R else kgrouped_capacity(T, E, _mod(fmt))
    d = 2 if fmt == "mxfp4" else 1
    qb, sb, qt, st = _views(fmt, (E,) if R else (), C, cap)
    got = quantize_mx_t_grouped(x, offs, fmt=fmt, out=(qt, st), stacked_rows=R)
    assert got[0].data_ptr() == qt.data_ptr() and got[1].data_ptr() == st.data_ptr()
    torch.cuda.synchronize()
    q_ref, s_ref, written = quantize_mx_t_grouped_reference(x, offs, fmt, R)
    wq = written.reshape(written.shape[:-1] + (cap // d, d))[..., 0]    # per data byte
    ws = written.reshape(written.shape[:-1] + (cap // 32, 32))[..., 0]  # per scale byte
    want_q = torch.full_like(qb, SENT)
    want_s = torch.full_like(sb, SENT)
    mq = wq.unsqueeze(-2).expand(q_ref.shape)
    ms = ws.unsqueeze(-2).expand(s_ref.shape)
    want_q[..., :C, :cap // d] = torch.where(mq, q_ref, want_q[..., :C, :cap // d])
    want_s[..., :C, :cap // 32] = torch.where(ms, s_ref, want_s[..., :C, :cap // 32])
    assert torch.equal(sb, want_s), (fmt, x.dtype, C, "scales", int((sb != want_s).sum()))
    assert torch.equal(qb, want_q), (fmt, x.dtype, C, "data", int((qb != want_q).sum()))
    return written


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("fmt", FMTS)
def test_grouped_transposer_matches_reference(fmt, dtype):
    """Every offsets set x C in (8, 72, 128): a single vector column, a ragged second column tile,
    two whole ones. Random finite data over many binades."""
    for name, (counts, o0, tail) in OFFSET_SETS.items():
        o = _offsets(counts, o0)
        T = o[-1] + tail
        offs = torch.tensor(o, dtype=torch.int32, device=DEV)
        for C in (8, 72, 128):
            g = torch.Generator(device=DEV).manual_seed(100 * T + C + len(o))
            v = torch.randn((T, C), generator=g, device=DEV) * \
                torch.exp2(torch.randint(-12, 13, (T, C), generator=g, device=DEV).float())
            x = X.padded(v.to(dtype))
            written = _check(x, offs, fmt)
            k_end = _mod(fmt) * sum(-(-c // _mod(fmt)) for c in counts)
            assert int(written.sum()) == k_end and bool(written[:k_end].all()), name


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("fmt", FMTS)
def test_zero_tail_and_maximal_block(fmt, dtype):
    """A group whose last rows are all zero (its last blocks are all-zero blocks: scale byte 127,
    zero data, like the padding behind them), a block of the dtype's largest finite magnitude,
    and a subnormal-only block."""
    from ddlb_amd.ops.gemm import padded_offsets
    from ddlb_amd.ops.mx import quantize_mx_t_grouped

    mod = _mod(fmt)
    o = [0, 70, 70 + mod + 40, 70 + mod + 40 + 33]
    T, C = o[-1], 72
    g = torch.Generator(device=DEV).manual_seed(5)
    v = torch.randn((T, C), generator=g, device=DEV)
    v[o[1] + 64:o[2]] = 0.0                       # group 1: zero from its row 64 on
    big = torch.finfo(dtype).max
    v[o[2]:o[2] + 32, :8] = big                   # group 2, block 0 of columns 0..7
    v[o[2]:o[2] + 32, 8:16] = -big
    v[0:32, 3] = torch.finfo(dtype).smallest_normal / 4   # group 0: a subnormal-only block
    x = X.padded(v.to(dtype))
    offs = torch.tensor(o, dtype=torch.int32, device=DEV)
    _check(x, offs, fmt)
    qt, st = quantize_mx_t_grouped(x, offs, fmt=fmt)
    k0 = padded_offsets(offs, T, mod)
    zs = st[:, (k0[1] + 64) // 32:k0[2] // 32]
    assert bool((zs == 127).all()), "an all-zero block has the scale byte 127"
    zq = qt.view(torch.uint8)[:, (k0[1] + 64) // (2 if fmt == "mxfp4" else 1):
                              k0[2] // (2 if fmt == "mxfp4" else 1)]
    assert bool((zq == 0).all()), "an all-zero block has zero data"


@pytest.mark.parametrize("fmt", FMTS)
def test_stacked_weights_equal_per_expert_transposer(fmt):
    """``E = 3``, ``N = MOD``, ``K = 72``: one stacked launch over ``w.reshape(E * N, K)`` writes,
    slab by slab and byte for byte, what ``quantize_mx_t(w[g])`` writes."""
    from ddlb_amd.ops.mx import quantize_mx_t, quantize_mx_t_grouped

    E, N, K = 3, _mod(fmt), 72
    g = torch.Generator(device=DEV).manual_seed(11)
    w = (torch.randn((E, N, K), generator=g, device=DEV) * 3).to(torch.bfloat16)
    offs = torch.arange(E + 1, dtype=torch.int32, device=DEV) * N
    _check(w.reshape(E * N, K), offs, fmt, stacked_rows=N)
    qt, st = quantize_mx_t_grouped(w.reshape(E * N, K), offs, fmt=fmt, stacked_rows=N)
    assert tuple(st.shape) == (E, K, N // 32) and qt.shape[:2] == (E, K)
    for e in range(E):
        q1, s1 = quantize_mx_t(w[e], fmt=fmt)
        assert torch.equal(st[e], s1), (fmt, e)
        assert torch.equal(qt[e].view(torch.uint8), q1.view(torch.uint8)), (fmt, e)


@pytest.mark.parametrize("fmt", FMTS)
def test_stacked_group_longer_than_slab_is_cut(fmt):
    """Group 0 has ``2 R`` rows, group 2 none: slab 0 holds the first ``R`` rows of group 0 and
    nothing is written outside it, slab 2 stays sentinel (``_check`` compares whole buffers)."""
    from ddlb_amd.ops.mx import quantize_mx_t

    R = _mod(fmt)
    g = torch.Generator(device=DEV).manual_seed(12)
    x = torch.randn((3 * R, 72), generator=g, device=DEV).to(torch.float16)
    offs = torch.tensor([0, 2 * R, 3 * R, 3 * R], dtype=torch.int32, device=DEV)
    written = _check(x, offs, fmt, stacked_rows=R)
    assert written.sum(dim=1).tolist() == [R, R, 0]
    from ddlb_amd.ops.mx import quantize_mx_t_grouped
    qt, st = quantize_mx_t_grouped(x, offs, fmt=fmt, stacked_rows=R)
    for slab, lo in ((0, 0), (1, 2 * R)):
        q1, s1 = quantize_mx_t(x[lo:lo + R], fmt=fmt)
        assert torch.equal(st[slab], s1) and torch.equal(qt[slab].view(torch.uint8),
                                                         q1.view(torch.uint8))


def test_garbage_offsets_stay_inside():
    """Negative, decreasing and huge offsets complete and touch nothing outside the outputs."""
    T, C = 300, 72
    g = torch.Generator(device=DEV).manual_seed(13)
    x = X.padded(torch.randn((T, C), generator=g, device=DEV).to(torch.bfloat16))
    for raw in ([-5, 200, 100, 2 ** 31 - 1], [2 ** 31 - 1, -2 ** 31, 7, 7], [-9, -9, -9, -1]):
        offs = torch.tensor(raw, dtype=torch.int32, device=DEV)
        for fmt in FMTS:
            _check(x, offs, fmt)


def test_refusals_on_cpu_tensors():
    from ddlb_amd.ops.mx import quantize_mx_t_grouped

    x = torch.zeros((300, 72), dtype=torch.bfloat16)
    o = torch.tensor([0, 100, 300], dtype=torch.int32)
    bad = [
        (dict(x=x.double()), TypeError), (dict(x=x[0]), ValueError),
        (dict(x=torch.zeros((300, 4), dtype=torch.bfloat16)), ValueError),  # 8-byte rows
        (dict(x=x[:, ::2]), ValueError),
        (dict(offsets=o.long()), TypeError), (dict(offsets=o[:1]), ValueError),
        (dict(offsets=o.reshape(1, 3)), ValueError), (dict(offsets=[0, 100, 300]), TypeError),
        (dict(offsets=torch.zeros(1026, dtype=torch.int32)), ValueError),
        (dict(fmt="fp8"), ValueError), (dict(stacked_rows=100), ValueError),
        (dict(stacked_rows=-128), ValueError), (dict(fmt="mxfp4", stacked_rows=128), ValueError),
        (dict(out=(torch.zeros((72, 512), dtype=torch.uint8),
                   torch.zeros((72, 16), dtype=torch.uint8))), TypeError),      # data dtype
        (dict(out=(torch.zeros((72, 384), dtype=FP8),
                   torch.zeros((72, 16), dtype=torch.uint8))), ValueError),     # below capacity
        (dict(out=(torch.zeros((72, 512), dtype=FP8),
                   torch.zeros((72, 12), dtype=torch.uint8))), ValueError),
        (dict(out=(torch.zeros((72, 520), dtype=FP8)[:, :512],
                   torch.zeros((72, 16), dtype=torch.uint8))), ValueError),     # pitch off 16
        (dict(out=(torch.zeros((72, 512), dtype=FP8),
                   torch.zeros((72, 18), dtype=torch.uint8)[:, :16])), ValueError),  # pitch off 4
        (dict(out=torch.zeros((72, 512), dtype=FP8)), TypeError),
    ]
    for kw, exc in bad:
        args = dict(x=x, offsets=o, fmt="mx")
        args.update(kw)
        with pytest.raises(exc):
            quantize_mx_t_grouped(args.pop("x"), args.pop("offsets"), **args)
    # a CPU tensor that passes every other check reaches the device refusal
    with pytest.raises(ValueError, match="ROCm device"):
        quantize_mx_t_grouped(x, o)
