"""The references of the exact-arithmetic GPU tests (``tests/_exact.py``) hold the conditions
those tests rely on. Everything here runs on the CPU."""

import torch

import _exact as X
from _exact import (FP8, POISON, SENTINEL, dequant64, exact, exact64, exact_scaled,
                    extreme_scales, ints, padded, pow2_f64, sentinel_out, untouched)

from _exact_plan import (assert_exact, block_layout, gather, ksplit_operands, ksplit_specs,
                         only_written, padded_ld, scatter)

import pytest


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def test_ints_are_exact_in_every_dtype():
    x = ints((64, 64), torch.float64, _gen(1))
    assert set(x.unique().tolist()) == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0}
    for dt in (torch.bfloat16, torch.float16, torch.float32, FP8):
        assert torch.equal(x.to(torch.float32).to(dt).to(torch.float64), x)


def test_pow2_f64_is_the_power_of_two():
    e = torch.arange(-1022, 1024)
    p = pow2_f64(e)
    assert torch.equal(p, torch.tensor([2.0 ** int(k) for k in e], dtype=torch.float64))


def test_exact_scaled_equals_the_integer_model():
    """The extreme-scale case of the GPU test: bytes 0..254, net exponents -4..4, and the fp64
    product equal to per-block int64 dot products shifted by e_a + e_w; an exact f32."""
    M, N, K = 300, 202, 512
    g = _gen(2)
    a8, w8 = ints((M, K), FP8, g), ints((N, K), FP8, g)
    s_a, s_w, e_a, e_w = extreme_scales(M, N, K, g)
    for s in (s_a, s_w):
        assert int(s.min()) == 0 and int(s.max()) == 254
    net = e_a.unsqueeze(1) + e_w.unsqueeze(0)                       # [M, N, nb]
    assert int(net.min()) >= -4 and int(net.max()) <= 4
    ai = a8.float().to(torch.int64).reshape(M, K // 32, 32)
    wi = w8.float().to(torch.int64).reshape(N, K // 32, 32)
    dots = torch.einsum("mbk,nbk->mnb", ai, wi)                     # int64, exact
    model16 = (dots << (net + 4)).sum(dim=2)                        # 16 x the product
    got = exact_scaled(a8, w8, s_a, s_w)
    assert torch.equal(got * 16.0, model16.double())
    assert torch.equal(got.float().double(), got)                   # an exact f32
    assert float(got.abs().max()) < 2.0 ** 24 / 16


def test_dequant64_against_dequantize_mx():
    """Equal wherever the fp32 specification is finite; it overflows exactly at s = 254 with
    |q| >= 2, where the fp64 value (and a product with a small partner scale) is finite."""
    from ddlb_amd.ops.mx import dequantize_mx

    g = _gen(3)
    q = ints((64, 256), FP8, g)
    q[0, :8] = torch.tensor([1.0, 1.5, 1.75, 2.0, -2.0, 448.0, -1.0, 0.0]).to(FP8)
    s = torch.randint(0, 255, (64, 8), generator=g).to(torch.uint8)
    s[0, 0], s[1, 0], s[2, 0] = 254, 0, 254
    d32, d64 = dequantize_mx(q, s), dequant64(q, s)
    finite = torch.isfinite(d32)
    assert torch.equal(d32[finite].double(), d64[finite])
    over = (s.repeat_interleave(32, dim=1) == 254) & (q.float().abs() >= 2)
    assert torch.equal(~finite, over) and int(over.sum()) > 3
    assert bool(torch.isfinite(d64).all())


def _decode_e4m3(code):
    s, e, m = code >> 7, (code >> 3) & 0xF, code & 7
    if e == 0xF and m == 7:
        return float("nan")
    v = (m / 8.0) * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
    return -v if s else v


def test_every_e4m3_code():
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    vals = codes.view(FP8).float()
    assert int(torch.isfinite(vals).sum()) == 254
    assert bool(torch.isnan(vals[0x7F])) and bool(torch.isnan(vals[0xFF]))
    assert float(vals[0x80]) == 0.0 and bool(torch.signbit(vals[0x80]))
    assert float(vals[0x00]) == 0.0 and not bool(torch.signbit(vals[0x00]))
    assert float(vals[0x01]) == 2.0 ** -9 and float(vals[0x7E]) == 448.0
    model = torch.tensor([_decode_e4m3(c) for c in range(256)], dtype=torch.float32)
    keep = torch.isfinite(vals)
    assert torch.equal(vals[keep].view(torch.int32), model[keep].view(torch.int32))


def test_exact_rounds_to_the_output_dtype():
    """bf16 holds integers up to 256: at K = 1024 (sums of some hundreds) the rounding to the
    output dtype is really exercised; at the sweep's K of one to four K-tiles it rarely is, and
    what the sweep pins down there is the placement of every element."""
    g = _gen(4)
    a, w = ints((64, 1024), torch.bfloat16, g), ints((48, 1024), torch.bfloat16, g)
    f32 = exact(a, w, torch.float32)
    assert torch.equal(f32.double(), exact64(a, w))                 # nothing lost in f32
    bf = exact(a, w, torch.bfloat16)
    assert bf.dtype == torch.bfloat16
    assert int((bf.float() != f32).sum()) > 0                       # the rounding is exercised
    assert bool(((bf.float() - f32).abs() <= f32.abs() * 2.0 ** -8).all())
    assert torch.equal(exact(a, w, torch.float16).float(), f32)     # |sum| <= 2048: exact in f16


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32, FP8,
                                   torch.float64])
def test_padded_views(dtype):
    g = _gen(5)
    for cols in (128, 100, 256):
        x = ints((7, cols), dtype, g)
        v = padded(x)
        assert tuple(v.shape) == (7, cols) and v.stride(1) == 1 and v.stride(0) > cols
        assert v.data_ptr() % 16 == 0 and (v.stride(0) * v.element_size()) % 16 == 0
        assert torch.equal(v.float(), x.float())
        whole = torch.as_strided(v, (10, v.stride(0)), (v.stride(0), 1)).to(torch.float64)
        assert bool((whole[:7, cols:] == POISON).all()) and bool((whole[7:] == POISON).all())


def test_untouched_sees_a_planted_write():
    for dtype in (torch.bfloat16, torch.float32):
        buf, view = sentinel_out(5, 6, dtype, device="cpu")
        assert tuple(buf.shape) == (8, 10) and tuple(view.shape) == (5, 6)
        assert bool((buf.float() == SENTINEL).all())
        view.fill_(1.0)
        untouched(buf, 5, 6)
        for r, c in ((0, 6), (4, 9), (5, 0), (7, 9)):
            buf2 = buf.clone()
            buf2[r, c] = 1.0
            with pytest.raises(AssertionError):
                untouched(buf2, 5, 6)
    buf, _ = sentinel_out(8, 4, torch.float32, extra_rows=0, device="cpu")
    rows = torch.tensor([0, 1, 4, 5])
    buf[rows, :4] = 2.0
    untouched(buf, 8, 4, rows=rows)
    buf[2, 1] = 2.0
    with pytest.raises(AssertionError):
        untouched(buf, 8, 4, rows=rows)


# ------------------------------------------------------------------ tests/_exact_plan.py
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, FP8])
@pytest.mark.parametrize("M,shard_rows,nblocks", [(1024, 256, 4), (768, 256, 4), (960, 192, 5),
                                                  (1000, 250, 4), (1000, 256, 4), (64, 64, 1)])
def test_block_table_gather_inverts_scatter(dtype, M, shard_rows, nblocks):
    """The table builder followed by the gather is the identity; the blocks come in a permuted
    order over both buffers, and every row that is no block row holds poison, as does the
    padding of every row and the unused tail of a part-used block."""
    K = 128
    a = ints((M, K), dtype, _gen(6))
    lay = block_layout(nblocks, shard_rows)
    ld = padded_ld(K, dtype)
    assert ld > K and (ld * a.element_size()) % 16 == 0
    bufs = scatter(a, lay, ld)
    assert torch.equal(gather(bufs, lay, M, K).float(), a.float())
    assert len(set(lay.where)) == nblocks
    if nblocks > 1:
        assert {b for b, _ in lay.where} == {0, 1}
        order = sorted(range(nblocks), key=lambda b: lay.where[b])
        assert order != list(range(nblocks))
    live = [torch.zeros((r, ld), dtype=torch.bool) for r in lay.buf_rows]
    for b, (buf, row0) in enumerate(lay.where):
        n = max(0, min(M, (b + 1) * shard_rows) - b * shard_rows)
        live[buf][row0:row0 + n, :K] = True
        # poison really lies in front of and behind every block
        assert bool((bufs[buf][row0 - lay.gap:row0].float() == POISON).all())
        end = row0 + shard_rows
        assert bool((bufs[buf][end:end + lay.gap].float() == POISON).all())
        assert end + lay.gap <= lay.buf_rows[buf]
    for buf in (0, 1):
        assert bool((bufs[buf].float()[~live[buf]] == POISON).all())
        assert int(live[buf].sum()) == int((bufs[buf].float()[live[buf]] != POISON).sum())


def test_only_written_sees_a_stray_element_and_a_missing_region():
    def outputs():
        bufs = {"c": torch.full((12, 10), SENTINEL, dtype=torch.bfloat16),
                "slot": torch.full((7, 6), SENTINEL, dtype=torch.float32)}
        bufs["c"][2:6, :8] = 1.0
        bufs["c"][6:10, :8] = 2.0
        bufs["slot"][torch.tensor([0, 1, 3]), :4] = 3.0
        return bufs

    regions = [("c", slice(2, 6), 8), ("c", slice(6, 10), 8), ("slot", torch.tensor([0, 1, 3]), 4)]
    only_written(outputs(), regions)
    for name, r, c in (("c", 0, 0), ("c", 1, 7), ("c", 5, 8), ("c", 10, 0), ("c", 11, 9),
                       ("slot", 2, 0), ("slot", 0, 4), ("slot", 6, 5)):
        bufs = outputs()
        bufs[name][r, c] = 1.0                                      # a single stray element
        with pytest.raises(AssertionError, match=f"{name}: 1"):
            only_written(bufs, regions)
    for skip in range(len(regions)):                                # a single missing region
        with pytest.raises(AssertionError):
            only_written(outputs(), regions[:skip] + regions[skip + 1:])
    with pytest.raises(AssertionError, match="c: 64, slot: 12"):
        only_written(outputs(), [])


def test_assert_exact():
    assert_exact(1024)
    assert_exact((2 ** 24 - 1) // 9)
    with pytest.raises(AssertionError):
        assert_exact(2 ** 24 // 9 + 1)


@pytest.mark.parametrize("M", [256, 512])
def test_ksplit_specifications_differ(M):
    """The two specifications of the public K-split (``ksplit_specs``: f32 partials rounded once;
    output-dtype partials summed and rounded again) on the operands the GPU test uses, N = 256,
    K = 1024. bf16 holds the integers up to 256: about 4.6 % of the products are larger, so the
    single rounding is exercised, and with S = 2 (slice sums of standard deviation 90, 0.45 %
    beyond 256) the specifications differ in hundreds of elements: 226 at M = 256, 422 at
    M = 512. With S = 4 a slice sum has standard deviation 64 and passes 256 with probability
    6e-5, so only a handful of partials are rounded at all (3 and 13 elements differ: no seed
    reaches 100 there); f16 holds every integer up to 2048 and the products stay below 600, so
    in f16 the specifications coincide."""
    N, K = 256, 1024
    a, w = ksplit_operands(M, N, K, torch.bfloat16)
    f32 = exact(a, w, torch.float32)
    assert float(((f32.abs() > 256).float().mean())) > 0.04
    assert float(f32.abs().max()) < 2048
    once, twice = ksplit_specs(a, w, 2, torch.bfloat16)
    assert int((once != twice).sum()) > 100
    once4, twice4 = ksplit_specs(a, w, 4, torch.bfloat16)
    assert torch.equal(once4, once) and int((once4 != twice4).sum()) > 0
    a16, w16 = ksplit_operands(M, N, K, torch.float16)
    assert torch.equal(a16.float(), a.float())
    for S in (2, 4):
        o16, t16 = ksplit_specs(a16, w16, S, torch.float16)
        assert torch.equal(o16, t16) and torch.equal(o16.float(), f32)
        o32, t32 = ksplit_specs(a16.float(), w16.float(), S, torch.float32)
        assert torch.equal(o32, t32) and torch.equal(o32, f32)


# ------------------------------------------------------------------ far views and the gates
SMALL_GUARD, SMALL_LD = 4096, 1024
FAR_DTYPES = [torch.bfloat16, torch.float32, FP8, torch.uint8]


def _small_backing(R):
    return X.far_backing(X.far_span(R, SMALL_LD, SMALL_LD), guard=SMALL_GUARD, device="cpu")


@pytest.mark.parametrize("dtype", FAR_DTYPES)
def test_far_view_places_rows_and_poisons_the_rest(dtype):
    R, C = 9, 40
    x = ints((R, C), torch.float32, _gen(7)).to(dtype)
    backing = _small_backing(R + 2)
    assert backing.dtype == torch.uint8 and backing.numel() == SMALL_GUARD + (R + 2) * SMALL_LD
    esz = x.element_size()
    for row0 in (0, 2):
        v = X.far_view(backing, x, SMALL_LD, row0=row0)
        assert tuple(v.shape) == (R, C) and v.stride() == (SMALL_LD // esz, 1)
        assert v.data_ptr() == backing.data_ptr() + SMALL_GUARD + row0 * SMALL_LD
        assert v.data_ptr() % 16 == 0
        assert torch.equal(v.view(torch.uint8), x.view(torch.uint8))
        # everything else, the guard included, holds POISON in the view's dtype
        typed = backing.view(dtype).clone()
        poison = torch.tensor([POISON]).to(dtype)
        rows = typed[SMALL_GUARD // esz:].view(R + 2, SMALL_LD // esz)
        rows[row0:row0 + R, :C] = poison
        assert bool((typed.view(torch.uint8) == poison.view(torch.uint8)[0]).all()
                    if esz == 1 else (typed.float() == POISON).all())
    with pytest.raises(AssertionError):
        X.far_view(backing, x, SMALL_LD, row0=3)                    # past the backing's end
    with pytest.raises(AssertionError):
        X.far_view(backing, x, C * esz - esz)                       # overlapping rows


@pytest.mark.parametrize("dtype", FAR_DTYPES)
def test_untouched_far_sees_a_misplaced_write(dtype):
    """A write inside a row's padding, in the guard and one row early, one element each."""
    R, C = 6, 24
    esz = torch.empty((), dtype=dtype).element_size()
    backing = _small_backing(R + 3)
    view = X.far_out(backing, R, C, dtype, SMALL_LD, row0=1)
    word = X.fill_word(SENTINEL, dtype)
    assert bool((backing.view(torch.int64) == word).all())
    if dtype != torch.uint8:
        assert bool((backing.view(dtype).float() == SENTINEL).all())
    result = ints((R, C), torch.float32, _gen(8)).to(dtype)
    view.copy_(result)
    X.untouched_far(backing, view)
    assert torch.equal(view.view(torch.uint8), result.view(torch.uint8))  # put back as it was
    base = (SMALL_GUARD + SMALL_LD) // esz
    typed = backing.view(dtype)
    one = torch.tensor([1.0]).to(dtype)
    for name, at in (("row padding", base + C), ("row padding", base + 2 * SMALL_LD // esz - 1),
                     ("guard", 0), ("guard", SMALL_GUARD // esz - 1),
                     ("one row early", base - SMALL_LD // esz),
                     ("behind the last row", base + R * SMALL_LD // esz)):
        was = typed[at].clone()
        typed[at] = one[0]
        with pytest.raises(AssertionError, match="outside the view"):
            X.untouched_far(backing, view)
        typed[at] = was
        X.untouched_far(backing, view)
    # physical rows: the rows between the written ones must hold the sentinel
    rows = torch.tensor([0, 1, 4, 5])
    X.far_fill(backing, SENTINEL, dtype)
    view[rows] = result[rows]
    X.untouched_far(backing, view, rows=rows)
    view[2, 3] = one[0]
    with pytest.raises(AssertionError):
        X.untouched_far(backing, view, rows=rows)
    # two views of one backing (the K-split's partials)
    X.far_fill(backing, SENTINEL, dtype)
    v0 = X.far_out(backing, 3, C, dtype, SMALL_LD, fill=None)
    v1 = X.far_out(backing, 3, C, dtype, SMALL_LD, row0=3, fill=None)
    v0.copy_(result[:3])
    v1.copy_(result[3:])
    X.untouched_far(backing, v0, v1)
    with pytest.raises(AssertionError):
        X.untouched_far(backing, v0)


def test_an_aliased_operand_row_changes_the_product():
    """Rows pairwise distinct: a kernel that reads row j where row i belongs computes another
    product, and one that reads the padding reads POISON."""
    M, N, K = 9, 7, 64
    a, w = X.far_operands(M, N, K, torch.bfloat16)
    X.rows_distinct(a, SMALL_LD)
    backing = _small_backing(M)
    A = X.far_view(backing, a, SMALL_LD)
    ref = exact(A, w, torch.float32)
    assert torch.equal(ref, exact(a, w, torch.float32))
    for i, j in ((5, 1), (0, 8)):
        alias = A.clone()
        alias[i] = A[j]
        got = exact(alias, w, torch.float32)
        assert not torch.equal(got[i], ref[i]) and torch.equal(got[i], ref[j])
    pad = torch.as_strided(A, (M, K), A.stride(), A.storage_offset() + K)   # a row's padding
    assert bool((pad.float() == POISON).all())
    assert not torch.equal(exact(pad, w, torch.float32), ref)
    same = a.clone()
    same[3] = same[6]
    with pytest.raises(AssertionError, match="equal"):
        X.rows_distinct(same, SMALL_LD)
    with pytest.raises(AssertionError):       # 2^31 behind row 0 lies inside row 4
        X.rows_distinct(a, (2 ** 31 - 32) // 4)


@pytest.mark.parametrize("din", [torch.bfloat16, FP8, torch.float32])
def test_far_operand_rows_are_distinct_at_the_pitches_used(din):
    """The operands of every far GEMM case, at the pitch the case places them on."""
    k = 2 * 128 // torch.empty((), dtype=din).element_size()
    for (M, N), pitch in ((X.FAR_TILED, X.FAR_PITCH), (X.FAR_PING, X.FAR_PITCH),
                          (X.FAR_PT4, X.PT4_LD_BYTES), (X.GATE_C, X.PT4_LD_BYTES + 16)):
        for rows, cols in ((M, N), (N, M)):                          # W far swaps M and N
            a, w = X.far_operands(rows, cols, k, din)
            X.rows_distinct(a, pitch)
            X.rows_distinct(w, pitch)
            assert (rows - 1) * pitch > 2 ** 32 or rows < 300 or pitch < X.FAR_PITCH
    assert 127 * X.FAR_PITCH < 2 ** 31 <= 128 * X.FAR_PITCH
    assert 255 * X.FAR_PITCH < 2 ** 32 <= 256 * X.FAR_PITCH
    assert 1024 * X.PT4_LD_BYTES == 2 ** 32 and X.FAR_PT4[0] // 256 == 5


def test_gate_ld_straddles_every_gate():
    """``gate_ld`` on the Python copies of gates 1, 3 and 4, for the shapes the GPU tests use: the
    two leading dimensions lie one aligned step apart on either side of the gate, and the byte
    counts are where the kernels' 32-bit offsets end."""
    assert X.gate_ld(lambda v: v <= 100, 8) == (96, 104)
    assert X.gate_ld(lambda v: v < 96, 8) == (88, 96)
    M, N = X.GATE_C
    for osz in (2, 4):                                               # gate 1: bf16 and f32 C
        al = X.align_of(8, osz)
        last, nxt = X.gate_ld(lambda ld: X.c_fits_wt(M, N, ld, osz), al)
        assert nxt == last + al and last % al == 0 and last > N
        assert X.c_fits_wt(M, N, last, osz) and not X.c_fits_wt(M, N, nxt, osz)
        assert ((M - 1) * last + N) * osz < X.WT_LIMIT <= ((M - 1) * nxt + N) * osz
        assert ((M - 1) * nxt + N) * osz < X.WT_LIMIT + (M - 1) * 8
    # grouped C rows count the skipped rows
    assert X.c_fits_wt(768, 256, 1024, 2, 256, 2 ** 18) and \
        not X.c_fits_wt(768, 256, 1024, 2, 256, 2 ** 19)
    assert not X.c_fits_wt(0, 256, 8, 2)
    S, (M, N) = 2, X.GATE_KSPLIT                                     # gate 3: f32 partials
    last, nxt = X.gate_ld(lambda ld: X.ksplit_one_launch(S, M, ld, 4), 2)
    assert nxt == last + 2 and last > N
    assert S * M * last * 4 < X.WT_LIMIT <= S * M * nxt * 4
    assert X.c_fits_wt(M, N, nxt, 4)        # the slice loop's launches are write-through ones
    rows = X.GATE_SCALED[0]                                          # gate 4: fp8 and fp4 scales
    for al in (4, 8):
        last, nxt = X.gate_ld(lambda ld: X.scale_rows_ok(rows, ld), al)
        assert nxt == last + al and rows * last < 2 ** 31 <= rows * nxt
    assert X.pt4_ld_ok(X.PT4_LD_BYTES // 2, 2) and not X.pt4_ld_ok(X.PT4_LD_BYTES // 2 + 8, 2)
    assert X.gate_ld(lambda ld: X.pt4_ld_ok(ld, 4), 4) == (2 ** 20, 2 ** 20 + 4)


def test_fill_word():
    assert X.fill_word(SENTINEL, torch.uint8) == -0x0606060606060607        # bytes 0xF9
    assert X.fill_word(POISON, torch.uint8) == 0x0505050505050505
    assert X.fill_word(SENTINEL, torch.float32) == int.from_bytes(
        torch.tensor([SENTINEL, SENTINEL]).view(torch.uint8).numpy().tobytes(), "little",
        signed=True)
    for dtype in (torch.bfloat16, torch.float16, FP8, torch.float32, torch.float64):
        w = torch.tensor([X.fill_word(POISON, dtype)], dtype=torch.int64).view(dtype)
        assert bool((w.to(torch.float64) == POISON).all())


# ---------------------------------------------------------------------------- non-finite values
def _loop_classes(a, w):
    """The class rule as a Python triple loop over floats: every product is formed and classified
    by itself, nothing non-finite is ever added."""
    import math

    A, W = a.to(torch.float32).tolist(), w.to(torch.float32).tolist()
    out = []
    for ra in A:
        row = []
        for rw in W:
            nan = pos = neg = False
            total = 0.0
            for x, y in zip(ra, rw):
                if math.isnan(x) or math.isnan(y) or (math.isinf(x) and y == 0) \
                        or (math.isinf(y) and x == 0):
                    nan = True
                elif math.isinf(x) or math.isinf(y):
                    if (x > 0) == (y > 0):
                        pos = True
                    else:
                        neg = True
                else:
                    total += x * y
            row.append(float("nan") if nan or (pos and neg) else float("inf") if pos
                       else float("-inf") if neg else total)
        out.append(row)
    return torch.tensor(out, dtype=torch.float64)


def test_classes64_against_loops_and_fp64_matmul():
    nan, inf = float("nan"), float("inf")
    g = _gen(41)
    a, w = ints((7, 32), torch.float32, g), ints((5, 32), torch.float32, g)
    a[0, 0] = nan
    a[1, 31] = inf
    a[2, 3], a[2, 30] = inf, -inf
    a[3, 4] = -inf
    a[4, 8], w[1, 8] = inf, -inf               # Inf x Inf
    w[2, 16] = nan
    w[4, 0] = -inf
    w[0, 31], w[1, 31], w[3, 31] = -1.0, 0.0, 2.0
    a[5, 0], a[6, 0] = 0.0, 2.0
    got = X.classes64(a, w)
    X.same(got, _loop_classes(a, w))
    X.same(got, a.double() @ w.double().t())   # IEEE fp64 arithmetic has the same classes
    assert bool(torch.isnan(got[0]).all()) and bool(torch.isnan(got[:, 2]).all())
    assert bool((got == inf).any()) and bool((got == -inf).any())
    assert bool(torch.isfinite(got).any())
    fin = torch.isfinite(got)
    assert torch.equal(got[fin], exact64(torch.nan_to_num(a, 0, 0, 0), torch.nan_to_num(w, 0, 0, 0))[fin])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32, torch.float64,
                                   FP8])
def test_planted_puts_every_class_where_it_says(dtype):
    M, N, K = 70, 11, 64
    g = _gen(42)
    a0, w0 = ints((M, K), dtype, g), ints((N, K), dtype, g)
    a, w, p = X.planted(a0, w0)
    assert p["r0"] < 128 and p["r1"] == M - 1 and p["n1"] == N - 1
    assert len({p["r0"], p["r1"], p["r2"]}) == 3 and p["n0"] != p["n1"]
    ref = X.classes64(a, w)
    X.same(ref, _loop_classes(a, w))
    assert bool(torch.isnan(ref[p["r0"]]).all()) and bool(torch.isnan(ref[:, p["n0"]]).all())
    if dtype == FP8:                           # NaN bytes only: 0x7F in A, 0xFF in W
        assert int(a.view(torch.uint8)[p["r0"], 0]) == 0x7F
        assert int(w.view(torch.uint8)[p["n0"], K // 2]) == 0xFF
        assert int((~torch.isfinite(ref)).sum()) == M + N - 1
        return
    inf = float("inf")
    for line in (ref[p["r1"]], ref[p["r2"]], ref[:, p["n1"]]):
        assert bool(torch.isnan(line).any())
    for line in (ref[p["r1"]], ref[:, p["n1"]]):
        assert bool((line == inf).any()) and bool((line == -inf).any())
    clean = torch.ones((M, N), dtype=torch.bool)
    clean[[p["r0"], p["r1"], p["r2"]]] = False
    clean[:, [p["n0"], p["n1"]]] = False
    assert bool(torch.isfinite(ref[clean]).all())


def test_same_tells_classes_and_values_apart():
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([[1.0, nan, inf, -inf, 0.0]])
    X.same(x, x.clone())
    for i, v in ((0, 2.0), (1, 0.0), (2, -inf), (3, nan), (2, 3.4e38), (4, nan)):
        y = x.clone()
        y[0, i] = v
        with pytest.raises(AssertionError):
            X.same(y, x)


def test_nan_padded_fills_with_the_nonfinite_poison():
    def whole(v):  # the [R + 3, ld] buffer behind the view
        return torch.as_strided(v, (v.shape[0] + 3, v.stride(0)), (v.stride(0), 1), 0)

    g = _gen(43)
    for dt in (torch.bfloat16, torch.float16, torch.float32, torch.float64):
        x = ints((5, 12), dt, g)
        v = X.nan_padded(x)
        assert torch.equal(v, x) and v.stride(0) > 12
        assert int(torch.isnan(whole(v)).sum()) == 8 * v.stride(0) - 5 * 12
    x = ints((5, 16), FP8, g)
    v = X.nan_padded(x)
    assert v.dtype == FP8 and torch.equal(v.view(torch.uint8), x.view(torch.uint8))
    assert int((whole(v.view(torch.uint8)) == 0x7F).sum()) == 8 * v.stride(0) - 80
    s = X.nan_padded(torch.full((5, 16), 127, dtype=torch.uint8), "scale")
    assert int((whole(s) == 255).sum()) == 8 * s.stride(0) - 80
    q = X.nan_padded(torch.zeros((5, 16), dtype=torch.uint8), "fp4")
    assert int((whole(q) == 0x77).sum()) == 8 * q.stride(0) - 80
