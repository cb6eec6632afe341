"""Every e4m3 byte and every E2M1 code through the skinny, A16 and tiled W4A8 GEMMs, and the A16
kernel's documented exact range pair by pair.

The code cases are ``_check_codes``' idea (``tests/test_gemm_exact_gpu.py``): row ``r`` of one
operand holds code ``r`` at one K position (``tests/_exact.py`` ``code_case``: position ``r mod 32``
of a block that changes from row to row; E2M1 in the low and in the high nibble beside a different
non-zero code), the other operand is the identity partner (1.0 at that position under unit
scales), and the f32 output must be ``decode(code) * 2^(s - 127)``, compared as int32 bits with
the fp64 product of the table-decoded operands. The rows' scale bytes run over 125..129 and
differ between neighbouring blocks. The one -0 code is compared by value. NaN bytes are left to the
non-finite tests. ``tests/test_exact_refs_cpu.py`` shows that a nibble swap or a scale byte taken
from the neighbouring block changes these references.

The range test takes ``gemm_skinny_a16``'s contract literally: every (code, scale byte) pair for
which ``decode(code) * 2^(s - 127)`` is zero or a normal number of the activation dtype
(``a16_range_mask``) comes out as exactly that number."""

import functools

import pytest
import torch

import _exact as X
from _exact import FP8, sentinel_out, untouched
from ddlb_amd.ops import gemm as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
FP4 = torch.float4_e2m1fn_x2
BF16, F16, F32, U8 = torch.bfloat16, torch.float16, torch.float32, torch.uint8
K = X.CODE_K
dtypes = pytest.mark.parametrize("dt", (BF16, F16), ids=("bf16", "f16"))


@functools.lru_cache(maxsize=None)
def _codes(fmt):
    """``(data, s, decoded fp64, partner fp64, -0 rows)`` of ``code_case(fmt)``, on the CPU."""
    data, s, pos, neg0 = X.code_case(fmt)
    return data, s, X.decode64(data, s, fmt), X.one_hot(pos, K), neg0


def _stored(data, fmt):
    return data.to(DEV).view(FP4 if fmt == "e2m1" else FP8)


def _partner(p64, form):
    """The identity partner as an operand: e4m3, E2M1 (1.0 is code 2) or a 16-bit dtype."""
    if form == "e2m1":
        return X.pack_nibbles((p64 * 2).long()).to(DEV).view(FP4)
    return p64.to(F32).to(FP8 if form == "e4m3" else form).to(DEV)


def _unit(rows):
    return torch.full((rows, K // 32), 127, dtype=U8, device=DEV)


def _check(out, want64, neg0, codes_are_rows):
    """``out`` against ``want64``: bits, the diagonal's -0 element by value."""
    mask = torch.zeros(want64.shape, dtype=torch.bool)
    idx = neg0.nonzero().flatten()
    mask[idx, idx] = True
    assert int(mask.sum()) == int(neg0.sum()) >= 1
    assert bool((want64[mask] == 0).all())
    X.same_bits(out.cpu(), want64 + 0.0, mask if codes_are_rows else mask.t())


def _as_a(fmt, pform, run, slab=None):
    """The codes as ``a`` (in slabs of ``slab`` rows), the partner as ``w``."""
    data, s, dec, p64, neg0 = _codes(fmt)
    R = data.shape[0]
    a, s_a, w = _stored(data, fmt), s.to(DEV), _partner(p64, pform)
    want = dec @ p64.t()
    got = torch.empty((R, R), dtype=F32)
    for r0 in range(0, R, slab or R):
        r = slice(r0, min(R, r0 + (slab or R)))
        buf, out = sentinel_out(r.stop - r0, R, F32)
        run(a[r], w, out, s_a[r], _unit(R))
        untouched(buf, r.stop - r0, R)
        got[r] = out.cpu()
    _check(got, want, neg0, True)


def _as_w(fmt, pform, run, slab=None):
    """The codes as ``w``, the partner's rows (in slabs) as ``a``."""
    data, s, dec, p64, neg0 = _codes(fmt)
    R = data.shape[0]
    w, s_w, a = _stored(data, fmt), s.to(DEV), _partner(p64, pform)
    want = p64 @ dec.t()
    got = torch.empty((R, R), dtype=F32)
    for r0 in range(0, R, slab or R):
        r = slice(r0, min(R, r0 + (slab or R)))
        buf, out = sentinel_out(r.stop - r0, R, F32)
        run(a[r], w, out, _unit(r.stop - r0), s_w)
        untouched(buf, r.stop - r0, R)
        got[r] = out.cpu()
    _check(got, want, neg0, False)


def _skinny(ks):
    return lambda a, w, out, s_a, s_w: G.gemm_skinny(a, w, out, a_scale=s_a, w_scale=s_w,
                                                     ksplit=ks)


def _a16(ks):
    return lambda a, w, out, s_a, s_w: G.gemm_skinny_a16(a, w, out, w_scale=s_w, ksplit=ks)


def _w4a8(tile):
    return lambda a, w, out, s_a, s_w: G.gemm_w4a8(a, w, out, a_scale=s_a, w_scale=s_w, tile=tile)


# ---------------------------------------------------------------------------- e4m3: 254 bytes
@pytest.mark.parametrize("partner", ["e4m3", "e2m1"], ids=["mx", "w4a8"])
def test_e4m3_as_a_of_skinny(partner):
    _as_a("e4m3", partner, _skinny(1), slab=64)


@pytest.mark.parametrize("tile", G.W4A8_TILES)
def test_e4m3_as_a_of_w4a8(tile):
    _as_a("e4m3", "e2m1", _w4a8(tile))


def test_e4m3_as_w_of_skinny():
    _as_w("e4m3", "e4m3", _skinny(2), slab=64)


@dtypes
def test_e4m3_as_w_of_skinny_a16(dt):
    _as_w("e4m3", dt, _a16(1), slab=64)


# ---------------------------------------------------------------------------- E2M1: 16 codes x 2
@pytest.mark.parametrize("partner", ["e2m1", "e4m3"], ids=["mxfp4", "w4a8"])
def test_e2m1_as_w_of_skinny(partner):
    _as_w("e2m1", partner, _skinny(1))


@pytest.mark.parametrize("tile", G.W4A8_TILES)
def test_e2m1_as_w_of_w4a8(tile):
    _as_w("e2m1", "e4m3", _w4a8(tile))


@dtypes
def test_e2m1_as_w_of_skinny_a16(dt):
    _as_w("e2m1", dt, _a16(1))


def test_e2m1_as_a_of_skinny():
    _as_a("e2m1", "e2m1", _skinny(1))


# ---------------------------------------------------------------------------- the A16 range
@dtypes
@pytest.mark.parametrize("wfmt", ["mx", "mxfp4"])
def test_a16_exact_over_the_documented_range(wfmt, dt):
    """Every (code, scale byte 1..254) pair whose value is zero or a normal number of ``dt``: one
    launch, 64 blocks per weight row, ``a`` one-hot over block ``m`` in row ``m``, so the f32
    output ``[m, n]`` is the single dequantised weight of pair ``64 n + m``, bit for bit (a -0
    weight: +0, its sum with the +0 products of the row). Measured on an MI355X: every pair of all
    four sets is exact."""
    mask = X.a16_range_mask(wfmt, dt)
    pairs = mask.nonzero()
    data, s, want, used = X.a16_range_case(wfmt, pairs)
    N, B = s.shape
    a = torch.zeros((B, B * 32), dtype=dt)
    for m in range(B):
        a[m, 32 * m:32 * m + 32] = 1.0
    buf, out = sentinel_out(B, N, F32)
    G.gemm_skinny_a16(a.to(DEV), data.to(DEV).view(FP4 if wfmt == "mxfp4" else FP8), out,
                      w_scale=s.to(DEV), ksplit=1)
    untouched(buf, B, N)
    got = out.cpu()
    print(f"{wfmt} {dt}: {pairs.shape[0]} pairs in range, "
          f"{int((got.double() != want)[used].sum())} not exact")
    assert int(used.sum()) == pairs.shape[0] == int(mask.sum())
    X.same_bits(got, want + 0.0)
    assert bool((want[~used] == 0).all())
