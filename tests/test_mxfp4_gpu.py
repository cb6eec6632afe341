"""MXFP4 on the GPU: the HIP E2M1 quantiser against the torch specification, and the block-scaled
fp4 flavour of the tiled GEMM (two format-4 scaled MFMAs per 128-byte K-row).

Exactness is claimed where every partial sum is exact in fp32: integer operands in -3..3 (or all
sixteen E2M1 codes with scale exponents in -1..1) and power-of-two scales. The references are
computed in fp64 from the dequantised operands and compared bit for bit."""

import csv
import json
import os
import subprocess
import sys

import pytest
import torch

from _exact import pow2_f64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
FP4 = torch.float4_e2m1fn_x2
FP8 = torch.float8_e4m3fn
INT_CODE = (0, 2, 4, 5)  # E2M1 codes of |v| = 0, 1, 2, 3


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _ints(shape, g):
    """Integers in -3..3 (float32)."""
    return torch.randint(-3, 4, shape, generator=g, device=DEV).float()


def _pack_ints(v):
    """Integer values in -3..3 -> float4_e2m1fn_x2 ``[R, K/2]``."""
    from ddlb_amd.ops.mx import pack_e2m1

    code = torch.tensor(INT_CODE, device=v.device)[v.abs().long()]
    return pack_e2m1(code | ((v < 0).long() << 3))


def _wide(rows, k, g, dtype=torch.bfloat16):
    """randn * 2^U{-20..20}, one exponent per 32-element block."""
    x = torch.randn(rows, k // 32, 32, generator=g, device=DEV)
    ex = torch.randint(-20, 21, (rows, k // 32, 1), generator=g, device=DEV)
    x = torch.ldexp(x, ex).reshape(rows, k)
    if dtype == torch.float16:
        x = x.clamp(-60000, 60000)
    return x.to(dtype)


def _ref(a4, w4, s_a, s_w):
    """The exact product of the dequantised operands (fp64, returned as fp32)."""
    from ddlb_amd.ops.mx import dequantize_mxfp4

    a = dequantize_mxfp4(a4, s_a).double()
    w = dequantize_mxfp4(w4, s_w).double()
    return (a @ w.t()).float()


def _scaled(a4, w4, s_a, s_w, **kw):
    from ddlb_amd.ops.gemm import gemm

    out = gemm(a4, w4, out_dtype=kw.pop("out_dtype", torch.float32), a_scale=s_a, w_scale=s_w,
               **kw)
    torch.cuda.synchronize()
    return out


def _tiles():
    from ddlb_amd.ops.gemm import SCALED_FP4_TILES

    return ("auto",) + tuple(SCALED_FP4_TILES)


def _same(q, q_ref):
    return torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8))


# ------------------------------------------------------------------ 1. the quantiser
TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_quantizer_matches_reference(dtype):
    from ddlb_amd.ops.mx import quantize_mxfp4, quantize_mxfp4_reference, unpack_e2m1

    x = _wide(300, 512, _gen(11), dtype)
    x[0] = 0                                   # zero blocks (a whole row ...
    x[1, 32:64] = 0                            # ... and one inside a row)
    x[2] = 0
    x[2, 77] = -1.5                            # a lone maximum
    for i, j in enumerate((-9, -1, 0, 2, 6)):  # the 6 boundary: e = j, then e = j + 1
        x[3 + i, 0:32] = 1.0 * 2.0 ** j
        x[3 + i, 7] = 6.0 * 2.0 ** j
        x[3 + i, 32:64] = -2.0 * 2.0 ** j
        x[3 + i, 40] = 6.03125 * 2.0 ** j      # the next bf16 above 6 (exact in f16, f32 too)
    x[8, 0:32] = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -130  # subnormal amax
    x[9] = 0                                   # every tie, both signs, under e = 0; signed zeros
    x[9, 0] = 6.0
    for i, v in enumerate(TIES):
        x[9, 1 + i] = v
        x[9, 9 + i] = -v
    x[9, 20] = -0.0
    x[9, 21] = -0.1                            # a negative value that rounds to zero
    if dtype != torch.float16:                 # e = -127 (s = 0): subnormal inputs and scale
        x[10, 0:32] = 0
        x[10, 0:5] = torch.tensor([2.0 ** -125, 2.0 ** -126, -2.0 ** -127, 2.0 ** -128,
                                   1.5 * 2.0 ** -127]).to(dtype)
        x[10, 32:64] = 0                       # clamped to e = -127: 3 * 2^-127 stays 3
        x[10, 32:35] = torch.tensor([3.0 * 2.0 ** -127, -2.0 ** -127, 2.0 ** -129]).to(dtype)
    q, s = quantize_mxfp4(x)
    torch.cuda.synchronize()
    q_ref, s_ref = quantize_mxfp4_reference(x)
    if dtype != torch.float16:
        assert s_ref[10, :2].tolist() == [0, 0]
        assert unpack_e2m1(q_ref)[10, 0:5].tolist() == [4.0, 2.0, -1.0, 0.5, 1.5]
        assert unpack_e2m1(q_ref)[10, 32:35].tolist() == [3.0, -1.0, 0.0]
    assert q.dtype == FP4 and s.dtype == torch.uint8
    assert tuple(q.shape) == (300, 256) and tuple(s.shape) == (300, 16)
    assert torch.equal(s, s_ref), (s.int() - s_ref.int()).abs().max()
    bad = int((q.view(torch.uint8) != q_ref.view(torch.uint8)).sum())
    assert bad == 0, f"{bad} bytes differ"
    assert int(s[0, 0]) == 127 and int(s[2, 2]) == 127 - 2  # 1.5 = 0.75 * 2^1: e = 1 - 3
    assert [int(v) - 127 for v in s[3:8, 0]] == [-9, -1, 0, 2, 6]
    assert [int(v) - 127 for v in s[3:8, 1]] == [-8, 0, 1, 3, 7]
    # (2^-24, f16's smallest subnormal, is the normal 0.5 * 2^-23 in fp32: e = -26)
    assert int(s[8, 0]) == (127 - 26 if dtype == torch.float16 else 0)
    v = unpack_e2m1(q)[9]
    assert v[1:8].tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    assert v[9:16].tolist() == [-0.0, -1.0, -1.0, -2.0, -2.0, -4.0, -4.0]
    nib = q.view(torch.uint8)[9]
    assert int(nib[4]) >> 4 == 0x8 and int(nib[10]) == 0x88  # elements 9, 20 and 21: 0x8


def test_quantizer_row_shapes():
    """Rows shorter and longer than one pass of a workgroup, a row count that is no multiple
    of the rows per pass, strided input rows."""
    from ddlb_amd.ops.mx import quantize_mxfp4, quantize_mxfp4_reference

    for rows, k, dtype in ((7, 256, torch.float32), (37, 768, torch.bfloat16),
                           (3, 4352, torch.float16)):
        x = _wide(rows, k, _gen(rows), dtype)
        q, s = quantize_mxfp4(x)
        q_ref, s_ref = quantize_mxfp4_reference(x)
        assert torch.equal(s, s_ref) and _same(q, q_ref), (rows, k)
    wide = _wide(33, 1024, _gen(5))
    view = wide[:, 256:768]
    q, s = quantize_mxfp4(view)
    q_ref, s_ref = quantize_mxfp4_reference(view)
    assert torch.equal(s, s_ref) and _same(q, q_ref)


def test_quantizer_refusals():
    from ddlb_amd.ops.mx import quantize_mxfp4

    x = torch.zeros(16, 512, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        quantize_mxfp4(x.double())
    with pytest.raises(ValueError):
        quantize_mxfp4(x.cpu())
    with pytest.raises(ValueError):
        quantize_mxfp4(x[:, :128])                       # K % 256
    with pytest.raises(ValueError):
        quantize_mxfp4(x[:, :384])
    with pytest.raises(ValueError):
        quantize_mxfp4(x.reshape(2, 8, 512))             # 2-D
    with pytest.raises(ValueError):
        quantize_mxfp4(torch.zeros(16, 512, device=DEV, dtype=torch.bfloat16)[:, ::2])
    with pytest.raises(ValueError):  # rows that start 2 bytes off a 16-byte boundary
        quantize_mxfp4(torch.zeros(16, 264, device=DEV, dtype=torch.bfloat16)[:, 1:257])


# ------------------------------------------------------------------ 2 - 7. the scaled GEMM
def _single_block_case(M, N, K, seed):
    """Row r of A is non-zero only in block (5 r + 3) % (K / 32); every (row, block) carries its
    own scale, so a wrong (row, block) -> lane map or byte select shows in almost every output."""
    g = _gen(seed)
    nb = K // 32
    a = _ints((M, K), g).reshape(M, nb, 32)
    keep = (5 * torch.arange(M, device=DEV) + 3) % nb
    a = a * (torch.arange(nb, device=DEV).unsqueeze(0) == keep.unsqueeze(1)).unsqueeze(2)
    a4, w4 = _pack_ints(a.reshape(M, K)), _pack_ints(_ints((N, K), g))
    r = torch.arange(M, device=DEV).unsqueeze(1)
    n = torch.arange(N, device=DEV).unsqueeze(1)
    b = torch.arange(nb, device=DEV).unsqueeze(0)
    s_a = ((3 * r + 7 * b) % 13 + 121).to(torch.uint8)
    s_w = ((5 * n + 11 * b) % 13 + 121).to(torch.uint8)
    return a4, w4, s_a, s_w


def test_single_block_rows_exact():
    """Fixes the lane map: which lane supplies the scale of (row, block), and which byte."""
    a4, w4, s_a, s_w = _single_block_case(300, 202, 512, 4)
    want = _ref(a4, w4, s_a, s_w)
    assert int((want != 0).sum()) > want.numel() // 2
    for tile in _tiles():
        assert torch.equal(_scaled(a4, w4, s_a, s_w, tile=tile), want), tile


@pytest.mark.parametrize("K", [256, 512, 768])
def test_k_tile_edges(K):
    a4, w4, s_a, s_w = _single_block_case(300, 202, K, 6 + K)
    want = _ref(a4, w4, s_a, s_w)
    for tile in _tiles():
        assert torch.equal(_scaled(a4, w4, s_a, s_w, tile=tile), want), tile


def test_all_codes_exact():
    """Operands over all 16 nibbles, scale exponents in -1..1: every partial sum is a multiple
    of 2^-4 below 2^21."""
    g = _gen(5)
    M, N, K = 300, 202, 512
    a4 = torch.randint(0, 256, (M, K // 2), generator=g, device=DEV).to(torch.uint8).view(FP4)
    w4 = torch.randint(0, 256, (N, K // 2), generator=g, device=DEV).to(torch.uint8).view(FP4)
    s_a = (127 + torch.randint(-1, 2, (M, K // 32), generator=g, device=DEV)).to(torch.uint8)
    s_w = (127 + torch.randint(-1, 2, (N, K // 32), generator=g, device=DEV)).to(torch.uint8)
    want = _ref(a4, w4, s_a, s_w)
    for tile in _tiles():
        got = _scaled(a4, w4, s_a, s_w, tile=tile)
        print(f"all codes, tile {tile}: max|err| {float((got - want).abs().max()):.4g}")
        assert torch.equal(got, want), tile


def test_wide_scales_exact():
    """Scale bytes far from 127 whose sum per block stays small: a sign-extended or truncated
    scale byte shows. The reference adds the two exponents before it scales (fp64)."""
    g = _gen(8)
    M, N, K = 300, 202, 512
    nb = K // 32
    av, wv = _ints((M, K), g), _ints((N, K), g)
    E = torch.round(torch.linspace(-120, 120, nb, device=DEV, dtype=torch.float64)).long()
    e_a = E.unsqueeze(0) + torch.randint(-2, 3, (M, nb), generator=g, device=DEV)
    e_w = -E.unsqueeze(0) + torch.randint(-2, 3, (N, nb), generator=g, device=DEV)
    s_a, s_w = (e_a + 127).to(torch.uint8), (e_w + 127).to(torch.uint8)
    assert int(s_a.min()) < 10 and int(s_a.max()) > 245
    want = torch.zeros(M, N, dtype=torch.float64, device=DEV)
    for b in range(nb):
        p = av[:, 32 * b:32 * b + 32].double() @ wv[:, 32 * b:32 * b + 32].double().t()
        want += p * pow2_f64(e_a[:, b].unsqueeze(1) + e_w[:, b].unsqueeze(0))
    want = want.float()
    a4, w4 = _pack_ints(av), _pack_ints(wv)
    for tile in _tiles():
        assert torch.equal(_scaled(a4, w4, s_a, s_w, tile=tile), want), tile


def test_unit_scales_equal_the_integer_product():
    g = _gen(2)
    M, N, K = 300, 202, 512
    av, wv = _ints((M, K), g), _ints((N, K), g)
    one_a = torch.full((M, K // 32), 127, dtype=torch.uint8, device=DEV)
    one_w = torch.full((N, K // 32), 127, dtype=torch.uint8, device=DEV)
    want = (av.double() @ wv.double().t()).float()
    for tile in _tiles():
        assert torch.equal(_scaled(_pack_ints(av), _pack_ints(wv), one_a, one_w, tile=tile),
                           want), tile


def _padded(t, pad, poison):
    """``t`` (one-byte elements) as a view of a buffer whose rows are ``pad`` bytes longer, the
    padding filled with ``poison``."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), poison, dtype=torch.uint8, device=t.device)
    buf[:, :t.shape[1]] = t.view(torch.uint8)
    return buf[:, :t.shape[1]].view(t.dtype)


def test_padded_operand_rows_and_scale_pitch_exact():
    """fp4 operands and their scales as views of wider buffers (lda > K / 2 bytes, a scale pitch
    greater than K / 32) with poison in the padding: 6.0 pairs beside the data, NaN bytes beside
    the scales. Two ragged row tiles, two K-tiles, bf16 out: one rounding of the exact sum."""
    g = _gen(12)
    M, N, K = 130, 136, 512
    nb = K // 32
    av, wv = _ints((M, K), g), _ints((N, K), g)
    e_a = torch.randint(-2, 3, (M, nb), generator=g, device=DEV)
    e_w = torch.randint(-2, 3, (N, nb), generator=g, device=DEV)
    want = torch.zeros(M, N, dtype=torch.float64, device=DEV)
    for b in range(nb):
        p = av[:, 32 * b:32 * b + 32].double() @ wv[:, 32 * b:32 * b + 32].double().t()
        want += p * pow2_f64(e_a[:, b].unsqueeze(1) + e_w[:, b].unsqueeze(0))
    want = want.float().to(torch.bfloat16)  # (the sum is exact in f32: 21 bits at the most)
    a4, w4 = _padded(_pack_ints(av), 32, 0x77), _padded(_pack_ints(wv), 48, 0x77)
    s_a = _padded((e_a + 127).to(torch.uint8), 8, 0xFF)
    s_w = _padded((e_w + 127).to(torch.uint8), 16, 0xFF)
    assert a4.stride(0) == K // 2 + 32 and s_a.stride(0) == nb + 8
    for tile in ("auto", "128x128"):
        got = _scaled(a4, w4, s_a, s_w, tile=tile, out_dtype=torch.bfloat16)
        assert torch.equal(got, want), tile


def test_scaled_gemm_keeps_epilogue_and_c_rows():
    """Grouped C rows and the fused activation ride along (the tiled kernel carries them)."""
    a4, w4, s_a, s_w = _single_block_case(256, 128, 256, 9)
    want = _ref(a4, w4, s_a, s_w)
    out = torch.zeros(512, 128, device=DEV, dtype=torch.float32)
    _scaled(a4, w4, s_a, s_w, out=out, c_grp=64, c_gstride=128, act="relu")
    rows = torch.cat([torch.arange(i * 128, i * 128 + 64) for i in range(4)]).to(DEV)
    assert torch.equal(out[rows], want.clamp(min=0))
    assert not bool(out[rows + 64].any())


# ------------------------------------------------------------------ 8. end to end
@pytest.fixture(scope="module")
def end_to_end():
    from ddlb_amd.ops.mx import dequantize_mxfp4, quantize_mxfp4_reference

    g = _gen(7)
    a, w = _wide(512, 512, g), _wide(256, 512, g)
    a_dq = dequantize_mxfp4(*quantize_mxfp4_reference(a)).double()
    w_dq = dequantize_mxfp4(*quantize_mxfp4_reference(w)).double()
    return a, w, (a_dq @ w_dq.t()).float(), (a_dq.abs() @ w_dq.abs().t()).float()


def _run_end_to_end(a, w):
    from ddlb_amd.ops.mx import quantize_mxfp4

    aq, a_s = quantize_mxfp4(a)
    wq, w_s = quantize_mxfp4(w)
    return _scaled(aq, wq, a_s, w_s, out_dtype=torch.bfloat16)


def test_end_to_end_bf16(end_to_end):
    a, w, ref, mag = end_to_end
    out = _run_end_to_end(a, w)
    assert out.dtype == torch.bfloat16
    err = (out.float() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -10 * mag
    print(f"end to end: max err/bound {float((err / bound.clamp(min=1e-30)).max()):.4g}")
    assert bool((err <= bound).all())


def test_end_to_end_repeats_bit_identical(end_to_end):
    a, w, _, _ = end_to_end
    first = _run_end_to_end(a, w)
    for _ in range(2):
        assert torch.equal(_run_end_to_end(a, w), first)


# ------------------------------------------------------------------ 9. refusals
def test_refusals_before_launch():
    from ddlb_amd.ops.gemm import gemm

    M, N, K = 256, 128, 512
    nb = K // 32
    a4 = _pack_ints(torch.ones(M, K, device=DEV))
    w4 = _pack_ints(torch.ones(N, K, device=DEV))
    s_a = torch.full((M, nb), 127, dtype=torch.uint8, device=DEV)
    s_w = torch.full((N, nb), 127, dtype=torch.uint8, device=DEV)
    out = torch.full((M, N), -7.0, device=DEV)

    def refused(exc, a=a4, w=w4, o=out, **kw):
        args = dict(a_scale=s_a, w_scale=s_w)
        args.update(kw)
        with pytest.raises(exc):
            gemm(a, w, out=o, **args)

    for tile in ("pt4", "t4", "t8", "pt8", "256x256", "256x256w4", "i256"):
        refused(ValueError, tile=tile)
    refused(ValueError, w_scale=None)                                # missing scales
    refused(ValueError, a_scale=None)
    refused(ValueError, a_scale=None, w_scale=None)
    refused(ValueError, a_scale=s_a[:, :nb - 8])                     # shape
    refused(ValueError, w_scale=s_w[:N - 1])
    refused(ValueError, a_scale=s_a.t().contiguous().t())            # inner stride
    refused(ValueError, a_scale=torch.zeros(M, nb + 4, dtype=torch.uint8, device=DEV)[:, :nb])
    flat = torch.zeros(M * nb + 8, dtype=torch.uint8, device=DEV)
    refused(ValueError, a_scale=flat[4:4 + M * nb].view(M, nb))      # 4-byte, not 8-byte aligned
    refused(TypeError, a_scale=s_a.to(torch.int8))                   # dtype
    refused(TypeError, w_scale=s_w.float())
    refused(ValueError, w_scale=s_w.cpu())
    refused(ValueError, ksplit=2)
    refused(ValueError, mode="generic")
    refused(ValueError, a_grp=64, a_gstride=64)
    refused(ValueError, a=a4[:, :192], w=w4[:, :192], a_scale=s_a[:, :12].contiguous(),
            w_scale=s_w[:, :12].contiguous())                        # K = 384
    refused(TypeError, o=torch.full((M, N), -7.0, device=DEV, dtype=torch.float64))
    refused(TypeError, o=torch.full((M, N), -7.0, device=DEV).to(FP8))
    a8 = torch.ones(M, K // 2, device=DEV).to(FP8)
    refused(TypeError, a=a8)                                         # mixed fp8 / fp4
    refused(TypeError, w=torch.ones(N, K // 2, device=DEV).to(FP8))
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())  # nothing was launched
    gemm(a4, w4, out=out, a_scale=s_a, w_scale=s_w)
    torch.cuda.synchronize()
    assert bool((out == float(K)).all())


def test_native_entry_refuses_what_python_would():
    """The launch entry itself refuses (never something substituted) when called direct."""
    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import DT_F32, DT_FP4, SCALED_FP4_TILES, TILES

    C = load()
    assert sorted(C.MX4_TILES) == sorted(TILES[t] for t in SCALED_FP4_TILES)
    M, N, K = 256, 256, 512
    a4 = _pack_ints(torch.ones(M, K, device=DEV))
    w4 = _pack_ints(torch.ones(N, K, device=DEV))
    s = torch.full((M, K // 32), 127, dtype=torch.uint8, device=DEV)
    out = torch.full((M, N), -7.0, device=DEV)

    def call(tile, ksplit, sa, sw, k=K):
        C.gemm(a4.data_ptr(), w4.data_ptr(), out.data_ptr(), K, K, N, M, N, k, DT_FP4, DT_F32,
               TILES[tile], 2, 0, 0, 0, 0, torch.cuda.current_stream().cuda_stream, 0, ksplit,
               sa, sw, K // 32, K // 32)

    with pytest.raises(RuntimeError, match="invalid"):
        call("auto", 1, s.data_ptr(), 0)
    with pytest.raises(RuntimeError, match="invalid"):
        call("auto", 1, 0, 0)
    with pytest.raises(RuntimeError, match="invalid"):
        call("auto", 1, s.data_ptr(), s.data_ptr(), k=384)
    for tile, ks in (("pt4", 1), ("t8", 1), ("256x256", 1), ("auto", 2)):
        with pytest.raises(RuntimeError, match="invalid"):
            call(tile, ks, s.data_ptr(), s.data_ptr())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    call("auto", 1, s.data_ptr(), s.data_ptr())
    torch.cuda.synchronize()
    assert bool((out == float(K)).all())


# ------------------------------------------------------------------ 10. compute_only;quant=mxfp4
@pytest.fixture(scope="module")
def comm():
    from conftest import free_port
    from ddlb_amd.communicator import Communicator

    os.environ["DDLB_CHILD_INIT_METHOD"] = f"tcp://127.0.0.1:{free_port()}"
    Communicator.reset()
    c = Communicator()
    yield c
    Communicator.reset()
    os.environ.pop("DDLB_CHILD_INIT_METHOD", None)


@pytest.mark.parametrize("primitive", ["tp_columnwise", "tp_rowwise"])
def test_compute_only_quant_mxfp4_world1(comm, primitive):
    from ddlb_amd.primitives.registry import resolve

    for dtype in ("bfloat16", "float16"):
        cls, o, _ = resolve(primitive, "compute_only", {"quant": "mxfp4"})
        impl = cls(m=512, n=256, k=512, dtype=dtype, **o)
        assert impl.w.dtype == FP4
        for _ in range(2):
            out = impl.run()
        torch.cuda.synchronize()
        assert out.dtype == impl.torch_dtype and tuple(out.shape) == (512, 256)
        impl.validate(out)
        num = impl.numerics(out)
        assert num["ok"], num
        impl.close()
    with pytest.raises(ValueError, match="quant=mxfp4"):
        cls(m=512, n=256, k=512, dtype="bfloat16", quant="mxfp4", gemm="torch")
    with pytest.raises(ValueError, match="quant=mxfp4"):
        cls(m=512, n=256, k=512, dtype="float8_e4m3fn", quant="mxfp4")
    with pytest.raises(ValueError, match="quant=mxfp4"):
        cls(m=512, n=256, k=384, dtype="bfloat16", quant="mxfp4")


def test_cli_row_quant_mxfp4(tmp_path):
    from conftest import free_port

    env = dict(os.environ, DDLB_PROGRESS="0", DDLB_MASTER_PORT=str(free_port()))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
              "DDLB_CHILD_INIT_METHOD", "LOCAL_WORLD_SIZE", "DDLB_DEVICE"):
        env.pop(k, None)
    out = tmp_path / "res_{timestamp}.csv"
    cmd = [sys.executable, "-m", "ddlb_amd", "--primitive", "tp_columnwise", "-m", "512", "-n",
           "256", "-k", "512", "--dtype", "bfloat16", "--num-iterations", "2", "--num-warmups",
           "1", "--output-csv", str(out), "--impl", "compute_only;quant=mxfp4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    files = list(tmp_path.glob("res_*.csv"))
    assert len(files) == 1, r.stdout[-2000:]
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 1
    assert json.loads(rows[0]["spec"]).get("quant") == "mxfp4"
    assert rows[0]["valid"] == "True", rows[0].get("error", "")
    assert float(rows[0]["mean_time (ms)"]) > 0
