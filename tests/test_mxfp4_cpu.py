"""The MXFP4 specification (``ddlb_amd.ops.mx``: E2M1 elements, E8M0 block scales; pure torch, CPU
tensors here) and ``compute_only;quant=mxfp4`` where no GPU is needed."""

import pytest
import torch

from ddlb_amd.ops.mx import (E2M1_VALUES, dequantize_mxfp4, quantize_mxfp4_reference,
                             unpack_e2m1)

K = 256  # 8 blocks per row, the smallest K the format takes
FP4 = torch.float4_e2m1fn_x2
TIES = ((0.25, 0.0), (0.75, 1.0), (1.25, 1.0), (1.75, 2.0), (2.5, 2.0), (3.5, 4.0), (5.0, 4.0))


def _wide(rows, k, seed):
    """randn * 2^U{-20..20}, one exponent per 32-element block."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, k // 32, 32, generator=g)
    ex = torch.randint(-20, 21, (rows, k // 32, 1), generator=g)
    return torch.ldexp(x, ex).reshape(rows, k)


def _nibbles(q):
    """``[R, K]`` int64 nibble codes (sign << 3 | code) of a quantised tensor."""
    b = q.view(torch.uint8)
    return torch.stack((b & 0xF, b >> 4), dim=2).reshape(b.shape[0], -1).long()


def test_all_sixteen_codes_round_trip():
    # every byte value: both nibbles run over all 16 codes; every block holds a 6, so e = 0
    b = torch.arange(256, dtype=torch.uint8).reshape(2, 128)
    s = torch.full((2, K // 32), 127, dtype=torch.uint8)
    x = dequantize_mxfp4(b.view(FP4), s)
    assert tuple(x.shape) == (2, K)
    want = torch.tensor(E2M1_VALUES)
    assert torch.equal(x[0, 0:32:2].abs(), torch.cat((want, want)))   # low nibbles of bytes 0..15
    assert torch.equal(x[0, 1:32:2], torch.zeros(16))                 # their high nibbles
    assert torch.equal(torch.signbit(x[0, 0:32:2]), torch.arange(16) >= 8)
    q, s2 = quantize_mxfp4_reference(x)
    assert q.dtype == FP4 and s2.dtype == torch.uint8
    assert tuple(q.shape) == (2, K // 2) and tuple(s2.shape) == (2, K // 32)
    assert torch.equal(s2, s)
    assert torch.equal(q.view(torch.uint8), b)


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_ties_go_to_the_even_code(sign):
    x = torch.zeros(1, K)
    x[0, 31] = 6.0  # pins e = 0
    for i, (v, _) in enumerate(TIES):
        x[0, i] = sign * v
    q, s = quantize_mxfp4_reference(x)
    assert int(s[0, 0]) == 127
    got = unpack_e2m1(q)[0, :7]
    assert torch.equal(got, sign * torch.tensor([w for _, w in TIES]))
    assert bool((_nibbles(q)[0, :7] & 1 == 0).all())  # even codes
    if sign < 0:
        assert int(_nibbles(q)[0, 0]) == 0x8  # a negative value that rounds to zero


@pytest.mark.parametrize("j", [-12, -1, 0, 3, 10])
def test_six_boundary(j):
    # amax = 6 * 2^j keeps e = j; the next bf16 above 6 (spacing 2^-5) needs e = j + 1
    up = 6.03125
    x = torch.zeros(2, K, dtype=torch.bfloat16)
    x[0, 5] = 6.0 * 2.0 ** j
    x[0, 6] = -3.0 * 2.0 ** j
    x[1, 37] = -up * 2.0 ** j
    x[1, 40] = 6.0 * 2.0 ** j
    assert float(x[1, 37]) == -up * 2.0 ** j
    q, s = quantize_mxfp4_reference(x)
    v = unpack_e2m1(q)
    assert int(s[0, 0]) - 127 == j and float(v[0, 5]) == 6.0 and float(v[0, 6]) == -3.0
    assert int(s[1, 1]) - 127 == j + 1 and float(v[1, 37]) == -3.0 and float(v[1, 40]) == 3.0
    assert int(s[0, 1]) == 127 and int(s[1, 0]) == 127  # the empty blocks


def test_zero_blocks_and_signed_zero():
    x = _wide(4, K, 2)
    x[1, 64:96] = 0
    x[3] = 0
    x[2, 10] = -0.0
    q, s = quantize_mxfp4_reference(x)
    assert s[1, 2] == 127 and bool((s[3] == 127).all())
    assert bool((_nibbles(q)[1, 64:96] == 0).all()) and bool((_nibbles(q)[3] == 0).all())
    assert int(_nibbles(q)[2, 10]) == 0x8
    assert torch.equal(dequantize_mxfp4(q, s)[3], torch.zeros(K))
    qn, sn = quantize_mxfp4_reference(-torch.zeros(1, K))
    assert bool((qn.view(torch.uint8) == 0x88).all()) and bool((sn == 127).all())


def test_exponent_clamps_and_no_255():
    x = torch.zeros(3, K, dtype=torch.float32)
    x[0, 0] = 2.0 ** -140          # subnormal amax: e would be -142
    x[0, 33] = 2.0 ** -126         # smallest normal: e would be -128
    x[1, 0] = torch.finfo(torch.float32).max  # m > 0.75, ex = 128: e = 126
    x[2, 0] = 2.0 ** -125          # 0.5 * 2^-124: e = -127 exactly, the clamp does not act
    q, s = quantize_mxfp4_reference(x)
    assert int(s[0, 0]) == 0 and int(s[0, 1]) == 0
    assert int(s[1, 0]) == 253 and float(unpack_e2m1(q)[1, 0]) == 4.0
    assert int(s[2, 0]) == 0 and float(unpack_e2m1(q)[2, 0]) == 4.0
    assert float(unpack_e2m1(q)[0, 33]) == 2.0  # 2^-126 / 2^-127
    assert int(s.max()) < 255
    y = _wide(64, 512, 9)
    assert int(quantize_mxfp4_reference(y)[1].max()) < 255


def test_packing_order_on_a_hand_written_row():
    x = torch.zeros(1, K)
    x[0, :8] = torch.tensor([0.5, -1.0, 1.5, 2.0, -3.0, 4.0, 6.0, -0.5])
    q, s = quantize_mxfp4_reference(x)
    assert int(s[0, 0]) == 127
    # element 2j in the low nibble of byte j, 2j + 1 in the high one
    assert q.view(torch.uint8)[0, :5].tolist() == [0xA1, 0x43, 0x6D, 0x97, 0x00]
    assert torch.equal(dequantize_mxfp4(q, s), x)
    # slicing and cloning the packed dtype keeps the bytes
    assert q[:, :4].clone().view(torch.uint8)[0].tolist() == [0xA1, 0x43, 0x6D, 0x97]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_scaled_block_maximum_lies_in_3_to_6(dtype):
    x = _wide(128, 512, 3)
    if dtype == torch.float16:
        x = x.clamp(-60000, 60000)
    x = x.to(dtype)
    q, s = quantize_mxfp4_reference(x)
    xb = x.float().reshape(128, 16, 32)
    e = (s.to(torch.int32) - 127).unsqueeze(2)
    top = torch.ldexp(xb, -e).abs().amax(dim=2)
    nz = xb.abs().amax(dim=2) > 0
    assert bool((top[nz] <= 6.0).all()) and bool((top[nz] > 3.0).all())
    # the error of one element is at most half the largest step (2) in the scaled domain
    dq = dequantize_mxfp4(q, s).reshape(128, 16, 32)
    assert bool(((dq - xb).abs() <= torch.ldexp(torch.ones(()), e)).all())


def test_shape_rules():
    with pytest.raises(ValueError):
        quantize_mxfp4_reference(torch.zeros(4, 128))   # K % 256
    with pytest.raises(ValueError):
        quantize_mxfp4_reference(torch.zeros(4, 384))
    with pytest.raises(ValueError):
        quantize_mxfp4_reference(torch.zeros(256))      # 2-D
    q, s = quantize_mxfp4_reference(torch.ones(2, K))
    with pytest.raises(ValueError):
        dequantize_mxfp4(q, s[:, :7])
    with pytest.raises(ValueError):
        dequantize_mxfp4(q, s[:1])


def test_hip_quantiser_refuses_a_cpu_tensor():
    from ddlb_amd.ops.mx import quantize_mxfp4

    with pytest.raises(ValueError):
        quantize_mxfp4(torch.zeros(4, K, dtype=torch.bfloat16))
    with pytest.raises(TypeError):
        quantize_mxfp4(torch.zeros(4, K, dtype=torch.float64))


def test_dtype_code_and_tiles():
    from ddlb_amd.ops import gemm as g

    assert g.DT_FP4 == 6
    assert (g.DT_F32, g.DT_F16, g.DT_BF16, g.DT_FP8, g.DT_F64, g.DT_U8) == (0, 1, 2, 3, 4, 5)
    assert set(g.SCALED_FP4_TILES) <= set(g.TILES) and "auto" not in g.SCALED_FP4_TILES
    assert g.SCALED_TILES == ("256x128", "128x256", "128x128", "256x128w4")


# ------------------------------------------------------------------ compute_only;quant=mxfp4
@pytest.fixture
def cpu_comm(monkeypatch):
    from ddlb_amd.communicator import Communicator

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "DDLB_CHILD_INIT_METHOD"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DDLB_DEVICE", "cpu")
    Communicator.reset()
    yield Communicator()
    Communicator.reset()


def _classes():
    from ddlb_amd.primitives.tp_columnwise.compute_only import ComputeOnlyTPColumnwise
    from ddlb_amd.primitives.tp_rowwise.compute_only import ComputeOnlyTPRowwise

    return ComputeOnlyTPColumnwise, ComputeOnlyTPRowwise


def test_quant_mxfp4_refused_off_gpu_and_for_float32(cpu_comm):
    for cls in _classes():
        with pytest.raises(ValueError, match="quant=mxfp4"):
            cls(m=64, n=32, k=256, dtype="bfloat16", quant="mxfp4")  # a CPU device
        with pytest.raises(ValueError, match="quant=mxfp4"):
            cls(m=64, n=32, k=256, dtype="float32", quant="mxfp4")
        with pytest.raises(ValueError, match="quant=mxfp4"):
            cls(m=64, n=32, k=256, dtype="bfloat16", quant="mxfp4", gemm="torch")


def test_quant_none_is_unchanged(cpu_comm):
    for cls in _classes():
        impl = cls(m=64, n=32, k=128, dtype="float32", quant="none")
        assert impl.options["quant"] == "none" and impl.mx is None
        out = impl.run()
        impl.validate(out)
        assert impl.numerics(out)["ok"]
        impl.close()
