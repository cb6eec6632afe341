"""The MX block-scaling specification (``ddlb_amd.ops.mx``: pure torch, CPU tensors here) and the
``quant`` option of the compute_only slots where no GPU is needed."""

import pytest
import torch

from ddlb_amd.ops.mx import dequantize_mx, quantize_mx_reference

K = 256  # 8 blocks per row


def _wide(rows, k, seed):
    """randn * 2^U{-20..20}, one exponent per 32-element block."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, k // 32, 32, generator=g)
    ex = torch.randint(-20, 21, (rows, k // 32, 1), generator=g)
    return torch.ldexp(x, ex).reshape(rows, k)


def test_ldexp_exact_is_ldexp():
    from ddlb_amd.ops.mx import ldexp_exact

    n = torch.arange(-252, 255).unsqueeze(1)
    x = torch.tensor([1.0, -1.75, 448.0, 2.0 ** -120, 1.5 * 2.0 ** 100, 0.0])
    want = (x.double() * torch.pow(torch.tensor(2.0, dtype=torch.float64), n.double())).float()
    assert torch.equal(ldexp_exact(x.expand(n.shape[0], -1), n), want)


def test_powers_of_two_round_trip():
    g = torch.Generator().manual_seed(1)
    top = torch.randint(-100, 101, (64, K // 32, 1), generator=g)  # block exponent
    down = torch.randint(0, 16, (64, K // 32, 32), generator=g)    # 2^8 .. 2^-7 after scaling
    sign = torch.randint(0, 2, (64, K // 32, 32), generator=g) * 2 - 1
    x = (sign * torch.ldexp(torch.ones(()), top - down)).reshape(64, K)
    q, s = quantize_mx_reference(x)
    assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.uint8
    assert tuple(q.shape) == (64, K) and tuple(s.shape) == (64, K // 32)
    assert torch.equal(dequantize_mx(q, s), x)


def test_zero_block():
    x = _wide(4, K, 2)
    x[1, 64:96] = 0
    x[3] = 0
    q, s = quantize_mx_reference(x)
    assert s[1, 2] == 127 and bool((s[3] == 127).all())
    assert bool((q.float()[1, 64:96] == 0).all()) and bool((q.float()[3] == 0).all())
    assert torch.equal(dequantize_mx(q, s)[3], torch.zeros(K))


@pytest.mark.parametrize("j", [-12, -1, 0, 3, 10])
def test_448_boundary(j):
    # a block maximum of exactly 448 * 2^j keeps e = j; the next bf16 value above (bf16 spacing
    # at 448 is 2) needs e = j + 1
    x = torch.zeros(2, 128, dtype=torch.bfloat16)
    x[0, 5] = 448.0 * 2.0 ** j
    x[0, 6] = -3.0 * 2.0 ** j
    x[1, 37] = -450.0 * 2.0 ** j
    x[1, 40] = 448.0 * 2.0 ** j
    assert float(x[1, 37]) == -450.0 * 2.0 ** j
    q, s = quantize_mx_reference(x)
    assert int(s[0, 0]) - 127 == j and float(q.float()[0, 5]) == 448.0
    assert float(q.float()[0, 6]) == -3.0
    assert int(s[1, 1]) - 127 == j + 1 and float(q.float()[1, 37]) == -224.0
    assert float(q.float()[1, 40]) == 224.0
    assert int(s[0, 1]) == 127 and int(s[1, 0]) == 127  # the empty blocks


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_nothing_saturates_and_block_max_survives(dtype):
    x = _wide(128, K, 3)
    if dtype == torch.float16:
        x = x.clamp(-60000, 60000)
    x = x.to(dtype)
    q, s = quantize_mx_reference(x)
    assert not bool(torch.isnan(q.float()).any())
    assert int(s.max()) < 255
    xb = x.float().reshape(128, K // 32, 32)
    e = (s.to(torch.int32) - 127).unsqueeze(2)
    scaled = torch.ldexp(xb, -e)
    assert float(scaled.abs().max()) <= 448.0  # before any clamp
    # ... and by the SMALLEST such exponent: one less would overflow
    amax = xb.abs().amax(dim=2, keepdim=True)
    assert bool((torch.ldexp(amax, -(e - 1)) > 448.0)[amax > 0].all())
    dq = dequantize_mx(q, s).reshape(128, K // 32, 32)
    err = (dq - xb).abs().amax(dim=2, keepdim=True)
    assert bool((err <= 2.0 ** -4 * amax).all())
    at_max = (xb.abs() == amax)
    assert bool((((dq - xb).abs() <= 2.0 ** -4 * xb.abs()) | ~at_max).all())


def test_exponent_clamps():
    x = torch.zeros(3, 128, dtype=torch.float32)
    x[0, 0] = 2.0 ** -140          # subnormal amax: e would be -148
    x[0, 33] = 2.0 ** -126         # smallest normal: e would be -134
    x[1, 0] = torch.finfo(torch.float32).max  # e = 120, the largest a finite fp32 reaches
    x[2, 0] = 2.0 ** -118          # e = -126: the first value not clamped
    q, s = quantize_mx_reference(x)
    assert int(s[0, 0]) == 0 and int(s[0, 1]) == 0
    assert int(s[1, 0]) == 247
    assert int(s[2, 0]) == 1 and float(q.float()[2, 0]) == 256.0
    assert not bool(torch.isnan(q.float()).any())
    assert float(q.float()[1, 0]) == 256.0  # fp32 max / 2^120 = 256 (1 - 2^-24) rounds to 256
    assert int(s.max()) < 255


def test_shape_rules():
    with pytest.raises(ValueError):
        quantize_mx_reference(torch.zeros(4, 96))
    with pytest.raises(ValueError):
        quantize_mx_reference(torch.zeros(128))
    q, s = quantize_mx_reference(torch.ones(2, 128))
    with pytest.raises(ValueError):
        dequantize_mx(q, s[:, :3])


# ------------------------------------------------------------------ compute_only;quant=...
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


def test_quant_mx_refused_off_gpu_and_for_float32(cpu_comm):
    for cls in _classes():
        with pytest.raises(ValueError, match="quant=mx"):
            cls(m=64, n=32, k=128, dtype="bfloat16", quant="mx")  # a CPU device
        with pytest.raises(ValueError, match="quant=mx"):
            cls(m=64, n=32, k=128, dtype="float32", quant="mx")
        with pytest.raises(ValueError):
            cls(m=64, n=32, k=128, dtype="bfloat16", quant="fp4")


def test_quant_none_is_the_old_slot(cpu_comm):
    for cls in _classes():
        for opts in ({}, {"quant": "none"}, {"quant": "none", "size": "unsharded"}):
            impl = cls(m=64, n=32, k=128, dtype="float32", **opts)
            assert impl.options["quant"] == "none" and impl.mx is None
            out = impl.run()
            impl.validate(out)
            b = impl.B if cls.NAME == "tp_columnwise" else impl._b_ref
            assert torch.equal(impl.expected(), impl.a_in.float() @ b.float())
            assert impl.numerics(out)["ok"]
            impl.close()
