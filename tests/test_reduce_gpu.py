"""The d-way reduce kernel of the native reduce-scatter (`csrc/runtime/kernels.hip`): every
source count (the fixed-count unrolled kernels 2..8 and the runtime-count kernel beyond), every
dtype, ragged tails; compared with an fp32 PyTorch sum in the same source order."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DT = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


@pytest.mark.parametrize("dtype", list(DT))
@pytest.mark.parametrize("nsrc", [1, 2, 3, 4, 5, 7, 8, 9, 16])
@pytest.mark.parametrize("count", [8, 1000, 1 << 20])
def test_reduce_sum(dtype, nsrc, count):
    from ddlb_amd.ops import load

    C = load()
    gen = torch.Generator(device="cuda").manual_seed(nsrc * 131 + count)
    # 16-byte aligned sources: one slab, rows padded to a multiple of 8 elements
    pad = (count + 7) // 8 * 8
    slab = torch.rand((nsrc, pad), generator=gen, device="cuda", dtype=torch.float32)
    slab = (2 * slab - 1).to(dtype)
    out = torch.full((pad,), float("nan"), device="cuda", dtype=dtype)
    s = torch.cuda.current_stream().cuda_stream
    C.reduce_sum(out.data_ptr(), [slab[i].data_ptr() for i in range(nsrc)], count, DT[dtype], s)
    torch.cuda.synchronize()
    ref = slab[0, :count].float()
    for i in range(1, nsrc):
        ref = ref + slab[i, :count].float()
    tol = 1e-6 if dtype == torch.float32 else 1e-2 * nsrc
    torch.testing.assert_close(out[:count].float(), ref.to(dtype).float(), rtol=0, atol=tol)
    if pad > count:
        assert torch.isnan(out[count:].float()).all()  # nothing written past count


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("nsrc", [1, 2, 4, 8, 9])
@pytest.mark.parametrize("count", [8, 1003, (1 << 20) + 5])
def test_reduce_sum_f32_sources(dtype, nsrc, count):
    """f32 sources into a 16-bit destination (the K-split GEMM's partials, rounded once): equal
    to the fp32 sum in source order, rounded to the destination dtype."""
    from ddlb_amd.ops import load

    C = load()
    gen = torch.Generator(device="cuda").manual_seed(nsrc * 7 + count)
    pad = (count + 7) // 8 * 8
    slab = 2 * torch.rand((nsrc, pad), generator=gen, device="cuda", dtype=torch.float32) - 1
    out = torch.full((pad,), float("nan"), device="cuda", dtype=dtype)
    s = torch.cuda.current_stream().cuda_stream
    C.reduce_sum(out.data_ptr(), [slab[i].data_ptr() for i in range(nsrc)], count, DT[dtype], s,
                 DT[torch.float32])
    torch.cuda.synchronize()
    ref = slab[0, :count].clone()
    for i in range(1, nsrc):
        ref = ref + slab[i, :count]
    assert torch.equal(out[:count], ref.to(dtype))
    if pad > count:
        assert torch.isnan(out[count:].float()).all()
    with pytest.raises(RuntimeError):  # f32 sources only, 16-bit destinations only
        C.reduce_sum(out.data_ptr(), [slab[0].data_ptr()], count, DT[dtype], s, DT[dtype] ^ 3)


def _int_slab(nsrc, pad, dtype, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(-3, 4, (nsrc, pad), generator=gen, device="cuda").float().to(dtype)


@pytest.mark.parametrize("count", [8, 1003, 4099])
def test_reduce_sum_exact(count):
    """Integer-valued sources in -3..3: every partial sum is exact, so the result is the sum
    rounded once (not at all here: |sum| <= 48), compared bit for bit. Every source count of the
    same-dtype form (1, the unrolled 2..8, the runtime-count kernel up to 16) and of the
    f32-source form (1..9); a vector body with and without a scalar tail; the NaN-filled
    elements after ``count`` stay NaN."""
    from ddlb_amd.ops import load

    C = load()
    s = torch.cuda.current_stream().cuda_stream
    pad = (count + 7) // 8 * 8 + 8
    for dtype in DT:
        slab = _int_slab(16, pad, dtype, count)
        for nsrc in range(1, 17):
            out = torch.full((pad,), float("nan"), device="cuda", dtype=dtype)
            C.reduce_sum(out.data_ptr(), [slab[i].data_ptr() for i in range(nsrc)], count,
                         DT[dtype], s)
            want = slab[:nsrc, :count].double().sum(dim=0).float().to(dtype)
            assert torch.equal(out[:count], want), (dtype, nsrc)
            assert bool(torch.isnan(out[count:].float()).all()), (dtype, nsrc)
    slab = _int_slab(9, pad, torch.float32, count + 1)
    for dtype in (torch.float16, torch.bfloat16):
        for nsrc in range(1, 10):
            out = torch.full((pad,), float("nan"), device="cuda", dtype=dtype)
            C.reduce_sum(out.data_ptr(), [slab[i].data_ptr() for i in range(nsrc)], count,
                         DT[dtype], s, DT[torch.float32])
            want = slab[:nsrc, :count].double().sum(dim=0).float().to(dtype)
            assert torch.equal(out[:count], want), (dtype, nsrc)
            assert bool(torch.isnan(out[count:].float()).all()), (dtype, nsrc)
