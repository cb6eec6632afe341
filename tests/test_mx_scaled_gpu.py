"""MX block scaling on the GPU: the HIP quantiser against the torch specification, and the
block-scaled flavour of the tiled fp8 GEMM (per-lane E8M0 scales into the scaled MFMA).

Exactness is claimed on integer operands in -3..3 with power-of-two scales: every product and
every partial sum is then an exact fp32 (and fp64) number, so the references below are computed in
fp64 and compared bit for bit."""

import csv
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
FP8 = torch.float8_e4m3fn


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _ints(shape, g):
    return torch.randint(-3, 4, shape, generator=g, device=DEV).float()


def _wide(rows, k, g, dtype=torch.bfloat16):
    """randn * 2^U{-20..20}, one exponent per 32-element block."""
    x = torch.randn(rows, k // 32, 32, generator=g, device=DEV)
    ex = torch.randint(-20, 21, (rows, k // 32, 1), generator=g, device=DEV)
    x = torch.ldexp(x, ex).reshape(rows, k)
    if dtype == torch.float16:
        x = x.clamp(-60000, 60000)
    return x.to(dtype)


def _ref(a8, w8, s_a, s_w):
    """The exact product of the dequantised operands (fp64, returned as fp32)."""
    from ddlb_amd.ops.mx import dequantize_mx

    a = dequantize_mx(a8, s_a).double()
    w = dequantize_mx(w8, s_w).double()
    return (a @ w.t()).float()


def _scaled(a8, w8, s_a, s_w, **kw):
    from ddlb_amd.ops.gemm import gemm

    out = gemm(a8, w8, out_dtype=kw.pop("out_dtype", torch.float32), a_scale=s_a, w_scale=s_w,
               **kw)
    torch.cuda.synchronize()
    return out


def _tiles():
    from ddlb_amd.ops.gemm import SCALED_TILES

    return ("auto",) + tuple(SCALED_TILES)


# ------------------------------------------------------------------ 1. the quantiser
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_quantizer_matches_reference(dtype):
    from ddlb_amd.ops.mx import quantize_mx, quantize_mx_reference

    x = _wide(300, 256, _gen(11), dtype)
    x[0] = 0                                   # zero blocks (a whole row ...
    x[1, 32:64] = 0                            # ... and one inside a row)
    x[2] = 0
    x[2, 77] = -1.5                            # a lone maximum
    big = 2.0 ** (10 if dtype != torch.float16 else 3)
    for i, j in enumerate((-9, -1, 0, 2, 6)):  # the 448 boundary: e = j, then e = j + 1
        x[3 + i, 0:32] = 3.0 * 2.0 ** j
        x[3 + i, 7] = 448.0 * 2.0 ** j
        x[3 + i, 32:64] = -5.0 * 2.0 ** j
        x[3 + i, 40] = 480.0 * 2.0 ** j        # (representable in bf16, f16 and f32)
    x[8, 0:32] = big
    x[9, 0:32] = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -130  # subnormal amax
    q, s = quantize_mx(x)
    torch.cuda.synchronize()
    q_ref, s_ref = quantize_mx_reference(x)
    assert q.dtype == FP8 and s.dtype == torch.uint8
    assert tuple(q.shape) == (300, 256) and tuple(s.shape) == (300, 8)
    assert torch.equal(s, s_ref), (s.int() - s_ref.int()).abs().max()
    assert torch.equal(q.float(), q_ref.float())
    assert int(s[0, 0]) == 127 and int(s[2, 2]) == 127 - 8  # 1.5 = 0.75 * 2^1: e = 1 - 9
    assert [int(v) - 127 for v in s[3:8, 0]] == [-9, -1, 0, 2, 6]
    assert [int(v) - 127 for v in s[3:8, 1]] == [-8, 0, 1, 3, 7]


def test_quantizer_row_shapes():
    """Rows shorter and longer than one pass of a workgroup, a row count that is no multiple
    of the rows per pass, strided input rows."""
    from ddlb_amd.ops.mx import quantize_mx, quantize_mx_reference

    for rows, k, dtype in ((7, 128, torch.float32), (37, 384, torch.bfloat16),
                           (3, 4224, torch.float16), (5, 2048, torch.float32)):
        x = _wide(rows, k, _gen(rows), dtype)
        q, s = quantize_mx(x)
        q_ref, s_ref = quantize_mx_reference(x)
        assert torch.equal(s, s_ref) and torch.equal(q.float(), q_ref.float()), (rows, k)
    wide = _wide(33, 512, _gen(5))
    view = wide[:, 128:384]
    q, s = quantize_mx(view)
    q_ref, s_ref = quantize_mx_reference(view)
    assert torch.equal(s, s_ref) and torch.equal(q.float(), q_ref.float())


def test_quantizer_refusals():
    from ddlb_amd.ops.mx import quantize_mx

    x = torch.zeros(16, 256, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        quantize_mx(x.double())
    with pytest.raises(ValueError):
        quantize_mx(x.cpu())
    with pytest.raises(ValueError):
        quantize_mx(x[:, :96])
    with pytest.raises(ValueError):
        quantize_mx(torch.zeros(16, 512, device=DEV, dtype=torch.bfloat16)[:, ::2])
    with pytest.raises(ValueError):  # rows that start 2 bytes off a 16-byte boundary
        quantize_mx(torch.zeros(16, 264, device=DEV, dtype=torch.bfloat16)[:, 1:257])


# ------------------------------------------------------------------ 2 - 6. the scaled GEMM
def test_unit_scales_equal_the_mx_kernel():
    from ddlb_amd.ops.gemm import gemm

    g = _gen(2)
    M, N, K = 512, 256, 512
    a8, w8 = _ints((M, K), g).to(FP8), _ints((N, K), g).to(FP8)
    one_a = torch.full((M, K // 32), 127, dtype=torch.uint8, device=DEV)
    one_w = torch.full((N, K // 32), 127, dtype=torch.uint8, device=DEV)
    base = gemm(a8, w8, mode="mx", out_dtype=torch.float32)
    torch.cuda.synchronize()
    assert torch.equal(base, (a8.double() @ w8.double().t()).float())
    for tile in _tiles():
        assert torch.equal(_scaled(a8, w8, one_a, one_w, tile=tile), base), tile


def test_per_row_scales_exact():
    from ddlb_amd.ops.gemm import gemm
    from ddlb_amd.ops.mx import ldexp_exact

    g = _gen(3)
    M, N, K = 512, 256, 512
    a8, w8 = _ints((M, K), g).to(FP8), _ints((N, K), g).to(FP8)
    ea = torch.arange(M, device=DEV) % 7 - 3
    ew = torch.arange(N, device=DEV) % 5 - 2
    s_a = (127 + ea).to(torch.uint8).unsqueeze(1).expand(M, K // 32).contiguous()
    s_w = (127 + ew).to(torch.uint8).unsqueeze(1).expand(N, K // 32).contiguous()
    unit = gemm(a8, w8, mode="mx", out_dtype=torch.float32)
    assert torch.equal(unit, (a8.double() @ w8.double().t()).float())
    want = ldexp_exact(unit, ea.unsqueeze(1) + ew.unsqueeze(0))
    for tile in _tiles():
        assert torch.equal(_scaled(a8, w8, s_a, s_w, tile=tile), want), tile


def _single_block_case(M, N, K, seed):
    """Row r of A is non-zero only in block (5 r + 3) % (K / 32); every (row, block) carries its
    own scale, so a wrong (row, block) -> lane map or byte select shows in almost every output."""
    g = _gen(seed)
    nb = K // 32
    a = _ints((M, K), g).reshape(M, nb, 32)
    keep = (5 * torch.arange(M, device=DEV) + 3) % nb
    a = a * (torch.arange(nb, device=DEV).unsqueeze(0) == keep.unsqueeze(1)).unsqueeze(2)
    a8, w8 = a.reshape(M, K).to(FP8), _ints((N, K), g).to(FP8)
    r = torch.arange(M, device=DEV).unsqueeze(1)
    n = torch.arange(N, device=DEV).unsqueeze(1)
    b = torch.arange(nb, device=DEV).unsqueeze(0)
    s_a = ((3 * r + 7 * b) % 13 + 121).to(torch.uint8)
    s_w = ((5 * n + 11 * b) % 13 + 121).to(torch.uint8)
    return a8, w8, s_a, s_w


def test_single_block_rows_exact():
    a8, w8, s_a, s_w = _single_block_case(300, 202, 512, 4)
    want = _ref(a8, w8, s_a, s_w)
    assert int((want != 0).sum()) > want.numel() // 2
    for tile in _tiles():
        assert torch.equal(_scaled(a8, w8, s_a, s_w, tile=tile), want), tile


def test_random_blocks_exact():
    g = _gen(5)
    M, N, K = 300, 202, 512
    a8, w8 = _ints((M, K), g).to(FP8), _ints((N, K), g).to(FP8)
    s_a = (127 + torch.randint(-2, 3, (M, K // 32), generator=g, device=DEV)).to(torch.uint8)
    s_w = (127 + torch.randint(-2, 3, (N, K // 32), generator=g, device=DEV)).to(torch.uint8)
    want = _ref(a8, w8, s_a, s_w)
    for tile in _tiles():
        got = _scaled(a8, w8, s_a, s_w, tile=tile)
        print(f"random blocks, tile {tile}: max|err| {float((got - want).abs().max()):.4g}")
        assert torch.equal(got, want), tile


@pytest.mark.parametrize("K", [128, 256, 384])
def test_k_tile_edges(K):
    a8, w8, s_a, s_w = _single_block_case(300, 202, K, 6 + K)
    want = _ref(a8, w8, s_a, s_w)
    for tile in _tiles():
        assert torch.equal(_scaled(a8, w8, s_a, s_w, tile=tile), want), tile


def test_scaled_gemm_keeps_epilogue_and_c_rows():
    """Grouped C rows and the fused activation ride along (the tiled kernel carries them)."""
    a8, w8, s_a, s_w = _single_block_case(256, 128, 256, 9)
    want = _ref(a8, w8, s_a, s_w)
    out = torch.zeros(512, 128, device=DEV, dtype=torch.float32)
    _scaled(a8, w8, s_a, s_w, out=out, c_grp=64, c_gstride=128, act="relu")
    rows = torch.cat([torch.arange(i * 128, i * 128 + 64) for i in range(4)]).to(DEV)
    assert torch.equal(out[rows], want.clamp(min=0))
    assert not bool(out[rows + 64].any())


# ------------------------------------------------------------------ 7, 10. end to end
@pytest.fixture(scope="module")
def end_to_end():
    from ddlb_amd.ops.mx import dequantize_mx, quantize_mx_reference

    g = _gen(7)
    a, w = _wide(512, 512, g), _wide(256, 512, g)
    a_dq = dequantize_mx(*quantize_mx_reference(a)).double()
    w_dq = dequantize_mx(*quantize_mx_reference(w)).double()
    return a, w, (a_dq @ w_dq.t()).float(), (a_dq.abs() @ w_dq.abs().t()).float()


def _run_end_to_end(a, w):
    from ddlb_amd.ops.mx import quantize_mx

    aq, a_s = quantize_mx(a)
    wq, w_s = quantize_mx(w)
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


# ------------------------------------------------------------------ 8. refusals
def test_refusals_before_launch():
    from ddlb_amd.ops.gemm import gemm

    M, N, K = 256, 128, 512
    nb = K // 32
    a8 = torch.ones(M, K, device=DEV).to(FP8)
    w8 = torch.ones(N, K, device=DEV).to(FP8)
    s_a = torch.full((M, nb), 127, dtype=torch.uint8, device=DEV)
    s_w = torch.full((N, nb), 127, dtype=torch.uint8, device=DEV)
    out = torch.full((M, N), -7.0, device=DEV)

    def refused(exc, **kw):
        args = dict(a_scale=s_a, w_scale=s_w)
        args.update(kw)
        with pytest.raises(exc):
            gemm(a8, w8, out=out, **args)

    for tile in ("pt4", "t4", "t8", "pt8", "256x256", "i256"):
        refused(ValueError, tile=tile)
    refused(ValueError, w_scale=None)
    refused(ValueError, a_scale=None)
    refused(ValueError, a_scale=s_a[:, :nb - 4])                     # shape
    refused(ValueError, w_scale=s_w[:N - 1])
    refused(ValueError, a_scale=s_a.t().contiguous().t())            # inner stride
    refused(ValueError, a_scale=torch.zeros(M, nb + 2, dtype=torch.uint8, device=DEV)[:, :nb])
    flat = torch.zeros(M * nb + 4, dtype=torch.uint8, device=DEV)
    refused(ValueError, a_scale=flat[1:1 + M * nb].view(M, nb))      # misaligned view
    refused(TypeError, a_scale=s_a.to(torch.int8))                   # dtype
    refused(TypeError, w_scale=s_w.float())
    refused(ValueError, w_scale=s_w.cpu())
    refused(ValueError, ksplit=2)
    refused(ValueError, mode="generic")
    refused(ValueError, a_grp=64, a_gstride=64)
    with pytest.raises(TypeError):                                   # bf16 operands
        gemm(a8.to(torch.bfloat16), w8.to(torch.bfloat16), a_scale=s_a, w_scale=s_w)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())  # nothing was launched
    gemm(a8, w8, out=out, a_scale=s_a, w_scale=s_w)
    torch.cuda.synchronize()
    assert bool((out == float(K)).all())


def test_native_entry_refuses_what_python_would():
    """The launch entry itself refuses (never unit scales in their place) when called direct."""
    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import DT_F32, DT_FP8, TILES

    C = load()
    M, N, K = 256, 256, 512
    a8 = torch.ones(M, K, device=DEV).to(FP8)
    w8 = torch.ones(N, K, device=DEV).to(FP8)
    s = torch.full((M, K // 32), 127, dtype=torch.uint8, device=DEV)
    out = torch.full((M, N), -7.0, device=DEV)

    def call(tile, ksplit, sa, sw):
        C.gemm(a8.data_ptr(), w8.data_ptr(), out.data_ptr(), K, K, N, M, N, K, DT_FP8, DT_F32,
               TILES[tile], 2, 0, 0, 0, 0, torch.cuda.current_stream().cuda_stream, 0, ksplit,
               sa, sw, K // 32, K // 32)

    with pytest.raises(RuntimeError, match="invalid"):
        call("auto", 1, s.data_ptr(), 0)
    for tile, ks in (("pt4", 1), ("t8", 1), ("256x256", 1), ("auto", 2)):
        with pytest.raises(RuntimeError):
            call(tile, ks, s.data_ptr(), s.data_ptr())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    call("auto", 1, s.data_ptr(), s.data_ptr())
    torch.cuda.synchronize()
    assert bool((out == float(K)).all())


def test_auto_tile_where_the_unit_scale_choice_is_pt4():
    """128 whole 256x256 tiles: choose_tile answers pt4, which takes no scales; `auto` must land
    on a tiled shape the scaled flavour has (never pt4 with the scales dropped)."""
    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import DT_FP8, TILES

    M, N, K = 8192, 1024, 256
    assert load().choose_tile(M, N, K, DT_FP8) == TILES["pt4"]
    g = _gen(12)
    a8, w8 = _ints((M, K), g).to(FP8), _ints((N, K), g).to(FP8)
    s_a = (127 + torch.randint(-2, 3, (M, K // 32), generator=g, device=DEV)).to(torch.uint8)
    s_w = (127 + torch.randint(-2, 3, (N, K // 32), generator=g, device=DEV)).to(torch.uint8)
    assert torch.equal(_scaled(a8, w8, s_a, s_w), _ref(a8, w8, s_a, s_w))


# ------------------------------------------------------------------ 9. compute_only;quant=mx
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
def test_compute_only_quant_mx_world1(comm, primitive):
    from ddlb_amd.primitives.registry import resolve

    for dtype in ("bfloat16", "float16"):
        cls, o, _ = resolve(primitive, "compute_only", {"quant": "mx"})
        impl = cls(m=512, n=256, k=512, dtype=dtype, **o)
        for _ in range(2):
            out = impl.run()
        torch.cuda.synchronize()
        assert out.dtype == impl.torch_dtype and tuple(out.shape) == (512, 256)
        impl.validate(out)
        num = impl.numerics(out)
        assert num["ok"], num
        impl.close()
    with pytest.raises(ValueError, match="quant=mx"):
        cls(m=512, n=256, k=512, dtype="bfloat16", quant="mx", gemm="torch")
    with pytest.raises(ValueError, match="quant=mx"):
        cls(m=512, n=256, k=512, dtype="float8_e4m3fn", quant="mx")


def test_cli_row_quant_mx(tmp_path):
    from conftest import free_port

    env = dict(os.environ, DDLB_PROGRESS="0", DDLB_MASTER_PORT=str(free_port()))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
              "DDLB_CHILD_INIT_METHOD", "LOCAL_WORLD_SIZE", "DDLB_DEVICE"):
        env.pop(k, None)
    out = tmp_path / "res_{timestamp}.csv"
    cmd = [sys.executable, "-m", "ddlb_amd", "--primitive", "tp_columnwise", "-m", "512", "-n",
           "256", "-k", "512", "--dtype", "bfloat16", "--num-iterations", "2", "--num-warmups",
           "1", "--output-csv", str(out), "--impl", "compute_only;quant=mx"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    files = list(tmp_path.glob("res_*.csv"))
    assert len(files) == 1, r.stdout[-2000:]
    with open(files[0], newline="") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 1
    assert json.loads(rows[0]["spec"]).get("quant") == "mx"
    assert rows[0]["valid"] == "True", rows[0].get("error", "")
    assert float(rows[0]["mean_time (ms)"]) > 0
