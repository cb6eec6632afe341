"""Quantised GEMM output, host side (no GPU): every refusal of ``_check_out_quant`` on CPU
tensors, the untouched ``out_quant=None`` path, and ``MxMLP``'s reference chain."""

import types

import pytest
import torch

from ddlb_amd.models.mx_mlp import MxMLP
from ddlb_amd.ops import gemm as G
from ddlb_amd.ops.gemm import _check_out_quant

FP8 = torch.float8_e4m3fn
FP4 = torch.float4_e2m1fn_x2
M, N, K = 64, 256, 256


def _bf16(rows=M, k=K):
    return torch.zeros(rows, k, dtype=torch.bfloat16)


def _fp8(rows=M, k=K):
    return torch.zeros(rows, k).to(FP8)


def _fp4(rows=M, k=K):
    return torch.zeros(rows, k // 2, dtype=torch.uint8).view(FP4)


def _sc(rows=M, k=K):
    return torch.full((rows, k // 32), 127, dtype=torch.uint8)


def _q(fmt, rows=M, n=N):
    if fmt == "mx":
        return torch.zeros(rows, n, dtype=torch.uint8).view(FP8)
    return torch.zeros(rows, n // 2, dtype=torch.uint8).view(FP4)


# ------------------------------------------------------------------ what is accepted
@pytest.mark.parametrize("fmt", ["mx", "mxfp4"])
def test_accepts_every_offered_form(fmt):
    assert _check_out_quant(_bf16(), _bf16(N), fmt) == (M, N, K)
    assert _check_out_quant(_bf16().half(), _bf16(N).half(), fmt) == (M, N, K)
    assert _check_out_quant(_fp8(), _fp8(N), fmt, a_scale=_sc(), w_scale=_sc(N)) == (M, N, K)
    assert _check_out_quant(_fp4(), _fp4(N), fmt, a_scale=_sc(), w_scale=_sc(N)) == (M, N, K)
    for tile in ("auto",) + tuple(G.SCALED_TILES):
        _check_out_quant(_bf16(), _bf16(N), fmt, tile=tile)
    # preallocated outputs, dense and as views of larger buffers (rows stay 16-byte aligned)
    _check_out_quant(_bf16(), _bf16(N), fmt, _q(fmt), _sc(M, N), ksplit=1, M=M)
    big, sbig = _q(fmt, M + 3, N + 64), torch.zeros(M + 3, N // 32 + 8, dtype=torch.uint8)
    ncol = N if fmt == "mx" else N // 2
    _check_out_quant(_bf16(), _bf16(N), fmt, big[:M, :ncol], sbig[:M, :N // 32])
    assert _check_out_quant(_bf16(), _bf16(N), fmt, M=10) == (10, N, K)


# ------------------------------------------------------------------ every refusal
def test_refuses_unknown_format_and_out_dtype():
    with pytest.raises(ValueError, match="out_quant"):
        _check_out_quant(_bf16(), _bf16(N), "fp8")
    with pytest.raises(TypeError, match="out_dtype"):
        _check_out_quant(_bf16(), _bf16(N), "mx", out_dtype=torch.bfloat16)
    _check_out_quant(_bf16(), _bf16(N), "mx", out_dtype=FP8)


def test_refuses_partial_blocks_of_n():
    for n in (32, 64, 96, 200, 320):
        with pytest.raises(ValueError, match="N % 128"):
            _check_out_quant(_bf16(), _bf16(n), "mx")
    for n in (128, 384, 320):
        with pytest.raises(ValueError, match="N % 256"):
            _check_out_quant(_bf16(), _bf16(n), "mxfp4")


def test_refuses_other_inputs():
    with pytest.raises(TypeError, match="bf16, f16, scaled fp8 or scaled fp4"):
        _check_out_quant(_bf16().float(), _bf16(N).float(), "mx")
    with pytest.raises(TypeError, match="bf16, f16, scaled fp8 or scaled fp4"):
        _check_out_quant(_bf16().double(), _bf16(N).double(), "mx")
    with pytest.raises(TypeError, match="dtype"):
        _check_out_quant(_bf16(), _bf16(N).half(), "mx")
    with pytest.raises(ValueError, match="K mismatch"):
        _check_out_quant(_bf16(), _bf16(N, 128), "mx")
    # fp8 without scales (no unit-scale kernel has this epilogue), or with one only
    with pytest.raises(ValueError, match="needs a_scale and w_scale"):
        _check_out_quant(_fp8(), _fp8(N), "mx")
    with pytest.raises(ValueError, match="needs a_scale and w_scale"):
        _check_out_quant(_fp8(), _fp8(N), "mx", a_scale=_sc())
    with pytest.raises(ValueError, match="a_scale and w_scale"):
        _check_out_quant(_fp4(), _fp4(N), "mx")
    # scales with 16-bit operands
    with pytest.raises(TypeError, match="block scales need"):
        _check_out_quant(_bf16(), _bf16(N), "mx", a_scale=_sc(), w_scale=_sc(N))
    # the scaled inputs' own rules still hold
    with pytest.raises(ValueError, match="shape"):
        _check_out_quant(_fp8(), _fp8(N), "mx", a_scale=_sc(M, 128), w_scale=_sc(N))
    with pytest.raises(ValueError, match="K % 256"):
        _check_out_quant(_fp4(M, 128), _fp4(N, 128), "mx", a_scale=_sc(M, 128),
                         w_scale=_sc(N, 128))


def test_refuses_tiles_modes_splits_and_grouped_rows():
    for tile in ("256x256", "256x256w4", "i256", "i128", "t8", "pt8", "t4", "pt4"):
        with pytest.raises(ValueError, match="tile"):
            _check_out_quant(_bf16(), _bf16(N), "mx", tile=tile)
    with pytest.raises(ValueError, match="generic"):
        _check_out_quant(_bf16(), _bf16(N), "mx", mode="generic")
    with pytest.raises(ValueError, match="mode='mx'"):
        _check_out_quant(_bf16(), _bf16(N), "mx", mode="mx")
    for ks in (2, 4):
        with pytest.raises(ValueError, match="K-split"):
            _check_out_quant(_bf16(), _bf16(N), "mx", ksplit=ks)
    with pytest.raises(ValueError, match="grouped"):
        _check_out_quant(_bf16(), _bf16(N), "mx", a_grp=16)
    with pytest.raises(ValueError, match="grouped"):
        _check_out_quant(_bf16(), _bf16(N), "mx", c_grp=16)
    with pytest.raises(ValueError, match="outside A"):
        _check_out_quant(_bf16(), _bf16(N), "mx", M=M + 1)


@pytest.mark.parametrize("fmt", ["mx", "mxfp4"])
def test_refuses_bad_out_and_out_scale(fmt):
    a, w = _bf16(), _bf16(N)
    ncol = N if fmt == "mx" else N // 2
    other = "mxfp4" if fmt == "mx" else "mx"
    with pytest.raises(TypeError, match="out must be"):
        _check_out_quant(a, w, fmt, torch.zeros(M, ncol, dtype=torch.bfloat16))
    with pytest.raises(TypeError, match="out must be"):
        _check_out_quant(a, w, fmt, torch.zeros(M, ncol, dtype=torch.uint8))
    with pytest.raises((TypeError, ValueError)):
        _check_out_quant(a, w, fmt, _q(other))
    with pytest.raises(ValueError, match="shape"):
        _check_out_quant(a, w, fmt, _q(fmt, M - 1))
    with pytest.raises(ValueError, match="shape"):
        _check_out_quant(a, w, fmt, _q(fmt, M, 2 * N))
    with pytest.raises(ValueError, match="shape"):
        _check_out_quant(a, w, fmt, _q(fmt)[0])
    with pytest.raises(ValueError, match="stride"):  # rows 8 bytes off a multiple of 16
        _check_out_quant(a, w, fmt, torch.zeros(M, ncol + 8, dtype=torch.uint8)
                         .view(FP8 if fmt == "mx" else FP4)[:, :ncol])
    with pytest.raises(ValueError, match="stride"):
        _check_out_quant(a, w, fmt, _q(fmt, M, 2 * N)[:, ::2])
    buf = torch.zeros(M * ncol + 16, dtype=torch.uint8)
    off = (-buf.data_ptr()) % 16 + 8
    mis = buf[off:off + M * ncol].view(M, ncol).view(FP8 if fmt == "mx" else FP4)
    with pytest.raises(ValueError, match="16-byte-aligned"):
        _check_out_quant(a, w, fmt, mis)
    out_meta = _q(fmt).to("meta")
    with pytest.raises(ValueError, match="out is on"):
        _check_out_quant(a, w, fmt, out_meta)
    # the scales
    nb = N // 32
    with pytest.raises(TypeError, match="uint8"):
        _check_out_quant(a, w, fmt, out_scale=torch.zeros(M, nb, dtype=torch.int8))
    with pytest.raises(ValueError, match="shape"):
        _check_out_quant(a, w, fmt, out_scale=torch.zeros(M, nb + 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="shape"):
        _check_out_quant(a, w, fmt, out_scale=torch.zeros(M - 1, nb, dtype=torch.uint8))
    with pytest.raises(ValueError, match="stride"):  # a pitch of nb + 2: no multiple of 4
        _check_out_quant(a, w, fmt, out_scale=torch.zeros(M, nb + 2, dtype=torch.uint8)[:, :nb])
    if fmt == "mxfp4":  # a multiple of 4 is not enough for fp4 data: 8
        with pytest.raises(ValueError, match="multiple of 8"):
            _check_out_quant(a, w, fmt,
                             out_scale=torch.zeros(M, nb + 4, dtype=torch.uint8)[:, :nb])
    with pytest.raises(ValueError, match="stride"):
        _check_out_quant(a, w, fmt, out_scale=torch.zeros(M, 2 * nb, dtype=torch.uint8)[:, ::2])
    sbuf = torch.zeros(M * nb + 16, dtype=torch.uint8)
    soff = (-sbuf.data_ptr()) % 8 + 2
    with pytest.raises(ValueError, match="aligned"):
        _check_out_quant(a, w, fmt, out_scale=sbuf[soff:soff + M * nb].view(M, nb))
    with pytest.raises(ValueError, match="out_scale is on"):
        _check_out_quant(a, w, fmt, out_scale=torch.zeros(M, nb, dtype=torch.uint8, device="meta"))


def test_refuses_a_scale_span_of_2_gib():
    """Meta tensors: shapes and strides without the bytes."""
    rows = 2 ** 31 // (N // 32)
    a = torch.zeros(rows, K, dtype=torch.bfloat16, device="meta")
    w = torch.zeros(N, K, dtype=torch.bfloat16, device="meta")
    with pytest.raises(ValueError, match="2 GiB"):
        _check_out_quant(a, w, "mx")
    _check_out_quant(a, w, "mx", M=rows - 1)
    sc = torch.zeros(M, 2 ** 25, dtype=torch.uint8, device="meta")[:, :N // 32]
    am = torch.zeros(M, K, dtype=torch.bfloat16, device="meta")
    with pytest.raises(ValueError, match="2 GiB"):
        _check_out_quant(am, w, "mx", out_scale=sc)


def test_gemm_refuses_before_the_extension_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("load() reached before the refusal")

    monkeypatch.setattr(G, "load", no_load)
    with pytest.raises(ValueError, match="N % 128"):
        G.gemm(_bf16(), _bf16(96), out_quant="mx")
    with pytest.raises(ValueError, match="K-split"):
        G.gemm(_bf16(), _bf16(N), out_quant="mx", ksplit=2)
    with pytest.raises(ValueError, match="out_scale goes with out_quant"):
        G.gemm(_bf16(), _bf16(N), out_scale=_sc(M, N))


# ------------------------------------------------------------------ out_quant=None: the old path
class _Recorder:
    def __init__(self):
        self.calls = []

    def gemm(self, *args):
        self.calls.append(args)

    def gemm_fast_path_ok(self, *args):
        return True


def test_out_quant_none_reaches_the_old_path_unchanged(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(G, "load", lambda: rec)
    monkeypatch.setattr(G, "_check_operands", lambda *a, **k: None)
    a, w = _bf16(), _bf16(N)
    out = torch.zeros(M, N, dtype=torch.bfloat16)
    assert G.gemm(a, w, out, tile="128x128", act="gelu", stream=0, ksplit=1) is out
    assert G.gemm(a, w, out, tile="128x128", act="gelu", stream=0, ksplit=1,
                  out_quant=None, out_scale=None) is out
    want = (a.data_ptr(), w.data_ptr(), out.data_ptr(), K, K, N, M, N, K, G.DT_BF16, G.DT_BF16,
            G.TILES["128x128"], G.MODES["auto"], 0, 0, 0, 0, 0, G.ACTS["gelu"])
    assert rec.calls == [want, want]
    # the block-scaled path: 24 positional arguments as before, no output scales among them
    a8, w8, sa, sw = _fp8(), _fp8(N), _sc(), _sc(N)
    rec.calls.clear()
    G.gemm(a8, w8, out, stream=0, a_scale=sa, w_scale=sw)
    assert rec.calls == [(a8.data_ptr(), w8.data_ptr(), out.data_ptr(), K, K, N, M, N, K,
                          G.DT_FP8, G.DT_BF16, 0, G.MODES["mx"], 0, 0, 0, 0, 0, 0, 1,
                          sa.data_ptr(), sw.data_ptr(), K // 32, K // 32)]


def test_automatic_k_split_does_not_engage(monkeypatch):
    """A shape for which a plain bf16 GEMM would split K runs as ONE quantising launch."""
    rec = _Recorder()
    monkeypatch.setattr(G, "load", lambda: rec)
    monkeypatch.setattr(G, "_check_placement", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "current_stream",
                        lambda dev=None: types.SimpleNamespace(cuda_stream=0))
    m, n, k = 256, 256, 2048
    assert G.split_k_factor(m, n, k, 2, 256) > 1
    a, w = _bf16(m, k), _bf16(n, k)
    q, s = G.gemm(a, w, out_quant="mx", act="silu")
    assert q.dtype == FP8 and tuple(q.shape) == (m, n) and q.stride(0) % 16 == 0
    assert s.dtype == torch.uint8 and tuple(s.shape) == (m, n // 32) and s.stride(0) % 4 == 0
    assert rec.calls == [(a.data_ptr(), w.data_ptr(), q.data_ptr(), k, k, n, m, n, k, G.DT_BF16,
                          G.DT_FP8, 0, G.MODES["auto"], 0, 0, 0, 0, 0, G.ACTS["silu"], 1,
                          0, 0, 0, 0, s.data_ptr(), n // 32)]
    rec.calls.clear()
    q4, s4 = G.gemm(a, w, out_quant="mxfp4")   # fp4: ldc in elements
    assert q4.dtype == FP4 and tuple(q4.shape) == (m, n // 2) and s4.stride(0) % 8 == 0
    assert rec.calls[0][5] == n and rec.calls[0][10] == G.DT_FP4 and rec.calls[0][19] == 1


# ------------------------------------------------------------------ MxMLP
def _gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


@pytest.mark.parametrize("fmt", ["mx", "mxfp4"])
def test_mlp_reference_is_the_dequantised_chain(fmt):
    from ddlb_amd.ops import mx

    g = torch.Generator().manual_seed(3)
    S, H, F = 5, 256, 256
    X = (torch.rand(S, H, generator=g) * 2 - 1).to(torch.bfloat16)
    W1 = ((torch.rand(F, H, generator=g) * 2 - 1) / 16).to(torch.bfloat16)
    W2 = ((torch.rand(H, F, generator=g) * 2 - 1) / 16).to(torch.bfloat16)
    qr, dq = ((mx.quantize_mx_reference, mx.dequantize_mx) if fmt == "mx"
              else (mx.quantize_mxfp4_reference, mx.dequantize_mxfp4))
    xd, w1d, w2d = dq(*qr(X)), dq(*qr(W1)), dq(*qr(W2))
    h = _gelu_tanh(xd @ w1d.t())
    want = dq(*qr(h)) @ w2d.t()
    got = MxMLP.reference_chain(X, W1, W2, "gelu", fmt)
    assert got.dtype == torch.float32 and tuple(got.shape) == (S, H)
    # (the hand-written gelu and torch's differ by rounding: a few quantisation steps of h at most)
    torch.testing.assert_close(got, want, rtol=0, atol=1e-3 * F)
    relu = MxMLP.reference_chain(X, W1, W2, "relu", fmt)
    assert torch.equal(relu, dq(*qr(torch.relu(xd @ w1d.t()))) @ w2d.t())
    # reference() of an instance is that chain on its own tensors
    m = MxMLP.__new__(MxMLP)
    m.X, m.W1, m.W2, m.act, m.fmt = X, W1, W2, "relu", fmt
    assert torch.equal(m.reference(), relu)


def test_mlp_refuses_construction_off_a_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        MxMLP(256, 256, 8)
    with pytest.raises(ValueError, match="fmt"):
        MxMLP(256, 256, 8, fmt="fp6")
    with pytest.raises(ValueError, match="multiples of 256"):
        MxMLP(256, 384, 8, fmt="mxfp4")
    with pytest.raises(TypeError, match="bfloat16 / float16"):
        MxMLP(256, 256, 8, dtype="float32")
