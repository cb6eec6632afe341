"""Gated (GLU) GEMM epilogue, host side (no GPU): the weight packing, the torch specification,
every refusal of ``_check_glu`` on CPU tensors, what ``gemm(glu=True)`` passes to the extension
and allocates (a stub extension), and ``MxMLP``'s gated reference chain."""

import types

import pytest
import torch

from ddlb_amd.models.mx_mlp import MxMLP
from ddlb_amd.ops import gemm as G
from ddlb_amd.ops.gemm import _check_glu, glu_reference, pack_glu, unpack_glu

FP8 = torch.float8_e4m3fn
FP4 = torch.float4_e2m1fn_x2
M, N, K = 64, 512, 256


def _bf16(rows=M, k=K):
    return torch.zeros(rows, k, dtype=torch.bfloat16)


def _fp8(rows=M, k=K):
    return torch.zeros(rows, k).to(FP8)


def _fp4(rows=M, k=K):
    return torch.zeros(rows, k // 2, dtype=torch.uint8).view(FP4)


def _sc(rows=M, k=K):
    return torch.full((rows, k // 32), 127, dtype=torch.uint8)


def _q(fmt, rows=M, cols=N // 2):
    if fmt == "mx":
        return torch.zeros(rows, cols, dtype=torch.uint8).view(FP8)
    return torch.zeros(rows, cols // 2, dtype=torch.uint8).view(FP4)


# ------------------------------------------------------------------ packing
def test_pack_glu_against_an_index_loop():
    F, k = 96, 5
    gate = torch.arange(F * k, dtype=torch.float32).reshape(F, k)
    up = -gate - 1
    w = pack_glu(gate, up)
    assert tuple(w.shape) == (2 * F, k) and w.dtype == gate.dtype
    for r in range(2 * F):
        g, c = divmod(r, 64)
        src = gate if c < 32 else up
        assert torch.equal(w[r], src[32 * g + c % 32]), r


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.uint8, FP8,
                                   FP4])
def test_pack_unpack_round_trip(dtype):
    g = torch.Generator().manual_seed(1)
    F, k = 64, 48
    gate, up = (torch.randint(0, 120, (F, k), generator=g, dtype=torch.uint8) for _ in range(2))
    if dtype in (FP8, FP4):
        gate, up = gate.view(dtype), up.view(dtype)
    elif dtype != torch.uint8:
        gate, up = gate.to(dtype), up.to(dtype)
    w = pack_glu(gate, up)
    assert w.dtype == dtype and tuple(w.shape) == (2 * F, k)
    g2, u2 = unpack_glu(w)
    assert g2.dtype == dtype and u2.dtype == dtype
    assert torch.equal(g2.view(torch.uint8) if dtype in (FP8, FP4) else g2,
                       gate.view(torch.uint8) if dtype in (FP8, FP4) else gate)
    assert torch.equal(u2.view(torch.uint8) if dtype in (FP8, FP4) else u2,
                       up.view(torch.uint8) if dtype in (FP8, FP4) else up)


@pytest.mark.parametrize("fmt", ["mx", "mxfp4"])
def test_packing_quantised_pairs_commutes_with_quantising_the_packed_weight(fmt):
    from ddlb_amd.ops import mx

    qr = mx.quantize_mx_reference if fmt == "mx" else mx.quantize_mxfp4_reference
    g = torch.Generator().manual_seed(2)
    F, k = 64, 256
    gate, up = (torch.randn(F, k, generator=g).to(torch.bfloat16) for _ in range(2))
    (gq, gs), (uq, us) = qr(gate), qr(up)
    wq, ws = qr(pack_glu(gate, up))
    pq, ps = pack_glu(gq, uq), pack_glu(gs, us)
    assert pq.dtype == wq.dtype and ps.dtype == torch.uint8
    assert torch.equal(pq.view(torch.uint8), wq.view(torch.uint8)) and torch.equal(ps, ws)
    g2, u2 = unpack_glu(wq)
    assert torch.equal(g2.view(torch.uint8), gq.view(torch.uint8))
    assert torch.equal(u2.view(torch.uint8), uq.view(torch.uint8))
    assert torch.equal(unpack_glu(ws)[1], us)


def test_pack_glu_refusals():
    with pytest.raises(ValueError, match="F % 32"):
        pack_glu(torch.zeros(48, 4), torch.zeros(48, 4))
    with pytest.raises(ValueError, match="one shape and dtype"):
        pack_glu(torch.zeros(32, 4), torch.zeros(64, 4))
    with pytest.raises(ValueError, match="one shape and dtype"):
        pack_glu(torch.zeros(32, 4), torch.zeros(32, 4, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="one shape and dtype"):
        pack_glu(torch.zeros(32), torch.zeros(32))
    with pytest.raises(ValueError, match="multiple of 64"):
        unpack_glu(torch.zeros(96, 4))


# ------------------------------------------------------------------ the specification
def _gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


_NAIVE = {"none": lambda x: x, "relu": lambda x: torch.clamp(x, min=0),
          "silu": lambda x: x * torch.sigmoid(x), "gelu": _gelu_tanh}


@pytest.mark.parametrize("act", ["none", "relu", "silu", "gelu"])
def test_glu_reference_against_a_column_loop(act):
    g = torch.Generator().manual_seed(3)
    m, n = 5, 192
    c = torch.randn(m, n, generator=g) * 2
    out = glu_reference(c, act)
    assert out.dtype == torch.float32 and tuple(out.shape) == (m, n // 2)
    want = torch.empty(m, n // 2)
    for j in range(n // 2):
        grp, col = divmod(j, 32)
        want[:, j] = _NAIVE[act](c[:, 64 * grp + col]) * c[:, 64 * grp + 32 + col]
    if act in ("none", "relu"):
        assert torch.equal(out, want)
    else:  # torch's fused activations against the written-out formulas: f32 rounding only
        torch.testing.assert_close(out, want, rtol=1e-5, atol=1e-6)


def test_glu_reference_is_the_product_of_the_unpacked_halves():
    g = torch.Generator().manual_seed(4)
    F, k, m = 64, 32, 7
    gate, up, x = (torch.randn(r, k, generator=g) for r in (F, F, m))
    c = x @ pack_glu(gate, up).t()
    assert torch.equal(glu_reference(c, "relu"), torch.relu(x @ gate.t()) * (x @ up.t()))
    with pytest.raises(ValueError, match="unknown activation"):
        glu_reference(c, "tanh")
    with pytest.raises(ValueError, match="f32"):
        glu_reference(c.double(), "none")
    with pytest.raises(ValueError, match="2F % 64"):
        glu_reference(c[:, :96], "none")


# ------------------------------------------------------------------ what is accepted
def test_accepts_every_offered_form():
    bf, f32 = torch.bfloat16, torch.float32
    assert _check_glu(_bf16(), _bf16(N)) == (M, N, K, bf)
    assert _check_glu(_bf16(), _bf16(64)) == (M, 64, K, bf)
    assert _check_glu(_bf16(), _bf16(N), out_dtype=f32) == (M, N, K, f32)
    assert _check_glu(_bf16().half(), _bf16(N).half()) == (M, N, K, torch.float16)
    sc = dict(a_scale=_sc(), w_scale=_sc(N))
    for odt in (bf, torch.float16, f32):
        assert _check_glu(_fp8(), _fp8(N), out_dtype=odt, **sc) == (M, N, K, odt)
        assert _check_glu(_fp4(), _fp4(N), out_dtype=odt, **sc) == (M, N, K, odt)
    assert _check_glu(_fp8(), _fp8(N), **sc)[3] == bf
    for fmt, qdt in (("mx", FP8), ("mxfp4", FP4)):
        assert _check_glu(_bf16(), _bf16(N), out_quant=fmt) == (M, N, K, qdt)
        assert _check_glu(_fp8(), _fp8(N), out_quant=fmt, **sc) == (M, N, K, qdt)
        assert _check_glu(_fp4(), _fp4(N), out_quant=fmt, **sc) == (M, N, K, qdt)
        for tile in ("auto",) + tuple(G.SCALED_TILES):
            _check_glu(_bf16(), _bf16(N), out_quant=fmt, tile=tile, act="silu")
        # preallocated, dense and as views of larger buffers: N / 2 columns, N / 64 scales
        _check_glu(_bf16(), _bf16(N), _q(fmt), _sc(M, N // 2), out_quant=fmt)
        big = _q(fmt, M + 3, N // 2 + 64)
        sbig = torch.zeros(M + 3, N // 64 + 8, dtype=torch.uint8)
        ncol = N // 2 if fmt == "mx" else N // 4
        _check_glu(_bf16(), _bf16(N), big[:M, :ncol], sbig[:M, :N // 64], out_quant=fmt)
    _check_glu(_bf16(), _bf16(256), out_quant="mx")
    out = torch.zeros(M + 2, N // 2 + 8, dtype=torch.bfloat16)[:M, :N // 2]
    assert _check_glu(_bf16(), _bf16(N), out, M=10) == (10, N, K, bf)


# ------------------------------------------------------------------ every refusal
def test_refuses_n_off_the_modulus():
    for n in (32, 96, 200):
        with pytest.raises(ValueError, match="N % 64"):
            _check_glu(_bf16(), _bf16(n))
    for n in (64, 128, 384, 320):
        with pytest.raises(ValueError, match="N % 256"):
            _check_glu(_bf16(), _bf16(n), out_quant="mx")
    for n in (256, 768, 320):
        with pytest.raises(ValueError, match="N % 512"):
            _check_glu(_bf16(), _bf16(n), out_quant="mxfp4")


def test_refuses_other_inputs_and_outputs():
    sc = dict(a_scale=_sc(), w_scale=_sc(N))
    with pytest.raises(TypeError, match="bf16, f16, scaled fp8 or scaled fp4"):
        _check_glu(_bf16().float(), _bf16(N).float())
    with pytest.raises(TypeError, match="bf16, f16, scaled fp8 or scaled fp4"):
        _check_glu(_bf16().double(), _bf16(N).double())
    with pytest.raises(TypeError, match="dtype"):
        _check_glu(_bf16(), _bf16(N).half())
    with pytest.raises(ValueError, match="K mismatch"):
        _check_glu(_bf16(), _bf16(N, 128))
    # unit-scale fp8 (the unit-scale kernels have no gated epilogue), or one scale only
    with pytest.raises(ValueError, match="needs a_scale and w_scale"):
        _check_glu(_fp8(), _fp8(N))
    with pytest.raises(ValueError, match="needs a_scale and w_scale"):
        _check_glu(_fp8(), _fp8(N), a_scale=_sc())
    with pytest.raises(ValueError, match="a_scale and w_scale"):
        _check_glu(_fp4(), _fp4(N))
    with pytest.raises(TypeError, match="block scales need"):
        _check_glu(_bf16(), _bf16(N), **sc)
    with pytest.raises(ValueError, match="shape"):
        _check_glu(_fp8(), _fp8(N), a_scale=_sc(M, 128), w_scale=_sc(N))
    with pytest.raises(ValueError, match="K % 256"):
        _check_glu(_fp4(M, 128), _fp4(N, 128), a_scale=_sc(M, 128), w_scale=_sc(N, 128))
    # dense outputs: only what the operands pair with
    with pytest.raises(TypeError, match="writes one of"):
        _check_glu(_bf16(), _bf16(N), out_dtype=torch.float16)
    with pytest.raises(TypeError, match="writes one of"):
        _check_glu(_bf16().half(), _bf16(N).half(), out_dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="writes one of"):
        _check_glu(_fp8(), _fp8(N), out_dtype=torch.float64, **sc)
    with pytest.raises(TypeError, match="writes one of"):
        _check_glu(_bf16(), _bf16(N), torch.zeros(M, N // 2, dtype=torch.float16))
    with pytest.raises(TypeError, match="out_dtype"):
        _check_glu(_bf16(), _bf16(N), out_quant="mx", out_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="out_quant"):
        _check_glu(_bf16(), _bf16(N), out_quant="fp8")
    with pytest.raises(ValueError, match="out_scale goes with out_quant"):
        _check_glu(_bf16(), _bf16(N), out_scale=_sc(M, N // 2))
    with pytest.raises(ValueError, match="unknown activation"):
        _check_glu(_bf16(), _bf16(N), act="tanh")


def test_refuses_tiles_modes_splits_and_grouped_rows():
    for tile in ("256x256", "256x256w4", "i256", "i128", "i256w4", "t8", "pt8", "t4", "pt4"):
        with pytest.raises(ValueError, match="tile"):
            _check_glu(_bf16(), _bf16(N), tile=tile)
        with pytest.raises(ValueError, match="tile"):
            _check_glu(_fp8(), _fp8(N), a_scale=_sc(), w_scale=_sc(N), tile=tile,
                       out_quant="mx")
    with pytest.raises(ValueError, match="generic"):
        _check_glu(_bf16(), _bf16(N), mode="generic")
    with pytest.raises(ValueError, match="mode='mx'"):
        _check_glu(_bf16(), _bf16(N), mode="mx")
    with pytest.raises(ValueError, match="unknown mode"):
        _check_glu(_bf16(), _bf16(N), mode="fast")
    for ks in (2, 4):
        with pytest.raises(ValueError, match="K-split"):
            _check_glu(_bf16(), _bf16(N), ksplit=ks)
    with pytest.raises(ValueError, match="grouped"):
        _check_glu(_bf16(), _bf16(N), a_grp=16)
    with pytest.raises(ValueError, match="grouped"):
        _check_glu(_bf16(), _bf16(N), c_grp=16)
    with pytest.raises(ValueError, match="outside A"):
        _check_glu(_bf16(), _bf16(N), M=M + 1)


def test_refuses_bad_dense_out():
    a, w, F = _bf16(), _bf16(N), N // 2
    with pytest.raises(ValueError, match="shape"):   # the ungated width
        _check_glu(a, w, torch.zeros(M, N, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="shape"):
        _check_glu(a, w, torch.zeros(M - 1, F, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="shape"):
        _check_glu(a, w, torch.zeros(F, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="stride"):  # ldc = N / 2 - 1: rows overlap
        _check_glu(a, w, torch.as_strided(torch.zeros(M * F, dtype=torch.bfloat16), (M, F),
                                          (F - 1, 1)))
    with pytest.raises(ValueError, match="stride"):
        _check_glu(a, w, torch.zeros(M, N, dtype=torch.bfloat16)[:, ::2])
    with pytest.raises(ValueError, match="out is on"):
        _check_glu(a, w, torch.zeros(M, F, dtype=torch.bfloat16, device="meta"))


@pytest.mark.parametrize("fmt", ["mx", "mxfp4"])
def test_refuses_bad_quantised_out_and_out_scale(fmt):
    a, w, F = _bf16(), _bf16(N), N // 2
    nb = F // 32
    with pytest.raises(TypeError, match="out must be"):
        _check_glu(a, w, torch.zeros(M, F, dtype=torch.bfloat16), out_quant=fmt)
    with pytest.raises(ValueError, match="shape"):   # the ungated width
        _check_glu(a, w, _q(fmt, M, N), out_quant=fmt)
    with pytest.raises(ValueError, match="shape"):   # the ungated number of scales
        _check_glu(a, w, out_scale=_sc(M, N), out_quant=fmt)
    with pytest.raises(ValueError, match="shape"):
        _check_glu(a, w, out_scale=torch.zeros(M - 1, nb, dtype=torch.uint8), out_quant=fmt)
    # a short scale pitch: rows of N / 64 bytes, N / 64 - 4 apart
    short = torch.as_strided(torch.zeros(M * nb, dtype=torch.uint8), (M, nb), (nb - 4, 1))
    with pytest.raises(ValueError, match="stride"):
        _check_glu(a, w, out_scale=short, out_quant=fmt)
    with pytest.raises(ValueError, match="stride"):  # a pitch of nb + 2: no multiple of 4
        _check_glu(a, w, out_scale=torch.zeros(M, nb + 2, dtype=torch.uint8)[:, :nb],
                   out_quant=fmt)
    ncol = F if fmt == "mx" else F // 2
    with pytest.raises(ValueError, match="stride"):  # rows 8 bytes off a multiple of 16
        _check_glu(a, w, torch.zeros(M, ncol + 8, dtype=torch.uint8)
                   .view(FP8 if fmt == "mx" else FP4)[:, :ncol], out_quant=fmt)
    with pytest.raises(TypeError, match="uint8"):
        _check_glu(a, w, out_scale=torch.zeros(M, nb, dtype=torch.int8), out_quant=fmt)


def test_gemm_refuses_before_the_extension_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError("load() reached before the refusal")

    monkeypatch.setattr(G, "load", no_load)
    sc = dict(a_scale=_sc(), w_scale=_sc(N))
    bad = [
        (ValueError, "N % 64", dict(w=_bf16(96))),
        (ValueError, "N % 256", dict(w=_bf16(384), out_quant="mx")),
        (ValueError, "N % 512", dict(w=_bf16(768), out_quant="mxfp4")),
        (ValueError, "K-split", dict(ksplit=2)),
        (ValueError, "grouped", dict(a_grp=16, a_gstride=16)),
        (ValueError, "grouped", dict(c_grp=16, c_gstride=16)),
        (ValueError, "tile", dict(tile="pt4")),
        (ValueError, "tile", dict(tile="256x256")),
        (ValueError, "generic", dict(mode="generic")),
        (ValueError, "needs a_scale and w_scale", dict(a=_fp8(), w=_fp8(N))),
        (TypeError, "bf16, f16, scaled fp8", dict(a=_bf16().float(), w=_bf16(N).float())),
        (TypeError, "bf16, f16, scaled fp8", dict(a=_bf16().double(), w=_bf16(N).double())),
        (TypeError, "writes one of", dict(out_dtype=torch.float16)),
        (ValueError, "stride", dict(out=torch.as_strided(
            torch.zeros(M * N, dtype=torch.bfloat16), (M, N // 2), (N // 2 - 1, 1)))),
        (ValueError, "stride", dict(out_quant="mx", out_scale=torch.as_strided(
            torch.zeros(M * N, dtype=torch.uint8), (M, N // 64), (N // 64 - 4, 1)))),
        (ValueError, "out_scale goes with out_quant", dict(out_scale=_sc(M, N // 2))),
        (ValueError, "K % 256", dict(a=_fp4(M, 128), w=_fp4(N, 128), a_scale=_sc(M, 128),
                                     w_scale=_sc(N, 128))),
        (TypeError, "block scales need", dict(**sc)),
    ]
    for exc, match, kw in bad:
        kw = dict(kw)
        a, w = kw.pop("a", _bf16()), kw.pop("w", _bf16(N))
        out = kw.pop("out", None)
        with pytest.raises(exc, match=match):
            G.gemm(a, w, out, glu=True, **kw)


# ------------------------------------------------------------------ the call of the extension
class _Recorder:
    def __init__(self):
        self.calls = []

    def gemm(self, *args):
        self.calls.append(args)

    def gemm_fast_path_ok(self, *args):
        return True


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(G, "load", lambda: r)
    monkeypatch.setattr(G, "_check_placement", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "current_stream",
                        lambda dev=None: types.SimpleNamespace(cuda_stream=0))
    return r


def test_dense_glu_call_and_allocation(rec):
    m, n, k = 130, 320, 2048   # (a shape whose ungated bf16 GEMM might split K: glu never does)
    a, w = _bf16(m, k), _bf16(n, k)
    out = G.gemm(a, w, glu=True, act="silu", tile="128x128")
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (m, n // 2)
    assert rec.calls == [(a.data_ptr(), w.data_ptr(), out.data_ptr(), k, k, n // 2, m, n, k,
                          G.DT_BF16, G.DT_BF16, G.TILES["128x128"], G.MODES["auto"], 0, 0, 0, 0,
                          0, G.ACTS["silu"], 1, 0, 0, 0, 0, 0, 0, 1)]
    rec.calls.clear()
    o32 = G.gemm(a, w, glu=True, out_dtype=torch.float32)
    assert o32.dtype == torch.float32 and tuple(o32.shape) == (m, n // 2)
    assert rec.calls[0][10] == G.DT_F32 and rec.calls[0][-1] == 1 and len(rec.calls[0]) == 27
    # a preallocated view: its own pitch goes down as ldc, and it is what comes back
    rec.calls.clear()
    view = torch.zeros(m + 3, n // 2 + 8, dtype=torch.bfloat16)[:m, :n // 2]
    assert G.gemm(a, w, view, glu=True) is view
    assert rec.calls[0][2] == view.data_ptr() and rec.calls[0][5] == n // 2 + 8
    # block-scaled operands: the scales in their places, mode mx, glu last
    rec.calls.clear()
    a8, w8, sa, sw = _fp8(m, 256), _fp8(n, 256), _sc(m, 256), _sc(n, 256)
    o8 = G.gemm(a8, w8, glu=True, a_scale=sa, w_scale=sw, act="relu")
    assert o8.dtype == torch.bfloat16 and tuple(o8.shape) == (m, n // 2)
    assert rec.calls == [(a8.data_ptr(), w8.data_ptr(), o8.data_ptr(), 256, 256, n // 2, m, n,
                          256, G.DT_FP8, G.DT_BF16, 0, G.MODES["mx"], 0, 0, 0, 0, 0,
                          G.ACTS["relu"], 1, sa.data_ptr(), sw.data_ptr(), 8, 8, 0, 0, 1)]
    # glu=False: the old call, no trailing arguments
    rec.calls.clear()
    monkeypatch_out = torch.zeros(m, n, dtype=torch.bfloat16)
    G.gemm(a, w, monkeypatch_out, glu=False, ksplit=1, stream=0)
    assert len(rec.calls[0]) == 19


@pytest.mark.parametrize("fmt", ["mx", "mxfp4"])
def test_quantised_glu_call_and_allocation(rec, fmt):
    m, n, k = 130, 1024, 256
    a, w = _bf16(m, k), _bf16(n, k)
    q, s = G.gemm(a, w, glu=True, out_quant=fmt, act="silu")
    q4 = fmt == "mxfp4"
    assert q.dtype == (FP4 if q4 else FP8)
    assert tuple(q.shape) == (m, n // 4 if q4 else n // 2) and q.stride(0) % 16 == 0
    assert s.dtype == torch.uint8 and tuple(s.shape) == (m, n // 64)
    assert s.stride(0) % (8 if q4 else 4) == 0
    # ldc in elements (fp4: two per byte): N / 2 either way
    assert rec.calls == [(a.data_ptr(), w.data_ptr(), q.data_ptr(), k, k, n // 2, m, n, k,
                          G.DT_BF16, G.DT_FP4 if q4 else G.DT_FP8, 0, G.MODES["auto"], 0, 0, 0, 0,
                          0, G.ACTS["silu"], 1, 0, 0, 0, 0, s.data_ptr(), n // 64, 1)]
    rec.calls.clear()
    a4, w4, sa, sw = _fp4(m, k), _fp4(n, k), _sc(m, k), _sc(n, k)
    q, s = G.gemm(a4, w4, glu=True, out_quant=fmt, a_scale=sa, w_scale=sw)
    assert rec.calls == [(a4.data_ptr(), w4.data_ptr(), q.data_ptr(), k, k, n // 2, m, n, k,
                          G.DT_FP4, G.DT_FP4 if q4 else G.DT_FP8, 0, G.MODES["mx"], 0, 0, 0, 0,
                          0, 0, 1, sa.data_ptr(), sw.data_ptr(), k // 32, k // 32, s.data_ptr(),
                          n // 64, 1)]


# ------------------------------------------------------------------ MxMLP
@pytest.mark.parametrize("fmt", ["mx", "mxfp4"])
def test_gated_mlp_reference_is_the_chain_written_out(fmt):
    from ddlb_amd.ops import mx

    g = torch.Generator().manual_seed(5)
    S, H, F = 5, 256, 256
    X = (torch.rand(S, H, generator=g) * 2 - 1).to(torch.bfloat16)
    Wg = ((torch.rand(F, H, generator=g) * 2 - 1) / 16).to(torch.bfloat16)
    Wu = ((torch.rand(F, H, generator=g) * 2 - 1) / 16).to(torch.bfloat16)
    W2 = ((torch.rand(H, F, generator=g) * 2 - 1) / 16).to(torch.bfloat16)
    qr, dq = ((mx.quantize_mx_reference, mx.dequantize_mx) if fmt == "mx"
              else (mx.quantize_mxfp4_reference, mx.dequantize_mxfp4))
    xd, gd, ud, w2d = dq(*qr(X)), dq(*qr(Wg)), dq(*qr(Wu)), dq(*qr(W2))
    W1 = pack_glu(Wg, Wu)
    assert tuple(W1.shape) == (2 * F, H)
    h = torch.relu(xd @ gd.t()) * (xd @ ud.t())
    want = dq(*qr(h)) @ w2d.t()
    got = MxMLP.reference_chain(X, W1, W2, "relu", fmt, gated=True)
    assert got.dtype == torch.float32 and tuple(got.shape) == (S, H)
    assert torch.equal(got, want)
    hs = (xd @ gd.t()) * torch.sigmoid(xd @ gd.t()) * (xd @ ud.t())
    silu = MxMLP.reference_chain(X, W1, W2, "silu", fmt, gated=True)
    # (the written-out silu and torch's differ by rounding: a few quantisation steps of h)
    torch.testing.assert_close(silu, dq(*qr(hs)) @ w2d.t(), rtol=0, atol=1e-3 * F)
    # reference() of a gated instance is that chain; flops count fc1's 2F rows
    m = MxMLP.__new__(MxMLP)
    m.X, m.W1, m.W2, m.act, m.fmt, m.gated = X, W1, W2, "relu", fmt, True
    m.S, m.H, m.F = S, H, F
    assert torch.equal(m.reference(), want)
    assert m.flops == 6.0 * S * H * F
    m.gated = False
    assert m.flops == 4.0 * S * H * F
