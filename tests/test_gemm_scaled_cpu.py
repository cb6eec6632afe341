"""Block-scaled GEMM front-end, host side (no GPU): every refusal ``gemm`` makes for fp8 operands
with scales and for fp4 operands, on CPU tensors and before anything is launched, and the exact
positional tuples the accepted calls hand to the extension (the quantised-output tuples are
pinned in ``test_qout_cpu.py``)."""

import pytest
import torch

from ddlb_amd.ops import gemm as G

FP8 = torch.float8_e4m3fn
FP4 = torch.float4_e2m1fn_x2
M, N, K = 64, 128, 512
NB = K // 32


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
    monkeypatch.setattr(G, "_check_operands", lambda *a, **k: None)
    return r


def _fp8(rows, k=K, ld=None):
    return torch.zeros(rows, ld or k).to(FP8)[:, :k]


def _fp4(rows, k=K, ld=None):
    return torch.zeros(rows, (ld or k) // 2, dtype=torch.uint8).view(FP4)[:, :k // 2]


def _sc(rows, nb=NB, ld=None):
    return torch.full((rows, ld or nb), 127, dtype=torch.uint8)[:, :nb]


FORMATS = {
    # operand maker, scale alignment, the noun of the messages, tiles refused
    "fp8": (_fp8, 4, "block scales", ("pt4", "t4", "t8", "pt8", "256x256", "i256")),
    "fp4": (_fp4, 8, "the fp4 GEMM", ("pt4", "t4", "t8", "pt8", "256x256", "256x256w4", "i256")),
}


@pytest.mark.parametrize("fmt", ["fp8", "fp4"])
def test_refusals_before_launch(rec, fmt):
    make, al, noun, bad_tiles = FORMATS[fmt]
    a, w, s_a, s_w = make(M), make(N), _sc(M), _sc(N)
    out = torch.zeros(M, N)

    def refused(exc, match, a=a, w=w, o=out, **kw):
        args = dict(a_scale=s_a, w_scale=s_w, stream=0)
        args.update(kw)
        with pytest.raises(exc, match=match):
            G.gemm(a, w, out=o, **args)
        assert rec.calls == []

    for tile in bad_tiles:
        refused(ValueError, f"{noun} (is|are) offered for tile auto", tile=tile)
    if fmt == "fp8":
        refused(ValueError, "go together", w_scale=None)
        refused(ValueError, "go together", a_scale=None)
    else:
        refused(ValueError, "need a_scale and w_scale", w_scale=None)
        refused(ValueError, "need a_scale and w_scale", a_scale=None)
        refused(ValueError, "need a_scale and w_scale", a_scale=None, w_scale=None)
    refused(ValueError, "a_scale must have shape", a_scale=s_a[:, :NB - 8])
    refused(ValueError, "w_scale must have shape", w_scale=s_w[:N - 1])
    refused(ValueError, "a_scale needs unit inner stride", a_scale=s_a.t().contiguous().t())
    refused(ValueError, f"w_scale needs unit inner stride and a row stride that is a multiple "
            f"of {al}", w_scale=_sc(N, ld=NB + al // 2))
    flat = torch.zeros(M * NB + 8, dtype=torch.uint8)
    off = al // 2 if fmt == "fp4" else 1  # fp4: 4-byte, not 8-byte aligned
    refused(ValueError, f"a_scale must start at an? {al}-byte-aligned",
            a_scale=flat[off:off + M * NB].view(M, NB))
    refused(TypeError, "a_scale must be a uint8 tensor", a_scale=s_a.to(torch.int8))
    refused(TypeError, "w_scale must be a uint8 tensor", w_scale=s_w.float())
    refused(TypeError, "a_scale must be a uint8 tensor", a_scale=[1, 2])
    refused(ValueError, "w_scale is on meta", w_scale=s_w.to("meta"))
    refused(ValueError, f"{noun} do(es)? not combine with a K-split", ksplit=2)
    refused(ValueError, r"mode auto / mx\), not mode='generic'", mode="generic")
    refused(ValueError, f"{noun} needs? plain A rows", a_grp=32, a_gstride=32)
    if fmt == "fp8":
        refused(ValueError, r"K % 128 == 0 \(K = 96\)", a=make(M, 96), w=make(N, 96),
                a_scale=_sc(M, 3, 4), w_scale=_sc(N, 3, 4))
        with pytest.raises(TypeError, match="block scales need float8_e4m3fn operands"):
            G.gemm(a.to(torch.bfloat16), w.to(torch.bfloat16), a_scale=s_a, w_scale=s_w, stream=0)
    else:
        refused(ValueError, r"K % 256 == 0 \(K = 384\)", a=a[:, :192], w=w[:, :192],
                a_scale=s_a[:, :12].contiguous(), w_scale=s_w[:, :12].contiguous())
        refused(TypeError, "fp4 GEMM output must be bf16, f16 or f32",
                o=torch.zeros(M, N, dtype=torch.float64))
        refused(TypeError, "fp4 GEMM output must be bf16, f16 or f32", o=torch.zeros(M, N).to(FP8))
        refused(TypeError, "do not mix", a=_fp8(M, K // 2))
        refused(TypeError, "do not mix", w=_fp8(N, K // 2))
    assert rec.calls == []
    # the same operands are accepted, and nothing else was recorded on the way
    G.gemm(a, w, out=out, a_scale=s_a, w_scale=s_w, stream=0)
    assert len(rec.calls) == 1 and len(rec.calls[0]) == 24


def test_scale_span_of_2_gib_is_refused(rec):
    """rows * pitch >= 2^31. Meta tensors: shapes and strides without the bytes."""
    for make in (_fp8, _fp4):
        a, w = make(M).to("meta"), make(N).to("meta")
        out = torch.zeros(M, N, device="meta")
        ok = torch.zeros(N, NB, dtype=torch.uint8, device="meta")
        wide = torch.zeros(M, 2 ** 25, dtype=torch.uint8, device="meta")[:, :NB]
        with pytest.raises(ValueError, match="a_scale spans 2 GiB or more"):
            G.gemm(a, w, out, a_scale=wide, w_scale=ok, stream=0)
        with pytest.raises(ValueError, match="w_scale spans 2 GiB or more"):
            G.gemm(w, a, out.t().contiguous(), a_scale=ok, w_scale=wide, stream=0)
        assert rec.calls == []
        just = torch.zeros(M, 2 ** 25 - 8, dtype=torch.uint8, device="meta")[:, :NB]
        G.gemm(a, w, out, a_scale=just, w_scale=ok, stream=0)
        assert len(rec.calls) == 1 and rec.calls[0][22] == 2 ** 25 - 8
        rec.calls.clear()


@pytest.mark.parametrize("tile", ["auto", "256x128", "128x256", "128x128", "256x128w4"])
def test_accepted_fp8_tuple(rec, tile):
    a, w = _fp8(M, ld=K + 64), _fp8(N, ld=K + 128)
    s_a, s_w = _sc(M, ld=NB + 4), _sc(N, ld=NB + 8)
    out = torch.zeros(96, N + 32, dtype=torch.float16)[:, :N]
    got = G.gemm(a, w, out, tile=tile, mode="mx", stream=7, act="relu", c_grp=32, c_gstride=64,
                 a_scale=s_a, w_scale=s_w)
    assert got is out
    assert rec.calls == [(a.data_ptr(), w.data_ptr(), out.data_ptr(), K + 64, K + 128, N + 32,
                          M, N, K, G.DT_FP8, G.DT_F16, G.TILES[tile], G.MODES["mx"], 0, 0, 32, 64,
                          7, G.ACTS["relu"], 1, s_a.data_ptr(), s_w.data_ptr(), NB + 4, NB + 8)]


@pytest.mark.parametrize("tile", ["auto", "256x128", "128x256", "128x128", "256x128w4"])
def test_accepted_fp4_tuple(rec, tile):
    """K in elements, doubled strides, MODES['mx'] whatever the mode, ksplit 1, four scale
    arguments; a_grp = M is plain rows and goes in as 0."""
    a, w = _fp4(M, ld=K + 64), _fp4(N, ld=K + 128)
    s_a, s_w = _sc(M, ld=NB + 8), _sc(N, ld=NB + 16)
    out = torch.zeros(96, N + 32, dtype=torch.bfloat16)[:, :N]
    assert a.stride(0) == (K + 64) // 2
    got = G.gemm(a, w, out, tile=tile, mode="auto", stream=7, act="silu", c_grp=32, c_gstride=64,
                 a_grp=M, a_gstride=M, a_scale=s_a, w_scale=s_w)
    assert got is out
    assert rec.calls == [(a.data_ptr(), w.data_ptr(), out.data_ptr(), K + 64, K + 128, N + 32,
                          M, N, K, G.DT_FP4, G.DT_BF16, G.TILES[tile], G.MODES["mx"], 0, 0, 32, 64,
                          7, G.ACTS["silu"], 1, s_a.data_ptr(), s_w.data_ptr(), NB + 8, NB + 16)]
    # dense operands, default output (bf16), the defaults of everything else
    rec.calls.clear()
    a, w, s_a, s_w = _fp4(M), _fp4(N), _sc(M), _sc(N)
    out = G.gemm(a, w, stream=0, a_scale=s_a, w_scale=s_w)
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (M, N)
    assert rec.calls == [(a.data_ptr(), w.data_ptr(), out.data_ptr(), K, K, N, M, N, K, G.DT_FP4,
                          G.DT_BF16, 0, G.MODES["mx"], 0, 0, 0, 0, 0, 0, 1, s_a.data_ptr(),
                          s_w.data_ptr(), NB, NB)]


def test_fast_path_is_asked_with_the_byte_view(monkeypatch):
    """What gemm_fast_path_ok is asked: fp4 operands as byte matrices (K / 2, strides in bytes),
    fp8 ones as they are; a refusal there raises before the launch."""
    asked = []

    class R(_Recorder):
        def gemm_fast_path_ok(self, *args):
            asked.append(args)
            return False

    r = R()
    monkeypatch.setattr(G, "load", lambda: r)
    monkeypatch.setattr(G, "_check_operands", lambda *a, **k: None)
    out = torch.zeros(M, N, dtype=torch.float32)
    a, w = _fp4(M, ld=K + 64), _fp4(N)
    with pytest.raises(ValueError, match="the fp4 GEMM needs the MFMA fast path"):
        G.gemm(a, w, out, stream=0, a_scale=_sc(M), w_scale=_sc(N))
    a8, w8 = _fp8(M, ld=K + 64), _fp8(N)
    with pytest.raises(ValueError, match="block scales need the MFMA fast path"):
        G.gemm(a8, w8, out, stream=0, a_scale=_sc(M), w_scale=_sc(N))
    assert asked == [(a.data_ptr(), w.data_ptr(), out.data_ptr(), (K + 64) // 2, K // 2, N, M, N,
                      K // 2, G.DT_U8, G.DT_F32),
                     (a8.data_ptr(), w8.data_ptr(), out.data_ptr(), K + 64, K, N, M, N, K,
                      G.DT_FP8, G.DT_F32)]
    assert r.calls == []
