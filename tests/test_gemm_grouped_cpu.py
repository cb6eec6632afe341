"""Grouped GEMM, the host side (no GPU): every refusal of ``ops.gemm._check_grouped`` on CPU
tensors, one perturbation at a time and each with its own message; ``grouped_reference`` against
a hand-written loop; the ``pack_glu_grouped`` round trip; ``MxMoE.reference_chain`` against the
per-expert chain; the build's copy of the tiled kernel's body for the grouped kernel."""

import pytest
import torch

from ddlb_amd.ops import gemm as G

FP8 = torch.float8_e4m3fn
FP4 = getattr(torch, "float4_e2m1fn_x2", None)
T, N, K, E = 40, 256, 256, 3


def _good(form="bf16"):
    """Arguments ``_check_grouped`` accepts: ``(a, w, offsets, kw)``."""
    offs = torch.tensor([0, 10, 10, 40], dtype=torch.int32)
    if form in ("bf16", "f16"):
        dt = torch.bfloat16 if form == "bf16" else torch.float16
        return torch.zeros(T, K, dtype=dt), torch.zeros(E, N, K, dtype=dt), offs, {}
    if form == "mxfp8":
        a, w = torch.zeros(T, K, dtype=torch.uint8).view(FP8), \
            torch.zeros(E, N, K, dtype=torch.uint8).view(FP8)
    else:
        a, w = torch.zeros(T, K // 2, dtype=torch.uint8).view(FP4), \
            torch.zeros(E, N, K // 2, dtype=torch.uint8).view(FP4)
    kw = dict(a_scale=torch.full((T, K // 32), 127, dtype=torch.uint8),
              w_scale=torch.full((E, N, K // 32), 127, dtype=torch.uint8))
    return a, w, offs, kw


FORMS = ("bf16", "f16", "mxfp8") + (("mxfp4",) if FP4 is not None else ())


@pytest.mark.parametrize("form", FORMS)
def test_accepted_forms(form):
    a, w, offs, kw = _good(form)
    dense0 = torch.float16 if form == "f16" else torch.bfloat16
    assert G._check_grouped(a, w, offs, **kw) == (T, N, K, E, dense0)
    assert G._check_grouped(a, w, offs, out_dtype=torch.float32, act="relu", **kw)[4] == \
        torch.float32
    for tile in G.SCALED_TILES:
        G._check_grouped(a, w, offs, tile=tile, **kw)
    assert G._check_grouped(a, w, offs, glu=True, act="silu", **kw)[4] == dense0
    assert G._check_grouped(a, w, offs, out_quant="mx", **kw)[4] == FP8
    assert G._check_grouped(a, w, offs, glu=True, out_quant="mx", **kw)[4] == FP8
    # outputs, where given: [>= T, columns]
    G._check_grouped(a, w, offs, torch.zeros(T + 3, N, dtype=torch.float32), **kw)
    G._check_grouped(a, w, offs, torch.zeros(T, N // 2, dtype=dense0), glu=True, **kw)
    # any expert stride of at least N rows, the scales' likewise
    wide = torch.zeros(E, N + 4, w.shape[2], dtype=torch.uint8).view(w.dtype) \
        if w.element_size() == 1 else torch.zeros(E, N + 4, K, dtype=w.dtype)
    kw2 = dict(kw)
    if kw:
        kw2["w_scale"] = torch.full((E, N + 4, K // 32), 127, dtype=torch.uint8)[:, :N]
    G._check_grouped(a, wide[:, :N], offs, **kw2)


def _raises(exc, match, *args, **kw):
    with pytest.raises(exc, match=match):
        G._check_grouped(*args, **kw)


def test_offsets_refusals():
    a, w, offs, _ = _good()
    _raises(TypeError, "offsets must be an int32 tensor", a, w, offs.to(torch.int64))
    _raises(TypeError, "offsets must be an int32 tensor", a, w, [0, 10, 10, 40])
    _raises(ValueError, r"offsets must be contiguous with shape \(4,\)", a, w, offs[:3])
    _raises(ValueError, r"offsets must be contiguous with shape \(4,\)", a, w,
            torch.zeros(5, dtype=torch.int32))
    _raises(ValueError, r"offsets must be contiguous with shape \(4,\)", a, w,
            offs.reshape(2, 2))
    _raises(ValueError, r"offsets must be contiguous with shape \(4,\)", a, w,
            torch.zeros(8, dtype=torch.int32)[::2])
    _raises(ValueError, "offsets is on meta, the operands on cpu", a, w, offs.to("meta"))


def test_weight_refusals():
    a, w, offs, _ = _good()
    _raises(ValueError, r"takes w as \[E, N, K\] \(3-D\)", a, w[0], offs)
    _raises(ValueError, r"takes a as \[T, K\] \(2-D\)", a[None], w, offs)
    big = torch.zeros(1, 64, K, dtype=torch.bfloat16).expand(1025, 64, K)
    _raises(ValueError, "at most 1024 groups, not 1025", a, big,
            torch.zeros(1026, dtype=torch.int32))
    _raises(ValueError, "at least one group", a, w[:0], torch.zeros(1, dtype=torch.int32))
    _raises(ValueError, "experts at least N rows apart", a,
            torch.zeros(E, N // 2, K, dtype=torch.bfloat16)[:, None].expand(E, 2, N // 2, K)
            .reshape(E, N, K).as_strided((E, N, K), (N * K // 2, K, 1)), offs)
    _raises(ValueError, "unit inner stride", a,
            torch.zeros(E, N, 2 * K, dtype=torch.bfloat16)[:, :, ::2], offs)
    _raises(ValueError, "K mismatch", a, torch.zeros(E, N, 2 * K, dtype=torch.bfloat16), offs)
    _raises(TypeError, "A dtype torch.bfloat16 != W dtype torch.float16", a, w.to(torch.float16),
            offs)
    _raises(TypeError, "takes bf16, f16, scaled fp8 or scaled fp4 operands, not torch.float32",
            a.float(), w.float(), offs)
    _raises(TypeError, "takes bf16, f16, scaled fp8 or scaled fp4 operands, not torch.float64",
            a.double(), w.double(), offs)
    _raises(TypeError, "block scales need fp8 / fp4 operands", a, w, offs,
            a_scale=torch.zeros(T, K // 32, dtype=torch.uint8),
            w_scale=torch.zeros(E, N, K // 32, dtype=torch.uint8))


def test_tile_refusals():
    a, w, offs, _ = _good()
    for tile in ("pt4", "t4", "pt8", "t8", "256x256", "256x256w4", "i256", "i128", "i256w4"):
        _raises(ValueError, "a grouped GEMM is offered for tile auto", a, w, offs, tile=tile)
    _raises(ValueError, "unknown activation", a, w, offs, act="tanh")


def test_scale_refusals():
    a, w, offs, kw = _good("mxfp8")
    a8u, w8u = a, w
    _raises(ValueError, "needs a_scale and w_scale", a8u, w8u, offs)          # unit-scale fp8
    _raises(ValueError, "needs a_scale and w_scale", a8u, w8u, offs, a_scale=kw["a_scale"])
    _raises(ValueError, r"w_scale must have shape \(3, 256, 8\)", a, w, offs,
            a_scale=kw["a_scale"], w_scale=kw["w_scale"][0])
    _raises(ValueError, r"w_scale must have shape \(3, 256, 8\)", a, w, offs,
            a_scale=kw["a_scale"], w_scale=kw["w_scale"][:, :, :4])
    _raises(ValueError, r"a_scale must have shape \(40, 8\)", a, w, offs,
            a_scale=kw["a_scale"][:, :4], w_scale=kw["w_scale"])
    _raises(ValueError, r"a_scale must have shape \(40, 8\)", a, w, offs,
            a_scale=kw["a_scale"][:30], w_scale=kw["w_scale"])
    _raises(TypeError, "a_scale must be a uint8 tensor", a, w, offs,
            a_scale=kw["a_scale"].to(torch.int8), w_scale=kw["w_scale"])
    odd = torch.full((E, N * (K // 32) + 2), 127, dtype=torch.uint8)[:, :N * (K // 32)] \
        .unflatten(1, (N, K // 32))
    assert odd.stride(0) % 4 == 2
    _raises(ValueError, "w_scale needs experts a multiple of 4 bytes", a, w, offs,
            a_scale=kw["a_scale"], w_scale=odd)


def test_epilogue_refusals():
    a, w, offs, _ = _good()
    w96 = torch.zeros(E, 96, K, dtype=torch.bfloat16)
    _raises(ValueError, r"glu with out_quant=None needs N % 64 == 0 \(N = 96\)", a, w96, offs,
            glu=True)
    w128 = torch.zeros(E, 128, K, dtype=torch.bfloat16)
    _raises(ValueError, r"out_quant='mx' needs N % 128 == 0 \(N = 96\)", a, w96, offs,
            out_quant="mx")
    _raises(ValueError, r"out_quant='mxfp4' needs N % 256 == 0 \(N = 128\)", a, w128, offs,
            out_quant="mxfp4")
    _raises(ValueError, r"glu with out_quant='mx' needs N % 256 == 0 \(N = 128\)", a, w128, offs,
            glu=True, out_quant="mx")
    _raises(ValueError, r"glu with out_quant='mxfp4' needs N % 512 == 0 \(N = 256\)", a, w, offs,
            glu=True, out_quant="mxfp4")
    _raises(ValueError, "out_quant must be None or one of", a, w, offs, out_quant="int8")
    _raises(ValueError, "out_scale goes with out_quant", a, w, offs,
            out_scale=torch.zeros(T, N // 32, dtype=torch.uint8))
    _raises(TypeError, "writes one of", a, w, offs, out_dtype=torch.float16)
    _raises(ValueError, r"out must have shape \(>= 40, 256\)", a, w, offs,
            torch.zeros(T - 1, N, dtype=torch.bfloat16))
    _raises(ValueError, r"out must have shape \(>= 40, 128\)", a, w, offs,
            torch.zeros(T, N, dtype=torch.bfloat16), glu=True)


def test_gemm_grouped_refuses_before_the_extension_loads(monkeypatch):
    """``gemm_grouped`` runs ``_check_grouped`` first: a refusal never reaches ``load()``."""
    def no_load():
        raise AssertionError("the extension was loaded before the checks")

    monkeypatch.setattr(G, "load", no_load)
    a, w, offs, _ = _good()
    with pytest.raises(ValueError, match="a grouped GEMM is offered for tile auto"):
        G.gemm_grouped(a, w, offs, tile="pt4")
    with pytest.raises(TypeError, match="offsets must be an int32 tensor"):
        G.gemm_grouped(a, w, offs.long())


def test_grouped_reference_against_a_hand_written_loop():
    g = torch.Generator().manual_seed(5)
    a = torch.randint(-3, 4, (23, 16), generator=g).float()
    w = torch.randint(-3, 4, (4, 6, 16), generator=g).float()
    for raw, clamped in (([0, 5, 5, 20, 23], [0, 5, 5, 20, 23]),
                         ([2, 9, 4, 30, 11], [2, 9, 9, 23, 23]),
                         ([-4, 0, 0, 0, 0], [0, 0, 0, 0, 0]),
                         ([40, 1, 2, 3, 4], [23, 23, 23, 23, 23])):
        offs = torch.tensor(raw, dtype=torch.int32)
        assert G.clamp_offsets(offs, 23) == clamped
        want = torch.zeros(23, 6)
        for e in range(4):
            for i in range(clamped[e], clamped[e + 1]):
                for n in range(6):
                    want[i, n] = sum(float(a[i, k]) * float(w[e, n, k]) for k in range(16))
        got = G.grouped_reference(a.to(torch.bfloat16), w.to(torch.bfloat16), offs)
        assert got.dtype == torch.float32 and torch.equal(got, want), raw
    with pytest.raises(ValueError, match="offsets must have shape"):
        G.grouped_reference(a, w, torch.zeros(4, dtype=torch.int32))


def test_pack_glu_grouped_round_trip():
    g = torch.Generator().manual_seed(6)
    gate = torch.randn(3, 64, 32, generator=g)
    up = torch.randn(3, 64, 32, generator=g)
    p = G.pack_glu_grouped(gate, up)
    assert tuple(p.shape) == (3, 128, 32)
    for e in range(3):
        assert torch.equal(p[e], G.pack_glu(gate[e], up[e]))
        ge, ue = G.unpack_glu(p[e])
        assert torch.equal(ge, gate[e]) and torch.equal(ue, up[e])
    # one-byte dtypes pack as bytes; scales (uint8) too
    q = (gate * 8).to(FP8)
    pq = G.pack_glu_grouped(q, (up * 8).to(FP8))
    assert pq.dtype == FP8 and torch.equal(pq[1].view(torch.uint8),
                                           G.pack_glu(q[1], (up * 8).to(FP8)[1]).view(torch.uint8))
    # 2-D behaviour of pack_glu is what it was
    with pytest.raises(ValueError, match="pack_glu takes two 2-D tensors"):
        G.pack_glu(gate, up)
    with pytest.raises(ValueError, match="pack_glu_grouped takes two 3-D tensors"):
        G.pack_glu_grouped(gate[0], up[0])
    with pytest.raises(ValueError, match="F % 32 == 0"):
        G.pack_glu_grouped(gate[:, :48], up[:, :48])


@pytest.mark.parametrize("fmt", ("mx", "mxfp4"))
def test_mx_moe_reference_equals_the_per_expert_chain(fmt):
    from ddlb_amd.models.mx_mlp import MxMLP
    from ddlb_amd.models.mx_moe import MxMoE, expert_ids

    if fmt == "mxfp4" and FP4 is None:
        pytest.skip("torch has no float4_e2m1fn_x2")
    S, H, F, experts = 48, 256, 256, 5
    ids = expert_ids(S, experts, seed=3)
    counts = torch.bincount(ids, minlength=experts)
    assert ids.dtype == torch.int64 and int(counts.sum()) == S
    assert int(counts[experts // 2]) == 0 and len(set(counts.tolist())) > 2
    assert torch.equal(ids, expert_ids(S, experts, seed=3))
    g = torch.Generator().manual_seed(9)
    X = (torch.rand(S, H, generator=g) * 2 - 1).to(torch.bfloat16)
    gate, up = ((torch.rand(experts, F, H, generator=g) * 2 - 1).mul(H ** -0.5)
                .to(torch.bfloat16) for _ in range(2))
    W1 = G.pack_glu_grouped(gate, up)
    W2 = ((torch.rand(experts, H, F, generator=g) * 2 - 1) * F ** -0.5).to(torch.bfloat16)
    got = MxMoE.reference_chain(X, W1, W2, ids, "silu", fmt)
    assert tuple(got.shape) == (S, H) and got.dtype == torch.float32
    seen = torch.zeros(S, dtype=torch.bool)
    for e in range(experts):  # expert by expert: its chain on its own rows, in token order
        mask = ids == e
        if not bool(mask.any()):
            continue
        want = MxMLP.reference_chain(X[mask], W1[e], W2[e], "silu", fmt, gated=True)
        assert torch.equal(got[mask], want), e
        seen |= mask
    assert bool(seen.all()) and float(got.abs().max()) > 0
