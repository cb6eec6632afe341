"""Skinny-M GEMM for bf16 / f16 activations, the host side (no GPU): the three weight forms reach
``load()``, every refusal is raised before it, and the models refuse the tiled kernel."""

import pytest
import torch

from ddlb_amd.ops import gemm as G
from test_gemm_skinny_cpu import E, FP4, FP8, K, M, N, no_load  # noqa: F401

BF16, U8 = torch.bfloat16, torch.uint8
KTILE = {"mxfp4": 256, "mx": 128, "same": 64}


def _good(wfmt, grouped, dt=BF16):
    wshape = (E, N) if grouped else (N,)
    a = torch.zeros(M, K, dtype=dt)
    w = {"mxfp4": lambda: torch.zeros(*wshape, K // 2, dtype=U8).view(FP4),
         "mx": lambda: torch.zeros(*wshape, K, dtype=U8).view(FP8),
         "same": lambda: torch.zeros(*wshape, K, dtype=dt)}[wfmt]()
    s = None if wfmt == "same" else torch.full((*wshape, K // 32), 127, dtype=U8)
    rest = (torch.tensor([0, 1, 1, 4], dtype=torch.int32),) if grouped else ()
    return a, w, rest, s


@pytest.mark.parametrize("grouped", (False, True))
@pytest.mark.parametrize("dt", (BF16, torch.float16))
@pytest.mark.parametrize("wfmt", tuple(KTILE))
def test_accepted_then_every_refusal(no_load, wfmt, dt, grouped):
    a, w, rest, s = _good(wfmt, grouped, dt)
    nk = K // KTILE[wfmt]
    assert G._check_skinny_a16(a, w, *rest, grouped=grouped, ksplit=nk, w_scale=s) == (
        M, N, K, E if grouped else 0, dt, nk)
    run = G.gemm_skinny_a16_grouped if grouped else G.gemm_skinny_a16

    def bad(exc, match, na, nw, *out, **kw):
        with pytest.raises(exc, match=match):
            run(na, nw, *rest, *out, **dict(dict(w_scale=s), **kw))

    bad(AssertionError, "load", a, w)
    bad(TypeError, "takes bf16 or f16 activations", a.float(), w)
    bad(TypeError, "takes w as", a, torch.zeros(w.shape[:-1] + (K,), dtype=torch.float32),
        w_scale=None)
    other = torch.float16 if dt == BF16 else BF16
    bad(TypeError, "takes w as", a, torch.zeros(w.shape[:-1] + (K,), dtype=other), w_scale=None)
    bad(ValueError, "K mismatch", a[:, :K // 2], w)
    bad(ValueError, "needs w_scale for MX weights and only for them", a, w,
        w_scale=torch.full((*w.shape[:-1], K // 32), 127, dtype=U8) if s is None else None)
    cut = KTILE[wfmt] // 2  # half a K-tile less: rows stay 16-byte aligned
    bad(ValueError, f"K % {KTILE[wfmt]} == 0", a[:, :-cut],
        w[..., :-(cut // 2 if wfmt == "mxfp4" else cut)],
        w_scale=None if s is None else s[..., :-(cut // 32)])
    shifted = torch.zeros(a.numel() + 4, dtype=dt)[4:].view(a.shape)
    bad(ValueError, "16-byte-aligned rows of a", shifted, w)
    bad(ValueError, "glu=True needs N % 64 == 0", a, w, glu=True)
    for ks in (0, nk + 1, True, 2.0, "all"):
        bad(ValueError, "ksplit must be 'auto' or an int", a, w, ksplit=ks)
    bad(TypeError, "workspace must be a float32 tensor", a, w, ksplit=2,
        workspace=torch.zeros(2 * M * N, dtype=torch.float64))
    bad(ValueError, "hold at least", a, w, ksplit=2, workspace=torch.zeros(2 * M * N - 1))
    bad(ValueError, "unknown activation", a, w, act="tanh")
    bad(TypeError, "writes one of", a, w, out_dtype=other)
    bad(ValueError, "out must have shape", a, w, torch.zeros(M, N + 1, dtype=dt))
    if s is not None:
        al = 8 if wfmt == "mxfp4" else 4
        off = torch.full((s.numel() + al // 2,), 127, dtype=U8)[al // 2:].view(s.shape)
        assert off.data_ptr() % al == al // 2
        bad(ValueError, f"{al}-byte-aligned base", a, w, w_scale=off)
        bad(ValueError, "w_scale must have shape", a, w, w_scale=s[..., :-1])
        bad(TypeError, "w_scale must be a uint8 tensor", a, w, w_scale=s.float())
    if grouped:
        with pytest.raises(ValueError, match="offsets must be contiguous with shape"):
            run(a, w, rest[0][:-1], w_scale=s)


@pytest.mark.parametrize("fmt", ("w4a16", "w8a16"))
@pytest.mark.parametrize("model", ("MxMLP", "MxMoE"))
def test_models_refuse_the_tiled_kernel(model, fmt):
    from ddlb_amd.models import mx_mlp, mx_moe

    cls, kw = (mx_mlp.MxMLP, {}) if model == "MxMLP" else (mx_moe.MxMoE, dict(experts=4))
    with pytest.raises(ValueError, match="needs kernel='skinny'"):
        cls(hidden=256, ffn=256, seq=8, fmt=fmt, kernel="tiled", **kw)
