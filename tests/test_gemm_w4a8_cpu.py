"""Tiled W4A8 GEMM, the host side (no GPU): the accepted case reaches ``load()``, every refusal of
``_check_w4a8`` is raised before it, and the models' ``kernel=`` refusals."""

import pytest
import torch

from ddlb_amd.ops import gemm as G
from test_gemm_skinny_cpu import E, FP4, FP8, K, M, N, no_load  # noqa: F401

N64 = 64


@pytest.mark.parametrize("grouped", (False, True))
def test_accepted_then_every_refusal(no_load, grouped):
    wshape = (E, N64) if grouped else (N64,)
    a = torch.zeros(M, K, dtype=torch.uint8).view(FP8)
    w = torch.zeros(*wshape, K // 2, dtype=torch.uint8).view(FP4)
    kw = dict(a_scale=torch.full((M, K // 32), 127, dtype=torch.uint8),
              w_scale=torch.full((*wshape, K // 32), 127, dtype=torch.uint8))
    rest = (torch.tensor([0, 1, 1, 4], dtype=torch.int32),) if grouped else ()
    fn = G.gemm_w4a8_grouped if grouped else G.gemm_w4a8
    assert G._check_w4a8(a, w, *rest, grouped=grouped, glu=True, out_quant=None, **kw) == (
        M, N64, K, E if grouped else 0, torch.bfloat16)

    def bad(exc, match, na, nw, **new_kw):
        with pytest.raises(exc, match=match):
            fn(na, nw, *rest, **dict(kw, **new_kw))

    bad(AssertionError, "load", a, w)
    bad(TypeError, "float8_e4m3fn a on float4_e2m1fn_x2 w", a.view(torch.uint8).view(FP4),
        w.view(torch.uint8).view(FP8))                                   # the dtypes swapped
    bad(ValueError, "W4A8 GEMM needs K % 256 == 0", a[:, :-128], w[..., :-64],
        a_scale=kw["a_scale"][:, :-4], w_scale=kw["w_scale"][..., :-4])
    bad(ValueError, "a_scale must have shape", a, w, a_scale=kw["a_scale"][:, :-1])
    bad(ValueError, "w_scale must have shape", a, w, w_scale=kw["w_scale"][..., :-1, :])
    s = torch.full((kw["a_scale"].numel() + 2,), 127, dtype=torch.uint8)[2:].view(M, K // 32)
    bad(ValueError, "a_scale must start at a 4-byte-aligned", a, w, a_scale=s)
    bad(ValueError, "no out_quant='mxfp4'", a, w, out_quant="mxfp4")
    bad(ValueError, r"glu=True, out_quant=None needs N % 64 == 0", a, w[..., :40, :],
        w_scale=kw["w_scale"][..., :40, :], glu=True)
    bad(ValueError, r"out_quant='mx' needs N % 128 == 0", a, w, out_quant="mx")
    bad(ValueError, "offered for tile auto / .*not '128x256'", a, w, tile="128x256")
    if grouped:
        with pytest.raises(TypeError, match="offsets must be an int32 tensor"):
            fn(a, w, rest[0].long(), **kw)


@pytest.mark.parametrize("model", ("MxMLP", "MxMoE"))
def test_model_kernel_refusals(model):
    from ddlb_amd.models import mx_mlp, mx_moe

    cls, kw = (mx_mlp.MxMLP, {}) if model == "MxMLP" else (mx_moe.MxMoE, dict(experts=4))
    with pytest.raises(ValueError, match="kernel='mixed' .* takes fmt='w4a8' only, not fmt='mx'"):
        cls(hidden=256, ffn=256, seq=96, fmt="mx", kernel="mixed", **kw)
    with pytest.raises(ValueError, match="needs kernel='skinny': only the skinny GEMM"):
        cls(hidden=256, ffn=256, seq=96, fmt="w4a8", kernel="tiled", **kw)
