"""Skinny-M GEMM, MX-fp8 ``a`` on MXFP4 ``w`` (W4A8), the host side (no GPU): the accepted case
reaches ``load()``, each new refusal is raised before it, and the models refuse the tiled kernel."""

import pytest
import torch

from ddlb_amd.ops import gemm as G
from test_gemm_skinny_cpu import E, FP4, FP8, K, M, N, _refused, no_load  # noqa: F401


@pytest.mark.parametrize("grouped", (False, True))
def test_accepted_then_every_new_refusal(no_load, grouped):
    wshape = (E, N) if grouped else (N,)
    a = torch.zeros(M, K, dtype=torch.uint8).view(FP8)
    w = torch.zeros(*wshape, K // 2, dtype=torch.uint8).view(FP4)
    kw = dict(a_scale=torch.full((M, K // 32), 127, dtype=torch.uint8),
              w_scale=torch.full((*wshape, K // 32), 127, dtype=torch.uint8))
    rest = (torch.tensor([0, 1, 1, 4], dtype=torch.int32),) if grouped else ()
    nk = K // 256  # K-tiles are w's
    assert G._check_skinny(a, w, *rest, grouped=grouped, ksplit=nk, **kw) == (
        M, N, K, E if grouped else 0, torch.bfloat16, nk)

    def bad(exc, match, na, nw, **new_kw):
        _refused(exc, match, grouped, (na, nw) + rest, dict(kw, **new_kw))

    bad(ValueError, "fp8 x fp4 skinny GEMM needs K % 256 == 0", a[:, :-128], w[..., :-64],
        a_scale=kw["a_scale"][:, :-4], w_scale=kw["w_scale"][..., :-4])
    # a_scale may sit on a 4-byte boundary (the fp8 rule: load() is reached), w_scale may not
    for name, exc, match in (("a_scale", AssertionError, "load"),
                             ("w_scale", ValueError, "w_scale must start at an 8-byte-aligned")):
        s = torch.full((kw[name].numel() + 4,), 127, dtype=torch.uint8)[4:].view(kw[name].shape)
        assert s.data_ptr() % 8 == 4
        bad(exc, match, a, w, **{name: s})
    bad(ValueError, "a_scale must have shape", a, w, a_scale=kw["a_scale"][:, :-1])
    bad(TypeError, "A dtype", a.view(torch.uint8)[:, :K // 2].view(FP4),
        w.view(torch.uint8).view(FP8))                                   # fp4 a on fp8 w
    bad(TypeError, "A dtype", a[:, :K // 2], w)                          # fp8 a, K mismatch
    bad(AssertionError, "load", a, w)


@pytest.mark.parametrize("model", ("MxMLP", "MxMoE"))
def test_models_refuse_the_tiled_kernel(model):
    from ddlb_amd.models import mx_mlp, mx_moe

    cls, kw = (mx_mlp.MxMLP, {}) if model == "MxMLP" else (mx_moe.MxMoE, dict(experts=4))
    with pytest.raises(ValueError, match="needs kernel='skinny': only the skinny GEMM"):
        cls(hidden=256, ffn=256, seq=8, fmt="w4a8", kernel="tiled", **kw)
