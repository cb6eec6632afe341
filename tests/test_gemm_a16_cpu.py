"""Tiled A16 GEMM, the host side (no GPU): the accepted case reaches ``load()``, every refusal of
``_check_a16`` is raised before it, and the models' ``kernel="a16"`` refusals."""

import pytest
import torch

from ddlb_amd.ops import gemm as G
from test_gemm_skinny_a16_cpu import BF16, KTILE, U8, _good
from test_gemm_skinny_cpu import E, FP8, K, M, N, no_load  # noqa: F401


@pytest.mark.parametrize("grouped", (False, True))
@pytest.mark.parametrize("dt", (BF16, torch.float16))
@pytest.mark.parametrize("wfmt", ("mxfp4", "mx"))
def test_accepted_then_every_refusal(no_load, wfmt, dt, grouped):
    a, w, rest, s = _good(wfmt, grouped, dt)
    assert G._check_a16(a, w, *rest, grouped=grouped, w_scale=s, tile="256x128") == (
        M, N, K, E if grouped else 0, dt)
    run = G.gemm_a16_grouped if grouped else G.gemm_a16

    def bad(exc, match, na, nw, **kw):
        with pytest.raises(exc, match=match):
            run(na, nw, *rest, **dict(dict(w_scale=s), **kw))

    bad(AssertionError, "load", a, w)
    bad(TypeError, "takes bf16 or f16 activations, not torch.float8_e4m3fn",
        torch.zeros(M, K, dtype=U8).view(FP8), w)                        # quantised a
    bad(TypeError, "16-bit weights stay with gemm", a, torch.zeros(w.shape[:-1] + (K,), dtype=dt))
    cut = KTILE[wfmt] // 2  # half a K-tile of the skinny kernel less: rows stay 16-byte aligned
    bad(ValueError, f"K % {KTILE[wfmt]} == 0", a[:, :-cut],
        w[..., :-(cut // 2 if wfmt == "mxfp4" else cut)], w_scale=s[..., :-(cut // 32)])
    bad(ValueError, "needs w_scale", a, w, w_scale=None)
    bad(ValueError, "w_scale must have shape", a, w, w_scale=s[..., :-1])
    off = torch.full((s.numel() + 2,), 127, dtype=U8)[2:].view(s.shape)
    assert off.data_ptr() % 4 == 2
    bad(ValueError, "4-byte-aligned base", a, w, w_scale=off)
    bad(ValueError, "offered for tile auto / .*not '128x256'", a, w, tile="128x256")
    bad(ValueError, "glu=True needs N % 64 == 0", a, w, glu=True)
    if grouped:
        with pytest.raises(TypeError, match="offsets must be an int32 tensor"):
            run(a, w, rest[0].long(), w_scale=s)


@pytest.mark.parametrize("fmt", ("mx", "w4a8"))
@pytest.mark.parametrize("model", ("MxMLP", "MxMoE"))
def test_models_refuse_other_formats(model, fmt):
    from ddlb_amd.models import mx_mlp, mx_moe

    cls, kw = (mx_mlp.MxMLP, {}) if model == "MxMLP" else (mx_moe.MxMoE, dict(experts=4))
    with pytest.raises(ValueError, match=f"kernel='a16' .* 'w8a16' only, not fmt='{fmt}'"):
        cls(hidden=256, ffn=256, seq=96, fmt=fmt, kernel="a16", **kw)
