"""Skinny-M GEMM, gated / quantising epilogues, host side: every new refusal of ``_check_skinny``
on CPU tensors before the extension is loaded; the defaults return the tuple they always have."""

import pytest
import torch

from ddlb_amd.ops import gemm as G

FP8 = torch.float8_e4m3fn
M, K, E = 4, 512, 3


@pytest.fixture
def no_load(monkeypatch):
    def fail():
        raise AssertionError("load() reached before the refusal")
    monkeypatch.setattr(G, "load", fail)


@pytest.mark.parametrize("grouped", (False, True))
@pytest.mark.parametrize("fmt", ("mx", "mxfp4"))
def test_defaults_then_every_new_refusal(no_load, fmt, grouped):
    def call(f, N, *out, **new_kw):
        dt, kb = (FP8, K) if fmt == "mx" else (torch.float4_e2m1fn_x2, K // 2)
        wshape = (E, N) if grouped else (N,)
        args = (torch.zeros(M, kb, dtype=torch.uint8).view(dt),
                torch.zeros(*wshape, kb, dtype=torch.uint8).view(dt))
        args += (torch.tensor([0, 1, 1, 4], dtype=torch.int32),) if grouped else ()
        return f(*args, *out, **dict(
            new_kw, a_scale=torch.full((M, K // 32), 127, dtype=torch.uint8),
            w_scale=torch.full((*wshape, K // 32), 127, dtype=torch.uint8)))

    def bad(exc, match, N, *out, **new_kw):
        with pytest.raises(exc, match=match):
            call(G.gemm_skinny_grouped if grouped else G.gemm_skinny, N, *out, **new_kw)

    want = (M, 40, K, E if grouped else 0, torch.bfloat16, 2)
    assert call(G._check_skinny, 40, grouped=grouped, ksplit=2) == want
    assert call(G._check_skinny, 40, grouped=grouped, ksplit=2, glu=False, out_quant=None,
                out_scale=None) == want
    for N in (40, 96):
        bad(ValueError, "N % 64 == 0", N, glu=True)
    for q, mod in (("mx", 128), ("mxfp4", 256)):  # whole K-tiles of the reader, of N or N / 2
        bad(ValueError, f"N % {mod} == 0", mod // 2, out_quant=q)
        bad(ValueError, f"N % {2 * mod} == 0", mod, glu=True, out_quant=q)
    q = torch.zeros(M + 1, 512 + 32, dtype=torch.uint8).view(FP8)
    s = torch.zeros(M + 1, 16 + 8, dtype=torch.uint8)
    bad(ValueError, "out_quant must be None or one of", 512, out_quant="fp8")
    bad(ValueError, "out_scale goes with out_quant", 512, out_scale=s[:, :16])
    bad(TypeError, "writes", 512, out_quant="mx", out_dtype=torch.bfloat16)
    bad(TypeError, "out must be a", 512, torch.zeros(M, 512, dtype=torch.bfloat16), out_quant="mx")
    bad(TypeError, "out_scale must be a uint8", 512, out_quant="mx", out_scale=s.float())
    bad(ValueError, "out must have shape", 512, q[:, :512], glu=True, out_quant="mx")
    bad(ValueError, "out_scale must have shape", 512, glu=True, out_quant="mx",
        out_scale=s[:, :16])
    bad(ValueError, "out must have shape", 512, torch.zeros(M, 512, dtype=torch.bfloat16),
        glu=True)
    # pitches off the reading GEMM's alignment (a pitch shorter than F / 32 cannot be a view)
    bad(ValueError, "out_scale needs unit inner stride", 512, out_quant="mx",
        out_scale=torch.zeros(M, 18, dtype=torch.uint8)[:, :16])
    bad(ValueError, "out_scale must start at", 512, out_quant="mx", out_scale=s[:, 2:18])
    bad(ValueError, "out needs unit inner stride", 512, out_quant="mx",
        out=torch.zeros(M, 520, dtype=torch.uint8).view(FP8)[:, :512])
    # what is accepted reaches load(): views with larger, aligned pitches included
    bad(AssertionError, "load", 512, q[:, :256], glu=True, out_quant="mx", out_scale=s[:, :8])
