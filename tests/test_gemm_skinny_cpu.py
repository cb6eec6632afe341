"""Skinny-M GEMM, the host side (no GPU): every refusal of ``gemm_skinny`` and
``gemm_skinny_grouped`` on CPU tensors, raised before the extension is loaded, and the launch
arithmetic (strips, slices, the automatic slice count, the workspace) against plain loops."""

import pytest
import torch

from ddlb_amd.ops import available, load
from ddlb_amd.ops import gemm as G

FP8 = torch.float8_e4m3fn
FP4 = torch.float4_e2m1fn_x2
M, N, K, E = 4, 40, 512, 3


def _good(fmt="mx", grouped=False):
    """Arguments the checks accept: ``(args, kw)``."""
    dt, kb = (FP8, K) if fmt == "mx" else (FP4, K // 2)
    wshape = (E, N) if grouped else (N,)
    a = torch.zeros(M, kb, dtype=torch.uint8).view(dt)
    w = torch.zeros(*wshape, kb, dtype=torch.uint8).view(dt)
    kw = dict(a_scale=torch.full((M, K // 32), 127, dtype=torch.uint8),
              w_scale=torch.full((*wshape, K // 32), 127, dtype=torch.uint8))
    offs = (torch.tensor([0, 1, 1, 4], dtype=torch.int32),) if grouped else ()
    return (a, w) + offs, kw


@pytest.fixture
def no_load(monkeypatch):
    def fail():
        raise AssertionError("load() reached before the refusal")
    monkeypatch.setattr(G, "load", fail)


def _refused(exc, match, grouped, args, kw):
    with pytest.raises(exc, match=match):
        (G.gemm_skinny_grouped if grouped else G.gemm_skinny)(*args, **kw)


@pytest.mark.parametrize("grouped", (False, True))
@pytest.mark.parametrize("fmt", ("mx", "mxfp4"))
def test_accepted_then_every_refusal(no_load, fmt, grouped):
    args, kw = _good(fmt, grouped)
    nk = K // (128 if fmt == "mx" else 256)
    t = G._check_skinny(*args, grouped=grouped, ksplit=nk, **kw)
    assert t == (M, N, K, E if grouped else 0, torch.bfloat16, nk)
    a, w = args[:2]
    rest = args[2:]

    def bad(exc, match, na, nw, *out, **new_kw):
        _refused(exc, match, grouped, (na, nw) + rest + out, dict(kw, **new_kw))

    bad(TypeError, "block-scaled fp8 or fp4 operands", a.view(torch.uint8).to(torch.bfloat16),
        w.view(torch.uint8).to(torch.bfloat16))
    bad(TypeError, "A dtype", a, w.view(torch.uint8).view(FP4 if fmt == "mx" else FP8))
    bad(ValueError, "needs a_scale and w_scale", a, w, a_scale=None)
    bad(ValueError, r"K % (128|256) == 0", a[:, :-16], w[..., :-16],
        a_scale=kw["a_scale"][:, :-1], w_scale=kw["w_scale"][..., :-1])
    bad(ValueError, "a_scale must have shape", a, w, a_scale=kw["a_scale"][:, :-1])
    bad(TypeError, "a_scale must be a uint8 tensor", a, w, a_scale=kw["a_scale"].float())
    shifted = torch.zeros(a.numel() + 8, dtype=torch.uint8)[8:].view(a.shape).view(a.dtype)
    bad(ValueError, "16-byte-aligned rows of a", shifted, w)
    for ks in (0, nk + 1, True, 2.0, "all"):
        bad(ValueError, "ksplit must be 'auto' or an int", a, w, ksplit=ks)
    bad(TypeError, "workspace must be a float32 tensor", a, w, ksplit=2,
        workspace=torch.zeros(2 * M * N, dtype=torch.float64))
    bad(ValueError, "hold at least", a, w, ksplit=2, workspace=torch.zeros(2 * M * N - 1))
    bad(ValueError, "unknown activation", a, w, act="tanh")
    bad(TypeError, "writes one of", a, w, out_dtype=torch.float64)
    bad(ValueError, "out must have shape", a, w, torch.zeros(M, N + 1, dtype=torch.bfloat16))
    if grouped:
        offs = rest[0]
        for o in (offs.long(), [0, 1, 1, 4]):
            _refused(TypeError, "offsets must be an int32 tensor", True, (a, w, o), kw)
        _refused(ValueError, "offsets must be contiguous with shape", True, (a, w, offs[:3]), kw)
        _refused(ValueError, "offsets is on meta", True, (a, w, offs.to("meta")), kw)
        big = torch.zeros(G.MAX_GROUPS + 1, 1, 1, dtype=torch.uint8).view(a.dtype)
        _refused(ValueError, "takes 1 .. 1024 groups", True,
                 (a, big.expand(-1, N, a.shape[1]), offs), kw)
        _refused(ValueError, "w_scale must have shape", True, (a, w, offs),
                 dict(kw, w_scale=kw["w_scale"][0]))
    # what is accepted reaches load(), and nothing before it refuses
    with pytest.raises(AssertionError, match="load"):
        (G.gemm_skinny_grouped if grouped else G.gemm_skinny)(*args, **kw)


@pytest.mark.parametrize("N,nk,groups,cus", [(4096, 32, 1, 256), (8192, 64, 1, 256),
                                             (152, 5, 1, 256), (3072, 16, 32, 256),
                                             (1, 1, 1, 304), (40000, 3, 2, 64)])
def test_launch_arithmetic(N, nk, groups, cus):
    strips = G.skinny_strips(N)
    assert (strips - 1) * G.SKINNY_STRIP < N <= strips * G.SKINNY_STRIP
    cap = min(nk, 16)
    fits = [S for S in range(1, cap + 1) if strips * S * groups >= 2 * cus]
    S = G.skinny_auto_slices(strips, nk, groups, cus)
    assert S == (fits[0] if fits else cap)
    for S in {1, S, nk}:
        sl = G.skinny_slices(nk, S)
        assert sl[0][0] == 0 and sl[-1][1] == nk and all(k1 > k0 for k0, k1 in sl)
        assert all(sl[i][1] == sl[i + 1][0] for i in range(S - 1))
        assert G.skinny_workspace_floats(S, 7, N) == (S * 7 * N if S > 1 else 0)
    if available():  # gemm_skinny.h's own numbers, where the extension is built
        assert load().skinny_plan(N, nk, groups, cus) == (
            strips, G.skinny_auto_slices(strips, nk, groups, cus))
