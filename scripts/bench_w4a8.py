"""Microbenchmark: the tiled W4A8 GEMM (MX-fp8 activations on MXFP4 weights) beside the tiled
kernel on MX-fp8 x MX-fp8 (the same MFMA rate, twice the W bytes) and on MXFP4 x MXFP4.

In ONE process, alternating per shape, all three on the same tile code:

* dense ``(N, K)`` in (4096, 4096), (8192, 8192) with ``M`` in 512, 2048, 8192;
* the gated fc1 with ``out_quant="mx"`` (``N = 2 x 4096``, ``K = 4096``, the same ``M``) against
  the fp8 tiled form of the same call;
* ``gemm_w4a8_grouped`` against ``gemm_grouped`` (fp8) at E = 32 experts, top-4, H = 4096,
  F = 1536 (the fc1 and fc2 shapes), 4096 and 16384 tokens.

Before anything is timed the W4A8 output is compared with the product of the dequantised operands
(``atol = 1e-3 K``). Every shape is warmed; device events surround ``iters`` back-to-back calls;
variants alternate over ``rounds`` rounds and the median, minimum and round-to-round spread are
reported, with the FLOP/s the shape's ``2 M N K`` gives. ``--tiles`` lists the tile codes (default:
both the W4A8 kernel offers, and ``auto`` for it alone).

    python scripts/bench_w4a8.py --json out/w4a8.json
"""

from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_skinny import summarise, timeit  # noqa: E402

DENSE_MS = (512, 2048, 8192)
DENSE_NK = ((4096, 4096), (8192, 8192))
MOE = dict(E=32, top_k=4, H=4096, F=1536, tokens=(4096, 16384))


def _quant(shape, fmt, gen, scale=1.0):
    import torch

    from ddlb_amd.models.mx_mlp import _fmt_ops

    x = torch.randn(shape, generator=gen, device=gen.device, dtype=torch.bfloat16) * scale
    return x, _fmt_ops(fmt)[0](x)


def _measure(variants, flops, iters, rounds):
    ts = {k: [] for k in variants}
    for fn in variants.values():
        timeit(fn, 2, 2)
    for _ in range(rounds):
        for k, fn in variants.items():
            ts[k].append(timeit(fn, iters, 1))
    out = {k: summarise(v) for k, v in ts.items()}
    for k in out:
        out[k]["flops_per_s"] = flops / (out[k]["ms_median"] * 1e-3)
    for k in variants:
        if k != "w4a8":
            out[f"w4a8_over_{k}"] = out["w4a8"]["ms_median"] / out[k]["ms_median"]
    return out


def bench(kind, M, N, K, tile, iters, rounds, gen, tokens=0, layer=""):
    """One shape: ``kind`` dense / fc1q (gated, quantised output) / grouped."""
    import torch

    from ddlb_amd.ops import gemm as G
    from ddlb_amd.ops import mx

    E = MOE["E"] if kind == "grouped" else 1
    x, (a8, sa8) = _quant((M, K), "mx", gen)
    a4, sa4 = mx.quantize_mxfp4(x)
    wf, (w8, sw8) = _quant((E * N, K), "mx", gen, K ** -0.5)
    w4, sw4 = mx.quantize_mxfp4(wf)
    pre = ()
    if kind == "grouped":
        counts = torch.bincount(torch.randint(0, E, (M,), generator=gen, device=gen.device),
                                minlength=E)
        offs = torch.zeros(E + 1, dtype=torch.int32, device=gen.device)
        offs[1:] = torch.cumsum(counts, 0)
        w8, sw8, w4, sw4 = (t.reshape(E, N, -1) for t in (w8, sw8, w4, sw4))
        pre = (offs,)
    fw, ft = (G.gemm_w4a8_grouped, G.gemm_grouped) if kind == "grouped" else (G.gemm_w4a8, G.gemm)
    kw = dict(act="silu", glu=True, out_quant="mx") if kind == "fc1q" else {}
    ttile = "256x128" if tile == "auto" else tile  # the tiled kernel beside `auto`: 256x128
    variants = {
        "w4a8": lambda: fw(a8, w4, *pre, a_scale=sa8, w_scale=sw4, tile=tile, **kw),
        "fp8": lambda: ft(a8, w8, *pre, a_scale=sa8, w_scale=sw8, tile=ttile, **kw)}
    if kind == "dense":
        variants["fp4"] = lambda: ft(a4, w4, a_scale=sa4, w_scale=sw4, tile=ttile)
        got = variants["w4a8"]()
        ref = mx.dequantize_mx(a8, sa8) @ mx.dequantize_mxfp4(w4, sw4).t()
        torch.testing.assert_close(got.float(), ref, rtol=2.0 ** -7, atol=1e-3 * K)
    r = _measure(variants, 2.0 * M * N * K, iters, rounds)
    r.update(kind=kind, M=M, N=N, K=K, tile=tile, tokens=tokens, layer=layer)
    return r


def show(r):
    what = f"moe {r['layer']} tok={r['tokens']}" if r["kind"] == "grouped" else f"{r['kind']}"
    line = f"{what:18s} M={r['M']:<6d} N={r['N']:<5d} K={r['K']:<5d} {r['tile']:8s}"
    for k in ("w4a8", "fp8", "fp4"):
        if k in r:
            v = r[k]
            line += (f" | {k} {v['ms_median'] * 1e3:8.1f} us (spread {100 * v['spread']:.1f} %) "
                     f"{v['flops_per_s'] / 1e12:6.0f} TF/s")
    for k in ("fp8", "fp4"):
        if f"w4a8_over_{k}" in r:
            line += f" | w4a8 / {k} {r[f'w4a8_over_{k}']:.3f}"
    print(line, flush=True)


def main(argv=None):
    import torch

    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--tiles", default="256x128,128x128,auto")
    p.add_argument("--kinds", default="dense,fc1q,grouped")
    p.add_argument("--json", default="")
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_w4a8.py measures on a ROCm GPU; none is visible")
    from ddlb_amd.ops import gemm as G
    from ddlb_amd.ops import load

    gen = torch.Generator(device="cuda").manual_seed(0)
    rows, kinds = [], a.kinds.split(",")

    def run(*args, **kw):
        rows.append(bench(*args, a.iters, a.rounds, gen, **kw))
        show(rows[-1])

    for tile in a.tiles.split(","):
        for N, K in DENSE_NK if "dense" in kinds else ():
            for M in DENSE_MS:
                run("dense", M, N, K, tile)
        for M in DENSE_MS if "fc1q" in kinds else ():
            run("fc1q", M, 2 * 4096, 4096, tile)
        for tokens in MOE["tokens"] if "grouped" in kinds else ():
            for layer, N, K in (("fc1", 2 * MOE["F"], MOE["H"]), ("fc2", MOE["H"], MOE["F"])):
                run("grouped", tokens * MOE["top_k"], N, K, tile, tokens=tokens, layer=layer)
    res = {"device": torch.cuda.get_device_name(0), "cus": G.device_cus(),
           "stages": load().W4A8_STAGES, "iters": a.iters, "rounds": a.rounds, "rows": rows}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
