"""Microbenchmark: the tiled A16 GEMM (bf16 activations on MXFP4 / MX-fp8 weights) beside what a
caller without it runs.

In ONE process, alternating per shape, for both weight forms and each tile code:

* ``a16``: ``gemm_a16`` on the packed weights;
* ``bf16``: ``gemm`` in bf16 on weights dequantised once, outside the timed window, on the same
  tile code of the plain tiled kernel, and ``bf16_auto``: the same with ``tile="auto"``;
* ``deq_bf16``: the dequantisation (the torch chain of ``ops.mx``) inside the window, then
  ``bf16_auto``: the cost of not keeping a second copy;
* ``w4a8`` (MXFP4 weights only): ``quantize_mx`` of the activations, then ``gemm_w4a8``: the price
  of keeping the activations 16-bit.

Shapes: dense ``(N, K)`` in (4096, 4096), (8192, 8192) with ``M`` in 512, 2048, 8192; the gated
fc1 (``N = 2 x 4096``, ``K = 4096``); the grouped form at E = 32 experts, top-4, H = 4096,
F = 1536 (fc1 and fc2), 4096 and 16384 tokens. Before anything is timed the A16 output is compared
with the bf16 route's (``atol = 1e-3 K``). Every shape is warmed; device events surround a window
of back-to-back calls, at least ``iters`` of them and ``--window-ms`` of work; variants alternate
over ``rounds`` rounds and the median, minimum and round-to-round spread are reported, with the
weight bytes each route keeps resident. ``--tiles`` lists the tile codes (``auto``: both routes'
own choice, so ``bf16`` and ``bf16_auto`` are the same call there).

    python scripts/bench_a16.py --json out/a16.json
"""

from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_skinny import summarise, timeit, weight_bytes  # noqa: E402
from scripts.bench_w4a8 import DENSE_MS, DENSE_NK, MOE  # noqa: E402


def bench(kind, wfmt, M, N, K, tile, iters, rounds, window_ms, gen, tokens=0, layer=""):
    """One shape: ``kind`` dense / fc1 (gated) / grouped; ``wfmt`` mxfp4 / mx."""
    import torch

    from ddlb_amd.models.mx_mlp import _fmt_ops
    from ddlb_amd.ops import gemm as G
    from ddlb_amd.ops import mx

    E = MOE["E"] if kind == "grouped" else 1
    bf = torch.bfloat16
    a = torch.randn((M, K), generator=gen, device=gen.device, dtype=bf)
    wf = torch.randn((E * N, K), generator=gen, device=gen.device, dtype=bf) * K ** -0.5
    quant, _, deq = _fmt_ops(wfmt)
    wq, ws = quant(wf)
    w16 = deq(wq, ws).to(bf)
    pre, shape = (), lambda t: t
    if kind == "grouped":
        counts = torch.bincount(torch.randint(0, E, (M,), generator=gen, device=gen.device),
                                minlength=E)
        offs = torch.zeros(E + 1, dtype=torch.int32, device=gen.device)
        offs[1:] = torch.cumsum(counts, 0)
        pre, shape = (offs,), lambda t: t.reshape(E, N, -1)
    wq3, ws3, w163 = shape(wq), shape(ws), shape(w16)
    grouped = kind == "grouped"
    fa, fb, fm = (G.gemm_a16_grouped, G.gemm_grouped, G.gemm_w4a8_grouped) if grouped else \
        (G.gemm_a16, G.gemm, G.gemm_w4a8)
    kw = dict(act="silu", glu=True) if kind == "fc1" else {}
    variants = {
        "a16": lambda: fa(a, wq3, *pre, w_scale=ws3, tile=tile, **kw),
        "bf16": lambda: fb(a, w163, *pre, tile=tile, **kw),
        "bf16_auto": lambda: fb(a, w163, *pre, **kw),
        "deq_bf16": lambda: fb(a, shape(deq(wq, ws).to(bf)), *pre, **kw)}
    if wfmt == "mxfp4":
        def w4a8():
            q, s = mx.quantize_mx(a)
            return fm(q, wq3, *pre, a_scale=s, w_scale=ws3, **kw)
        variants["w4a8"] = w4a8
    got, ref = variants["a16"](), variants["bf16"]()
    live = slice(0, M)
    torch.testing.assert_close(got[live].float(), ref[live].float(), rtol=2.0 ** -7,
                               atol=1e-3 * K)
    ts = {k: [] for k in variants}
    # warm every variant, then size its window: at least `iters` calls and `window_ms` of work
    n = {k: max(iters, int(window_ms / timeit(fn, 2, 2)) + 1) for k, fn in variants.items()}
    for _ in range(rounds):
        for k, fn in variants.items():
            ts[k].append(timeit(fn, n[k], 1))
    r = {k: summarise(v) for k, v in ts.items()}
    for k in variants:
        if k != "a16":
            r[f"a16_over_{k}"] = r["a16"]["ms_median"] / r[k]["ms_median"]
    r["tflops"] = 2.0 * M * N * K / (r["a16"]["ms_median"] * 1e-3) / 1e12
    packed = weight_bytes(E * N, K, wfmt)
    r["resident_bytes"] = {"a16": packed, "bf16": packed + 2 * E * N * K, "deq_bf16": packed,
                           "w4a8": packed}
    r.update(kind=kind, wfmt=wfmt, M=M, N=N, K=K, tile=tile, tokens=tokens, layer=layer)
    return r


def show(r):
    what = f"moe {r['layer']} tok={r['tokens']}" if r["kind"] == "grouped" else r["kind"]
    line = (f"{r['wfmt']:5s} {what:18s} M={r['M']:<6d} N={r['N']:<5d} K={r['K']:<5d} "
            f"{r['tile']:8s} a16 {r['a16']['ms_median'] * 1e3:8.1f} us (spread "
            f"{100 * r['a16']['spread']:.1f} %) {r['tflops']:5.0f} TF/s")
    for k in ("bf16", "bf16_auto", "deq_bf16", "w4a8"):
        if f"a16_over_{k}" in r:
            line += f" | / {k} {r[f'a16_over_{k}']:.3f} (spread {100 * r[k]['spread']:.1f} %)"
    rb = r["resident_bytes"]
    print(line + f" | resident MiB a16 {rb['a16'] / 2 ** 20:.0f}, bf16 {rb['bf16'] / 2 ** 20:.0f}",
          flush=True)


def main(argv=None):
    import torch

    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--window-ms", type=float, default=100.0)
    p.add_argument("--tiles", default="128x128,256x128,auto")
    p.add_argument("--forms", default="mxfp4,mx")
    p.add_argument("--kinds", default="dense,fc1,grouped")
    p.add_argument("--json", default="")
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_a16.py measures on a ROCm GPU; none is visible")
    from ddlb_amd.ops import gemm as G

    gen = torch.Generator(device="cuda").manual_seed(0)
    rows, kinds = [], a.kinds.split(",")

    def run(*args, **kw):
        rows.append(bench(*args, a.iters, a.rounds, a.window_ms, gen, **kw))
        show(rows[-1])

    for wfmt in a.forms.split(","):
        for tile in a.tiles.split(","):
            for N, K in DENSE_NK if "dense" in kinds else ():
                for M in DENSE_MS:
                    run("dense", wfmt, M, N, K, tile)
            for M in DENSE_MS if "fc1" in kinds else ():
                run("fc1", wfmt, M, 2 * 4096, 4096, tile)
            for tokens in MOE["tokens"] if "grouped" in kinds else ():
                for layer, N, K in (("fc1", 2 * MOE["F"], MOE["H"]), ("fc2", MOE["H"], MOE["F"])):
                    run("grouped", wfmt, tokens * MOE["top_k"], N, K, tile, tokens=tokens,
                        layer=layer)
    res = {"device": torch.cuda.get_device_name(0), "cus": G.device_cus(), "iters": a.iters,
           "rounds": a.rounds, "rows": rows}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
