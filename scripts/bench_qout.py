"""Microbenchmark: the GEMM with a quantising epilogue beside the two-launch route it replaces.

Per shape, input form (bf16, block-scaled fp8) and output form (MX-fp8, MXFP4), in ONE process:
``fused`` is ``gemm(..., out_quant=)``, one launch that writes ``(q, s)``; ``pair`` is the same
GEMM with bf16 output followed by the streaming quantiser (``quantize_mx`` / ``quantize_mxfp4``),
both with the same ``--tile`` (``auto``: each side gets the front-end's own choice, pt4 and the
K-split included for the pair). Then ``MxMLP`` fused against unfused. Variants are interleaved
over several rounds, device events around ``iters`` back-to-back calls; reported are the median,
the minimum and the round-to-round spread (max - min over the rounds, as a share of the median).
``not slower`` means: the fused median is at most the pair's plus the larger of the two spreads.

    python scripts/bench_qout.py --json out/qout.json

``--gated`` times the gated fc1 instead (``act = silu``, ``W = pack_glu(Wg, Wu)`` of ``2 N`` rows
for a shape's ``N``): ``fused`` is ``gemm(..., glu=True, out_quant=)``, one launch; ``chain`` is
what it replaces, the ungated GEMM to a bf16 ``[M, 2N]`` intermediate, torch's ``silu(g) * u`` on
its halves, then the streaming quantiser.

    python scripts/bench_qout.py --gated --json out/qout_gated.json
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(65536, 1024, 1024), (8192, 1024, 8192)]
FMTS = ("mx", "mxfp4")


def timeit(fn, iters, warm=3):
    import torch

    for _ in range(warm):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def summarise(ts):
    med = statistics.median(ts)
    return {"ms_median": med, "ms_min": min(ts), "ms_max": max(ts),
            "spread": (max(ts) - min(ts)) / med}


def compare(times, fused, pair):
    f, p = summarise(times[fused]), summarise(times[pair])
    slack = max(f["spread"], p["spread"]) * p["ms_median"]
    return {"fused": f, "pair": p, "speedup": p["ms_median"] / f["ms_median"],
            "not_slower": f["ms_median"] <= p["ms_median"] + slack}


def run_rounds(variants, rounds, iters):
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(timeit(fn, iters))
    return times


def run_gated(a, shapes, g):
    """The fused gated fc1 against the unfused chain, per shape, input and output form."""
    import torch

    from ddlb_amd.ops.gemm import gemm, pack_glu
    from ddlb_amd.ops.mx import quantize_mx, quantize_mxfp4

    quant = {"mx": quantize_mx, "mxfp4": quantize_mxfp4}
    results = []
    for (M, F, K) in shapes:
        X = (torch.rand((M, K), generator=g, device="cuda") * 2 - 1).to(torch.bfloat16)
        Wg, Wu = ((torch.rand((F, K), generator=g, device="cuda") * 2 - 1).to(torch.bfloat16)
                  * K ** -0.5 for _ in range(2))
        Wt = pack_glu(Wg, Wu)
        a8, sa8 = quantize_mx(X)
        w8, sw8 = quantize_mx(Wt)
        inputs = {"bf16": (X, Wt, {}), "mxfp8": (a8, w8, dict(a_scale=sa8, w_scale=sw8))}
        bf = torch.empty((M, 2 * F), dtype=torch.bfloat16, device="cuda")
        halves = bf.view(M, F // 32, 2, 32)
        variants = {}
        for form, (xa, xw, kw) in inputs.items():
            for fmt in FMTS:
                ncol = F if fmt == "mx" else F // 2
                q = torch.empty((M, ncol), dtype=torch.uint8, device="cuda").view(
                    torch.float8_e4m3fn if fmt == "mx" else torch.float4_e2m1fn_x2)
                s = torch.empty((M, F // 32), dtype=torch.uint8, device="cuda")

                def fused(xa=xa, xw=xw, kw=kw, fmt=fmt, q=q, s=s):
                    gemm(xa, xw, q, tile=a.tile, act="silu", glu=True, out_quant=fmt,
                         out_scale=s, **kw)

                def chain(xa=xa, xw=xw, kw=kw, fmt=fmt):
                    gemm(xa, xw, bf, tile=a.tile, **kw)
                    h = torch.nn.functional.silu(halves[:, :, 0]) * halves[:, :, 1]
                    quant[fmt](h.reshape(M, F))

                variants[f"{form}->{fmt} fused"] = fused
                variants[f"{form}->{fmt} pair"] = chain
        times = run_rounds(variants, a.rounds, a.iters)
        print(f"\ngated fc1 {M}x{2 * F}x{K} -> [{M}, {F}]  silu  tile={a.tile}")
        for form in inputs:
            for fmt in FMTS:
                c = compare(times, f"{form}->{fmt} fused", f"{form}->{fmt} pair")
                c.update(M=M, N=2 * F, K=K, input=form, out=fmt, tile=a.tile, act="silu")
                results.append(c)
                print(f"  {form:6s}-> {fmt:6s} fused {c['fused']['ms_median']:8.4f} ms "
                      f"(spread {100 * c['fused']['spread']:4.1f} %)   chain "
                      f"{c['pair']['ms_median']:8.4f} ms "
                      f"(spread {100 * c['pair']['spread']:4.1f} %)"
                      f"   x{c['speedup']:.3f}  {'ok' if c['not_slower'] else 'SLOWER'}")
        del X, Wg, Wu, Wt, a8, w8, bf, halves, variants, inputs
        torch.cuda.empty_cache()
    return results


def dump(path, results):
    if path:
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        with open(path, "w") as f:
            json.dump(results, f, indent=1)


def main():
    import torch

    from ddlb_amd.models.mx_mlp import MxMLP
    from ddlb_amd.ops.gemm import gemm
    from ddlb_amd.ops.mx import quantize_mx, quantize_mxfp4

    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--shapes", default="all", help="all, or indices into SHAPES")
    p.add_argument("--tile", default="auto")
    p.add_argument("--no-mlp", action="store_true")
    p.add_argument("--gated", action="store_true",
                   help="the gated (GLU) fc1, fused against GEMM + torch silu(g) * u + quantiser")
    p.add_argument("--json", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_qout needs a ROCm GPU")
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    shapes = SHAPES if a.shapes == "all" else [SHAPES[int(i)] for i in a.shapes.split(",")]
    quant = {"mx": quantize_mx, "mxfp4": quantize_mxfp4}
    results = {"gemm": [], "mlp": []}
    if a.gated:  # (no MLP part: --no-mlp changes nothing here)
        dump(a.json, {"gated": run_gated(a, shapes, g)})
        return
    for (M, N, K) in shapes:
        X = (torch.rand((M, K), generator=g, device="cuda") * 2 - 1).to(torch.bfloat16)
        Wt = (torch.rand((N, K), generator=g, device="cuda") * 2 - 1).to(torch.bfloat16)
        a8, sa8 = quantize_mx(X)
        w8, sw8 = quantize_mx(Wt)
        inputs = {"bf16": (X, Wt, {}), "mxfp8": (a8, w8, dict(a_scale=sa8, w_scale=sw8))}
        bf = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
        variants = {}
        for form, (xa, xw, kw) in inputs.items():
            for fmt in FMTS:
                ncol = N if fmt == "mx" else N // 2
                q = torch.empty((M, ncol), dtype=torch.uint8, device="cuda").view(
                    torch.float8_e4m3fn if fmt == "mx" else torch.float4_e2m1fn_x2)
                s = torch.empty((M, N // 32), dtype=torch.uint8, device="cuda")

                def fused(xa=xa, xw=xw, kw=kw, fmt=fmt, q=q, s=s):
                    gemm(xa, xw, q, tile=a.tile, out_quant=fmt, out_scale=s, **kw)

                def pair(xa=xa, xw=xw, kw=kw, fmt=fmt):
                    gemm(xa, xw, bf, tile=a.tile, **kw)
                    quant[fmt](bf)

                variants[f"{form}->{fmt} fused"] = fused
                variants[f"{form}->{fmt} pair"] = pair
        times = run_rounds(variants, a.rounds, a.iters)
        print(f"\n{M}x{N}x{K}  tile={a.tile}  (GEMM alone)")
        for form in inputs:
            for fmt in FMTS:
                c = compare(times, f"{form}->{fmt} fused", f"{form}->{fmt} pair")
                c.update(M=M, N=N, K=K, input=form, out=fmt, tile=a.tile)
                results["gemm"].append(c)
                print(f"  {form:6s}-> {fmt:6s} fused {c['fused']['ms_median']:8.4f} ms "
                      f"(spread {100 * c['fused']['spread']:4.1f} %)   pair "
                      f"{c['pair']['ms_median']:8.4f} ms (spread {100 * c['pair']['spread']:4.1f} %)"
                      f"   x{c['speedup']:.3f}  {'ok' if c['not_slower'] else 'SLOWER'}")
        del X, Wt, a8, w8, bf, variants, inputs
        torch.cuda.empty_cache()
        if a.no_mlp:
            continue
        S, H, F = M, K, N  # fc1 is the shape above; fc2 maps back to H
        mlps = {}
        for fmt in FMTS:
            for fused_ in (True, False):
                m = MxMLP(H, F, S, "bfloat16", "gelu", fmt=fmt, fused=fused_)
                mlps[f"MxMLP[{fmt}] {'fused' if fused_ else 'pair'}"] = m.forward
        times = run_rounds(mlps, a.rounds, a.iters)
        print(f"MxMLP S={S} H={H} F={F} gelu")
        for fmt in FMTS:
            c = compare(times, f"MxMLP[{fmt}] fused", f"MxMLP[{fmt}] pair")
            c.update(S=S, H=H, F=F, fmt=fmt)
            results["mlp"].append(c)
            print(f"  {fmt:6s} fused {c['fused']['ms_median']:8.4f} ms (spread "
                  f"{100 * c['fused']['spread']:4.1f} %)   pair {c['pair']['ms_median']:8.4f} ms "
                  f"(spread {100 * c['pair']['spread']:4.1f} %)   x{c['speedup']:.3f}  "
                  f"{'ok' if c['not_slower'] else 'SLOWER'}")
        del mlps
        torch.cuda.empty_cache()
    dump(a.json, results)


if __name__ == "__main__":
    main()
