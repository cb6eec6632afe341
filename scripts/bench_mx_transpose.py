"""Microbenchmark: the transposing MX quantiser beside the route it replaces, and the MX linear
layer's forward + backward beside the same three GEMMs in bf16.

Per shape ``R x C`` (bf16 input) and format (MX-fp8, MXFP4), in ONE process:

    a  x.t().contiguous() then the row-wise quantiser   (the route without this kernel)
    b  quantize_mx_t                                     (one pass, transpose inside)
    c  the row-wise quantiser alone
    d  the row-wise quantiser plus quantize_mx_t         (two launches, x read twice)
    e  quantize_mx_2way                                  (one launch, x read once)

Variants are interleaved over several rounds, device events around ``iters`` back-to-back calls;
reported are the median, the round-to-round spread and GB/s of the bytes each route MUST move
(a: the transpose's read and write count). ``not slower`` means: the median is at most the other
side's plus the larger of the two spreads. Then ``mx_linear`` forward + backward against the
three bf16 GEMMs through ``ops.gemm.gemm`` on operands transposed beforehand (outside the timed
region: the bf16 side is not charged for its transposes).

    python scripts/bench_mx_transpose.py --json out/mx_transpose.json
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(8192, 8192), (65536, 1024), (16384, 8192)]
LINEAR_SHAPES = [(8192, 8192, 8192), (65536, 1024, 1024)]
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


def not_slower(new, old):
    return new["ms_median"] <= old["ms_median"] * (1 + max(new["spread"], old["spread"]))


def run_rounds(variants, rounds, iters):
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(timeit(fn, iters))
    return {k: summarise(v) for k, v in times.items()}


def quant_bytes(n, fmt):
    """One quantisation of n bf16 elements: read, data written, scales written."""
    return 2 * n + (n // 2 if fmt == "mxfp4" else n) + n // 32


def main():
    import torch

    from ddlb_amd.models.mx_linear import mx_linear
    from ddlb_amd.ops.gemm import gemm
    from ddlb_amd.ops.mx import quantize_mx, quantize_mx_2way, quantize_mx_t, quantize_mxfp4

    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--shapes", default="all", help="all, or indices into SHAPES")
    p.add_argument("--fmts", default=",".join(FMTS))
    p.add_argument("--no-linear", action="store_true")
    p.add_argument("--json", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mx_transpose needs a ROCm GPU")
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    shapes = SHAPES if a.shapes == "all" else [SHAPES[int(i)] for i in a.shapes.split(",")]
    rowwise = {"mx": quantize_mx, "mxfp4": quantize_mxfp4}
    results = {"quantiser": [], "linear": []}
    for (R, C) in shapes:
        x = torch.randn((R, C), generator=g, device="cuda").to(torch.bfloat16)
        n = R * C
        for fmt in a.fmts.split(","):
            row = rowwise[fmt]
            variants = {
                "a": lambda: row(x.t().contiguous()),
                "b": lambda: quantize_mx_t(x, fmt=fmt),
                "c": lambda: row(x),
                "d": lambda: (row(x), quantize_mx_t(x, fmt=fmt)),
                "e": lambda: quantize_mx_2way(x, fmt=fmt),
            }
            t = run_rounds(variants, a.rounds, a.iters)
            qb = quant_bytes(n, fmt)
            must = {"a": 4 * n + qb, "b": qb, "c": qb, "d": 2 * qb, "e": 2 * qb - 2 * n}
            for k in t:
                t[k]["GBps"] = must[k] / t[k]["ms_median"] * 1e-6
            rec = {"R": R, "C": C, "fmt": fmt, "times": t,
                   "b_over_a": t["b"]["ms_median"] / t["a"]["ms_median"],
                   "b_over_c": t["b"]["ms_median"] / t["c"]["ms_median"],
                   "e_over_d": t["e"]["ms_median"] / t["d"]["ms_median"],
                   "b_not_slower_than_a": not_slower(t["b"], t["a"]),
                   "e_not_slower_than_d": not_slower(t["e"], t["d"])}
            results["quantiser"].append(rec)
            print(f"\n{R}x{C} bf16 -> {fmt}")
            for k in "abcde":
                print(f"  ({k}) {t[k]['ms_median']:8.4f} ms (spread {100 * t[k]['spread']:4.1f} %)"
                      f"  {t[k]['GBps']:7.1f} GB/s")
            print(f"  b/a {rec['b_over_a']:.3f} {'ok' if rec['b_not_slower_than_a'] else 'SLOWER'}"
                  f"   b/c {rec['b_over_c']:.3f}   e/d {rec['e_over_d']:.3f} "
                  f"{'ok' if rec['e_not_slower_than_d'] else 'SLOWER'}")
        del x
        torch.cuda.empty_cache()
    for (M, N, K) in ([] if a.no_linear else LINEAR_SHAPES):
        x = (torch.rand((M, K), generator=g, device="cuda") * 2 - 1).to(torch.bfloat16)
        w = ((torch.rand((N, K), generator=g, device="cuda") * 2 - 1) * K ** -0.5).to(
            torch.bfloat16)
        dy = (torch.rand((M, N), generator=g, device="cuda") * 2 - 1).to(torch.bfloat16)
        xt, wt, dyt = (t.t().contiguous() for t in (x, w, dy))
        y, dx, dw = (torch.empty(s, dtype=torch.bfloat16, device="cuda")
                     for s in ((M, N), (M, K), (N, K)))
        xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()

        def fwd_bwd(fmt):
            xg.grad = wg.grad = None
            mx_linear(xg, wg, fmt).backward(dy)

        def bf16_gemms():
            gemm(x, w, y)         # contracts K
            gemm(dy, wt, dx)      # contracts N
            gemm(dyt, xt, dw)     # contracts M

        variants = {"bf16 3 GEMMs": bf16_gemms}
        for fmt in a.fmts.split(","):
            variants[f"mx_linear[{fmt}] fwd+bwd"] = lambda fmt=fmt: fwd_bwd(fmt)
        t = run_rounds(variants, a.rounds, a.iters)
        print(f"\nlinear M={M} N={N} K={K}")
        for k, v in t.items():
            v["TFLOPs"] = 6.0 * M * N * K / v["ms_median"] * 1e-9
            print(f"  {k:28s} {v['ms_median']:8.4f} ms (spread {100 * v['spread']:4.1f} %)  "
                  f"{v['TFLOPs']:7.1f} TFLOP/s")
        results["linear"].append({"M": M, "N": N, "K": K, "times": t})
        del x, w, dy, xt, wt, dyt, y, dx, dw, xg, wg
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
