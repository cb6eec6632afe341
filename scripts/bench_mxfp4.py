"""Microbenchmark: the block-scaled MXFP4 GEMM beside the block-scaled MX-fp8 GEMM.

Both formats in ONE process, variants interleaved over several rounds, median reported; device
events around ``iters`` back-to-back calls. Per shape: the GEMM alone (operands quantised once,
outside the clock) for ``auto`` and every offered tile, the GEMM plus the activation's
quantisation (what ``compute_only;quant=mx`` / ``quant=mxfp4`` time), and each quantiser alone
with the bytes it reads and writes. TFLOP/s is ``2 M N K / t`` for both formats.

    python scripts/bench_mxfp4.py --json out/mxfp4.json
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(65536, 1024, 1024), (8192, 8192, 8192)]


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


def main():
    import torch

    from ddlb_amd.ops.gemm import SCALED_FP4_TILES, SCALED_TILES, gemm
    from ddlb_amd.ops.mx import quantize_mx, quantize_mxfp4

    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--shapes", default="all", help="all, or indices into SHAPES")
    p.add_argument("--json", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mxfp4 needs a ROCm GPU")
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    shapes = SHAPES if a.shapes == "all" else [SHAPES[int(i)] for i in a.shapes.split(",")]
    results = []
    for (M, N, K) in shapes:
        X = (torch.rand((M, K), generator=g, device="cuda") * 2 - 1).to(torch.bfloat16)
        Wt = (torch.rand((N, K), generator=g, device="cuda") * 2 - 1).to(torch.bfloat16)
        out = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
        a8, sa8 = quantize_mx(X)
        w8, sw8 = quantize_mx(Wt)
        a4, sa4 = quantize_mxfp4(X)
        w4, sw4 = quantize_mxfp4(Wt)
        gemms = {}
        for t in ("auto",) + tuple(SCALED_TILES):
            gemms[f"mxfp8[{t}]"] = lambda t=t: gemm(a8, w8, out, tile=t, a_scale=sa8, w_scale=sw8)
        for t in ("auto",) + tuple(SCALED_FP4_TILES):
            gemms[f"mxfp4[{t}]"] = lambda t=t: gemm(a4, w4, out, tile=t, a_scale=sa4, w_scale=sw4)

        def step8():
            q, s = quantize_mx(X)
            gemm(q, w8, out, a_scale=s, w_scale=sw8)

        def step4():
            q, s = quantize_mxfp4(X)
            gemm(q, w4, out, a_scale=s, w_scale=sw4)

        gemms["mxfp8[auto] + quantise A"] = step8
        gemms["mxfp4[auto] + quantise A"] = step4
        quants = {  # name -> (callable, bytes read + written)
            "quantize_mx[bf16]": (lambda: quantize_mx(X), M * K * 2 + M * K + M * K // 32),
            "quantize_mxfp4[bf16]": (lambda: quantize_mxfp4(X),
                                     M * K * 2 + M * K // 2 + M * K // 32),
        }
        times = {k: [] for k in list(gemms) + list(quants)}
        for _ in range(a.rounds):
            for k, fn in gemms.items():
                times[k].append(timeit(fn, a.iters))
            for k, (fn, _) in quants.items():
                times[k].append(timeit(fn, a.iters))
        flop = 2.0 * M * N * K
        row = {"M": M, "N": N, "K": K, "out": "bfloat16", "variants": {}}
        print(f"\n{M}x{N}x{K}, bf16 output")
        for k, ts in times.items():
            med = statistics.median(ts)
            if k in quants:
                gbs = quants[k][1] / (med * 1e-3) / 1e9
                row["variants"][k] = {"ms_median": med, "ms_min": min(ts), "gb_per_s": gbs}
                print(f"  {k:28s} {med:8.4f} ms  (min {min(ts):.4f})  {gbs:8.1f} GB/s")
                continue
            tf = flop / (med * 1e-3) / 1e12
            row["variants"][k] = {"ms_median": med, "ms_min": min(ts), "tflops": tf}
            print(f"  {k:28s} {med:8.4f} ms  (min {min(ts):.4f})  {tf:8.1f} TFLOP/s")
        results.append(row)
        del X, Wt, out, a8, w8, a4, w4
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
