"""Microbenchmark: the routed gated FFN (``MxMoE``) with one grouped GEMM launch per layer beside
the same work as one ``gemm()`` per non-empty expert.

Per expert count and format, in ONE process: ``grouped`` is ``MxMoE.forward`` (routing on the
device, one quantiser launch, two ``gemm_grouped`` launches, the scatter back). ``loop`` does the
same routing, gather, quantisation and scatter, and runs fc1 / fc2 as one ``gemm(glu=True,
out_quant=)`` / ``gemm()`` per expert that received tokens, on row slices of the same buffers; its
row counts are read back ONCE, outside the timed loop (inside it they would be a host sync per
forward, which is what the grouped launch removes). Both results pass ``MxMoE.validate`` before
anything is timed, and whether they are the same bytes is reported (asserted with an explicit
``--tile``). Variants are interleaved over several rounds, device events around
``iters`` back-to-back calls; reported are the median, the minimum and the round-to-round spread.

    python scripts/bench_moe.py --json out/moe.json
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def loop_forward(moe, bounds):
    """``MxMoE.forward`` with one ``gemm()`` per non-empty expert in place of each grouped launch.
    ``bounds``: the experts' (index, first row, end row), read back once by the caller."""
    import torch

    from ddlb_amd.models.mx_mlp import _fmt_ops
    from ddlb_amd.ops.gemm import gemm

    quant, _, _ = _fmt_ops(moe.fmt)
    q4 = moe.fmt == "mxfp4"
    hq = torch.empty((moe.S, moe.F // 2 if q4 else moe.F), dtype=torch.uint8,
                     device=moe.X.device).view(moe.w2q.dtype)
    hs = torch.empty((moe.S, moe.F // 32), dtype=torch.uint8, device=moe.X.device)

    def forward():
        perm, _ = moe.route()
        xq, xs = quant(moe.X.index_select(0, perm))
        for e, lo, hi in bounds:
            gemm(xq[lo:hi], moe.w1q[e], hq[lo:hi], a_scale=xs[lo:hi], w_scale=moe.w1s[e],
                 act=moe.act, tile=moe.tile, glu=True, out_quant=moe.fmt, out_scale=hs[lo:hi])
        for e, lo, hi in bounds:
            gemm(hq[lo:hi], moe.w2q[e], moe.ysorted[lo:hi], a_scale=hs[lo:hi],
                 w_scale=moe.w2s[e], tile=moe.tile)
        moe.out.index_copy_(0, perm, moe.ysorted)
        return moe.out

    return forward


def main():
    import torch

    from ddlb_amd.models.mx_moe import MxMoE

    p = argparse.ArgumentParser()
    p.add_argument("--hidden", type=int, default=2048)
    p.add_argument("--ffn", type=int, default=1024)
    p.add_argument("--seq", type=int, default=8192)
    p.add_argument("--experts", default="8,64")
    p.add_argument("--fmts", default="mx,mxfp4")
    p.add_argument("--tile", default="auto")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--json", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe needs a ROCm GPU")
    results = []
    for E in (int(x) for x in a.experts.split(",")):
        for fmt in a.fmts.split(","):
            moe = MxMoE(a.hidden, a.ffn, a.seq, E, fmt=fmt, act="silu", fused=True, tile=a.tile)
            offs = moe.route()[1].tolist()  # the one read-back, outside the timed loop
            bounds = [(e, offs[e], offs[e + 1]) for e in range(E) if offs[e + 1] > offs[e]]
            loop = loop_forward(moe, bounds)
            y = moe.forward().clone()
            yl = loop().clone()
            same = torch.equal(y, yl)
            moe.validate(y)
            moe.validate(yl)
            variants = {"grouped": moe.forward, "loop": loop}
            times = {k: [] for k in variants}
            for _ in range(a.rounds):
                for k, fn in variants.items():
                    times[k].append(timeit(fn, a.iters))
            g, lp = summarise(times["grouped"]), summarise(times["loop"])
            counts = [hi - lo for _, lo, hi in bounds]
            r = {"hidden": a.hidden, "ffn": a.ffn, "seq": a.seq, "experts": E, "fmt": fmt,
                 "tile": a.tile, "non_empty": len(bounds), "rows_min": min(counts),
                 "rows_max": max(counts), "same_bytes": same, "grouped": g, "loop": lp,
                 "loop_over_grouped": lp["ms_median"] / g["ms_median"],
                 "grouped_tflops": moe.flops / g["ms_median"] * 1e-9}
            results.append(r)
            print(f"E={E:3d} ({len(bounds)} non-empty, {min(counts)}..{max(counts)} rows) {fmt:6s}"
                  f" grouped {g['ms_median']:8.4f} ms (spread {100 * g['spread']:4.1f} %)   loop "
                  f"{lp['ms_median']:8.4f} ms (spread {100 * lp['spread']:4.1f} %)   loop / grouped "
                  f"x{r['loop_over_grouped']:.3f}   same bytes: {same}", flush=True)
            del moe, loop, variants
            torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)
    # (with tile auto the loop may pick another tile per expert than the grouped launch does for
    # all of them; with one explicit tile the bytes must be the same)
    if a.tile != "auto" and not all(r["same_bytes"] for r in results):
        raise SystemExit("the grouped launch and the per-expert loop wrote different bytes")


if __name__ == "__main__":
    main()
