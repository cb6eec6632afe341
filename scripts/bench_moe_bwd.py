"""Microbenchmark: the backward pass of a routed MX linear layer (``mx_grouped_linear``) and its
two new kernels, at the shapes of ``scripts/bench_moe.py`` (``x [seq, hidden]``,
``w [E, ffn, hidden]``, tokens routed to experts by seeded random ids).

Per expert count and format, in ONE process, four pairs:

* ``quant_t``: the grouped transposing quantiser of ``x`` beside ``quantize_mx_t`` on the same
  ``[T, C]`` (the ungrouped kernel moving the same bytes; it knows nothing of groups);
* ``wgrad``: ``gemm_kgrouped`` beside a loop of one ungrouped ``gemm`` per non-empty expert over
  the same column slices (the slices' bounds read back ONCE, outside the timed loop);
* ``weight_t``: the stacked weight transposer (one launch) beside ``E`` calls of
  ``quantize_mx_t(w[g])``;
* ``backward``: the whole backward (both quantisations of ``dy``, grouped dgrad, K-grouped wgrad)
  beside a bf16 torch loop over the experts (``dy[rows] @ w[g]``, ``dy[rows].T @ x[rows]``).

The wgrad pair is checked to write the same bytes before anything is timed. Variants are
interleaved over several rounds, device events around ``iters`` back-to-back calls; reported are
the median, the minimum and the round-to-round spread.

    python scripts/bench_moe_bwd.py --json out/moe_bwd.json
"""

from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.bench_moe import summarise, timeit  # noqa: E402


def main():
    import torch

    from ddlb_amd.models.mx_grouped_linear import mx_grouped_linear, quantize_weight
    from ddlb_amd.ops.gemm import gemm, gemm_kgrouped, padded_offsets
    from ddlb_amd.ops.mx import quantize_mx_t, quantize_mx_t_grouped

    p = argparse.ArgumentParser()
    p.add_argument("--hidden", type=int, default=2048)
    p.add_argument("--ffn", type=int, default=1024)
    p.add_argument("--seq", type=int, default=8192)
    p.add_argument("--experts", default="8,64")
    p.add_argument("--fmts", default="mx,mxfp4")
    p.add_argument("--tile", default="128x128")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--json", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe_bwd needs a ROCm GPU")
    dev = "cuda"
    T, K, N = a.seq, a.hidden, a.ffn
    results = []
    for E in (int(v) for v in a.experts.split(",")):
        g = torch.Generator(device=dev).manual_seed(E)
        ids = torch.randint(0, E, (T,), generator=g, device=dev)
        counts = torch.bincount(ids, minlength=E)
        offs = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).to(torch.int32)
        x = (torch.rand((T, K), generator=g, device=dev) * 2 - 1).bfloat16()
        w = ((torch.rand((E, N, K), generator=g, device=dev) * 2 - 1) * K ** -0.5).bfloat16()
        dy = (torch.rand((T, N), generator=g, device=dev) * 2 - 1).bfloat16()
        for fmt in a.fmts.split(","):
            mod = 256 if fmt == "mxfp4" else 128
            d = 2 if fmt == "mxfp4" else 1
            k0 = padded_offsets(offs, T, mod)  # the one read-back, outside the timed loops
            live = [e for e in range(E) if k0[e + 1] > k0[e]]
            xtq, xts = quantize_mx_t_grouped(x, offs, fmt=fmt)
            dytq, dyts = quantize_mx_t_grouped(dy, offs, fmt=fmt)
            dw = torch.empty((E, N, K), dtype=torch.bfloat16, device=dev)
            dwl = torch.zeros((E, N, K), dtype=torch.bfloat16, device=dev)

            def cols(t, s, e):
                lo, hi = k0[e], k0[e + 1]
                return (t.view(torch.uint8)[:, lo // d:hi // d].view(t.dtype),
                        s[:, lo // 32:hi // 32])

            slices = [(e, cols(dytq, dyts, e), cols(xtq, xts, e)) for e in live]

            def wgrad():
                return gemm_kgrouped(dytq, xtq, offs, T, dw, a_scale=dyts, w_scale=xts,
                                     tile=a.tile)

            def wgrad_loop():
                for e, (aq, asc), (bq, bsc) in slices:
                    gemm(aq, bq, dwl[e], a_scale=asc, w_scale=bsc, tile=a.tile)
                return dwl

            same = torch.equal(wgrad(), wgrad_loop())
            if not same:
                raise SystemExit("gemm_kgrouped and the per-expert loop wrote different bytes")
            w2 = w.reshape(E * N, K)
            slabs = torch.arange(E + 1, dtype=torch.int32, device=dev) * N
            wq = quantize_weight(w, fmt)
            xr = x.clone().requires_grad_()
            wr = w.clone().requires_grad_()
            y = mx_grouped_linear(xr, wr, offs, fmt, a.tile, w_quant=wq)
            o = offs.tolist()
            rows = [(e, o[e], o[e + 1]) for e in range(E) if o[e + 1] > o[e]]
            dxb = torch.zeros((T, K), dtype=torch.bfloat16, device=dev)
            dwb = torch.zeros((E, N, K), dtype=torch.bfloat16, device=dev)

            def backward():
                xr.grad = wr.grad = None
                y.backward(dy, retain_graph=True)

            def backward_bf16():
                for e, lo, hi in rows:
                    torch.matmul(dy[lo:hi], w[e], out=dxb[lo:hi])
                    torch.matmul(dy[lo:hi].t(), x[lo:hi], out=dwb[e])

            pairs = {
                "quant_t": (lambda: quantize_mx_t_grouped(x, offs, fmt=fmt, out=(xtq, xts)),
                            lambda: quantize_mx_t(x, fmt=fmt)),
                "wgrad": (wgrad, wgrad_loop),
                "weight_t": (lambda: quantize_mx_t_grouped(w2, slabs, fmt=fmt, stacked_rows=N),
                             lambda: [quantize_mx_t(w[e], fmt=fmt) for e in range(E)]),
                "backward": (backward, backward_bf16),
            }
            r = {"hidden": K, "ffn": N, "seq": T, "experts": E, "fmt": fmt, "tile": a.tile,
                 "non_empty": len(live), "rows_min": int(counts.min()),
                 "rows_max": int(counts.max()), "padded_columns": k0[-1], "wgrad_same_bytes": same}
            for name, (new, old) in pairs.items():
                tn, to = [], []
                for _ in range(a.rounds):
                    tn.append(timeit(new, a.iters))
                    to.append(timeit(old, a.iters))
                sn, so = summarise(tn), summarise(to)
                r[name] = {"new": sn, "baseline": so,
                           "baseline_over_new": so["ms_median"] / sn["ms_median"]}
                print(f"E={E:3d} {fmt:6s} {name:9s} new {sn['ms_median']:8.4f} ms (spread "
                      f"{100 * sn['spread']:4.1f} %)   baseline {so['ms_median']:8.4f} ms (spread "
                      f"{100 * so['spread']:4.1f} %)   baseline / new "
                      f"x{r[name]['baseline_over_new']:.3f}", flush=True)
            results.append(r)
            del y, xr, wr, pairs
            torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
