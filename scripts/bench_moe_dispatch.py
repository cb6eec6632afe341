"""Microbenchmark: the token side of the routed FFN (``MxMoE``) as the chain of torch ops
(``dispatch="torch"``) beside the native dispatch layer (``dispatch="native"``: ``ops.moe.route``,
``ops.mx.quantize_mx_gather``, ``ops.moe.combine``).

Per format, in ONE process and at the same ``S, H, E``:

* the dispatch alone, top-1: ``dispatch`` = routing + gather + quantise (torch: ``argsort`` /
  ``scatter_add_`` / ``cumsum`` / ``index_select`` / the row quantiser; native: ``route`` +
  ``quantize_mx_gather``) and ``combine`` = the un-permute (torch: ``index_copy_``; native:
  ``combine`` with gates of 1). Offsets, quantised bytes and scales and the combined rows must be
  equal before anything is timed;
* the whole ``MxMoE.forward`` with ``dispatch="torch"`` against ``"native"`` at ``top_k = 1``
  (``torch.equal`` outputs), then ``"native"`` at ``top_k = 2, 4, 8`` (validated), where only the
  native path exists.

Variants are interleaved over several rounds, device events around ``iters`` back-to-back calls;
reported are the median, the minimum and the round-to-round spread.

    python scripts/bench_moe_dispatch.py --json out/moe_dispatch.json
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


def interleaved(variants, rounds, iters):
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(timeit(fn, iters))
    return {k: summarise(v) for k, v in times.items()}


def dispatch_variants(old, new):
    """The four token-side pieces as closures over one torch-dispatch and one native-dispatch
    instance of the same layer (same X, same routing)."""
    from ddlb_amd.models.mx_mlp import _fmt_ops
    from ddlb_amd.ops.moe import combine, route
    from ddlb_amd.ops.mx import quantize_mx_gather

    quant, _, _ = _fmt_ops(old.fmt)

    def torch_dispatch():
        perm, offsets = old.route()
        xq, xs = quant(old.X.index_select(0, perm))
        return perm, offsets, xq, xs

    def native_dispatch():
        offsets, row_token, slot_row = route(new.ids, new.E)
        xq, xs = quantize_mx_gather(new.X, row_token, fmt=new.fmt)
        return slot_row, offsets, xq, xs

    perm = torch_dispatch()[0]
    slot_row = native_dispatch()[0]

    def torch_combine():
        return old.out.index_copy_(0, perm, old.ysorted)

    def native_combine():
        return combine(new.ysorted, slot_row, new.gates, out=new.out)

    return {"torch_dispatch": torch_dispatch, "native_dispatch": native_dispatch,
            "torch_combine": torch_combine, "native_combine": native_combine}


def check_dispatch(v, old, new):
    import torch

    _, o_t, q_t, s_t = v["torch_dispatch"]()
    _, o_n, q_n, s_n = v["native_dispatch"]()
    new.ysorted.copy_(old.ysorted)
    same = (torch.equal(o_t, o_n) and torch.equal(s_t, s_n)
            and torch.equal(q_t.view(torch.uint8), q_n.view(torch.uint8))
            and torch.equal(v["torch_combine"](), v["native_combine"]()))
    torch.cuda.synchronize()
    return same


def main():
    import torch

    from ddlb_amd.models.mx_moe import MxMoE

    p = argparse.ArgumentParser()
    p.add_argument("--hidden", type=int, default=2048)
    p.add_argument("--ffn", type=int, default=1024)
    p.add_argument("--seq", type=int, default=8192)
    p.add_argument("--experts", type=int, default=64)
    p.add_argument("--fmts", default="mx,mxfp4")
    p.add_argument("--top-ks", default="2,4,8")
    p.add_argument("--tile", default="auto")
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--json", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe_dispatch needs a ROCm GPU")
    results = []
    shape = {"hidden": a.hidden, "ffn": a.ffn, "seq": a.seq, "experts": a.experts, "tile": a.tile}
    for fmt in a.fmts.split(","):
        kw = dict(fmt=fmt, act="silu", fused=True, tile=a.tile)
        old = MxMoE(a.hidden, a.ffn, a.seq, a.experts, **kw)
        new = MxMoE(a.hidden, a.ffn, a.seq, a.experts, dispatch="native", **kw)
        y_old = old.forward().clone()
        y_new = new.forward().clone()
        old.validate(y_old)
        if not torch.equal(y_old, y_new):
            raise SystemExit(f"{fmt}: the native forward differs from the torch forward at top-1")
        v = dispatch_variants(old, new)
        if not check_dispatch(v, old, new):
            raise SystemExit(f"{fmt}: the native dispatch differs from the torch chain")
        parts = interleaved(v, a.rounds, 4 * a.iters)
        whole = interleaved({"torch": old.forward, "native": new.forward}, a.rounds, a.iters)
        r = dict(shape, fmt=fmt, top_k=1, same_bytes=True, **parts,
                 forward_torch=whole["torch"], forward_native=whole["native"],
                 dispatch_torch_over_native=(parts["torch_dispatch"]["ms_median"]
                                             / parts["native_dispatch"]["ms_median"]),
                 combine_torch_over_native=(parts["torch_combine"]["ms_median"]
                                            / parts["native_combine"]["ms_median"]),
                 forward_torch_over_native=(whole["torch"]["ms_median"]
                                            / whole["native"]["ms_median"]),
                 native_tflops=new.flops / whole["native"]["ms_median"] * 1e-9)
        results.append(r)
        for name in ("dispatch", "combine"):
            t, n = parts[f"torch_{name}"], parts[f"native_{name}"]
            print(f"{fmt:6s} top-1 {name:9s} torch {t['ms_median']:8.4f} ms (spread "
                  f"{100 * t['spread']:4.1f} %)   native {n['ms_median']:8.4f} ms (spread "
                  f"{100 * n['spread']:4.1f} %)   torch / native "
                  f"x{t['ms_median'] / n['ms_median']:.3f}", flush=True)
        t, n = whole["torch"], whole["native"]
        print(f"{fmt:6s} top-1 forward   torch {t['ms_median']:8.4f} ms (spread "
              f"{100 * t['spread']:4.1f} %)   native {n['ms_median']:8.4f} ms (spread "
              f"{100 * n['spread']:4.1f} %)   torch / native x{r['forward_torch_over_native']:.3f}"
              f"   {r['native_tflops']:.1f} TFLOP/s", flush=True)
        del old, new, v
        torch.cuda.empty_cache()
        for k in (int(x) for x in a.top_ks.split(",") if x):
            moe = MxMoE(a.hidden, a.ffn, a.seq, a.experts, top_k=k, dispatch="native", **kw)
            moe.validate(moe.forward())
            n = interleaved({"native": moe.forward}, a.rounds, a.iters)["native"]
            results.append(dict(shape, fmt=fmt, top_k=k, forward_native=n,
                                native_tflops=moe.flops / n["ms_median"] * 1e-9))
            print(f"{fmt:6s} top-{k} forward   native {n['ms_median']:8.4f} ms (spread "
                  f"{100 * n['spread']:4.1f} %)   {results[-1]['native_tflops']:.1f} TFLOP/s",
                  flush=True)
            del moe
            torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(a.json) or ".", exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
