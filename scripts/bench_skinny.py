"""Microbenchmark: the skinny-M GEMM beside the tiled kernel on the same block-scaled operands.

In ONE process, alternating per shape: ``gemm_skinny`` against ``gemm`` (dense: M in 1, 4, 16, 64
times (N, K) in (4096, 4096), (8192, 8192)) and ``gemm_skinny_grouped`` against ``gemm_grouped``
(E = 32 experts, 8 and 64 tokens routed top-4, H = 4096, F = 1536: the fc1 and fc2 shapes), MX-fp8
and MXFP4. ``w4a8`` (MX-fp8 activations on MXFP4 weights) is a third format column over the same
shapes: only the skinny kernel takes it, so its rows have no tiled time and its output is checked
against the product of the dequantised operands. Before anything is timed the two outputs are
compared on the same seeded inputs (``atol = 1e-3 K``: both accumulate in f32, in different
orders). Every shape is warmed; device events surround ``iters`` back-to-back calls; variants
alternate over ``rounds`` rounds and the median, minimum and round-to-round spread are reported.
Successive calls walk through copies of the weights that together exceed the 256 MB last-level
cache, so the weights come from HBM.

Printed per row: time per call, the weight-plus-scale bytes the shape needs (computed here from
the shape; grouped: the experts that received rows), the bytes/s that gives, and its share of
the HBM peak (8.0 TB/s, the MI355X specification).

    python scripts/bench_skinny.py --json out/skinny.json

``--fused`` compares, by the same method, two ways of running a gated fc1 on the skinny kernel:
the chain (f32 ``gemm_skinny``, ``ops.glu.glu``, the row quantiser) and the one fused call
(``glu=True, out_quant=fmt``): dense M in 1, 16, 64 at N = 2 x 4096, K = 4096 and the two MoE fc1
shapes. The two write the same bytes, which is checked before anything is timed. ``--shapes moe``
keeps the MoE shapes only (a kernel-trace run).
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12         # bytes/s, specification
ROTATE_BYTES = 512 << 20  # weight copies walked through: twice the last-level cache
DENSE_MS = (1, 4, 16, 64)
FUSED_MS = (1, 16, 64)
DENSE_NK = ((4096, 4096), (8192, 8192))
MOE = dict(E=32, top_k=4, H=4096, F=1536, tokens=(8, 64))


def timeit(fn, iters, warm):
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


def weight_bytes(rows, K, fmt):
    """Data plus scale bytes of ``rows`` weight rows of K elements."""
    return rows * (K // (1 if fmt == "mx" else 2) + K // 32)


def _quant(shape, fmt, gen, scale=1.0, weight=False):
    """Random bf16 data quantised as the activations of ``fmt``, or as its weights."""
    import torch

    from ddlb_amd.models.mx_mlp import _fmt_ops, _fmt_pair

    x = torch.randn(shape, generator=gen, device=gen.device, dtype=torch.bfloat16) * scale
    return _fmt_ops(_fmt_pair(fmt)[weight])[0](x)


def _check_mixed(out, a, sa, w, sw, K):
    """``w4a8`` has no tiled kernel to compare with: the dequantised operands' product."""
    import torch

    from ddlb_amd.ops import mx

    ref = mx.dequantize_mx(a, sa) @ mx.dequantize_mxfp4(w, sw).t()
    torch.testing.assert_close(out.float(), ref, rtol=2.0 ** -7, atol=1e-3 * K)


def _copies(q, s, nbytes):
    """Enough copies of a weight and its scales to exceed ``ROTATE_BYTES`` (at most 64)."""
    n = max(1, min(64, -(-ROTATE_BYTES // nbytes)))
    return [(q, s)] + [(q.clone(), s.clone()) for _ in range(n - 1)]


def _cycler(fn, sets):
    state = [0]

    def call():
        state[0] = (state[0] + 1) % len(sets)
        return fn(*sets[state[0]])
    return call


def _measure(variants, nbytes, iters, rounds):
    """``variants``: name -> zero-argument call. Alternating rounds; bytes/s from the median."""
    ts = {k: [] for k in variants}
    for k, fn in variants.items():   # every shape and kernel warmed before the timed rounds
        timeit(fn, 3, 3)
    for _ in range(rounds):
        for k, fn in variants.items():
            ts[k].append(timeit(fn, iters, 2))
    out = {k: summarise(v) for k, v in ts.items()}
    for k in out:
        out[k]["bytes_per_s"] = nbytes / (out[k]["ms_median"] * 1e-3)
        out[k]["share_of_hbm_peak"] = out[k]["bytes_per_s"] / HBM_PEAK
    if len(variants) == 2:
        a, b = list(variants)
        out[f"{a}_over_{b}"] = out[a]["ms_median"] / out[b]["ms_median"]
    return out


def bench_dense(fmt, M, N, K, iters, rounds, gen):
    import torch

    from ddlb_amd.ops.gemm import gemm, gemm_skinny

    a, sa = _quant((M, K), fmt, gen)
    w, sw = _quant((N, K), fmt, gen, K ** -0.5, weight=True)
    nbytes = weight_bytes(N, K, fmt)
    sets = _copies(w, sw, nbytes)
    out_s = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    out_t = torch.empty_like(out_s)
    skinny = lambda w, sw: gemm_skinny(a, w, out_s, a_scale=sa, w_scale=sw)       # noqa: E731
    tiled = lambda w, sw: gemm(a, w, out_t, a_scale=sa, w_scale=sw)               # noqa: E731
    variants = {"skinny": _cycler(skinny, sets)}
    skinny(w, sw)
    if fmt == "w4a8":
        _check_mixed(out_s, a, sa, w, sw, K)
    else:
        tiled(w, sw)
        torch.cuda.synchronize()
        torch.testing.assert_close(out_s.float(), out_t.float(), rtol=2.0 ** -7, atol=1e-3 * K)
        variants["tiled"] = _cycler(tiled, sets)
    r = _measure(variants, nbytes, iters, rounds)
    r.update(kind="dense", fmt=fmt, M=M, N=N, K=K, weight_bytes=nbytes, copies=len(sets))
    return r


def bench_grouped(fmt, tokens, N, K, layer, iters, rounds, gen):
    import torch

    from ddlb_amd.ops.gemm import gemm_grouped, gemm_skinny_grouped

    E, T = MOE["E"], tokens * MOE["top_k"]
    ids = torch.randint(0, E, (T,), generator=gen, device=gen.device)
    counts = torch.bincount(ids, minlength=E)
    offs = torch.zeros(E + 1, dtype=torch.int32, device=gen.device)
    offs[1:] = torch.cumsum(counts, 0)
    a, sa = _quant((T, K), fmt, gen)
    w, sw = _quant((E * N, K), fmt, gen, K ** -0.5, weight=True)
    w, sw = w.reshape(E, N, -1), sw.reshape(E, N, -1)
    nbytes = weight_bytes(int((counts > 0).sum()) * N, K, fmt)
    sets = _copies(w, sw, weight_bytes(E * N, K, fmt))
    out_s = torch.empty((T, N), dtype=torch.bfloat16, device=a.device)
    out_t = torch.empty_like(out_s)
    skinny = lambda w, sw: gemm_skinny_grouped(a, w, offs, out_s, a_scale=sa,      # noqa: E731
                                               w_scale=sw)
    tiled = lambda w, sw: gemm_grouped(a, w, offs, out_t, a_scale=sa, w_scale=sw)  # noqa: E731
    variants = {"skinny": _cycler(skinny, sets)}
    skinny(w, sw)
    if fmt == "w4a8":  # the expert with the most rows, against the dequantised operands
        e = int(counts.argmax())
        rows = slice(int(offs[e]), int(offs[e + 1]))
        _check_mixed(out_s[rows], a[rows], sa[rows], w[e], sw[e], K)
    else:
        tiled(w, sw)
        torch.cuda.synchronize()
        torch.testing.assert_close(out_s.float(), out_t.float(), rtol=2.0 ** -7, atol=1e-3 * K)
        variants["tiled"] = _cycler(tiled, sets)
    r = _measure(variants, nbytes, iters, rounds)
    r.update(kind="grouped", layer=layer, fmt=fmt, tokens=tokens, T=T, E=E, N=N, K=K,
             experts_with_rows=int((counts > 0).sum()), weight_bytes=nbytes, copies=len(sets))
    return r


def bench_fused(fmt, rows, N, K, grouped, iters, rounds, gen):
    """fc1 of a gated layer, ``rows`` rows (grouped: tokens routed top-k over E experts): the
    chain against the fused call, ``act="silu"``."""
    import torch

    from ddlb_amd.models.mx_mlp import _fmt_ops, _fmt_pair
    from ddlb_amd.ops.gemm import gemm_skinny, gemm_skinny_grouped
    from ddlb_amd.ops.glu import glu

    E = MOE["E"] if grouped else 1
    T = rows * MOE["top_k"] if grouped else rows
    afmt = _fmt_pair(fmt)[0]  # what fc1 writes: the activations' format
    a, sa = _quant((T, K), fmt, gen)
    w, sw = _quant((E * N, K), fmt, gen, K ** -0.5, weight=True)
    pre, used = (), E
    if grouped:
        counts = torch.bincount(torch.randint(0, E, (T,), generator=gen, device=gen.device),
                                minlength=E)
        offs = torch.zeros(E + 1, dtype=torch.int32, device=gen.device)
        offs[1:] = torch.cumsum(counts, 0)
        w, sw, pre, used = w.reshape(E, N, -1), sw.reshape(E, N, -1), (offs,), int((counts > 0).sum())
    f = gemm_skinny_grouped if grouped else gemm_skinny
    quant = _fmt_ops(afmt)[0]
    nbytes = weight_bytes(used * N, K, fmt)
    sets = _copies(w, sw, weight_bytes(E * N, K, fmt))
    chain = lambda w, sw: quant(glu(f(a, w, *pre, a_scale=sa, w_scale=sw,          # noqa: E731
                                      out_dtype=torch.float32), "silu"))
    fused = lambda w, sw: f(a, w, *pre, a_scale=sa, w_scale=sw, act="silu",        # noqa: E731
                            glu=True, out_quant=afmt)
    (q0, s0), (q1, s1) = chain(w, sw), fused(w, sw)
    torch.cuda.synchronize()
    assert torch.equal(q0.view(torch.uint8), q1.view(torch.uint8)) and torch.equal(s0, s1)
    r = _measure({"fused": _cycler(fused, sets), "chain": _cycler(chain, sets)}, nbytes, iters,
                 rounds)
    r.update(kind="fused-grouped" if grouped else "fused-dense", layer="fc1", fmt=fmt, M=rows,
             tokens=rows, T=T, N=N, K=K, weight_bytes=nbytes, copies=len(sets))
    return r


def show(r):
    what = (f"dense M={r['M']:<3d}" if r["kind"].endswith("dense")
            else f"moe {r['layer']} tok={r['tokens']:<3d}")
    line = f"{r['fmt']:6s} {what} N={r['N']:<5d} K={r['K']:<5d} {r['weight_bytes'] / 1e6:8.1f} MB"
    if r["kind"].startswith("fused"):
        for k in ("fused", "chain"):
            v = r[k]
            line += (f" | {k} {v['ms_median'] * 1e3:8.1f} us (min {v['ms_min'] * 1e3:.1f}, "
                     f"spread {100 * v['spread']:.1f} %)")
        print(line + f" | fused / chain {r['fused_over_chain']:.3f}", flush=True)
        return
    for k in ("skinny", "tiled"):
        if k not in r:
            continue
        v = r[k]
        line += (f" | {k} {v['ms_median'] * 1e3:8.1f} us (min {v['ms_min'] * 1e3:.1f}, spread "
                 f"{100 * v['spread']:.1f} %) {v['bytes_per_s'] / 1e12:5.2f} TB/s "
                 f"{100 * v['share_of_hbm_peak']:5.1f} % of peak")
    if "tiled" in r:
        line += f" | skinny / tiled {r['skinny_over_tiled']:.3f}"
    print(line, flush=True)


def main(argv=None):
    import torch

    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--iters", type=int, default=300)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--fmts", default="mx,mxfp4,w4a8")
    p.add_argument("--json", default="")
    p.add_argument("--fused", action="store_true", help="gated fc1: the chain against one call")
    p.add_argument("--shapes", default="all", choices=("all", "moe"), help="with --fused")
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_skinny.py measures on a ROCm GPU; none is visible")
    from ddlb_amd.ops import gemm as G

    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for fmt in a.fmts.split(",") if a.fused else ():
        for M in FUSED_MS if a.shapes == "all" else ():
            rows.append(bench_fused(fmt, M, 2 * 4096, 4096, False, a.iters, a.rounds, gen))
            show(rows[-1])
        for tokens in MOE["tokens"]:
            rows.append(bench_fused(fmt, tokens, 2 * MOE["F"], MOE["H"], True, a.iters, a.rounds,
                                    gen))
            show(rows[-1])
    for fmt in () if a.fused else a.fmts.split(","):
        for N, K in DENSE_NK:
            for M in DENSE_MS:
                rows.append(bench_dense(fmt, M, N, K, a.iters, a.rounds, gen))
                show(rows[-1])
        for tokens in MOE["tokens"]:
            for layer, N, K in (("fc1", 2 * MOE["F"], MOE["H"]), ("fc2", MOE["H"], MOE["F"])):
                rows.append(bench_grouped(fmt, tokens, N, K, layer, a.iters, a.rounds, gen))
                show(rows[-1])
    res = {"device": torch.cuda.get_device_name(0), "cus": G.device_cus(), "nr": G.SKINNY_NR,
           "iters": a.iters, "rounds": a.rounds, "hbm_peak": HBM_PEAK, "rows": rows}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
