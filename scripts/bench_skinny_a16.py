"""Microbenchmark: the A16 skinny GEMM (bf16 activations, not quantised) beside the two routes a
16-bit user had before it.

In ONE process, alternating per shape, for each weight form (``mxfp4``: W4A16, ``mx``: W8A16,
``same``: bf16 weights):

    a16    ``gemm_skinny_a16(x, w, w_scale=)`` on the stored weight
    tiled  ``gemm(x, wd)`` in bf16 on the dequantised weight (grouped: ``gemm_grouped``)
    quant  ``quantize_mx(x)`` then ``gemm_skinny`` with MX-fp8 ``x`` on the same MX weight (two
           launches, 8-bit activation error; MX forms only)

Dense M in 1, 16, 64 times (N, K) in (4096, 4096), (8192, 8192), and the MoE shapes of
``bench_skinny.py`` (E = 32, 8 and 64 tokens routed top-4, H = 4096, F = 1536, fc1 and fc2). The
method is ``bench_skinny.py``'s: outputs compared before anything is timed, every variant warmed,
device events around ``iters`` back-to-back calls, variants alternating over ``rounds`` rounds,
median / minimum / spread reported, successive calls walking through weight copies that exceed the
last-level cache. Printed per row: time per call and the stored weight bytes / time of each variant
(``tiled`` streams the bf16 bytes).

    python scripts/bench_skinny_a16.py --json out/skinny_a16.json
"""

from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_skinny import DENSE_NK, MOE, ROTATE_BYTES, _cycler, _measure  # noqa: E402

FORMS = ("mxfp4", "mx", "same")
DENSE_MS = (1, 16, 64)


def _weights(shape, form, gen):
    """``(w, w_scale | None, wd bf16, stored bytes)`` of a random ``[.., N, K]`` weight."""
    import torch

    from ddlb_amd.models.mx_mlp import _fmt_ops

    K = shape[-1]
    x = torch.randn(shape, generator=gen, device=gen.device, dtype=torch.bfloat16) * K ** -0.5
    if form == "same":
        return x, None, x, x.numel() * 2
    quant, _, deq = _fmt_ops(form)
    w, s = quant(x.reshape(-1, K))
    wd = deq(w, s).to(torch.bfloat16).reshape(shape)
    return w.reshape(*shape[:-1], -1), s.reshape(*shape[:-1], -1), wd, w.numel() + s.numel()


def bench(form, rows, N, K, grouped, iters, rounds, gen):
    import torch

    from ddlb_amd.ops import gemm as G
    from ddlb_amd.ops.mx import quantize_mx

    E = MOE["E"] if grouped else 1
    T = rows * MOE["top_k"] if grouped else rows
    x = torch.randn((T, K), generator=gen, device=gen.device, dtype=torch.bfloat16)
    w, sw, wd, stored = _weights((E, N, K) if grouped else (N, K), form, gen)
    pre, used = (), 1
    if grouped:
        counts = torch.bincount(torch.randint(0, E, (T,), generator=gen, device=gen.device),
                                minlength=E)
        offs = torch.zeros(E + 1, dtype=torch.int32, device=gen.device)
        offs[1:] = torch.cumsum(counts, 0)
        pre, used = (offs,), int((counts > 0).sum())
    outs = {k: torch.zeros((T, N), dtype=torch.bfloat16, device=x.device)
            for k in ("a16", "tiled", "quant")}
    a16_f = G.gemm_skinny_a16_grouped if grouped else G.gemm_skinny_a16
    tiled_f = G.gemm_grouped if grouped else G.gemm
    quant_f = G.gemm_skinny_grouped if grouped else G.gemm_skinny

    def quant_first(w, sw):
        xq, xs = quantize_mx(x)
        return quant_f(xq, w, *pre, outs["quant"], a_scale=xs, w_scale=sw)

    calls = {"a16": (lambda w, sw: a16_f(x, w, *pre, outs["a16"], w_scale=sw), (w, sw), stored),
             "tiled": (lambda wd, _: tiled_f(x, wd, *pre, outs["tiled"]), (wd, None),
                       2 * wd.numel())}
    if form != "same":
        calls["quant"] = (quant_first, (w, sw), stored)
    variants = {}
    for k, (fn, first, nbytes) in calls.items():
        fn(*first)
        copies = max(1, min(64, -(-ROTATE_BYTES // nbytes)))  # together past the last-level cache
        sets = [first] + [tuple(None if t is None else t.clone() for t in first)
                          for _ in range(copies - 1)]
        variants[k] = _cycler(fn, sets)
    torch.cuda.synchronize()
    # same operands, f32 accumulation in different orders; quant adds the 8-bit activation error
    torch.testing.assert_close(outs["a16"].float(), outs["tiled"].float(), rtol=2.0 ** -7,
                               atol=1e-3 * K)
    nbytes = stored // E * used
    r = _measure(variants, nbytes, iters, rounds)
    r.update(kind="grouped" if grouped else "dense", form=form, rows=rows, T=T, N=N, K=K,
             weight_bytes=nbytes, experts_with_rows=used)
    return r


def show(r):
    what = f"moe tok={r['rows']:<3d}" if r["kind"] == "grouped" else f"dense M={r['rows']:<3d}"
    line = f"{r['form']:6s} {what} N={r['N']:<5d} K={r['K']:<5d} {r['weight_bytes'] / 1e6:7.1f} MB"
    for k in ("a16", "tiled", "quant"):
        if k in r:
            v = r[k]
            line += (f" | {k} {v['ms_median'] * 1e3:7.1f} us (min {v['ms_min'] * 1e3:.1f}, spread "
                     f"{100 * v['spread']:.1f} %) {v['bytes_per_s'] / 1e12:5.2f} TB/s")
    line += f" | a16 / tiled {r['a16']['ms_median'] / r['tiled']['ms_median']:.3f}"
    if "quant" in r:
        line += f" | a16 / quant {r['a16']['ms_median'] / r['quant']['ms_median']:.3f}"
    print(line, flush=True)


def main(argv=None):
    import torch

    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--iters", type=int, default=200)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--forms", default=",".join(FORMS))
    p.add_argument("--json", default="")
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_skinny_a16.py measures on a ROCm GPU; none is visible")
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for form in a.forms.split(","):
        for N, K in DENSE_NK:
            for M in DENSE_MS:
                rows.append(bench(form, M, N, K, False, a.iters, a.rounds, gen))
                show(rows[-1])
        for tokens in MOE["tokens"]:
            for N, K in ((2 * MOE["F"], MOE["H"]), (MOE["H"], MOE["F"])):
                rows.append(bench(form, tokens, N, K, True, a.iters, a.rounds, gen))
                show(rows[-1])
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds,
           "rows": rows}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
