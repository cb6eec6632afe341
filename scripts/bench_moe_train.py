"""Microbenchmark: one training step of the routed gated FFN (``MxMoEFFN``) and the three
streaming kernels it adds, in ONE process at a transformer-sized shape.

* ``forward`` and ``forward+backward`` of ``MxMoEFFN`` (gradients of ``x``, both weights and the
  gates);
* each new kernel alone with the bytes it moves and the GB/s it reaches: ``glu``, ``glu_bwd``,
  ``gather``, ``combine_bwd`` (with and without ``dgate``);
* the yardsticks in the same run: ``combine`` (it moves rows exactly as the new kernels do) and the
  row quantiser ``quantize_mx``;
* the same three ops written with torch ops (``index_select``; silu * up and its autograd
  backward; the multiply, ``index_copy`` and row dot products of the combine's backward).

Variants are interleaved over several rounds, device events around ``iters`` back-to-back calls;
reported are the median, the minimum and the round-to-round spread. Results are checked against
the references before anything is timed.

    python scripts/bench_moe_train.py --json out/moe_train.json
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


def summarise(ts, nbytes=None):
    med = statistics.median(ts)
    out = {"ms_median": med, "ms_min": min(ts), "ms_max": max(ts),
           "spread": (max(ts) - min(ts)) / med}
    if nbytes:
        out["bytes"] = nbytes
        out["gbps"] = nbytes / med / 1e6
    return out


def interleaved(variants, rounds, iters):
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, _) in variants.items():
            times[k].append(timeit(fn, iters))
    return {k: summarise(times[k], variants[k][1]) for k in variants}


def main(argv=None):
    import torch

    from ddlb_amd.models.mx_moe import expert_ids_topk
    from ddlb_amd.models.mx_moe_ffn import MxMoEFFN
    from ddlb_amd.ops.glu import glu, glu_bwd, glu_bwd_reference
    from ddlb_amd.ops.moe import (combine, combine_bwd, combine_bwd_reference, gather,
                                  gather_reference, route)
    from ddlb_amd.ops.mx import quantize_mx

    p = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    p.add_argument("--seq", type=int, default=8192)
    p.add_argument("--hidden", type=int, default=4096)
    p.add_argument("--ffn", type=int, default=2048)
    p.add_argument("--experts", type=int, default=8)
    p.add_argument("--top-k", type=int, default=2)
    p.add_argument("--fmt", default="mx")
    p.add_argument("--act", default="silu")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--json", default=None)
    a = p.parse_args(argv)
    S, H, F, E, k = a.seq, a.hidden, a.ffn, a.experts, a.top_k
    T = S * k
    dev = torch.device("cuda", torch.cuda.current_device())
    bf = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)

    def pm1(*shape):
        return (torch.rand(shape, generator=g, device=dev) * 2 - 1).to(bf)

    ids, gates = (t.to(dev) for t in expert_ids_topk(S, E, k))
    x, dout = pm1(S, H), pm1(S, H)
    offsets, row_token, slot_row = route(ids, E)
    c1, dh, yp = pm1(T, 2 * F), pm1(T, F), pm1(T, H)
    ones = torch.ones_like(gates)

    # ---- the results, before anything is timed
    assert torch.equal(gather(x, row_token), gather_reference(x, row_token))
    dy, dgate = combine_bwd(dout, slot_row, gates, row_token, yp)
    dy_ref, dg_ref = combine_bwd_reference(dout, slot_row, gates, row_token, yp)
    assert torch.equal(dy, dy_ref)
    assert float((dgate.double() - dg_ref).abs().max()) <= 1e-3 * float(dg_ref.abs().max())
    dc = glu_bwd(dh[:256], c1[:256], a.act)
    torch.testing.assert_close(dc.double(), glu_bwd_reference(dh[:256], c1[:256], a.act),
                               rtol=2.0 ** -7, atol=2.0 ** -14)

    # ---- the same ops in torch
    def torch_glu():
        v = c1.view(T, -1, 2, 32)
        return (torch.nn.functional.silu(v[:, :, 0].float()) * v[:, :, 1].float()).to(bf) \
            .reshape(T, F)

    c1r = c1.clone().requires_grad_()

    def torch_glu_fwd_bwd():
        v = c1r.view(T, -1, 2, 32)
        h = (torch.nn.functional.silu(v[:, :, 0].float()) * v[:, :, 1].float()).to(bf)
        return torch.autograd.grad(h.reshape(T, F), c1r, dh)[0]

    tok = row_token.clamp(min=0).long()
    flat_gate = torch.zeros(T, device=dev)      # the gate of the slot sorted to row r
    valid = slot_row.reshape(-1) >= 0
    flat_gate[slot_row.reshape(-1)[valid].long()] = gates.reshape(-1)[valid]

    def torch_gather():
        return x.index_select(0, tok)

    def torch_combine_bwd():
        d = dout.index_select(0, tok).float()
        return (flat_gate.unsqueeze(1) * d).to(bf), (d * yp.float()).sum(dim=1)

    esz = 2
    row_bytes = H * esz
    variants = {
        "glu": (lambda: glu(c1, a.act), T * 3 * F * esz),
        "glu_bwd": (lambda: glu_bwd(dh, c1, a.act), T * 5 * F * esz),
        "gather": (lambda: gather(x, row_token), 2 * T * row_bytes),
        "combine_bwd": (lambda: combine_bwd(dout, slot_row, gates, row_token, yp),
                        (S + 2 * T) * row_bytes),
        "combine_bwd_no_dgate": (lambda: combine_bwd(dout, slot_row, gates, row_token),
                                 (S + T) * row_bytes),
        "combine (yardstick)": (lambda: combine(yp, slot_row, gates), (S + T) * row_bytes),
        "gather_bwd = combine(ones)": (lambda: combine(yp, slot_row, ones), (S + T) * row_bytes),
        "quantize_mx (yardstick)": (lambda: quantize_mx(yp), T * H * (esz + 1) + T * H // 32),
        "torch glu": (torch_glu, None),
        "torch glu fwd+bwd": (torch_glu_fwd_bwd, None),
        "torch gather (index_select)": (torch_gather, None),
        "torch combine_bwd": (torch_combine_bwd, None),
    }
    res = {"shape": dict(S=S, H=H, F=F, E=E, k=k, fmt=a.fmt, act=a.act, dtype="bfloat16"),
           "kernels": interleaved(variants, a.rounds, a.iters)}

    # ---- the layer
    layer = MxMoEFFN(E, H, F, fmt=a.fmt, act=a.act, device=dev)
    xr = x.clone().requires_grad_()
    gr = gates.clone().requires_grad_()
    params = [xr, layer.fc1.weight, layer.fc2.weight, gr]

    def fwd():
        with torch.no_grad():
            return layer(x, ids, gates)

    def fwd_bwd():
        return torch.autograd.grad(layer(xr, ids, gr), params, dout)

    flops = 6.0 * T * H * F
    lay = interleaved({"forward": (fwd, None), "forward+backward": (fwd_bwd, None)}, a.rounds,
                      max(2, a.iters // 4))
    lay["forward"]["tflops"] = flops / lay["forward"]["ms_median"] / 1e9
    lay["forward+backward"]["tflops"] = 3 * flops / lay["forward+backward"]["ms_median"] / 1e9
    res["layer"] = lay

    yard = res["kernels"]["combine (yardstick)"]["gbps"]
    print(f"MxMoEFFN S={S} H={H} F={F} E={E} k={k} {a.fmt} {a.act} bf16 (T = {T} rows)")
    for name, r in res["kernels"].items():
        bw = (f"{r['gbps']:8.0f} GB/s  {100 * r['gbps'] / yard:5.0f} % of combine"
              if "gbps" in r else "")
        print(f"  {name:30s} {r['ms_median'] * 1e3:9.1f} us (min {r['ms_min'] * 1e3:.1f}, "
              f"spread {100 * r['spread']:.0f} %) {bw}")
    for name, r in lay.items():
        print(f"  {name:30s} {r['ms_median']:9.3f} ms (min {r['ms_min']:.3f}, spread "
              f"{100 * r['spread']:.0f} %) {r['tflops']:7.1f} TFLOP/s")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
