"""One-GPU routed (mixture-of-experts) gated FFN on the block-scaled matrix pipe, MX-fp8 or MXFP4.

    perm, offsets = sort tokens by expert                 on the device, no host sync
    Xq, sX = quantise(X[perm])                            one streaming quantiser launch
    Hq, sH = act(Xq Wg[e].T) * (Xq Wu[e].T)  quantised    fc1: ONE grouped GEMM, glu + (q, s) out
    Yp     = Hq W2[e].T                                   fc2: ONE grouped GEMM, bf16 out
    Y[perm] = Yp

``X [S, H]``; expert ``e`` owns ``W1[e] = pack_glu(Wg[e], Wu[e])`` ``[2F, H]`` and ``W2[e]``
``[H, F]``, quantised once at set-up. Every token has one seeded expert id
(:func:`expert_ids`): the counts are uneven and, with four experts or more, at least one expert
gets no token. Rows are sorted by expert (a stable sort), so an expert's tokens are one
contiguous run of rows and ``ops.gemm.gemm_grouped`` multiplies each run by its expert's weight
in one launch per layer, whatever the counts: the int32 offsets are computed on the device
(``scatter_add`` / ``cumsum``) and read only by the kernel, so ``forward()`` never waits for the
device and can be captured in a graph. A row-wise quantisation commutes with a row permutation,
so the gathered rows are quantised once.

``reference()`` applies :meth:`MxMLP.reference_chain` (gated) to each expert's rows.

``dispatch="native"`` runs the token side on the HIP dispatch layer (``ddlb_amd.ops.moe``) and
routes every token to ``top_k`` experts::

    offsets, row_token, slot_row = route(ids [S, k])      counting sort, three small launches
    Xq, sX = quantize_mx_gather(X, row_token)             the gather is the quantiser's read
    ...the same two grouped GEMMs over T = S * top_k rows...
    Y = combine(Yp, slot_row, gates)                      weighted sum in j order, deterministic

``top_k = 1`` with gates of 1 is the layer above, bit for bit. The default ``dispatch="torch"`` is
the chain of torch ops at the top and knows only ``top_k = 1``.
"""

from __future__ import annotations

from ddlb_amd.models.mx_mlp import MxMLP, _fmt_ops


def expert_ids(seq: int, experts: int, seed: int = 0):
    """A seeded expert id per token (int64, CPU): expert ``e`` is drawn with weight ``e + 1``, and
    with ``experts >= 4`` expert ``experts // 2`` with weight 0, so it gets no token."""
    import torch

    if experts < 1 or seq < 1:
        raise ValueError("seq and experts must be positive")
    g = torch.Generator()
    g.manual_seed(1000003 * seed + experts)
    return torch.multinomial(_weights(experts), seq, replacement=True, generator=g)


def _weights(experts: int):
    import torch

    wts = torch.arange(1, experts + 1, dtype=torch.float32)
    if experts >= 4:
        wts[experts // 2] = 0.0
    return wts


def expert_ids_topk(seq: int, experts: int, k: int, seed: int = 0):
    """``(ids [S, k] int64, gates [S, k] float32)`` on the CPU, seeded: every token draws ``k``
    distinct experts with :func:`expert_ids`' uneven weights (with ``experts >= 4`` expert
    ``experts // 2`` is never drawn), and non-negative gate weights that sum to 1 per token."""
    import torch

    if experts < 1 or seq < 1 or k < 1:
        raise ValueError("seq, experts and k must be positive")
    wts = _weights(experts)
    drawable = int((wts > 0).sum())
    if k > drawable:
        raise ValueError(f"k = {k} distinct experts per token need at least {k} experts that "
                         f"can be drawn; {experts} experts have {drawable}")
    g = torch.Generator()
    g.manual_seed(1000003 * seed + 1009 * k + experts)
    ids = torch.multinomial(wts.expand(seq, experts), k, replacement=False, generator=g)
    raw = torch.rand((seq, k), generator=g, dtype=torch.float32) + 0.125
    return ids, raw / raw.sum(dim=1, keepdim=True)


DISPATCHES = ("torch", "native")


class MxMoE:
    def __init__(self, hidden: int, ffn: int, seq: int, experts: int, fmt: str = "mx",
                 act: str = "silu", fused: bool = True, seed: int = 0, tile: str = "auto",
                 top_k: int = 1, dispatch: str = "torch"):
        import torch

        from ddlb_amd.ops.gemm import ACTS, MAX_GROUPS, pack_glu_grouped
        from ddlb_amd.primitives.base import uniform_pm1

        quant, _, _ = _fmt_ops(fmt)
        if act not in ACTS:
            raise ValueError(f"act must be one of {tuple(ACTS)}, not {act!r}")
        mod = 256 if fmt == "mxfp4" else 128
        if hidden % mod or ffn % mod:
            raise ValueError(f"fmt={fmt!r} needs hidden and ffn to be multiples of {mod} "
                             f"(hidden = {hidden}, ffn = {ffn})")
        if not 1 <= experts <= MAX_GROUPS:
            raise ValueError(f"experts must be in 1 .. {MAX_GROUPS}, not {experts}")
        if seq <= 0:
            raise ValueError("seq must be positive")
        if dispatch not in DISPATCHES:
            raise ValueError(f"dispatch must be one of {DISPATCHES}, not {dispatch!r}")
        if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 1:
            raise ValueError(f"top_k must be a positive int, not {top_k!r}")
        if top_k > 1 and dispatch != "native":
            raise ValueError(f"top_k = {top_k} needs dispatch='native' (the torch chain routes "
                             "every token to one expert)")
        if experts < top_k:
            raise ValueError(f"top_k = {top_k} needs at least that many experts, not {experts}")
        if not torch.cuda.is_available():
            raise RuntimeError("MxMoE runs the native grouped GEMMs: it needs a ROCm GPU "
                               "(MxMoE.reference_chain runs anywhere)")
        self.H, self.F, self.S, self.E = hidden, ffn, seq, experts
        self.act, self.fmt, self.fused, self.tile = act, fmt, bool(fused), tile
        self.top_k, self.dispatch = top_k, dispatch
        dev = torch.device("cuda", torch.cuda.current_device())
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        bf = torch.bfloat16
        self.X = uniform_pm1((seq, hidden), "bfloat16", g, dev)
        gate, up = ((uniform_pm1((experts, ffn, hidden), "float32", g, dev)
                     * hidden ** -0.5).to(bf) for _ in range(2))
        self.W1 = pack_glu_grouped(gate, up)                                    # [E, 2F, H]
        self.W2 = (uniform_pm1((experts, hidden, ffn), "float32", g, dev) * ffn ** -0.5).to(bf)
        if dispatch == "native" and top_k > 1:
            ids, gates = expert_ids_topk(seq, experts, top_k, seed)
            self.ids, self.gates = ids.to(dev), gates.to(dev)
        elif dispatch == "native":  # the torch path's routing as [S, 1], every gate 1
            self.ids = expert_ids(seq, experts, seed).to(dev).reshape(seq, 1)
            self.gates = torch.ones((seq, 1), dtype=torch.float32, device=dev)
        else:
            self.ids = expert_ids(seq, experts, seed).to(dev)
        # weights quantised once, row by row: [E * rows, K] for the quantiser, [E, rows, K] back
        w1q, w1s = quant(self.W1.reshape(experts * 2 * ffn, hidden))
        w2q, w2s = quant(self.W2.reshape(experts * hidden, ffn))
        self.w1q, self.w1s = (t.reshape(experts, 2 * ffn, -1) for t in (w1q, w1s))
        self.w2q, self.w2s = (t.reshape(experts, hidden, -1) for t in (w2q, w2s))
        self.ysorted = torch.empty((seq * top_k, hidden), dtype=bf, device=dev)
        self.out = torch.empty((seq, hidden), dtype=bf, device=dev)
        torch.cuda.synchronize()

    @property
    def flops(self) -> float:
        """FLOPs of one forward: fc1 has 2F rows per expert, every token visits top_k experts."""
        return 6.0 * self.S * self.top_k * self.H * self.F

    def route(self):
        """``(perm, offsets)`` on the device with no host sync: the stable sort permutation of the
        tokens by expert and the int32 ``[E + 1]`` row offsets of the experts' runs.
        (``scatter_add_`` counts the tokens: ``torch.bincount`` reads its output size back.)"""
        import torch

        perm = torch.argsort(self.ids, stable=True)
        counts = torch.zeros(self.E, dtype=torch.int32, device=self.ids.device)
        counts.scatter_add_(0, self.ids, torch.ones_like(self.ids, dtype=torch.int32))
        offsets = torch.zeros(self.E + 1, dtype=torch.int32, device=self.ids.device)
        offsets[1:] = torch.cumsum(counts, 0)
        return perm, offsets

    def forward(self):
        import torch

        from ddlb_amd.ops.gemm import gemm_grouped

        quant, _, _ = _fmt_ops(self.fmt)
        native = self.dispatch == "native"
        if native:
            from ddlb_amd.ops.moe import combine, route
            from ddlb_amd.ops.mx import quantize_mx_gather

            offsets, row_token, slot_row = route(self.ids, self.E)
            xq, xs = quantize_mx_gather(self.X, row_token, fmt=self.fmt)
        else:
            perm, offsets = self.route()
            xq, xs = quant(self.X.index_select(0, perm))
        if self.fused:
            hq, hs = gemm_grouped(xq, self.w1q, offsets, a_scale=xs, w_scale=self.w1s,
                                  act=self.act, tile=self.tile, glu=True, out_quant=self.fmt)
        else:
            h = gemm_grouped(xq, self.w1q, offsets, a_scale=xs, w_scale=self.w1s, act=self.act,
                             tile=self.tile, glu=True, out_dtype=torch.bfloat16)
            hq, hs = quant(h)
        gemm_grouped(hq, self.w2q, offsets, self.ysorted, a_scale=hs, w_scale=self.w2s,
                     tile=self.tile)
        if native:
            combine(self.ysorted, slot_row, self.gates, out=self.out)
        else:
            self.out.index_copy_(0, perm, self.ysorted)
        return self.out

    @staticmethod
    def reference_chain(X, W1, W2, ids, act: str = "silu", fmt: str = "mx"):
        """The fp32 torch chain (any device): :meth:`MxMLP.reference_chain` (gated) with expert
        ``e``'s weights on the rows whose id is ``e``. ``W1 [E, 2F, H]`` packed, ``W2 [E, H, F]``."""
        import torch

        out = torch.zeros((X.shape[0], W2.shape[1]), dtype=torch.float32, device=X.device)
        for e in range(W1.shape[0]):
            rows = torch.nonzero(ids == e).flatten()
            if rows.numel():
                out[rows] = MxMLP.reference_chain(X[rows], W1[e], W2[e], act, fmt, gated=True)
        return out

    @staticmethod
    def reference_chain_topk(X, W1, W2, ids, gates, act: str = "silu", fmt: str = "mx"):
        """The fp32 chain of a top-k layer (any device): :meth:`reference_chain` per choice ``j``
        of ``ids [S, k]``, weighted by ``gates[:, j]`` and summed in ``j`` order."""
        import torch

        out = torch.zeros((X.shape[0], W2.shape[1]), dtype=torch.float32, device=X.device)
        for j in range(ids.shape[1]):
            out = out + gates[:, j:j + 1].to(torch.float32) * MxMoE.reference_chain(
                X, W1, W2, ids[:, j], act, fmt)
        return out

    def reference(self):
        if self.dispatch == "native":
            return self.reference_chain_topk(self.X, self.W1, self.W2, self.ids, self.gates,
                                             self.act, self.fmt)
        return self.reference_chain(self.X, self.W1, self.W2, self.ids, self.act, self.fmt)

    def validate(self, out=None) -> None:
        """:class:`MxMLP`'s bound: ``rtol = 0, atol = 1e-3 ffn`` (fc2's reduction length). It holds
        unchanged for ``top_k > 1``: the gates form a convex combination of rows that each meet
        it."""
        import torch

        out = self.out if out is None else out
        torch.testing.assert_close(out.float(), self.reference(), rtol=0, atol=1e-3 * self.F)
