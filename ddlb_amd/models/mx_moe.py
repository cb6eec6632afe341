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
    wts = torch.arange(1, experts + 1, dtype=torch.float32)
    if experts >= 4:
        wts[experts // 2] = 0.0
    return torch.multinomial(wts, seq, replacement=True, generator=g)


class MxMoE:
    def __init__(self, hidden: int, ffn: int, seq: int, experts: int, fmt: str = "mx",
                 act: str = "silu", fused: bool = True, seed: int = 0, tile: str = "auto"):
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
        if not torch.cuda.is_available():
            raise RuntimeError("MxMoE runs the native grouped GEMMs: it needs a ROCm GPU "
                               "(MxMoE.reference_chain runs anywhere)")
        self.H, self.F, self.S, self.E = hidden, ffn, seq, experts
        self.act, self.fmt, self.fused, self.tile = act, fmt, bool(fused), tile
        dev = torch.device("cuda", torch.cuda.current_device())
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        bf = torch.bfloat16
        self.X = uniform_pm1((seq, hidden), "bfloat16", g, dev)
        gate, up = ((uniform_pm1((experts, ffn, hidden), "float32", g, dev)
                     * hidden ** -0.5).to(bf) for _ in range(2))
        self.W1 = pack_glu_grouped(gate, up)                                    # [E, 2F, H]
        self.W2 = (uniform_pm1((experts, hidden, ffn), "float32", g, dev) * ffn ** -0.5).to(bf)
        self.ids = expert_ids(seq, experts, seed).to(dev)
        # weights quantised once, row by row: [E * rows, K] for the quantiser, [E, rows, K] back
        w1q, w1s = quant(self.W1.reshape(experts * 2 * ffn, hidden))
        w2q, w2s = quant(self.W2.reshape(experts * hidden, ffn))
        self.w1q, self.w1s = (t.reshape(experts, 2 * ffn, -1) for t in (w1q, w1s))
        self.w2q, self.w2s = (t.reshape(experts, hidden, -1) for t in (w2q, w2s))
        self.ysorted = torch.empty((seq, hidden), dtype=bf, device=dev)
        self.out = torch.empty((seq, hidden), dtype=bf, device=dev)
        torch.cuda.synchronize()

    @property
    def flops(self) -> float:
        """FLOPs of one forward: fc1 has 2F rows per expert, every token visits one expert."""
        return 6.0 * self.S * self.H * self.F

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

    def reference(self):
        return self.reference_chain(self.X, self.W1, self.W2, self.ids, self.act, self.fmt)

    def validate(self, out=None) -> None:
        """:class:`MxMLP`'s bound: ``rtol = 0, atol = 1e-3 ffn`` (fc2's reduction length)."""
        import torch

        out = self.out if out is None else out
        torch.testing.assert_close(out.float(), self.reference(), rtol=0, atol=1e-3 * self.F)
