"""The host-side rules of the tiled GEMM's forms as one table (no GPU): what ``_check_fp4``,
``_check_scales``, ``_check_out_quant``, ``_check_glu``, ``_check_grouped`` and ``_check_kgrouped``
(``ddlb_amd/ops/gemm.py``) answer for CPU tensors under a named list of perturbations, applied
singly (all of them to two forms per entry point, a selection to the rest) and, for those two
forms, in ordered pairs (the pairs fix the precedence between rules). One line per case,

    entry form perturbation[+perturbation] -> ExcType: message      or      -> ok <returned tuple>

compared line for line with ``tests/gemm_refusals_expected.txt``. The table was generated before
the checks were gathered into one rule set; a rewrite of the checks must reproduce it. The mxfp4
lines are a section of their own, skipped where torch has no ``float4_e2m1fn_x2``."""

import os

import pytest
import torch

from ddlb_amd.ops import gemm as G

FP8 = torch.float8_e4m3fn
FP4 = getattr(torch, "float4_e2m1fn_x2", None)
M, N, K, E = 64, 1024, 512, 3
EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_refusals_expected.txt")


def _operand(form, rows, k, dev):
    if form == "mxfp4":
        return torch.zeros(rows, k // 2, dtype=torch.uint8, device=dev).view(FP4)
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "mxfp8": FP8}[form]
    return torch.zeros(rows, k, device=dev).to(dt)


def _u8(dev, *shape):
    return torch.zeros(*shape, dtype=torch.uint8, device=dev)


def _base(entry, form, variant, dev="cpu"):
    """The accepted case of an entry point: tensors and keyword arguments by name."""
    scaled = form in ("mxfp8", "mxfp4")
    c = dict(entry=entry, form=form, variant=variant, dev=dev, scaled=scaled,
             glu=entry == "glu" or "glu" in variant,
             out_quant=next((q for q in ("mxfp4", "mx") if variant.endswith(q)), None),
             a=_operand(form, M, K, dev), out=None, out_scale=None, out_dtype=None, tile="auto",
             mode="auto", M=None, a_grp=0, c_grp=0, ksplit=0, act="none",
             a_scale=_u8(dev, M, K // 32) if scaled else None)
    if entry == "grouped":
        c["w"] = _operand(form, E * N, K, dev).view(torch.uint8 if form == "mxfp4" else
                                                    c["a"].dtype).reshape(E, N, -1)
        if form == "mxfp4":
            c["w"] = c["w"].view(FP4)
        c["w_scale"] = _u8(dev, E, N, K // 32) if scaled else None
        c["offsets"] = torch.zeros(E + 1, dtype=torch.int32, device=dev)
    elif entry == "kgrouped":
        mod = 256 if form == "mxfp4" else 128
        c["cap"] = G.kgrouped_capacity(300, E, mod)
        c["a"], c["w"] = _operand(form, M, c["cap"], dev), _operand(form, N, c["cap"], dev)
        c["a_scale"], c["w_scale"] = _u8(dev, M, c["cap"] // 32), _u8(dev, N, c["cap"] // 32)
        c["offsets"] = torch.zeros(E + 1, dtype=torch.int32, device=dev)
        c["rows"] = 300
    else:
        c["w"] = _operand(form, N, K, dev)
        c["w_scale"] = _u8(dev, N, K // 32) if scaled else None
    if entry in ("fp4", "scales"):
        c["out"] = torch.zeros(M, N, dtype=torch.bfloat16, device=dev)
    return c


def _call(c):
    e = c["entry"]
    if e == "fp4":
        return G._check_fp4(c["a"], c["w"], c["out"], c["a_scale"], c["w_scale"],
                            c["a"].shape[0] if c["M"] is None else c["M"], c["tile"], c["mode"],
                            c["a_grp"], c["ksplit"])
    if e == "scales":
        return G._check_scales(c["a"], c["w"], c["a_scale"], c["w_scale"],
                               c["a"].shape[0] if c["M"] is None else c["M"], c["tile"],
                               c["mode"], c["a_grp"], c["ksplit"])
    common = dict(a_scale=c["a_scale"], w_scale=c["w_scale"], tile=c["tile"],
                  out_dtype=c["out_dtype"])
    plain = dict(mode=c["mode"], M=c["M"], a_grp=c["a_grp"], c_grp=c["c_grp"], ksplit=c["ksplit"])
    if e == "out_quant":
        return G._check_out_quant(c["a"], c["w"], c["out_quant"], c["out"], c["out_scale"],
                                  **common, **plain)
    if e == "glu":
        return G._check_glu(c["a"], c["w"], c["out"], c["out_scale"], out_quant=c["out_quant"],
                            act=c["act"], **common, **plain)
    if e == "grouped":
        return G._check_grouped(c["a"], c["w"], c["offsets"], c["out"], c["out_scale"],
                                act=c["act"], out_quant=c["out_quant"], glu=c["glu"], **common)
    return G._check_kgrouped(c["a"], c["w"], c["offsets"], c["rows"], c["out"], **common)


# ---------------------------------------------------------------- perturbations
def _cols(c):
    """Columns of the output, and of its stored tensor."""
    n = c["w"].shape[-2] // 2 if c["glu"] else c["w"].shape[-2]
    return n, (n // 2 if c["out_quant"] == "mxfp4" else n)


def _make_out(c, dtype=None, rows=None, pad=0):
    """A well-formed preallocated output for the case (3-D for K-grouped)."""
    dev, (n, stored) = c["a"].device, _cols(c)
    rows = c["a"].shape[0] if rows is None else rows
    if c["entry"] == "kgrouped":
        return torch.zeros(E, rows, n + pad, dtype=dtype or torch.bfloat16, device=dev)[:, :, :n]
    if c["out_quant"] and dtype is None:
        return _u8(dev, rows, stored + pad).view(G.out_quant_dtype(c["out_quant"]))[:, :stored]
    dense = torch.bfloat16 if c["scaled"] else c["a"].dtype
    return torch.zeros(rows, n + pad, dtype=dtype or dense, device=dev)[:, :n]


def _set(key, fn, needs=None):
    def apply(c):
        if needs is not None and not needs(c):
            return False
        c[key] = fn(c)
        return True
    return apply


def _meta(c):
    for k, v in c.items():
        if isinstance(v, torch.Tensor):
            c[k] = v.to("meta")
    return True


def _wide(t):
    """The same shape with rows 2^25 bytes apart (meta: shapes and strides without the bytes)."""
    return torch.zeros(*t.shape[:-1], 2 ** 25, dtype=torch.uint8, device="meta")[..., :t.shape[-1]]


def _n_to(n):
    """w with ``n`` rows (per expert), its scales following."""
    def apply(c):
        c["w"] = c["w"][..., :n, :]
        if c["w_scale"] is not None:
            c["w_scale"] = c["w_scale"][..., :n, :]
        return True
    return apply


def _k_to(k):
    """Every operand cut to ``k`` elements per row, scales following (rows keep their pitch)."""
    def apply(c):
        if c["entry"] == "kgrouped":
            return False
        per = 2 if c["form"] == "mxfp4" else 1
        c["a"], c["w"] = c["a"][..., :k // per], c["w"][..., :k // per]
        for s in ("a_scale", "w_scale"):
            if c[s] is not None:
                c[s] = c[s][..., :k // 32]
        return True
    return apply


def _strided(t, shape, strides):
    """Zeros of ``t``'s dtype and device with the given shape and element strides."""
    raw = torch.uint8 if t.element_size() == 1 else t.dtype
    n = 1 + sum((d - 1) * st for d, st in zip(shape, strides))
    return torch.zeros(n, dtype=raw, device=t.device).as_strided(tuple(shape), strides).view(t.dtype)


def _has(key):
    return lambda c: c.get(key) is not None


def _takes(*keys):
    return lambda c: c["entry"] in keys


_PLAIN = _takes("fp4", "scales", "out_quant", "glu")
_OUT = _takes("out_quant", "glu", "grouped", "kgrouped")
_QUANT = lambda c: c["out_quant"] is not None  # noqa: E731
_GROUPED = _takes("grouped", "kgrouped")


def _other_dtype(c):
    return torch.float16 if c["a"].dtype == torch.bfloat16 else torch.bfloat16


def _offset_scale(key, off):
    def fn(c):
        s = c[key]
        flat = torch.zeros(s.numel() + 16, dtype=torch.uint8, device=s.device)
        return flat[off:off + s.numel()].view(s.shape)
    return fn


PERTURBATIONS = [
    # operands: dtype, rank, K
    ("w_dtype", _set("w", lambda c: torch.zeros(c["w"].shape, device=c["w"].device)
                     .to(_other_dtype(c)))),
    ("a_f32", _set("a", lambda c: torch.zeros(c["a"].shape, device=c["a"].device))),
    ("both_f32", lambda c: _set("a", lambda c: c["a"].view(torch.uint8).float()
                                if c["a"].element_size() == 1 else c["a"].float())(c) and
     _set("w", lambda c: c["w"].view(torch.uint8).float()
          if c["w"].element_size() == 1 else c["w"].float())(c)),
    ("a_3d", _set("a", lambda c: c["a"][None])),
    ("w_1d", _set("w", lambda c: c["w"].reshape(-1))),
    ("w_rank_other", _set("w", lambda c: c["w"][0] if c["w"].dim() == 3 else c["w"][None])),
    ("a_K-32", _set("a", lambda c: c["a"][:, :-32])),
    ("K=384", _k_to(384)),
    ("K=448", _k_to(448)),
    # scales: presence, dtype, shape, stride, alignment, span
    ("no_a_scale", _set("a_scale", lambda c: None, _has("a_scale"))),
    ("no_w_scale", _set("w_scale", lambda c: None, _has("w_scale"))),
    ("no_scales", lambda c: _set("a_scale", lambda c: None, _has("a_scale"))(c) and
     _set("w_scale", lambda c: None)(c)),
    ("scales_on_16_bit", lambda c: not c["scaled"] and
     _set("a_scale", lambda c: _u8(c["a"].device, c["a"].shape[0], K // 32))(c) and
     _set("w_scale", lambda c: _u8(c["a"].device, *c["w"].shape[:-1], K // 32))(c)),
    ("a_scale_only_on_16_bit", lambda c: not c["scaled"] and
     _set("a_scale", lambda c: _u8(c["a"].device, c["a"].shape[0], K // 32))(c)),
    ("a_scale_int8", _set("a_scale", lambda c: c["a_scale"].to(torch.int8), _has("a_scale"))),
    ("w_scale_list", _set("w_scale", lambda c: [1, 2], _has("w_scale"))),
    ("a_scale_short", _set("a_scale", lambda c: c["a_scale"][:, :-4], _has("a_scale"))),
    ("w_scale_rows-1", _set("w_scale", lambda c: c["w_scale"][..., :-1, :], _has("w_scale"))),
    ("w_scale_rank_other", _set("w_scale", lambda c: c["w_scale"][0] if c["w_scale"].dim() == 3
                                else c["w_scale"][None], _has("w_scale"))),
    ("a_scale_transposed", _set("a_scale", lambda c: c["a_scale"].t().contiguous().t(),
                                _has("a_scale"))),
    ("a_scale_pitch+4", _set("a_scale", lambda c: _u8(c["a"].device, c["a_scale"].shape[0],
                                                      c["a_scale"].shape[1] + 4)[:, :-4],
                             _has("a_scale"))),
    ("w_scale_pitch+2", _set("w_scale", lambda c: _u8(c["a"].device, *c["w_scale"].shape[:-1],
                                                      c["w_scale"].shape[-1] + 2)[..., :-2],
                             _has("w_scale"))),
    ("a_scale+1", _set("a_scale", _offset_scale("a_scale", 1), _has("a_scale"))),
    ("a_scale+4", _set("a_scale", _offset_scale("a_scale", 4), _has("a_scale"))),
    ("w_scale+4", _set("w_scale", _offset_scale("w_scale", 4), _has("w_scale"))),
    ("a_scale_meta", _set("a_scale", lambda c: c["a_scale"].to("meta"), _has("a_scale"))),
    ("a_scale_span", lambda c: c["a_scale"] is not None and _meta(c) and
     _set("a_scale", lambda c: _wide(c["a_scale"]))(c)),
    ("w_scale_span", lambda c: c["w_scale"] is not None and c["w_scale"].dim() == 2 and _meta(c)
     and _set("w_scale", lambda c: _wide(c["w_scale"]))(c)),
    # tile, mode, K-split, rows
    *[(f"tile={t}", _set("tile", lambda c, t=t: t))
      for t in G.TILES if t != "auto" and t not in G.SCALED_TILES],
    ("tile=nonsense", _set("tile", lambda c: "nonsense")),
    ("tile=128x128", _set("tile", lambda c: "128x128")),
    ("mode=generic", _set("mode", lambda c: "generic", _PLAIN)),
    ("mode=mx", _set("mode", lambda c: "mx", _PLAIN)),
    ("mode=nonsense", _set("mode", lambda c: "nonsense", _PLAIN)),
    ("ksplit=2", _set("ksplit", lambda c: 2, _PLAIN)),
    ("a_grp=32", _set("a_grp", lambda c: 32, _PLAIN)),
    ("c_grp=32", _set("c_grp", lambda c: 32, _takes("out_quant", "glu"))),
    ("M=32", _set("M", lambda c: 32, _PLAIN)),
    ("M=65", _set("M", lambda c: 65, _PLAIN)),
    ("M=-1", _set("M", lambda c: -1, _PLAIN)),
    # N off each modulus
    *[(f"N={n}", _n_to(n)) for n in (1024 - 32, 1024 - 64, 1024 - 128, 1024 - 256, 512, 0)],
    # the output
    ("out", _set("out", lambda c: _make_out(c), _OUT)),
    ("out_rows+8_pitch+16", _set("out", lambda c: _make_out(c, rows=c["a"].shape[0] + 8, pad=16),
                                 _OUT)),
    ("out_f32", _set("out", lambda c: _make_out(c, torch.float32))),
    ("out_f64", _set("out", lambda c: _make_out(c, torch.float64))),
    ("out_other_16_bit", _set("out", lambda c: _make_out(c, _other_dtype(c)), _OUT)),
    ("out_fp8", _set("out", lambda c: _make_out(c, torch.float32).to(FP8))),
    ("out_rows-1", _set("out", lambda c: _make_out(c, rows=c["a"].shape[0] - 1), _OUT)),
    ("out_cols-32", _set("out", lambda c: _make_out(c)[..., :-32], _OUT)),
    ("out_rank_other", _set("out", lambda c: _make_out(c)[0] if c["entry"] == "kgrouped"
                            else _make_out(c)[None], _OUT)),
    ("out_transposed", _set("out", lambda c: (lambda o: _strided(
        o, o.shape, (*o.stride()[:-2], 1, o.shape[-2])))(_make_out(c).contiguous()), _OUT)),
    ("out_pitch+1", _set("out", lambda c: _make_out(c, pad=1), _OUT)),
    ("out_meta", _set("out", lambda c: _make_out(c).to("meta"), _OUT)),
    ("out_scale", _set("out_scale", lambda c: _u8(c["a"].device, c["a"].shape[0],
                                                  _cols(c)[0] // 32), _OUT)),
    ("out_scale_int8", _set("out_scale", lambda c: _u8(c["a"].device, c["a"].shape[0],
                                                       _cols(c)[0] // 32).to(torch.int8), _QUANT)),
    ("out_scale_cols-4", _set("out_scale", lambda c: _u8(c["a"].device, c["a"].shape[0],
                                                         _cols(c)[0] // 32)[:, :-4], _QUANT)),
    ("out_scale_pitch+2", _set("out_scale", lambda c: _u8(c["a"].device, c["a"].shape[0],
                                                          _cols(c)[0] // 32 + 2)[:, :-2], _QUANT)),
    ("out_scale_pitch+4", _set("out_scale", lambda c: _u8(c["a"].device, c["a"].shape[0],
                                                          _cols(c)[0] // 32 + 4)[:, :-4], _QUANT)),
    ("out_scale_meta", _set("out_scale", lambda c: _u8("meta", c["a"].shape[0],
                                                       _cols(c)[0] // 32), _QUANT)),
    ("out_scale_span", lambda c: _QUANT(c) and _meta(c) and
     _set("out_scale", lambda c: _wide(_u8("meta", c["a"].shape[0], _cols(c)[0] // 32)))(c)),
    ("out_dtype=f32", _set("out_dtype", lambda c: torch.float32, _OUT)),
    ("out_dtype=f64", _set("out_dtype", lambda c: torch.float64, _OUT)),
    ("out_dtype=other_16_bit", _set("out_dtype", _other_dtype, _OUT)),
    ("out_dtype=fp8", _set("out_dtype", lambda c: FP8, _OUT)),
    ("out_quant=nonsense", _set("out_quant", lambda c: "nonsense",
                                _takes("out_quant", "glu", "grouped"))),
    ("act=silu", _set("act", lambda c: "silu", _takes("glu", "grouped"))),
    ("act=nonsense", _set("act", lambda c: "nonsense", _takes("glu", "grouped"))),
    # offsets, groups, expert strides, rows / capacity
    ("offsets_int64", _set("offsets", lambda c: c["offsets"].long(), _GROUPED)),
    ("offsets_list", _set("offsets", lambda c: [0] * (E + 1), _GROUPED)),
    ("offsets_2d", _set("offsets", lambda c: c["offsets"][None], _GROUPED)),
    ("offsets_E+2", _set("offsets", lambda c: torch.zeros(E + 2, dtype=torch.int32,
                                                          device=c["a"].device), _GROUPED)),
    ("offsets_strided", _set("offsets", lambda c: torch.zeros(2 * (E + 1), dtype=torch.int32,
                                                              device=c["a"].device)[::2],
                             _GROUPED)),
    ("offsets_meta", _set("offsets", lambda c: c["offsets"].to("meta"), _GROUPED)),
    ("offsets_1", _set("offsets", lambda c: c["offsets"][:1], _GROUPED)),
    ("offsets_1026", _set("offsets", lambda c: torch.zeros(1026, dtype=torch.int32,
                                                           device=c["a"].device), _GROUPED)),
    ("E=0", _set("w", lambda c: c["w"][:0], _takes("grouped"))),
    ("E=1025", lambda c: c["entry"] == "grouped" and
     _set("w", lambda c: c["w"][:1, :64].expand(1025, -1, -1))(c) and
     _set("offsets", lambda c: torch.zeros(1026, dtype=torch.int32, device=c["a"].device))(c)),
    ("w_experts_overlap", _set("w", lambda c: c["w"][:1].expand(E, -1, -1), _takes("grouped"))),
    ("w_experts_8_bytes_off", _set("w", lambda c: _strided(
        c["w"], c["w"].shape, (c["w"][0].numel() + 8 // c["w"].element_size(), c["w"].shape[2], 1)),
        _takes("grouped"))),
    ("w_inner_stride", _set("w", lambda c: _strided(
        c["w"], c["w"].shape, (c["w"][0].numel(), 1, c["w"].shape[1])), _takes("grouped"))),
    ("w_scale_experts_overlap", lambda c: c["entry"] == "grouped" and c["w_scale"] is not None and
     _set("w_scale", lambda c: c["w_scale"][:1].expand(E, -1, -1))(c)),
    ("w_scale_experts_2_bytes_off", lambda c: c["entry"] == "grouped" and c["w_scale"] is not None
     and _set("w_scale", lambda c: _u8(c["a"].device, E, c["w_scale"][0].numel() + 2)[:, :-2]
              .view(c["w_scale"].shape))(c)),
    ("rows=float", _set("rows", lambda c: 300.0, _takes("kgrouped"))),
    ("rows=True", _set("rows", lambda c: True, _takes("kgrouped"))),
    ("rows=-1", _set("rows", lambda c: -1, _takes("kgrouped"))),
    ("rows=2^31", _set("rows", lambda c: 2 ** 31, _takes("kgrouped"))),
    ("rows+256", _set("rows", lambda c: c["rows"] + 256, _takes("kgrouped"))),
    ("rows=0", _set("rows", lambda c: 0, _takes("kgrouped"))),
    ("a_inner_stride", _set("a", lambda c: _strided(c["a"], c["a"].shape, (1, c["a"].shape[0])),
                            _takes("kgrouped"))),
    ("out_groups_overlap", _set("out", lambda c: _make_out(c)[:1].expand(E, -1, -1),
                                _takes("kgrouped"))),
    ("out_groups_4_bytes_off", _set(
        "out", lambda c: torch.zeros(E, M * N + 2, dtype=torch.bfloat16,
                                     device=c["a"].device)[:, :-2].view(E, M, N),
        _takes("kgrouped"))),
]

# what a case runs: every perturbation ("full"), one per kind of rule ("core"), or the ones whose
# answer depends on the output of the variant ("out")
CORE_KEYS = ("w_dtype", "a_f32", "a_3d", "a_K-32", "K=384", "no_w_scale", "no_scales",
             "scales_on_16_bit", "a_scale_int8", "a_scale_short", "a_scale_pitch+4", "a_scale+4",
             "a_scale_span", "tile=pt4", "tile=256x256", "mode=generic", "mode=mx", "ksplit=2",
             "a_grp=32", "c_grp=32", "M=65", "N=992", "out_f64", "out_cols-32", "out_dtype=f64",
             "out_scale_cols-4", "act=nonsense", "offsets_int64", "E=1025", "w_experts_overlap",
             "w_scale_experts_2_bytes_off", "rows=-1", "rows+256", "out_groups_overlap")
# what the ordered pairs are made of
PAIR_KEYS = ("w_dtype", "K=384", "no_w_scale", "scales_on_16_bit", "a_scale_short", "tile=pt4",
             "mode=generic", "ksplit=2", "N=992", "out_f64", "offsets_int64", "rows=-1")


def _selected(kind):
    if kind == "full":
        return PERTURBATIONS
    if kind == "core":
        return [p for p in PERTURBATIONS if p[0] in CORE_KEYS]
    return [p for p in PERTURBATIONS if p[0].startswith(("N=", "out", "act"))]


# (entry point, form, variant, perturbations, ordered pairs too)
CASES = [
    ("fp4", "mxfp4", "dense", "full", True),
    ("scales", "mxfp8", "dense", "full", True),
    ("out_quant", "bf16", "mx", "full", True),
    ("out_quant", "mxfp8", "mx", "full", True),
    ("out_quant", "f16", "mxfp4", "core", False),
    ("out_quant", "mxfp4", "mxfp4", "core", False),
    ("out_quant", "bf16", "mxfp4", "out", False),
    ("out_quant", "mxfp8", "mxfp4", "out", False),
    ("glu", "bf16", "dense", "full", True),
    ("glu", "mxfp8", "mx", "full", True),
    ("glu", "f16", "mx", "core", False),
    ("glu", "mxfp4", "dense", "core", False),
    ("glu", "bf16", "mx", "out", False),
    ("glu", "bf16", "mxfp4", "out", False),
    ("glu", "mxfp8", "dense", "out", False),
    ("glu", "mxfp8", "mxfp4", "out", False),
    ("grouped", "f16", "dense", "full", True),
    ("grouped", "mxfp8", "glu+mxfp4", "full", True),
    ("grouped", "bf16", "mx", "core", False),
    ("grouped", "mxfp4", "glu", "core", False),
    ("grouped", "bf16", "glu", "out", False),
    ("grouped", "f16", "glu+mxfp4", "out", False),
    ("grouped", "mxfp8", "dense", "out", False),
    ("grouped", "mxfp8", "mx", "out", False),
    ("kgrouped", "mxfp8", "dense", "full", True),
    ("kgrouped", "mxfp4", "dense", "full", False),
]


def _show(v):
    if isinstance(v, tuple):
        return "(" + ", ".join(_show(x) for x in v) + ")"
    return "None" if v is None else str(v)


def _line(entry, form, variant, perts):
    c = _base(entry, form, variant)
    if not (variant.endswith("mxfp4") and FP4 is None):
        for _, apply in perts:
            if not apply(c):
                return None
    name = "+".join(n for n, _ in perts) or "base"
    try:
        res = "ok " + _show(_call(c))
    except (TypeError, ValueError) as e:
        res = f"{type(e).__name__}: {e}"
    return f"{entry} {form}/{variant} {name} -> {res}"


def table(fp4: bool):
    """The lines of one section: the mxfp4 operand forms (``fp4``) or every other form."""
    by_name = dict(PERTURBATIONS)
    out = []
    for entry, form, variant, kind, pairs in CASES:
        if (form == "mxfp4") != fp4:
            continue
        out.append(_line(entry, form, variant, ()))
        out += [_line(entry, form, variant, (p,)) for p in _selected(kind)]
        if pairs:
            out += [_line(entry, form, variant, ((p, by_name[p]), (q, by_name[q])))
                    for p in PAIR_KEYS for q in PAIR_KEYS if p != q]
    return [ln for ln in out if ln is not None]


def _expected(section):
    with open(EXPECTED, encoding="utf-8") as f:
        lines = f.read().splitlines()
    start = lines.index(f"# section: {section}") + 1
    end = next((i for i in range(start, len(lines)) if lines[i].startswith("# section: ")),
               len(lines))
    return lines[start:end]


def _compare(got, want):
    diff = [(g, w) for g, w in zip(got, want) if g != w][:5]
    assert got == want, f"{len(got)} lines, expected {len(want)}; first differences: {diff}"


def test_refusal_table_16_bit_and_mxfp8():
    _compare(table(False), _expected("bf16 f16 mxfp8"))


@pytest.mark.skipif(FP4 is None, reason="torch has no float4_e2m1fn_x2")
def test_refusal_table_mxfp4():
    _compare(table(True), _expected("mxfp4"))
