"""Python front-end of the CDNA4 MFMA GEMM (``csrc/gemm/gemm_mfma.hip``).

``gemm(a, w)`` computes ``a @ w.T`` for ``a: [M, K]`` and ``w: [N, K]`` (the weight kept
K-contiguous, like ``te.Linear``'s ``[out, in]``), with optional grouped-row addressing of A and C:
logical row ``i`` lives at physical row ``base + (i // grp) * gstride + i % grp``.

Every shape / dtype / device / alignment / bounds check happens here, on the host, before the
kernel launches (a bad launch can fault every GPU of the node).

dtypes: bf16 -> bf16|f32, f16 -> f16|f32, f32 -> f32 (exact f32 MFMA), float8_e4m3fn -> bf16|f16|f32
(``mode="mx"``: block-scaled MX-fp8 MFMA at 2x the bf16 rate; unit scales, or real per-block E8M0
scales with ``a_scale`` / ``w_scale``, see :mod:`ddlb_amd.ops.mx`), float4_e2m1fn_x2 -> bf16|f16|f32
(MXFP4: E2M1 pairs, always with block scales, at 2x the MX-fp8 rate), f64 (generic kernel).
``out_quant="mx" | "mxfp4"``: bf16 / f16 / block-scaled fp8 / block-scaled fp4 -> MX-fp8 or MXFP4
data and E8M0 scales per 32 output columns, quantised in the GEMM's epilogue.
``glu=True``: the same operands, ``w`` holding interleaved gate and up rows (``pack_glu``); the
epilogue writes ``act(gate) * up``, half as many columns, dense or quantised.
``gemm_grouped(a, w, offsets)``: per-expert weights ``w [E, N, K]`` over contiguous runs of rows
of ``a`` given by device-side int32 offsets, one launch, every form above on the tiled kernel.
"""

from __future__ import annotations

from typing import NamedTuple, Optional

from ddlb_amd.ops import load

DT_F32, DT_F16, DT_BF16, DT_FP8, DT_F64, DT_U8 = 0, 1, 2, 3, 4, 5
DT_FP4 = 6  # OCP E2M1, two elements per byte (torch.float4_e2m1fn_x2): gemm() with scales only
# (codes 5, 8, 9, 13-15 belonged to the pp256 / p256 / p128 / pi256 / pi256w4 / r256 families,
# retired in round 4: no auto path reached them and pt4 superseded them on every shape measured)
TILES = {"auto": 0, "256x256": 1, "256x128": 2, "128x256": 3, "128x128": 4, "256x256w4": 6,
         "256x128w4": 7, "i256": 10, "i128": 11, "i256w4": 12,
         "t8": 16, "pt8": 17, "t4": 18, "pt4": 19}
MODES = {"auto": 0, "generic": 1, "mx": 2}
ACTS = {"none": 0, "gelu": 1, "relu": 2, "silu": 3}

SUPPORTED_IN = ("float32", "float16", "bfloat16", "float8_e4m3fn", "float64")


def dtype_code(dt) -> int:
    import torch

    table = {torch.float32: DT_F32, torch.float16: DT_F16, torch.bfloat16: DT_BF16,
             torch.float8_e4m3fn: DT_FP8, torch.float64: DT_F64, torch.uint8: DT_U8}
    if dt not in table:
        raise TypeError(f"dtype {dt} is not supported by the native GEMM")
    return table[dt]


def check_supported(dtype_name: str) -> None:
    if dtype_name not in SUPPORTED_IN:
        raise TypeError(f"native GEMM supports {SUPPORTED_IN}, not {dtype_name}")


def default_out_dtype(in_dtype):
    import torch

    return torch.bfloat16 if in_dtype == torch.float8_e4m3fn else in_dtype


def _check_placement(*ts):
    """Where the operands live and how they are laid out: ROCm device tensors on one device, 2-D,
    unit inner stride."""
    if any(t.device.type != "cuda" for t in ts):
        raise ValueError("native GEMM operands must be ROCm device tensors")
    if any(t.device != ts[0].device for t in ts):
        raise ValueError("operands on different devices")
    if any(t.dim() != 2 for t in ts):
        raise ValueError("native GEMM expects 2-D operands")
    if any(t.stride(1) != 1 for t in ts):
        raise ValueError("operands must be row-major with unit inner stride")


def _check_same_dtype(a, w):
    if a.dtype != w.dtype:
        raise TypeError(f"A dtype {a.dtype} != W dtype {w.dtype}")


def _check_k(a, w):
    """``a [.., K]`` against ``w [.., N, K]`` (a stack of experts is shown whole)."""
    if a.shape[1] != w.shape[-1]:
        raise ValueError(f"K mismatch: A {tuple(a.shape)} vs W {tuple(w.shape)}")


def _check_32_bits(M, N, K):
    if M >= 2 ** 31 or N >= 2 ** 31 or K >= 2 ** 31:
        raise ValueError("dimensions must fit in 32 bits")


def _stream(stream, a):
    """The raw HIP stream of a launch: the caller's, or the current one of ``a``'s device."""
    import torch

    return stream if stream is not None else torch.cuda.current_stream(a.device).cuda_stream


def _check_operands(a, w, out, M, a_rows_phys):
    import torch

    _check_placement(a, w, out)
    _check_same_dtype(a, w)
    _check_k(a, w)
    if out.shape[1] < w.shape[0]:
        raise ValueError(f"output has {out.shape[1]} columns < N={w.shape[0]}")
    if a_rows_phys > a.shape[0]:
        raise ValueError(f"A row mapping reaches row {a_rows_phys - 1} >= {a.shape[0]}")
    if a.dtype == torch.float8_e4m3fn and out.dtype not in (torch.bfloat16, torch.float16,
                                                             torch.float32):
        raise TypeError("fp8 GEMM output must be bf16, f16 or f32")


def _phys_rows(M: int, grp: int, gstride: int, base_rows: int = 0) -> int:
    """One past the largest physical row the mapping touches."""
    if M == 0:
        return 0
    if grp <= 0:
        return M
    last = M - 1
    return (last // grp) * gstride + (last % grp) + 1


def device_cus() -> int:
    """CUs of the current device (256 on a whole MI355X; fewer in a compute partition), 256 when
    no GPU is visible (plans built on the CPU)."""
    import torch

    if not torch.cuda.is_available():
        return 256
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def split_k_factor(M: int, N: int, K: int, esz: int, ncu: int = 0) -> int:
    """K-slices for a GEMM whose 256x256 grid covers at most half the CUs and whose K is long
    (e.g. 8192 x 1024 x 8192: 128 tiles): ``S`` slices run as (slice, tile) pairs of ONE pt4
    launch (``GemmArgs::ksplit``), their partials summed by the reduce kernel. Each slice
    keeps >= 16 K-tiles (the fixed per-tile cost stays small, profiles/r04/r4_15_*); measured
    on the config #2 shape: 0.1009 ms vs 0.1338 unsplit (profiles/r04/r4_22_*). 1 = no split."""
    if M % 256 or N % 256 or M <= 0 or N <= 0:
        return 1
    ncu = ncu or device_cus()
    tiles = (M // 256) * (N // 256)
    nk = K * esz // 128
    if K * esz % 128:
        return 1
    for S in (4, 2):
        if tiles * S <= ncu and nk % (2 * S) == 0 and nk // S >= 16:
            return S
    return 1


SCALED_TILES = ("256x128", "128x256", "128x128", "256x128w4")  # gemm.h mxs_offers()
SCALED_FP4_TILES = SCALED_TILES  # gemm.h mx4_offers()


def _fp4_dtype():
    import torch

    return getattr(torch, "float4_e2m1fn_x2", None)


def _is_fp4(t) -> bool:
    dt = _fp4_dtype()
    return dt is not None and getattr(t, "dtype", None) == dt


class _ScaledFormat(NamedTuple):
    """What the two block-scaled operand formats differ in, wording of the refusals included."""
    per_byte: int   # elements per stored element: K = per_byte * a.shape[1]
    kmod: int       # K is a whole number of 128-byte K-tiles
    align: int      # scale base and row stride: the scales of a row's K-tile are one aligned load
    tiles: tuple
    noun: str       # the subject of the messages ...
    plural: bool    # ... and its number
    runs: str       # the subject of the mode message
    tile_note: str


_MX_FP8 = _ScaledFormat(1, 128, 4, SCALED_TILES, "block scales", True, "block scales",
                        " (the ping-pong kernels t8 / pt8 / t4 / pt4 take unit scales)")
_MX_FP4 = _ScaledFormat(2, 256, 8, SCALED_FP4_TILES, "the fp4 GEMM", False, "fp4 operands", "")


def _check_tile(noun, tile, note="", be="is", tiles=SCALED_TILES):
    if tile != "auto" and tile not in tiles:
        raise ValueError(f"{noun} {be} offered for tile auto / {tiles}, not {tile!r}{note}")


def _check_block_scaled(f, a, w, a_scale, w_scale, M, tile, mode, a_grp, ksplit):
    """The refusals the block-scaled formats share, before anything is launched."""
    import torch

    be, need, do = (("are", "need", "do") if f.plural else ("is", "needs", "does"))
    if mode not in ("auto", "mx"):
        raise ValueError(f"{f.runs} run the MX kernel (mode auto / mx), not mode={mode!r}")
    _check_tile(f.noun, tile, f.tile_note, be, f.tiles)
    if a_grp not in (0, M):
        raise ValueError(f"{f.noun} {need} plain A rows (no grouped A rows)")
    if ksplit > 1:
        raise ValueError(f"{f.noun} {do} not combine with a K-split")
    K = f.per_byte * a.shape[1]
    if K % f.kmod:
        raise ValueError(f"{f.noun} {need} K % {f.kmod} == 0 (K = {K})")
    for name, sc, rows in (("a_scale", a_scale, a.shape[0]), ("w_scale", w_scale, w.shape[0])):
        if not isinstance(sc, torch.Tensor) or sc.dtype != torch.uint8:
            raise TypeError(f"{name} must be a uint8 tensor of E8M0 bytes")
        if sc.device != a.device:
            raise ValueError(f"{name} is on {sc.device}, the operands on {a.device}")
        if tuple(sc.shape) != (rows, K // 32):
            raise ValueError(f"{name} must have shape {(rows, K // 32)}, not {tuple(sc.shape)}")
        if sc.stride(1) != 1 or sc.stride(0) % f.align or sc.stride(0) < K // 32:
            raise ValueError(f"{name} needs unit inner stride and a row stride that is a "
                             f"multiple of {f.align} (strides {tuple(sc.stride())})")
        if sc.data_ptr() % f.align:
            raise ValueError(f"{name} must start at {'an' if f.align == 8 else 'a'} "
                             f"{f.align}-byte-aligned address")
        if rows * sc.stride(0) >= 2 ** 31:
            raise ValueError(f"{name} spans 2 GiB or more")


def _check_fp4(a, w, out, a_scale, w_scale, M, tile, mode, a_grp, ksplit):
    """Every refusal of the block-scaled fp4 GEMM, before anything is launched. ``a`` / ``w``
    hold two E2M1 elements per byte: ``K = 2 * a.shape[1]``."""
    import torch

    if not (_is_fp4(a) and _is_fp4(w)):
        raise TypeError(f"fp4 operands do not mix with another dtype (A {a.dtype}, W {w.dtype})")
    if a_scale is None or w_scale is None:
        raise ValueError("float4_e2m1fn_x2 operands need a_scale and w_scale (MXFP4 has no "
                         "unit-scale kernel)")
    if out.dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise TypeError("fp4 GEMM output must be bf16, f16 or f32")
    _check_block_scaled(_MX_FP4, a, w, a_scale, w_scale, M, tile, mode, a_grp, ksplit)


def _check_scales(a, w, a_scale, w_scale, M, tile, mode, a_grp, ksplit):
    """Every refusal of the block-scaled fp8 GEMM, before anything is launched."""
    import torch

    if (a_scale is None) != (w_scale is None):
        raise ValueError("a_scale and w_scale go together: pass both or neither")
    if a.dtype != torch.float8_e4m3fn:
        raise TypeError(f"block scales need float8_e4m3fn operands, not {a.dtype}")
    _check_block_scaled(_MX_FP8, a, w, a_scale, w_scale, M, tile, mode, a_grp, ksplit)


OUT_QUANTS = ("mx", "mxfp4")


def out_quant_dtype(out_quant: str):
    import torch

    return _fp4_dtype() if out_quant == "mxfp4" else torch.float8_e4m3fn


class _Form(NamedTuple):
    """What the launch forms of the tiled kernel differ in on the host: the wording of their
    refusals."""
    noun: str       # the subject of the messages
    tile_note: str
    takes: str      # the subject of the operand refusal
    no_scales: str  # fp8 (fp4) operands without their scales
    fast_path: str  # what the MFMA fast path asks of the form


_WHOLE_K_TILES = ("16-byte-aligned operand rows, 8-byte-aligned output rows and K a whole number "
                  "of 128-byte K-tiles")
_QOUT = _Form("a quantised output", "", "out_quant",
              "a quantised output from fp8 operands needs a_scale and w_scale (there is no "
              "unit-scale kernel with this epilogue)",
              "16-byte-aligned operand rows and K a whole number of 128-byte K-tiles")
_GLU = _Form("a gated epilogue", " (the ping-pong, interleaved and 256x256 kernels have none)",
             "glu", "a gated epilogue on fp8 operands needs a_scale and w_scale (the unit-scale "
             "kernels have none)", _WHOLE_K_TILES)
_GROUPED = _Form("a grouped GEMM",
                 " (the ping-pong, interleaved and 256x256 kernels have no grouped form)",
                 "a grouped GEMM", "a grouped GEMM on fp8 / fp4 operands needs a_scale and "
                 "w_scale (the unit-scale kernels have no grouped form)", _WHOLE_K_TILES)
_KGROUPED = _Form("a K-grouped GEMM", "", "a K-grouped GEMM",
                  "a K-grouped GEMM needs a_scale and w_scale (the unit-scale kernels have no "
                  "K-grouped form)", "16-byte-aligned operand rows, 8-byte-aligned output rows")


class _Tiled(NamedTuple):
    """What :func:`_check_tiled` found: the extents in elements and the output dtype."""
    M: int
    N: int
    K: int
    odt: object


def _known_out_quant(out_quant, optional: bool):
    if out_quant not in OUT_QUANTS and not (optional and out_quant is None):
        raise ValueError(f"out_quant must be None or one of {OUT_QUANTS}, not {out_quant!r}")
    if out_quant == "mxfp4" and _fp4_dtype() is None:
        raise TypeError("out_quant='mxfp4' needs torch.float4_e2m1fn_x2")


def _check_quant_dtype(out_quant, out_dtype):
    qdt = out_quant_dtype(out_quant)
    if out_dtype is not None and out_dtype != qdt:
        raise TypeError(f"out_quant={out_quant!r} writes {qdt}, not out_dtype={out_dtype}")


def _refuse_operands(f, a):
    raise TypeError(f"{f.takes} takes bf16, f16, scaled fp8 or scaled fp4 operands, not {a.dtype}")


def _check_dense_out(what, a, out, out_dtype, dense, rows, cols, groups=0):
    """The dense output of a form (``what`` names it): its dtype, ``dense[0]`` unless ``out`` or
    ``out_dtype`` says otherwise, among the ones the operands pair with; ``out``, where given, on
    the operands' device as ``[>= rows, cols]`` rows, or exactly ``[groups, rows, cols]``."""
    odt = out.dtype if out is not None else (out_dtype or dense[0])
    if out is not None and out_dtype is not None and out_dtype != out.dtype:
        raise TypeError(f"out is {out.dtype}, out_dtype={out_dtype}")
    if odt not in dense:
        raise TypeError(f"{what} writes one of {dense}, not {odt}")
    if out is None:
        return odt
    if out.device != a.device:
        raise ValueError(f"out is on {out.device}, the operands on {a.device}")
    if groups:
        if out.dim() != 3 or tuple(out.shape) != (groups, rows, cols):
            raise ValueError(f"out must have shape {(groups, rows, cols)}, not {tuple(out.shape)}")
        need = ", rows of at least N and groups at least M rows apart"
        laid = out.stride(1) >= cols and (groups == 1 or out.stride(0) >= rows * out.stride(1))
    else:
        if out.dim() != 2 or out.shape[0] < rows or out.shape[1] != cols:
            raise ValueError(f"out must have shape (>= {rows}, {cols}), not {tuple(out.shape)}")
        need = f" and a row stride of at least {cols}"
        laid = out.stride(0) >= cols
    if out.stride(-1) != 1 or not laid:
        raise ValueError(f"out needs unit inner stride{need} (strides {tuple(out.stride())})")
    if groups and out.stride(0) * out.element_size() % 8:
        raise ValueError("the groups' outputs must be a multiple of 8 bytes apart")
    return odt


def _check_tiled(f, a, w, out, out_scale, *, out_quant, out_dtype, a_scale, w_scale, tile, mode,
                 M, a_grp, c_grp, ksplit, glu=False, own=None):
    """The rules the forms of the tiled kernel share, on the host and before anything is loaded
    or launched, worded for the form ``f``: ranks, K, ``M``; the entry point's ``own(N)`` rules;
    mode, tile, K-split, plain rows; the operand kind, the scales it carries and the dense dtypes
    it pairs with; the 32-bit extents; the output, dense or (``out_quant``) quantised, of ``N``
    columns or (``glu``) ``N / 2``. ``out`` / ``out_scale`` are checked when given."""
    import torch
    from types import SimpleNamespace

    if a.dim() != 2 or w.dim() != 2:
        raise ValueError("native GEMM expects 2-D operands")
    fp4 = _is_fp4(a) or _is_fp4(w)
    M = a.shape[0] if M is None else int(M)
    N = w.shape[0]
    K = 2 * a.shape[1] if fp4 else a.shape[1]
    _check_k(a, w)
    if not 0 <= M <= a.shape[0]:
        raise ValueError(f"M = {M} is outside A's {a.shape[0]} rows")
    if own is not None:
        own(N)
    if mode == "generic":
        raise ValueError(f"{f.noun} comes from the tiled MFMA kernel, not mode='generic'")
    if mode not in MODES:
        raise ValueError(f"unknown mode {mode!r}")
    _check_tile(f.noun, tile, f.tile_note)
    if int(ksplit) > 1:
        raise ValueError(f"{f.noun} does not combine with a K-split")
    if a_grp not in (0, M) or c_grp not in (0, M):
        raise ValueError(f"{f.noun} needs plain A and C rows (no grouped rows)")
    # the inputs: bf16, f16, block-scaled fp8, block-scaled fp4; the dense outputs they pair with
    dense = (torch.bfloat16, torch.float16, torch.float32)
    if fp4:
        _check_fp4(a, w, SimpleNamespace(dtype=torch.bfloat16), a_scale, w_scale, M, tile, mode,
                   a_grp, int(ksplit))
    elif a.dtype == torch.float8_e4m3fn or w.dtype == torch.float8_e4m3fn:
        _check_same_dtype(a, w)
        if a_scale is None or w_scale is None:
            raise ValueError(f.no_scales)
        _check_scales(a, w, a_scale, w_scale, M, tile, mode, a_grp, int(ksplit))
    elif a.dtype in (torch.bfloat16, torch.float16):
        _check_same_dtype(a, w)
        if a_scale is not None or w_scale is not None:
            raise TypeError(f"block scales need fp8 / fp4 operands, not {a.dtype}")
        if mode == "mx":
            raise ValueError(f"mode='mx' needs fp8 / fp4 operands, not {a.dtype}")
        dense = (a.dtype, torch.float32)
    else:
        _refuse_operands(f, a)
    _check_32_bits(M, N, K)
    cols = N // 2 if glu else N
    if out_quant is None:
        return _Tiled(M, N, K, _check_dense_out(f"{f.noun} on {a.dtype} operands", a, out,
                                                out_dtype, dense, M, cols))
    _check_quant_dtype(out_quant, out_dtype)
    _check_quant_outputs(a, out, out_scale, out_quant, M, cols)
    return _Tiled(M, N, K, out_quant_dtype(out_quant))


def _check_out_quant(a, w, out_quant, out=None, out_scale=None, *, a_scale=None, w_scale=None,
                     tile: str = "auto", mode: str = "auto", M: Optional[int] = None,
                     a_grp: int = 0, c_grp: int = 0, ksplit: int = 0, out_dtype=None):
    """Every refusal of the quantised-output GEMM (``out_quant="mx" | "mxfp4"``), on the host and
    before anything is loaded or launched (CPU tensors pass through it). ``out`` / ``out_scale``
    are checked when given. Returns ``(M, N, K)`` in elements."""
    _known_out_quant(out_quant, optional=False)

    def own(N):
        _check_quant_dtype(out_quant, out_dtype)
        nmod = 256 if out_quant == "mxfp4" else 128
        if N % nmod:
            raise ValueError(f"out_quant={out_quant!r} needs N % {nmod} == 0 (N = {N}): whole "
                             "32-column blocks, as many as the GEMM that reads them takes per "
                             "K-tile")

    return tuple(_check_tiled(_QOUT, a, w, out, out_scale, out_quant=out_quant,
                              out_dtype=out_dtype, a_scale=a_scale, w_scale=w_scale, tile=tile,
                              mode=mode, M=M, a_grp=a_grp, c_grp=c_grp, ksplit=ksplit,
                              own=own)[:3])


def _check_quant_outputs(a, out, out_scale, out_quant, M, cols):
    """``out`` / ``out_scale`` of a quantised output of ``cols`` columns (``N``; ``N / 2`` with
    ``glu``), where given: types, device, shape, layout, and the scales' 2 GiB span."""
    from ddlb_amd.ops.mx import check_quant_pair_layout, check_quant_pair_types

    q4 = out_quant == "mxfp4"
    qdt = out_quant_dtype(out_quant)
    ncol, sal = (cols // 2 if q4 else cols), (8 if q4 else 4)
    check_quant_pair_types(("out", "out_scale"), out, out_scale, qdt, f"out_quant={out_quant!r}")
    for name, t, tc in (("out", out, ncol), ("out_scale", out_scale, cols // 32)):
        if t is None:
            continue
        if t.device != a.device:
            raise ValueError(f"{name} is on {t.device}, the operands on {a.device}")
        if t.dim() != 2 or t.shape[0] < M or t.shape[1] != tc:
            raise ValueError(f"{name} must have shape (>= {M}, {tc}), not {tuple(t.shape)}")
    check_quant_pair_layout(("out", "out_scale"), out, out_scale, ncol, cols // 32, sal)
    if out_scale is not None and M * out_scale.stride(0) >= 2 ** 31:
        raise ValueError("out_scale spans 2 GiB or more")
    if M * (cols // 32) >= 2 ** 31:
        raise ValueError("out_scale spans 2 GiB or more")


def _launch(C, a, w, c, M, N, K, tile, mode, s, *, a_grp=0, a_gstride=0, c_grp=0, c_gstride=0,
            act=0, ksplit=None, a_scale=None, w_scale=None, out_scale=None, glu=False):
    """The one call of ``C.gemm``: pointers, leading dimensions and dtype codes from the tensors
    (fp4 data: two elements per stored byte, dimensions go in ELEMENTS), then the optional tail
    in the extension's positional order: ``ksplit``, the four operand-scale arguments (block
    scales always run ``mode="mx"``), the two output-scale arguments, ``glu`` (the whole tail
    then, zeros for what is absent)."""
    am, cm = (2 if _is_fp4(a) else 1), (2 if _is_fp4(c) else 1)
    scaled = a_scale is not None
    args = [a.data_ptr(), w.data_ptr(), c.data_ptr(), am * a.stride(0), am * w.stride(0),
            cm * c.stride(0), M, N, K, DT_FP4 if am == 2 else dtype_code(a.dtype),
            DT_FP4 if cm == 2 else dtype_code(c.dtype), TILES[tile],
            MODES["mx"] if scaled else MODES[mode], a_grp, a_gstride, c_grp, c_gstride, s, act]
    if ksplit is not None or scaled or out_scale is not None or glu:
        args.append(1 if ksplit is None else ksplit)
    if scaled:
        args += [a_scale.data_ptr(), w_scale.data_ptr(), a_scale.stride(0), w_scale.stride(0)]
    elif out_scale is not None or glu:
        args += [0, 0, 0, 0]
    if out_scale is not None:
        args += [out_scale.data_ptr(), out_scale.stride(0)]
    elif glu:
        args += [0, 0]
    if glu:
        args.append(1)
    C.gemm(*args)


def _need_fast_path(C, message, a, w, out, M, N, K, dout):
    """The MFMA fast path's alignment on the operands as the byte / element matrices the kernel
    reads (``K`` in elements; ``w`` and ``out`` 2-D: one expert's weight, one group's output)."""
    fp4 = _is_fp4(a)
    if M and N and not C.gemm_fast_path_ok(a.data_ptr(), w.data_ptr(), out.data_ptr(),
                                           a.stride(0), w.stride(0), out.stride(0), M, N,
                                           K // 2 if fp4 else K,
                                           DT_U8 if fp4 else dtype_code(a.dtype), dout):
        raise ValueError(message)


def _run_tiled(f, t, a, w, out, out_scale, launch, *, out_quant=None, glu=False, groups=0,
               stream=None):
    """The launch tail the forms share, after every refusal of ``_check_*`` (``t``): load the
    extension, allocate ``out`` / ``out_scale`` where absent (never zero-filled), placement, the
    fast path, the stream, ``launch(C, out, out_scale, s)``, and what ``gemm`` returns. ``w`` may
    be a stack of experts and ``out`` one of ``groups`` matrices."""
    import torch

    C = load()
    M, N, K, odt = t
    cols = N // 2 if glu else N
    if out is None and out_quant is not None:
        out = torch.empty((M, cols // 2 if out_quant == "mxfp4" else cols), dtype=torch.uint8,
                          device=a.device).view(odt)
    elif out is None:
        out = torch.empty((groups, M, cols) if groups else (M, cols), dtype=odt, device=a.device)
    if out_quant is not None and out_scale is None:
        out_scale = torch.empty((M, cols // 32), dtype=torch.uint8, device=a.device)
    w2, out2 = (w[0] if w.dim() == 3 else w), (out[0] if groups else out)
    _check_placement(a, w2, out2)
    _need_fast_path(C, f"{f.noun} needs the MFMA fast path: {f.fast_path}", a, w2, out2, M, N, K,
                    DT_U8 if out_quant else dtype_code(odt))
    s = _stream(stream, a)
    launch(C, out, out_scale, s)
    if stream is not None:  # the outputs stay allocated until that stream reaches them
        out.record_stream(torch.cuda.ExternalStream(s))
        if out_scale is not None:
            out_scale.record_stream(torch.cuda.ExternalStream(s))
    return out if out_quant is None else (out[:M], out_scale[:M])


GLU_GROUP = 32  # gate / up rows alternate in groups of one MX block (GemmArgs::glu)


def _as_bytes(t):
    """One-byte dtypes (fp8, fp4 pairs) as uint8, which torch stacks and reshapes everywhere."""
    import torch

    return t.view(torch.uint8) if t.element_size() == 1 and t.dtype != torch.uint8 else t


def pack_glu(gate, up):
    """``[F, K]`` gate and up rows -> the ``[2F, K]`` weight ``gemm(glu=True)`` reads: rows
    ``64g .. 64g + 31`` are gate rows ``32g .. 32g + 31``, rows ``64g + 32 .. 64g + 63`` the
    matching up rows. Any dtype: quantised data and their ``uint8`` scales pack row by row (a
    row-wise quantisation commutes with a row permutation). ``F % 32 == 0``."""
    import torch

    if gate.dim() != 2 or up.dim() != 2 or gate.shape != up.shape or gate.dtype != up.dtype:
        raise ValueError(f"pack_glu takes two 2-D tensors of one shape and dtype, not "
                         f"{tuple(gate.shape)} {gate.dtype} and {tuple(up.shape)} {up.dtype}")
    F, K = gate.shape
    if F % GLU_GROUP:
        raise ValueError(f"pack_glu needs F % {GLU_GROUP} == 0 (F = {F})")
    g, u = (_as_bytes(t).reshape(F // GLU_GROUP, GLU_GROUP, K) for t in (gate, up))
    return torch.stack((g, u), dim=1).reshape(2 * F, K).view(gate.dtype)


def unpack_glu(w):
    """The inverse of :func:`pack_glu`: ``[2F, K]`` -> ``(gate, up)``, ``[F, K]`` each."""
    if w.dim() != 2 or w.shape[0] % (2 * GLU_GROUP):
        raise ValueError(f"unpack_glu takes a 2-D tensor of a multiple of {2 * GLU_GROUP} rows, "
                         f"not {tuple(w.shape)}")
    N, K = w.shape
    v = _as_bytes(w).reshape(N // (2 * GLU_GROUP), 2, GLU_GROUP, K)
    return tuple(v[:, h].reshape(N // 2, K).view(w.dtype) for h in (0, 1))


def glu_reference(c, act: str = "none"):
    """The specification of the gated epilogue on an f32 ``[M, 2F]`` product ``c = a @ w.T`` (any
    device): ``out[i, 32g + j] = act(c[i, 64g + j]) * c[i, 64g + 32 + j]``, f32 ``[M, F]``."""
    import torch

    from ddlb_amd.parallel.sim import apply_act

    if act not in ACTS:
        raise ValueError(f"unknown activation {act!r}")
    if c.dim() != 2 or c.shape[1] % (2 * GLU_GROUP) or c.dtype != torch.float32:
        raise ValueError(f"glu_reference takes an f32 [M, 2F] product with 2F % "
                         f"{2 * GLU_GROUP} == 0, not {tuple(c.shape)} {c.dtype}")
    M, N = c.shape
    v = c.reshape(M, N // (2 * GLU_GROUP), 2, GLU_GROUP)
    return (apply_act(v[:, :, 0], ACTS[act]) * v[:, :, 1]).reshape(M, N // 2)


def _check_glu(a, w, out=None, out_scale=None, *, out_quant=None, out_dtype=None, a_scale=None,
               w_scale=None, tile: str = "auto", mode: str = "auto", M: Optional[int] = None,
               a_grp: int = 0, c_grp: int = 0, ksplit: int = 0, act: str = "none"):
    """Every refusal of the gated GEMM (``glu=True``), on the host and before anything is loaded
    or launched (CPU tensors pass through it). ``out`` / ``out_scale`` are checked when given.
    Returns ``(M, N, K, output dtype)``: ``N`` the rows of ``w``; the output has ``N / 2``
    columns."""
    if act not in ACTS:
        raise ValueError(f"unknown activation {act!r}")
    _known_out_quant(out_quant, optional=True)
    if out_quant is None and out_scale is not None:
        raise ValueError("out_scale goes with out_quant")

    def own(N):
        nmod = 512 if out_quant == "mxfp4" else 256 if out_quant else 2 * GLU_GROUP
        if N % nmod:
            why = ("N / 2 in whole 32-column blocks, as many as the GEMM that reads them takes "
                   "per K-tile" if out_quant else "whole groups of 32 gate and 32 up rows")
            raise ValueError(f"glu with out_quant={out_quant!r} needs N % {nmod} == 0 "
                             f"(N = {N}): {why}")

    return tuple(_check_tiled(_GLU, a, w, out, out_scale, out_quant=out_quant,
                              out_dtype=out_dtype, a_scale=a_scale, w_scale=w_scale, tile=tile,
                              mode=mode, M=M, a_grp=a_grp, c_grp=c_grp, ksplit=ksplit, glu=True,
                              own=own))


def gemm(a, w, out=None, *, out_dtype=None, tile: str = "auto", mode: str = "auto",
         M: Optional[int] = None, a_grp: int = 0, a_gstride: int = 0, c_grp: int = 0,
         c_gstride: int = 0, stream=None, act: str = "none", ksplit: int = 0,
         a_scale=None, w_scale=None, out_quant: Optional[str] = None, out_scale=None,
         glu: bool = False):
    """``out[:M] = act(a[:M] @ w.T)`` on the current HIP stream (grouped-row addressing and a
    fused epilogue activation — none / gelu (tanh) / relu / silu — optional). ``ksplit``: 0 =
    auto (:func:`split_k_factor` for plain-row auto-tile GEMMs with no activation and a dense
    output), 1 = never, S > 1 = S slices. A pt4 split runs one launch over (slice, tile) pairs
    into f32 partials, summed in slice order and rounded once by the reduce kernel (0.1122 ms on
    8192 x 1024 x 8192 bf16, ``profiles/r05/r5_14_*``).

    ``a_scale`` / ``w_scale`` (both or neither; fp8 operands): MX block scales, ``uint8``
    ``[rows, K / 32]`` E8M0 bytes (value ``2^(s - 127)`` for 32 consecutive K elements of a row,
    :mod:`ddlb_amd.ops.mx`). They run the block-scaled flavour of the tiled kernel (tiles
    :data:`SCALED_TILES`, ``auto`` picks among them; plain A rows, no K-split); anything else
    raises here, never a launch with unit scales in their place.

    ``float4_e2m1fn_x2`` operands (MXFP4, ``K = 2 * a.shape[1]``, ``K % 256 == 0``) always take
    ``a_scale`` / ``w_scale``, in the same layout with 8-byte-aligned rows; tiles
    :data:`SCALED_FP4_TILES`, output bf16 / f16 / f32, otherwise the rules above.

    ``out_quant="mx"`` / ``"mxfp4"`` (bf16, f16, scaled fp8 or scaled fp4 operands; tiles
    :data:`SCALED_TILES`; ``N % 128`` / ``N % 256 == 0``; plain rows, no K-split): the epilogue
    quantises ``act(acc)`` in f32 by the rule of :mod:`ddlb_amd.ops.mx`, in blocks of 32
    consecutive columns of a row, and ``gemm`` returns ``(q, s)``: ``float8_e4m3fn [M, N]`` or
    ``float4_e2m1fn_x2 [M, N / 2]`` and ``uint8 [M, N / 32]``, laid out so that they go straight
    back in as ``a`` and ``a_scale``. ``out`` / ``out_scale`` may be preallocated (16-byte-aligned
    data rows, a scale row stride that is a multiple of 4, 8 for fp4). :func:`_check_out_quant`
    holds every refusal.

    ``glu=True`` (SwiGLU / GeGLU / ReGLU / bilinear by ``act``): ``w`` is ``[2F, K]`` with gate
    and up rows interleaved in groups of 32 (:func:`pack_glu`) and the epilogue multiplies
    ``act(gate)`` by ``up`` in f32, so the result has ``F = N / 2`` columns
    (:func:`glu_reference`): dense (``N % 64 == 0``), or with ``out_quant`` as ``(q, s)`` of
    ``N / 2`` columns and ``N / 64`` scales per row (``N % 256``, fp4 ``N % 512 == 0``). Same
    operands, tiles and plain rows as ``out_quant`` (``a_grp`` / ``c_grp`` 0 or ``M``: one group,
    so ``a_gstride`` / ``c_gstride`` have nothing to act on); :func:`_check_glu` holds every
    refusal."""
    import torch

    if glu or out_quant is not None:
        # every refusal first, before the extension is loaded; then one launch (neither a
        # requested nor the automatic K-split engages on this path)
        kw = dict(a_scale=a_scale, w_scale=w_scale, tile=tile, mode=mode, M=M, a_grp=a_grp,
                  c_grp=c_grp, ksplit=ksplit, out_dtype=out_dtype)
        if glu:
            t = _Tiled(*_check_glu(a, w, out, out_scale, out_quant=out_quant, act=act, **kw))
        elif act not in ACTS:
            raise ValueError(f"unknown activation {act!r}")
        else:
            t = _Tiled(*_check_out_quant(a, w, out_quant, out, out_scale, **kw),
                       out_quant_dtype(out_quant))
        return _run_tiled(
            _GLU if glu else _QOUT, t, a, w, out, out_scale,
            lambda C, out, out_scale, s: _launch(C, a, w, out, t.M, t.N, t.K, tile, mode, s,
                                                 act=ACTS[act], a_scale=a_scale, w_scale=w_scale,
                                                 out_scale=out_scale, glu=glu),
            out_quant=out_quant, glu=glu, stream=stream)
    if out_scale is not None:
        raise ValueError("out_scale goes with out_quant")
    C = load()
    scaled = a_scale is not None or w_scale is not None
    fp4 = _is_fp4(a) or _is_fp4(w)
    if out is None:
        rows = M if M is not None else a.shape[0]
        dflt = torch.bfloat16 if fp4 else default_out_dtype(a.dtype)
        out = torch.empty((rows, w.shape[0]), dtype=out_dtype or dflt, device=a.device)
    M = a.shape[0] if M is None else int(M)
    N, K = w.shape
    a_need = _phys_rows(M, a_grp, a_gstride)
    c_need = _phys_rows(M, c_grp, c_gstride)
    _check_operands(a, w, out, M, a_need)
    if c_need > out.shape[0]:
        raise ValueError(f"C row mapping reaches row {c_need - 1} >= {out.shape[0]}")
    if a_grp and (a_grp < 0 or a_gstride < a_grp):
        raise ValueError("a_gstride must be >= a_grp")
    if c_grp and (c_grp < 0 or c_gstride < c_grp):
        raise ValueError("c_gstride must be >= c_grp")
    _check_32_bits(M, N, K)
    s = _stream(stream, a)
    plain = (a_grp in (0, M) and c_grp in (0, M) and ACTS[act] == 0 and out.stride(0) == N
             and mode != "generic" and a.dtype != torch.float64)
    S = int(ksplit)
    if fp4 or scaled:
        f = _MX_FP4 if fp4 else _MX_FP8
        if fp4:
            _check_fp4(a, w, out, a_scale, w_scale, M, tile, mode, a_grp, S)
        else:
            _check_scales(a, w, a_scale, w_scale, M, tile, mode, a_grp, S)
        K *= f.per_byte  # elements; the leading dimensions go in elements too
        _need_fast_path(C, f"{f.noun} {'need' if f.plural else 'needs'} the MFMA fast path: "
                        "16-byte-aligned operand rows, 8-byte-aligned output rows", a, w, out, M,
                        N, K, dtype_code(out.dtype))
        _launch(C, a, w, out, M, N, K, tile, mode, s, c_grp=c_grp, c_gstride=c_gstride,
                act=ACTS[act], a_scale=a_scale, w_scale=w_scale)
        return out
    if S == 0:
        S = split_k_factor(M, N, K, a.element_size()) if plain and tile == "auto" else 1
    if S > 1:
        if not plain or K % S or M % 256 or N % 256:
            raise ValueError("ksplit needs plain rows, no activation, a dense output, whole "
                             "256x256 tiles and S | K")
        if tile not in ("auto", "pt4"):
            # another kernel runs the slices one after another into output-dtype partials,
            # summed (f32) by a reduce kernel
            part = torch.empty((S, M, N), dtype=out.dtype, device=a.device)
            _launch(C, a, w, part[0], M, N, K // S, tile, mode, s, ksplit=S)
            C.reduce_sum(out.data_ptr(), [part[j].data_ptr() for j in range(S)], M * N,
                         dtype_code(out.dtype), s)
            if stream is not None:
                part.record_stream(torch.cuda.ExternalStream(s))
            return out
        # every (slice, tile) pair in one launch into f32 partials, summed in slice order and
        # rounded once by the reduce kernel (an unsplit GEMM's rounding)
        ws = torch.empty((S, M, N), dtype=torch.float32, device=a.device)
        _launch(C, a, w, ws[0], M, N, K // S, "pt4", mode, s, ksplit=S)
        if out.dtype == torch.float32:
            C.reduce_sum(out.data_ptr(), [ws[j].data_ptr() for j in range(S)], M * N, DT_F32, s)
        else:
            C.reduce_sum(out.data_ptr(), [ws[j].data_ptr() for j in range(S)], M * N,
                         dtype_code(out.dtype), s, DT_F32)
        if stream is not None:  # the workspace stays allocated until that stream reaches it
            ws.record_stream(torch.cuda.ExternalStream(s))
        return out
    _launch(C, a, w, out, M, N, K, tile, mode, s, a_grp=a_grp, a_gstride=a_gstride, c_grp=c_grp,
            c_gstride=c_gstride, act=ACTS[act])
    return out


def fast_path_ok(a, w, out) -> bool:
    C = load()
    return bool(C.gemm_fast_path_ok(a.data_ptr(), w.data_ptr(), out.data_ptr(), a.stride(0),
                                    w.stride(0), out.stride(0), a.shape[0], w.shape[0],
                                    a.shape[1], dtype_code(a.dtype), dtype_code(out.dtype)))


# ---------------------------------------------------------------- grouped GEMM (per-expert weights)
MAX_GROUPS = 1024  # gemm.h kMaxGroups


def pack_glu_grouped(gate, up):
    """:func:`pack_glu` per expert: ``[E, F, K]`` gate and up rows -> the ``[E, 2F, K]`` weight
    ``gemm_grouped(glu=True)`` reads. Any dtype, scales included."""
    import torch

    if gate.dim() != 3 or up.dim() != 3 or gate.shape != up.shape or gate.dtype != up.dtype:
        raise ValueError(f"pack_glu_grouped takes two 3-D tensors of one shape and dtype, not "
                         f"{tuple(gate.shape)} {gate.dtype} and {tuple(up.shape)} {up.dtype}")
    E, F, K = gate.shape
    if F % GLU_GROUP:
        raise ValueError(f"pack_glu_grouped needs F % {GLU_GROUP} == 0 (F = {F})")
    g, u = (_as_bytes(t).reshape(E, F // GLU_GROUP, GLU_GROUP, K) for t in (gate, up))
    return torch.stack((g, u), dim=2).reshape(E, 2 * F, K).view(gate.dtype)


def clamp_offsets(offsets, T: int):
    """The offsets as the grouped kernel uses them (a Python list): ``o'[0] = clamp(o[0], 0, T)``,
    ``o'[g + 1] = clamp(o[g + 1], o'[g], T)``. Reads the tensor on the host."""
    o = [int(v) for v in offsets.tolist()]
    out = [min(max(o[0], 0), T)]
    for v in o[1:]:
        out.append(min(max(v, out[-1]), T))
    return out


def grouped_reference(a, w, offsets):
    """The specification of :func:`gemm_grouped` on dense operands, as an f32 torch loop on any
    device: rows ``[o'[g], o'[g + 1])`` of the ``[T, N]`` result are ``a[rows] @ w[g].T`` with the
    offsets clamped by :func:`clamp_offsets`; every other row is zero."""
    import torch

    if a.dim() != 2 or w.dim() != 3 or a.shape[1] != w.shape[2]:
        raise ValueError(f"grouped_reference takes a [T, K] and w [E, N, K], not "
                         f"{tuple(a.shape)} and {tuple(w.shape)}")
    if offsets.dim() != 1 or offsets.shape[0] != w.shape[0] + 1:
        raise ValueError(f"offsets must have shape ({w.shape[0] + 1},), not {tuple(offsets.shape)}")
    T = a.shape[0]
    o = clamp_offsets(offsets, T)
    out = torch.zeros((T, w.shape[1]), dtype=torch.float32, device=a.device)
    for g in range(w.shape[0]):
        if o[g + 1] > o[g]:
            out[o[g]:o[g + 1]] = a[o[g]:o[g + 1]].float() @ w[g].float().t()
    return out


def _check_group_count(f, E):
    if E < 1:
        raise ValueError(f"{f.noun} needs at least one group")
    if E > MAX_GROUPS:
        raise ValueError(f"{f.noun} takes at most {MAX_GROUPS} groups, not {E}")


def _check_offsets_dtype(offsets):
    import torch

    if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int32:
        raise TypeError(f"offsets must be an int32 tensor, not "
                        f"{getattr(offsets, 'dtype', type(offsets))}")


def _check_grouped(a, w, offsets, out=None, out_scale=None, *, out_dtype=None,
                   tile: str = "auto", act: str = "none", a_scale=None, w_scale=None,
                   out_quant: Optional[str] = None, glu: bool = False):
    """Every refusal of the grouped GEMM, on the host and before anything is loaded or launched
    (CPU tensors pass through it; the offsets' content is never read). What the ungrouped forms
    already refuse is refused by their own checks (:func:`_check_tiled`, through
    :func:`_check_out_quant` and :func:`_check_glu` for those forms), applied to ``a`` and an
    expert's slice of ``w`` and ``w_scale``. Returns ``(T, N, K, E, output dtype)``: ``N`` the
    rows of an expert's weight."""
    import torch

    if act not in ACTS:
        raise ValueError(f"unknown activation {act!r}")
    if not isinstance(w, torch.Tensor) or w.dim() != 3:
        raise ValueError(f"a grouped GEMM takes w as [E, N, K] (3-D), not "
                         f"{tuple(getattr(w, 'shape', ()))}")
    if a.dim() != 2:
        raise ValueError(f"a grouped GEMM takes a as [T, K] (2-D), not {tuple(a.shape)}")
    E, N = w.shape[0], w.shape[1]
    T = a.shape[0]
    _check_group_count(_GROUPED, E)
    _check_offsets_dtype(offsets)
    if offsets.dim() != 1 or offsets.shape[0] != E + 1 or not offsets.is_contiguous():
        raise ValueError(f"offsets must be contiguous with shape ({E + 1},) for {E} groups, not "
                         f"{tuple(offsets.shape)}")
    if offsets.device != a.device:
        raise ValueError(f"offsets is on {offsets.device}, the operands on {a.device}")
    if w.device != a.device:
        raise ValueError("operands on different devices")
    _check_tile(_GROUPED.noun, tile, _GROUPED.tile_note)
    fp4 = _is_fp4(a) or _is_fp4(w)
    fp8 = a.dtype == torch.float8_e4m3fn or w.dtype == torch.float8_e4m3fn
    if not fp4 and not fp8 and a.dtype not in (torch.bfloat16, torch.float16):
        _refuse_operands(_GROUPED, a)
    _check_same_dtype(a, w)
    if (fp8 or fp4) and (a_scale is None or w_scale is None):
        raise ValueError(_GROUPED.no_scales)
    if w.stride(2) != 1 or w.stride(1) < w.shape[2] or (E > 1 and w.stride(0) < N * w.stride(1)):
        raise ValueError(f"w needs unit inner stride, rows of at least K and experts at least "
                         f"N rows apart (strides {tuple(w.stride())})")
    if w.stride(0) * w.element_size() % 16:
        raise ValueError("the experts' weights must be a multiple of 16 bytes apart")
    K = (2 if fp4 else 1) * a.shape[1]
    scaled = fp4 or fp8
    if scaled and w_scale is not None:
        align = 8 if fp4 else 4
        if not isinstance(w_scale, torch.Tensor) or w_scale.dim() != 3 or \
                tuple(w_scale.shape) != (E, N, K // 32):
            raise ValueError(f"w_scale must have shape {(E, N, K // 32)}, not "
                             f"{tuple(getattr(w_scale, 'shape', ()))}")
        if w_scale.stride(0) % align or (E > 1 and w_scale.stride(0) < N * w_scale.stride(1)):
            raise ValueError(f"w_scale needs experts a multiple of {align} bytes and at least N "
                             f"rows apart (strides {tuple(w_scale.stride())})")
    elif w_scale is not None and (not isinstance(w_scale, torch.Tensor) or w_scale.dim() != 3):
        raise TypeError(f"block scales need fp8 / fp4 operands, not {a.dtype}")
    if out_quant is None and out_scale is not None:
        raise ValueError("out_scale goes with out_quant")
    _check_32_bits(T, N, K)
    # what the ungrouped forms refuse, per expert slice (all slices share shape and strides; the
    # first and the last differ in their addresses)
    if not glu and out_quant is None:
        _check_k(a, w)
    odt = None
    for g in sorted({0, E - 1}):
        kw = dict(out_dtype=out_dtype, a_scale=a_scale, tile=tile,
                  w_scale=w_scale[g] if w_scale is not None else None)
        if glu:
            odt = _check_glu(a, w[g], out, out_scale, out_quant=out_quant, act=act, **kw)[3]
        elif out_quant is not None:
            _check_out_quant(a, w[g], out_quant, out, out_scale, **kw)
            odt = out_quant_dtype(out_quant)
        else:
            odt = _check_tiled(_GROUPED, a, w[g], out, None, out_quant=None, mode="auto", M=None,
                               a_grp=0, c_grp=0, ksplit=0, **kw).odt
    return T, N, K, E, odt


def gemm_grouped(a, w, offsets, out=None, *, out_dtype=None, tile: str = "auto",
                 act: str = "none", a_scale=None, w_scale=None, out_quant: Optional[str] = None,
                 out_scale=None, glu: bool = False, stream=None):
    """Grouped GEMM over per-expert weights in ONE launch: rows ``[o[g], o[g + 1])`` of ``a``
    ``[T, K]`` are multiplied by ``w[g]`` of ``w`` ``[E, N, K]`` (unit inner stride, any
    ``w.stride(0) >= N * w.stride(1)``; fp4: ``K / 2`` bytes per row). ``offsets`` is an int32
    ``[E + 1]`` tensor on ``a``'s device that only the kernel reads: no host sync, so the call can
    be captured in a graph. The kernel clamps the offsets as it reads them
    (:func:`clamp_offsets`): nothing in the array can make it touch a row ``>= T``, and empty
    groups are legal anywhere.

    Operands and epilogues are those of ``gemm(..., glu=..., out_quant=...)`` on the tiled kernel
    (tiles :data:`SCALED_TILES`): bf16 -> bf16 | f32, f16 -> f16 | f32, block-scaled fp8 / fp4
    (``a_scale [T, K / 32]``, ``w_scale [E, N, K / 32]``) -> bf16 | f16 | f32, each dense, with
    ``act``, with ``glu`` (:func:`pack_glu_grouped`), with ``out_quant`` or with both; every
    group's rows are bit for bit what ``gemm(a[rows], w[g], tile=...)`` writes. Returns what
    ``gemm`` returns: ``[T, N]``, ``[T, N / 2]`` with ``glu``, or ``(q, s)`` with ``out_quant``.

    Rows outside ``[o'[0], o'[E])`` are not written: they are unspecified in an ``out`` (and
    ``out_scale``) allocated here, which is never zero-filled, and untouched in one passed in.
    :func:`_check_grouped` holds every refusal."""
    T, N, K, E, odt = _check_grouped(a, w, offsets, out, out_scale, out_dtype=out_dtype,
                                     tile=tile, act=act, a_scale=a_scale, w_scale=w_scale,
                                     out_quant=out_quant, glu=glu)
    am = 2 if _is_fp4(a) else 1
    scaled = a_scale is not None

    def launch(C, out, out_scale, s):
        cm = 2 if _is_fp4(out) else 1
        C.gemm_grouped(
            a=a.data_ptr(), b=w.data_ptr(), c=out.data_ptr(), offs=offsets.data_ptr(), ngroups=E,
            lda=am * a.stride(0), ldb=am * w.stride(1), ldc=cm * out.stride(0),
            b_gstride=am * w.stride(0), M=T, N=N, K=K,
            din=DT_FP4 if am == 2 else dtype_code(a.dtype),
            dout=DT_FP4 if cm == 2 else dtype_code(out.dtype), tile=TILES[tile], stream=s,
            act=ACTS[act], a_scale=a_scale.data_ptr() if scaled else 0,
            b_scale=w_scale.data_ptr() if scaled else 0,
            a_scale_ld=a_scale.stride(0) if scaled else 0,
            b_scale_ld=w_scale.stride(1) if scaled else 0,
            b_scale_gstride=w_scale.stride(0) if scaled else 0,
            c_scale=out_scale.data_ptr() if out_scale is not None else 0,
            c_scale_ld=out_scale.stride(0) if out_scale is not None else 0, glu=1 if glu else 0)

    return _run_tiled(_GROUPED, _Tiled(T, N, K, odt), a, w, out, out_scale, launch,
                      out_quant=out_quant, glu=glu, stream=stream)


# ---------------------------------------------------------------- K-grouped GEMM (routed wgrad)
def kgrouped_capacity(T: int, E: int, mod: int) -> int:
    """Columns that hold the padded K layout of any ``E`` groups over ``T`` rows (tile_map.h
    ``kgrouped_capacity``): ``(T // mod + E) * mod``, ``mod`` = 128 for MX-fp8 and 256 for MXFP4."""
    return (int(T) // mod + int(E)) * mod


def padded_offsets(offsets, T: int, mod: int):
    """The padded K layout as a Python list ``k0`` of ``E + 1`` column offsets (reads the tensor on
    the host; the kernels derive the same numbers from the raw offsets, tile_map.h
    ``kgrouped_range``): with the offsets clamped by :func:`clamp_offsets` and ``n_g`` rows in
    group ``g``, ``k0[g + 1] - k0[g] = mod * ceil(n_g / mod)`` and ``k0[0] = 0``. Group ``g`` owns
    the columns ``[k0[g], k0[g + 1])``; ``k0[E] <= kgrouped_capacity(T, E, mod)``."""
    o = clamp_offsets(offsets, T)
    k0 = [0]
    for g in range(len(o) - 1):
        k0.append(k0[-1] + mod * -(-(o[g + 1] - o[g]) // mod))
    return k0


def _check_kgrouped(a, w, offsets, rows, out=None, *, a_scale=None, w_scale=None, out_dtype=None,
                    tile: str = "auto"):
    """Every refusal of the K-grouped GEMM, on the host and before anything is loaded or launched
    (CPU tensors pass through it; the offsets' content is never read). Returns
    ``(M, N, K, E, output dtype)``: ``K`` the operands' column extent in elements."""
    import torch

    if not isinstance(a, torch.Tensor) or not isinstance(w, torch.Tensor) or a.dim() != 2 \
            or w.dim() != 2:
        raise ValueError("a K-grouped GEMM takes a as [M, cap] and w as [N, cap] (2-D)")
    fp4 = _is_fp4(a) or _is_fp4(w)
    fp8 = a.dtype == torch.float8_e4m3fn or w.dtype == torch.float8_e4m3fn
    if not fp4 and not fp8:
        raise TypeError(f"a K-grouped GEMM takes block-scaled fp8 or fp4 operands, not {a.dtype}")
    _check_same_dtype(a, w)
    if a_scale is None or w_scale is None:
        raise ValueError(_KGROUPED.no_scales)
    _check_offsets_dtype(offsets)
    if offsets.dim() != 1 or not offsets.is_contiguous():
        raise ValueError(f"offsets must be contiguous and 1-D, not {tuple(offsets.shape)}")
    E = offsets.shape[0] - 1
    _check_group_count(_KGROUPED, E)
    if offsets.device != a.device or w.device != a.device:
        raise ValueError("operands and offsets on different devices")
    if not isinstance(rows, int) or isinstance(rows, bool) or rows < 0 or rows >= 2 ** 31:
        raise ValueError(f"rows (the bound the offsets are clamped to) must be an int in "
                         f"[0, 2^31), not {rows!r}")
    _check_tile(_KGROUPED.noun, tile)
    f = _MX_FP4 if fp4 else _MX_FP8
    M, N = a.shape[0], w.shape[0]
    K = f.per_byte * a.shape[1]
    _check_k(a, w)
    _check_32_bits(M, N, K)
    cap = kgrouped_capacity(rows, E, f.kmod)
    if K < cap:
        raise ValueError(f"the operands have {K} columns, below the capacity {cap} of the padded "
                         f"layout of {E} groups over {rows} rows")
    for name, t in (("a", a), ("w", w)):
        if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
            raise ValueError(f"{name} needs unit inner stride (strides {tuple(t.stride())})")
    _check_block_scaled(f, a, w, a_scale, w_scale, M, tile, "auto", 0, 0)
    odt = _check_dense_out(_KGROUPED.noun, a, out, out_dtype,
                           (torch.bfloat16, torch.float16, torch.float32), M, N, groups=E)
    return M, N, K, E, odt


def gemm_kgrouped(a, w, offsets, rows, out=None, *, a_scale, w_scale, out_dtype=None,
                  tile: str = "auto", stream=None):
    """K-grouped GEMM in ONE launch, the wgrad of a routed linear layer: the groups lie along the
    contraction axis and each writes its own matrix,
    ``out[g] = a[:, k0_g : k0_g + kl_g] @ w[:, k0_g : k0_g + kl_g].T`` under the block scales of
    the same columns. ``a [M, cap]`` and ``w [N, cap]`` are block-scaled fp8 or fp4 in the padded
    K layout :func:`ddlb_amd.ops.mx.quantize_mx_t_grouped` writes (``a_scale [M, cap / 32]``,
    ``w_scale [N, cap / 32]``; ``cap >= kgrouped_capacity(rows, E, 128 | 256)``); ``offsets`` is
    the int32 ``[E + 1]`` device tensor of row offsets that only the kernel reads, clamped to
    ``rows`` (``T``) as everywhere (:func:`clamp_offsets`), and :func:`padded_offsets` gives the
    column ranges the kernel derives from it. No host sync; nothing in ``offsets`` can address a
    column outside the operands.

    ``out [E, M, N]`` bf16 (default) / f16 / f32, ``out.stride(0) >= M * out.stride(1)``; every
    ``out[g]`` is bit for bit what ``gemm`` with the same tile writes for those column slices, and
    a group without rows gets ``+0.0`` everywhere. Tiles :data:`SCALED_TILES`.
    :func:`_check_kgrouped` holds every refusal."""
    M, N, K, E, odt = _check_kgrouped(a, w, offsets, rows, out, a_scale=a_scale, w_scale=w_scale,
                                      out_dtype=out_dtype, tile=tile)
    am = 2 if _is_fp4(a) else 1
    return _run_tiled(
        _KGROUPED, _Tiled(M, N, K, odt), a, w, out, None,
        lambda C, out, _, s: C.gemm_kgrouped(
            a=a.data_ptr(), b=w.data_ptr(), c=out.data_ptr(), offs=offsets.data_ptr(), ngroups=E,
            rows=rows, lda=am * a.stride(0), ldb=am * w.stride(0), ldc=out.stride(1),
            c_gstride=out.stride(0), M=M, N=N, K=K,
            din=DT_FP4 if am == 2 else dtype_code(a.dtype), dout=dtype_code(odt),
            tile=TILES[tile], stream=s, a_scale=a_scale.data_ptr(), b_scale=w_scale.data_ptr(),
            a_scale_ld=a_scale.stride(0), b_scale_ld=w_scale.stride(0)),
        groups=E, stream=stream)
