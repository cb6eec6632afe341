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
"""

from __future__ import annotations

from typing import Optional

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


def _check_operands(a, w, out, M, a_rows_phys):
    import torch

    if a.device.type != "cuda" or w.device.type != "cuda" or out.device.type != "cuda":
        raise ValueError("native GEMM operands must be ROCm device tensors")
    if not (a.device == w.device == out.device):
        raise ValueError("operands on different devices")
    if a.dim() != 2 or w.dim() != 2 or out.dim() != 2:
        raise ValueError("native GEMM expects 2-D operands")
    if a.stride(1) != 1 or w.stride(1) != 1 or out.stride(1) != 1:
        raise ValueError("operands must be row-major with unit inner stride")
    if a.dtype != w.dtype:
        raise TypeError(f"A dtype {a.dtype} != W dtype {w.dtype}")
    if a.shape[1] != w.shape[1]:
        raise ValueError(f"K mismatch: A {tuple(a.shape)} vs W {tuple(w.shape)}")
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
SCALED_FP4_TILES = ("256x128", "128x256", "128x128", "256x128w4")  # gemm.h mx4_offers()


def _fp4_dtype():
    import torch

    return getattr(torch, "float4_e2m1fn_x2", None)


def _is_fp4(t) -> bool:
    dt = _fp4_dtype()
    return dt is not None and getattr(t, "dtype", None) == dt


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
    if mode not in ("auto", "mx"):
        raise ValueError(f"fp4 operands run the MX kernel (mode auto / mx), not mode={mode!r}")
    if tile != "auto" and tile not in SCALED_FP4_TILES:
        raise ValueError(f"the fp4 GEMM is offered for tile auto / {SCALED_FP4_TILES}, not "
                         f"{tile!r}")
    if a_grp not in (0, M):
        raise ValueError("the fp4 GEMM needs plain A rows (no grouped A rows)")
    if ksplit > 1:
        raise ValueError("the fp4 GEMM does not combine with a K-split")
    K = 2 * a.shape[1]
    if K % 256:
        raise ValueError(f"the fp4 GEMM needs K % 256 == 0 (K = {K})")
    for name, sc, rows in (("a_scale", a_scale, a.shape[0]), ("w_scale", w_scale, w.shape[0])):
        if not isinstance(sc, torch.Tensor) or sc.dtype != torch.uint8:
            raise TypeError(f"{name} must be a uint8 tensor of E8M0 bytes")
        if sc.device != a.device:
            raise ValueError(f"{name} is on {sc.device}, the operands on {a.device}")
        if tuple(sc.shape) != (rows, K // 32):
            raise ValueError(f"{name} must have shape {(rows, K // 32)}, not {tuple(sc.shape)}")
        if sc.stride(1) != 1 or sc.stride(0) % 8 or sc.stride(0) < K // 32:
            raise ValueError(f"{name} needs unit inner stride and a row stride that is a "
                             f"multiple of 8 (strides {tuple(sc.stride())})")
        if sc.data_ptr() % 8:
            raise ValueError(f"{name} must start at an 8-byte-aligned address")
        if rows * sc.stride(0) >= 2 ** 31:
            raise ValueError(f"{name} spans 2 GiB or more")


def _check_scales(a, w, a_scale, w_scale, M, tile, mode, a_grp, ksplit):
    """Every refusal of the block-scaled GEMM, before anything is launched."""
    import torch

    if (a_scale is None) != (w_scale is None):
        raise ValueError("a_scale and w_scale go together: pass both or neither")
    if a.dtype != torch.float8_e4m3fn:
        raise TypeError(f"block scales need float8_e4m3fn operands, not {a.dtype}")
    if mode not in ("auto", "mx"):
        raise ValueError(f"block scales run the MX kernel (mode auto / mx), not mode={mode!r}")
    if tile != "auto" and tile not in SCALED_TILES:
        raise ValueError(f"block scales are offered for tile auto / {SCALED_TILES}, not "
                         f"{tile!r} (the ping-pong kernels t8 / pt8 / t4 / pt4 take unit scales)")
    if a_grp not in (0, M):
        raise ValueError("block scales need plain A rows (no grouped A rows)")
    if ksplit > 1:
        raise ValueError("block scales do not combine with a K-split")
    K = a.shape[1]
    if K % 128:
        raise ValueError(f"block scales need K % 128 == 0 (K = {K})")
    for name, sc, rows in (("a_scale", a_scale, a.shape[0]), ("w_scale", w_scale, w.shape[0])):
        if not isinstance(sc, torch.Tensor) or sc.dtype != torch.uint8:
            raise TypeError(f"{name} must be a uint8 tensor of E8M0 bytes")
        if sc.device != a.device:
            raise ValueError(f"{name} is on {sc.device}, the operands on {a.device}")
        if tuple(sc.shape) != (rows, K // 32):
            raise ValueError(f"{name} must have shape {(rows, K // 32)}, not {tuple(sc.shape)}")
        if sc.stride(1) != 1 or sc.stride(0) % 4 or sc.stride(0) < K // 32:
            raise ValueError(f"{name} needs unit inner stride and a row stride that is a "
                             f"multiple of 4 (strides {tuple(sc.stride())})")
        if sc.data_ptr() % 4:
            raise ValueError(f"{name} must start at a 4-byte-aligned address")
        if rows * sc.stride(0) >= 2 ** 31:
            raise ValueError(f"{name} spans 2 GiB or more")


OUT_QUANTS = ("mx", "mxfp4")


def out_quant_dtype(out_quant: str):
    import torch

    return _fp4_dtype() if out_quant == "mxfp4" else torch.float8_e4m3fn


def _check_out_quant(a, w, out_quant, out=None, out_scale=None, *, a_scale=None, w_scale=None,
                     tile: str = "auto", mode: str = "auto", M: Optional[int] = None,
                     a_grp: int = 0, c_grp: int = 0, ksplit: int = 0, out_dtype=None):
    """Every refusal of the quantised-output GEMM (``out_quant="mx" | "mxfp4"``), on the host and
    before anything is loaded or launched (CPU tensors pass through it). ``out`` / ``out_scale``
    are checked when given. Returns ``(M, N, K)`` in elements."""
    import torch
    from types import SimpleNamespace

    if out_quant not in OUT_QUANTS:
        raise ValueError(f"out_quant must be None or one of {OUT_QUANTS}, not {out_quant!r}")
    q4 = out_quant == "mxfp4"
    if q4 and _fp4_dtype() is None:
        raise TypeError("out_quant='mxfp4' needs torch.float4_e2m1fn_x2")
    qdt = out_quant_dtype(out_quant)
    if a.dim() != 2 or w.dim() != 2:
        raise ValueError("native GEMM expects 2-D operands")
    fp4 = _is_fp4(a) or _is_fp4(w)
    M = a.shape[0] if M is None else int(M)
    N = w.shape[0]
    K = 2 * a.shape[1] if fp4 else a.shape[1]
    if a.shape[1] != w.shape[1]:
        raise ValueError(f"K mismatch: A {tuple(a.shape)} vs W {tuple(w.shape)}")
    if not 0 <= M <= a.shape[0]:
        raise ValueError(f"M = {M} is outside A's {a.shape[0]} rows")
    if out_dtype is not None and out_dtype != qdt:
        raise TypeError(f"out_quant={out_quant!r} writes {qdt}, not out_dtype={out_dtype}")
    nmod = 256 if q4 else 128
    if N % nmod:
        raise ValueError(f"out_quant={out_quant!r} needs N % {nmod} == 0 (N = {N}): whole "
                         "32-column blocks, as many as the GEMM that reads them takes per K-tile")
    if mode == "generic":
        raise ValueError("a quantised output comes from the tiled MFMA kernel, not mode='generic'")
    if mode not in MODES:
        raise ValueError(f"unknown mode {mode!r}")
    if tile != "auto" and tile not in SCALED_TILES:
        raise ValueError(f"a quantised output is offered for tile auto / {SCALED_TILES}, not "
                         f"{tile!r}")
    if int(ksplit) > 1:
        raise ValueError("a quantised output does not combine with a K-split")
    if a_grp not in (0, M) or c_grp not in (0, M):
        raise ValueError("a quantised output needs plain A and C rows (no grouped rows)")
    # the inputs: bf16, f16, block-scaled fp8, block-scaled fp4
    if fp4:
        _check_fp4(a, w, SimpleNamespace(dtype=torch.bfloat16), a_scale, w_scale, M, tile, mode,
                   a_grp, int(ksplit))
    elif a.dtype == torch.float8_e4m3fn or w.dtype == torch.float8_e4m3fn:
        if a.dtype != w.dtype:
            raise TypeError(f"A dtype {a.dtype} != W dtype {w.dtype}")
        if a_scale is None or w_scale is None:
            raise ValueError("a quantised output from fp8 operands needs a_scale and w_scale "
                             "(there is no unit-scale kernel with this epilogue)")
        _check_scales(a, w, a_scale, w_scale, M, tile, mode, a_grp, int(ksplit))
    elif a.dtype in (torch.bfloat16, torch.float16):
        if a.dtype != w.dtype:
            raise TypeError(f"A dtype {a.dtype} != W dtype {w.dtype}")
        if a_scale is not None or w_scale is not None:
            raise TypeError(f"block scales need fp8 / fp4 operands, not {a.dtype}")
        if mode == "mx":
            raise ValueError(f"mode='mx' needs fp8 / fp4 operands, not {a.dtype}")
    else:
        raise TypeError(f"out_quant takes bf16, f16, scaled fp8 or scaled fp4 operands, not "
                        f"{a.dtype}")
    if M >= 2 ** 31 or N >= 2 ** 31 or K >= 2 ** 31:
        raise ValueError("dimensions must fit in 32 bits")
    ncol, sal = (N // 2 if q4 else N), (8 if q4 else 4)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != qdt:
            raise TypeError(f"out must be a {qdt} tensor for out_quant={out_quant!r}, not "
                            f"{getattr(out, 'dtype', type(out))}")
        if out.device != a.device:
            raise ValueError(f"out is on {out.device}, the operands on {a.device}")
        if out.dim() != 2 or out.shape[0] < M or out.shape[1] != ncol:
            raise ValueError(f"out must have shape (>= {M}, {ncol}), not {tuple(out.shape)}")
        if out.stride(1) != 1 or out.stride(0) < ncol or out.stride(0) % 16:
            raise ValueError(f"out needs unit inner stride and a row stride that is a multiple "
                             f"of 16 bytes (strides {tuple(out.stride())})")
        if out.data_ptr() % 16:
            raise ValueError("out must start at a 16-byte-aligned address")
    if out_scale is not None:
        if not isinstance(out_scale, torch.Tensor) or out_scale.dtype != torch.uint8:
            raise TypeError("out_scale must be a uint8 tensor of E8M0 bytes")
        if out_scale.device != a.device:
            raise ValueError(f"out_scale is on {out_scale.device}, the operands on {a.device}")
        if out_scale.dim() != 2 or out_scale.shape[0] < M or out_scale.shape[1] != N // 32:
            raise ValueError(f"out_scale must have shape (>= {M}, {N // 32}), not "
                             f"{tuple(out_scale.shape)}")
        if (out_scale.stride(1) != 1 or out_scale.stride(0) < N // 32
                or out_scale.stride(0) % sal):
            raise ValueError(f"out_scale needs unit inner stride and a row stride that is a "
                             f"multiple of {sal} (strides {tuple(out_scale.stride())})")
        if M * out_scale.stride(0) >= 2 ** 31:
            raise ValueError("out_scale spans 2 GiB or more")
        if out_scale.data_ptr() % sal:
            raise ValueError(f"out_scale must start at a {sal}-byte-aligned address")
    if M * (N // 32) >= 2 ** 31:
        raise ValueError("out_scale spans 2 GiB or more")
    return M, N, K


def _check_quant_operands(a, w):
    if a.device.type != "cuda" or w.device.type != "cuda":
        raise ValueError("native GEMM operands must be ROCm device tensors")
    if a.device != w.device:
        raise ValueError("operands on different devices")
    if a.stride(1) != 1 or w.stride(1) != 1:
        raise ValueError("operands must be row-major with unit inner stride")


def _gemm_out_quant(a, w, out, out_scale, out_quant, *, out_dtype, tile, mode, M, a_grp, c_grp,
                    stream, act, ksplit, a_scale, w_scale):
    """The quantised-output launch: ``(q, s)`` written by the tiled kernel's epilogue. Every
    refusal comes first, before the extension is loaded."""
    import torch

    if act not in ACTS:
        raise ValueError(f"unknown activation {act!r}")
    M, N, K = _check_out_quant(a, w, out_quant, out, out_scale, a_scale=a_scale, w_scale=w_scale,
                               tile=tile, mode=mode, M=M, a_grp=a_grp, c_grp=c_grp, ksplit=ksplit,
                               out_dtype=out_dtype)
    C = load()
    q4 = out_quant == "mxfp4"
    fp4 = _is_fp4(a)
    ncol = N // 2 if q4 else N
    _check_quant_operands(a, w)
    # dense rows are what the consumer asks of a / a_scale: N % 128 (256) makes a data row a
    # multiple of 16 bytes and a scale row a multiple of 4 (8)
    if out is None:
        out = torch.empty((M, ncol), dtype=torch.uint8,
                          device=a.device).view(out_quant_dtype(out_quant))
    if out_scale is None:
        out_scale = torch.empty((M, N // 32), dtype=torch.uint8, device=a.device)
    kb = K // 2 if fp4 else K  # the operands as the byte / element matrices the kernel reads
    if M and N and not C.gemm_fast_path_ok(a.data_ptr(), w.data_ptr(), out.data_ptr(),
                                           a.stride(0), w.stride(0), out.stride(0), M, N, kb,
                                           DT_U8 if fp4 else dtype_code(a.dtype), DT_U8):
        raise ValueError("a quantised output needs the MFMA fast path: 16-byte-aligned operand "
                         "rows and K a whole number of 128-byte K-tiles")
    s = stream if stream is not None else torch.cuda.current_stream(a.device).cuda_stream
    scaled = a_scale is not None
    # (ksplit 1: neither a requested nor the automatic K-split engages on this path)
    C.gemm(a.data_ptr(), w.data_ptr(), out.data_ptr(),
           (2 if fp4 else 1) * a.stride(0), (2 if fp4 else 1) * w.stride(0),
           (2 if q4 else 1) * out.stride(0), M, N, K,
           DT_FP4 if fp4 else dtype_code(a.dtype), DT_FP4 if q4 else DT_FP8, TILES[tile],
           MODES["mx"] if scaled else MODES["auto"], 0, 0, 0, 0, s, ACTS[act], 1,
           a_scale.data_ptr() if scaled else 0, w_scale.data_ptr() if scaled else 0,
           a_scale.stride(0) if scaled else 0, w_scale.stride(0) if scaled else 0,
           out_scale.data_ptr(), out_scale.stride(0))
    if stream is not None:  # the outputs stay allocated until that stream reaches them
        out.record_stream(torch.cuda.ExternalStream(s))
        out_scale.record_stream(torch.cuda.ExternalStream(s))
    return out[:M], out_scale[:M]


def gemm(a, w, out=None, *, out_dtype=None, tile: str = "auto", mode: str = "auto",
         M: Optional[int] = None, a_grp: int = 0, a_gstride: int = 0, c_grp: int = 0,
         c_gstride: int = 0, stream=None, act: str = "none", ksplit: int = 0,
         a_scale=None, w_scale=None, out_quant: Optional[str] = None, out_scale=None):
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
    holds every refusal."""
    import torch

    if out_quant is None and out_scale is not None:
        raise ValueError("out_scale goes with out_quant")
    if out_quant is not None:
        return _gemm_out_quant(a, w, out, out_scale, out_quant, out_dtype=out_dtype,
                               tile=tile, mode=mode, M=M, a_grp=a_grp, c_grp=c_grp,
                               stream=stream, act=act, ksplit=ksplit, a_scale=a_scale,
                               w_scale=w_scale)
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
    if M >= 2 ** 31 or N >= 2 ** 31 or K >= 2 ** 31:
        raise ValueError("dimensions must fit in 32 bits")
    s = stream if stream is not None else torch.cuda.current_stream(a.device).cuda_stream
    plain = (a_grp in (0, M) and c_grp in (0, M) and ACTS[act] == 0 and out.stride(0) == N
             and mode != "generic" and a.dtype != torch.float64)
    S = int(ksplit)
    if fp4:
        _check_fp4(a, w, out, a_scale, w_scale, M, tile, mode, a_grp, S)
        K = 2 * K  # elements; the leading dimensions go in elements too
        if M and N and not C.gemm_fast_path_ok(a.data_ptr(), w.data_ptr(), out.data_ptr(),
                                               a.stride(0), w.stride(0), out.stride(0), M, N,
                                               K // 2, DT_U8, dtype_code(out.dtype)):
            raise ValueError("the fp4 GEMM needs the MFMA fast path: 16-byte-aligned operand "
                             "rows, 8-byte-aligned output rows")
        C.gemm(a.data_ptr(), w.data_ptr(), out.data_ptr(), 2 * a.stride(0), 2 * w.stride(0),
               out.stride(0), M, N, K, DT_FP4, dtype_code(out.dtype), TILES[tile], MODES["mx"],
               0, 0, c_grp, c_gstride, s, ACTS[act], 1, a_scale.data_ptr(), w_scale.data_ptr(),
               a_scale.stride(0), w_scale.stride(0))
        return out
    if scaled:
        _check_scales(a, w, a_scale, w_scale, M, tile, mode, a_grp, S)
        if M and N and not C.gemm_fast_path_ok(a.data_ptr(), w.data_ptr(), out.data_ptr(),
                                               a.stride(0), w.stride(0), out.stride(0), M, N, K,
                                               DT_FP8, dtype_code(out.dtype)):
            raise ValueError("block scales need the MFMA fast path: 16-byte-aligned operand "
                             "rows, 8-byte-aligned output rows")
        C.gemm(a.data_ptr(), w.data_ptr(), out.data_ptr(), a.stride(0), w.stride(0),
               out.stride(0), M, N, K, DT_FP8, dtype_code(out.dtype), TILES[tile], MODES["mx"],
               0, 0, c_grp, c_gstride, s, ACTS[act], 1, a_scale.data_ptr(), w_scale.data_ptr(),
               a_scale.stride(0), w_scale.stride(0))
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
            C.gemm(a.data_ptr(), w.data_ptr(), part.data_ptr(), a.stride(0), w.stride(0), N, M,
                   N, K // S, dtype_code(a.dtype), dtype_code(out.dtype), TILES[tile],
                   MODES[mode], 0, 0, 0, 0, s, 0, S)
            C.reduce_sum(out.data_ptr(), [part[j].data_ptr() for j in range(S)], M * N,
                         dtype_code(out.dtype), s)
            if stream is not None:
                part.record_stream(torch.cuda.ExternalStream(s))
            return out
        # every (slice, tile) pair in one launch into f32 partials, summed in slice order and
        # rounded once by the reduce kernel (an unsplit GEMM's rounding)
        ws = torch.empty((S, M, N), dtype=torch.float32, device=a.device)
        C.gemm(a.data_ptr(), w.data_ptr(), ws.data_ptr(), a.stride(0), w.stride(0), N, M, N,
               K // S, dtype_code(a.dtype), DT_F32, TILES["pt4"], MODES[mode], 0, 0, 0, 0, s, 0, S)
        if out.dtype == torch.float32:
            C.reduce_sum(out.data_ptr(), [ws[j].data_ptr() for j in range(S)], M * N, DT_F32, s)
        else:
            C.reduce_sum(out.data_ptr(), [ws[j].data_ptr() for j in range(S)], M * N,
                         dtype_code(out.dtype), s, DT_F32)
        if stream is not None:  # the workspace stays allocated until that stream reaches it
            ws.record_stream(torch.cuda.ExternalStream(s))
        return out
    C.gemm(a.data_ptr(), w.data_ptr(), out.data_ptr(), a.stride(0), w.stride(0), out.stride(0),
           M, N, K, dtype_code(a.dtype), dtype_code(out.dtype), TILES[tile], MODES[mode],
           a_grp, a_gstride, c_grp, c_gstride, s, ACTS[act])
    return out


def fast_path_ok(a, w, out) -> bool:
    C = load()
    return bool(C.gemm_fast_path_ok(a.data_ptr(), w.data_ptr(), out.data_ptr(), a.stride(0),
                                    w.stride(0), out.stride(0), a.shape[0], w.shape[0],
                                    a.shape[1], dtype_code(a.dtype), dtype_code(out.dtype)))
