"""Exact tests with byte offsets past 2^31 and 2^32: every GEMM kernel family, the MX quantisers,
the copy kernel and the reduce kernel, and both sides of each host-side gate that keeps a 32-bit
offset in range.

The shapes stay small (M, N <= 1280, two K-tiles but for the K-split and one long-row case of
gate 2); the *leading dimensions* are large. One matrix
of a case at a time is a far view (``tests/_exact.py``: rows megabytes apart behind a 2 GiB front
guard, so that an offset truncated to 32 bits or sign-extended from them still lands inside the
one allocation and shows as a wrong value, not as a fault); the other two are the ordinary padded
operands and sentinel outputs. Operands are integers in -3..3 with pairwise distinct rows
(``tests/test_exact_refs_cpu.py``), every comparison is ``torch.equal`` with ``exact()`` /
``exact_scaled()`` or, for the quantisers, byte for byte with the torch specification, and after
every far output the whole backing outside the view must still hold the sentinel.

The gates (docs/ARCHITECTURE.md "32-bit offsets and their gates"); ``gate_ld`` finds the leading
dimensions on both sides from their Python copies, and both sides must be exact:
  1. ``c_fits_wt()``: pt4 / t4 store C through 32-bit buffer offsets below 0x7FFFFFF0 bytes;
  2. ``pt4_ok()``: operand row pitches up to 4 MiB, t4 beyond;
  3. the pt4 K-split: one launch while the partials stay below 0x7FFFFFF0 bytes, the slice loop
     from there on;
  4. ``scale_operands_ok()`` / the ``c_scale_ld`` check: ``rows * scale_ld < 2^31``, a refusal
     (of ``gemm()`` and of the native entry) from there on.

Out of scope: the in-kernel all-gather's 1 GiB copy-unit gate (``gemm_launch``'s
``flag_rows * lda * esz / ag_parts`` check). At world 1 there is no copy unit to run.

All GEMM and quantiser cases share one backing of just under 10 GiB, refilled per case; the copy
and reduce tests release it and allocate their own two buffers. The last test asserts that the
module's peak stayed below 10 GiB."""

import gc

import pytest
import torch

import _exact as X
from _exact import (FAR_GUARD, FAR_PITCH, FP8, SENTINEL, exact, exact_scaled, far_operands,
                    far_out, far_span, far_view, gate_ld, padded, sentinel_out, untouched,
                    untouched_far)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
GIB = 2 ** 30
PEAK_LIMIT = 10 * GIB

FORMS = [(BF16, BF16, "auto"), (FP8, F32, "mx"), (F32, F32, "auto")]
PING = ("t8", "pt8", "t4", "pt4")
# the largest far view of the module: 512 rows FAR_PITCH apart, rows of at most 4 KiB
BACKING_BYTES = far_span(512, 4096, FAR_PITCH)
PT4_C_PITCH = 9 << 20          # 511 rows reach past 2^32: not write-through
T_PITCH_X, T_PITCH_OUT = 17 << 20, 22 << 20   # row 255 of x, row 199 of qt / st past 2^32
SENT_BYTE = int(SENTINEL) & 0xFF


def _name(dt):
    return str(dt).replace("torch.", "").replace("float8_e4m3fn", "fp8").replace("float", "f")


def _form_id(form):
    return f"{_name(form[0])}-{_name(form[1])}-{form[2]}"


def _esz(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _k(din, ktiles):
    """K of ``ktiles`` 128-byte K-tiles."""
    return ktiles * 128 // _esz(din)


def _out_pad(N, dout):
    return next(p for p in range(4, 12) if ((N + p) * _esz(dout)) % 8 == 0)


def _tiled_codes():
    from ddlb_amd.ops.gemm import TILES

    return [t for t in TILES if t not in PING]


def _free_gpu_memory():
    gc.collect()
    torch.cuda.empty_cache()


def _need(nbytes, what):
    """Skip (never on an otherwise idle MI355X) when ``nbytes`` do not fit."""
    free, total = torch.cuda.mem_get_info()
    if free < nbytes + (64 << 20):
        pytest.skip(f"{what} needs {nbytes} bytes; {free} of {total} are free")


class _Backing:
    """The module's one far backing, allocated at first use and released on request."""

    def __init__(self):
        self.buf = None
        self.base = 0

    def get(self):
        if self.buf is None:
            _free_gpu_memory()
            _need(FAR_GUARD + BACKING_BYTES, "the far backing")
            self.buf = X.far_backing(BACKING_BYTES)
        return self.buf

    def release(self):
        self.buf = None
        _free_gpu_memory()


@pytest.fixture(scope="module")
def far():
    _free_gpu_memory()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    hold = _Backing()
    hold.base = torch.cuda.memory_allocated()   # what earlier modules keep alive
    yield hold
    hold.release()


# ---------------------------------------------------------------------------- the GEMM runner
def _operands(M, N, K, din, dout):
    """``(a, w, exact product)`` on the device. The references are computed on the CPU: a matrix
    product on the device would have the BLAS library allocate its workspace, tens of MiB that
    would count against this module's memory bound."""
    a, w = far_operands(M, N, K, din)
    return a.to(DEV), w.to(DEV), exact(a, w, dout).to(DEV)


def _gemm_far(far, form, tile, M, N, K, which, pitch, **kw):
    """One GEMM with operand ``which`` ("a", "w" or "c") in a far view whose rows lie ``pitch``
    bytes apart: the exact product, nothing written outside C."""
    from ddlb_amd.ops.gemm import fast_path_ok, gemm

    din, dout, mode = form
    a, w, ref = _operands(M, N, K, din, dout)
    backing = far.get()
    A = far_view(backing, a, pitch) if which == "a" else padded(a)
    W = far_view(backing, w, pitch) if which == "w" else padded(w)
    if which == "c":
        C = far_out(backing, M, N, dout, pitch)
    else:
        buf, C = sentinel_out(M, N, dout, pad_cols=_out_pad(N, dout))
    if mode != "generic":
        assert fast_path_ok(A, W, C), (form, tile, which)
    gemm(A, W, C, tile=tile, mode=mode, **kw)
    torch.cuda.synchronize()
    bad = int((C != ref).sum())
    assert bad == 0, (f"{_form_id(form)} {tile} {(M, N, K)} {which} far at pitch {pitch}: {bad} "
                      f"wrong elements, the first at {(C != ref).nonzero()[0].tolist()}")
    if which == "c":
        untouched_far(backing, C)
    else:
        untouched(buf, M, N)


def _each_operand_far(far, form, tile, shape, K, pitch):
    M, N = shape
    _gemm_far(far, form, tile, M, N, K, "a", pitch)
    _gemm_far(far, form, tile, N, M, K, "w", pitch)     # W far: its rows take the larger count
    _gemm_far(far, form, tile, M, N, K, "c", pitch)


# ---------------------------------------------------------------------------- a. 64-bit paths
@pytest.mark.parametrize("form", FORMS, ids=_form_id)
@pytest.mark.parametrize("tile", _tiled_codes())
def test_tiled_kernels_far(far, form, tile):
    """gemm_tn_kernel (``aptr`` / ``bptr`` / ``crow``), ragged 300 x 202: rows from 128 on lie
    past 2^31, rows from 256 on past 2^32; the clamped row loads of the last tile included."""
    assert 299 * FAR_PITCH > 2 ** 32 and 201 * FAR_PITCH > 2 ** 31
    _each_operand_far(far, form, tile, X.FAR_TILED, _k(form[0], 2), FAR_PITCH)


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_generic_kernel_far(far, form):
    din, dout, _ = form
    _each_operand_far(far, (din, dout, "generic"), "auto", X.FAR_TILED, _k(din, 2), FAR_PITCH)


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
@pytest.mark.parametrize("tile", ["t8", "pt8", "t4"])
def test_ping_pong_kernels_far(far, form, tile):
    """t8 / pt8 / t4 (``sB``, ``c_row()``; A and W rows 16 MiB + 16 apart are beyond pt4's reach),
    whole tiles 512 x 256: the second row panel starts past 2^32."""
    assert not X.pt4_ld_ok(FAR_PITCH, 1) and not X.c_fits_wt(512, 256, FAR_PITCH // 4, 4)
    _each_operand_far(far, form, tile, X.FAR_PING, _k(form[0], 2), FAR_PITCH)


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
@pytest.mark.parametrize("which", ["a", "w"])
def test_pt4_operand_far(far, form, which):
    """pt4 with A (W) rows exactly 4 MiB apart, the largest pitch ``pt4_ok`` takes: 1280 rows put
    the fifth row (column) panel past 2^32; the panel offsets stay 32-bit, the panel base not."""
    din = form[0]
    M, N = X.FAR_PT4 if which == "a" else X.FAR_PT4[::-1]
    assert X.pt4_ld_ok(X.PT4_LD_BYTES // _esz(din), _esz(din)) and 1024 * X.PT4_LD_BYTES == 2 ** 32
    _gemm_far(far, form, "pt4", M, N, _k(din, 2), which, X.PT4_LD_BYTES)


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_pt4_c_far(far, form):
    """pt4's plain 64-bit C stores: 512 x 256 on a C pitch of 9 MiB crosses 2^32."""
    din, dout, _ = form
    M, N = X.FAR_PING
    assert not X.c_fits_wt(M, N, PT4_C_PITCH // _esz(dout), _esz(dout))
    assert (M - 1) * PT4_C_PITCH > 2 ** 32
    _gemm_far(far, form, "pt4", M, N, _k(din, 2), "c", PT4_C_PITCH)


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
@pytest.mark.parametrize("tile", ["pt4", "t4"])
@pytest.mark.parametrize("which", ["a", "c"])
def test_grouped_rows_far(far, form, tile, which):
    """``map_row()`` with a large group stride: groups of 256 rows on a modest row pitch, group 1
    starting past 2^31 and group 2 past 2^32. The skipped A rows hold poison, the skipped C rows
    keep the sentinel."""
    from ddlb_amd.ops.gemm import gemm

    din, dout, mode = form
    (M, N), K, grp = X.FAR_GROUPED, _k(din, 2), 256
    ld_bytes = 4096 + 16
    gs = -(-(2 ** 31) // ld_bytes)                       # rows: group 1 starts past 2^31
    assert gs * ld_bytes >= 2 ** 31 and 2 * gs * ld_bytes >= 2 ** 32 and M // grp == 3
    phys = 2 * gs + grp
    rows = torch.cat([torch.arange(g * gs, g * gs + grp) for g in range(M // grp)]).to(DEV)
    a, w, ref = _operands(M, N, K, din, dout)
    backing = far.get()
    kw = dict(M=M, tile=tile, mode=mode)
    if which == "a":
        A = far_out(backing, phys, K, din, ld_bytes, fill=X.POISON)
        raw = X._WORD[_esz(din)]                 # (no indexed assignment of e4m3 elements)
        A.view(raw)[rows] = a.view(raw)
        buf, C = sentinel_out(M, N, dout, pad_cols=_out_pad(N, dout))
        gemm(A, padded(w), C, a_grp=grp, a_gstride=gs, **kw)
        torch.cuda.synchronize()
        assert torch.equal(C, ref)
        untouched(buf, M, N)
    else:
        C = far_out(backing, phys, N, dout, ld_bytes)
        assert not X.c_fits_wt(M, N, ld_bytes // _esz(dout), _esz(dout), grp, gs)
        gemm(padded(a), padded(w), C, c_grp=grp, c_gstride=gs, **kw)
        torch.cuda.synchronize()
        assert torch.equal(C[rows], ref)
        untouched_far(backing, C, rows=rows)


# ---------------------------------------------------------------------------- b. the gates
@pytest.mark.parametrize("dout", [BF16, F32], ids=_name)
@pytest.mark.parametrize("tile", ["pt4", "t4"])
def test_gate1_write_through_c(far, tile, dout):
    """``c_fits_wt``: the last ``ldc`` whose C is stored through 32-bit buffer offsets (the last
    byte just below 0x7FFFFFF0) and the next one, which takes the plain 64-bit stores."""
    M, N = X.GATE_C
    osz = _esz(dout)
    last, nxt = gate_ld(lambda ld: X.c_fits_wt(M, N, ld, osz), X.align_of(8, osz))
    for ldc in (last, nxt):
        _gemm_far(far, (BF16, dout, "auto"), tile, M, N, _k(BF16, 2), "c", ldc * osz)


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
@pytest.mark.parametrize("which", ["a", "w"])
def test_gate2_pt4_operand_pitch(far, form, which):
    """``pt4_ok``: a row pitch of exactly 4 MiB runs pt4 (32-bit offsets within a 256-row panel
    reach 1 GiB), 16 bytes more runs t4."""
    din = form[0]
    esz = _esz(din)
    last, nxt = gate_ld(lambda ld: X.pt4_ld_ok(ld, esz), X.align_of(16, esz))
    assert last * esz == 1 << 22 and nxt * esz == (1 << 22) + 16
    M, N = X.GATE_C if which == "a" else X.GATE_C[::-1]
    for ld in (last, nxt):
        _gemm_far(far, form, "pt4", M, N, _k(din, 2), which, ld * esz)


def test_gate2_long_rows_stay_off_pt4(far):
    """What ``pt4_ok``'s 4 MiB stands for: pt4 addresses a 256-row panel as ``row * pitch`` plus the
    K-tile's offset ``kt * 128`` within the row, both in one 32-bit offset below 0x7FFFFFF0, so
    with rows of up to 4 MiB a panel ends at 1 GiB. One step of the pitch past the gate changes
    nothing visible (255 rows of 4 MiB + 16 are far from 2^31); rows of 8 MiB that K fills to
    their end are the first at which row 255's last K-tiles lie past the descriptor's range,
    where a buffer load returns zeros. tile="pt4" must hand this shape to t4: A and W are
    256 x 4194304 bf16 (2 GiB each, both in the backing: zeros but for the first and the last
    K-tile of every row, so the product stays exact), the one case here with a long K."""
    from ddlb_amd.ops.gemm import gemm

    M, N = X.GATE_KSPLIT
    pitch = 2 * X.PT4_LD_BYTES
    K, kt = pitch // 2, _k(BF16, 1)
    assert not X.pt4_ld_ok(K, 2) and (M - 1) * pitch + K * 2 > X.WT_LIMIT
    assert (M - 1) * X.PT4_LD_BYTES + X.PT4_LD_BYTES < X.WT_LIMIT      # the gate's own margin
    a, w, ref = _operands(M, N, 2 * kt, BF16, F32)
    backing = far.get()
    A = far_out(backing, M, K, BF16, pitch, fill=0.0)
    W = far_out(backing, N, K, BF16, pitch, row0=M, fill=None)
    for big, small in ((A, a), (W, w)):
        big[:, :kt] = small[:, :kt]
        big[:, K - kt:] = small[:, kt:]
    buf, C = sentinel_out(M, N, F32)
    gemm(A, W, C, tile="pt4")
    torch.cuda.synchronize()
    bad = (C != ref).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} wrong elements, the first at {bad[0].tolist()}"
    untouched(buf, M, N)


@pytest.mark.parametrize("form", [(BF16, F32, "auto"), (FP8, F32, "mx")], ids=_form_id)
def test_gate3_ksplit_partials(far, form):
    """The extension's ``gemm`` with ``ksplit=2`` and f32 partials ``j`` at ``c + j * M * ldc``:
    pt4's one launch (32-bit partial offsets) while both partials stay below 0x7FFFFFF0 bytes,
    the slice-by-slice loop from there on. Both partials exact, their sum the unsplit product,
    nothing written outside the two partial views."""
    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import MODES, TILES, dtype_code

    din, dout, mode = form
    (M, N), S, ks = X.GATE_KSPLIT, 2, _k(din, 4)
    a, w = far_operands(M, N, S * ks, din)
    want = [exact(a[:, j * ks:(j + 1) * ks], w[:, j * ks:(j + 1) * ks], dout).to(DEV)
            for j in range(S)]
    whole = exact(a, w, dout).to(DEV)
    A, W = padded(a.to(DEV)), padded(w.to(DEV))
    last, nxt = gate_ld(lambda ld: X.ksplit_one_launch(S, M, ld, 4), 2)
    backing = far.get()
    stream = torch.cuda.current_stream().cuda_stream
    for ldc in (last, nxt):
        assert X.ksplit_one_launch(S, M, ldc, 4) == (ldc == last)
        parts = [far_out(backing, M, N, dout, ldc * 4, row0=0),
                 far_out(backing, M, N, dout, ldc * 4, row0=M, fill=None)]
        assert parts[1].data_ptr() == parts[0].data_ptr() + M * ldc * 4
        load().gemm(A.data_ptr(), W.data_ptr(), parts[0].data_ptr(), A.stride(0), W.stride(0),
                    ldc, M, N, ks, dtype_code(din), dtype_code(dout), TILES["pt4"], MODES[mode],
                    0, 0, 0, 0, stream, 0, S)
        torch.cuda.synchronize()
        for j in range(S):
            assert torch.equal(parts[j], want[j]), (ldc, j)
        assert torch.equal(parts[0] + parts[1], whole)
        untouched_far(backing, *parts)


def _scale_bytes(rows, k, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    s = (127 + torch.randint(-2, 3, (rows, k // 32), generator=g)).to(torch.uint8)
    assert int(torch.unique(s, dim=0).shape[0]) == rows       # an aliased row changes the product
    return s


INT_CODE = (0, 2, 4, 5)  # E2M1 codes of |v| = 0, 1, 2, 3


def _scaled_case(fp4, M, N, K):
    """Integer operands in -3..3 as MX-fp8 or MXFP4 data with scale bytes 125..129 and the exact
    product of the dequantised operands (f32; exact: integers times 2^-4..2^4)."""
    a, w = far_operands(M, N, K, FP8)
    s_a, s_w = _scale_bytes(M, K, 41), _scale_bytes(N, K, 42)
    ref64 = exact_scaled(a, w, s_a, s_w)                    # (on the CPU, as in _operands)
    ref = ref64.to(F32)
    assert torch.equal(ref.double(), ref64)
    a, w, s_a, s_w, ref = (t.to(DEV) for t in (a, w, s_a, s_w, ref))
    if fp4:
        from ddlb_amd.ops.mx import pack_e2m1

        def pack(t):
            v = t.to(F32)
            code = torch.tensor(INT_CODE, device=DEV)[v.abs().long()]
            return pack_e2m1(code | ((v < 0).long() << 3))

        a, w = pack(a), pack(w)
    return a, w, s_a, s_w, ref


def _near_bytes(rows, cols, pad):
    """``(buf, view)``: a uint8 ``[rows, cols]`` view of a sentinel-filled buffer."""
    buf = torch.full((rows + 3, cols + pad), SENT_BYTE, dtype=torch.uint8, device=DEV)
    return buf, buf[:rows, :cols]


def _near_untouched(buf, rows, cols):
    mask = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
    mask[:rows, :cols] = False
    bad = int((buf[mask] != SENT_BYTE).sum())
    assert bad == 0, f"{bad} bytes outside the [{rows}, {cols}] view were written"


@pytest.mark.parametrize("tile", ["128x128", "256x128"])
@pytest.mark.parametrize("fp4", [False, True], ids=["mxfp8", "mxfp4"])
@pytest.mark.parametrize("which", ["a_scale", "w_scale"])
def test_gate4_operand_scales(far, tile, fp4, which):
    """``scale_operands_ok``: ``sa_off`` / ``sb_off`` are 32-bit, so a scale tensor's rows may
    span just under 2^31 bytes. On the largest aligned pitch the product is exact; on the next
    one ``gemm()`` and the native entry refuse (the backing would hold that launch too)."""
    from ddlb_amd.ops import gemm as G

    M, N = X.GATE_SCALED
    K = 512 if fp4 else 256
    al = 8 if fp4 else 4
    a, w, s_a, s_w, ref = _scaled_case(fp4, M, N, K)
    last, nxt = gate_ld(lambda ld: X.scale_rows_ok(M, ld), al)
    assert M * last < 2 ** 31 <= M * nxt
    backing = far.get()
    A, W = padded(a.view(torch.uint8)).view(a.dtype), padded(w.view(torch.uint8)).view(w.dtype)
    for ld in (last, nxt):
        sc = far_view(backing, s_a if which == "a_scale" else s_w, ld)
        kw = dict(a_scale=sc, w_scale=s_w) if which == "a_scale" else dict(a_scale=s_a, w_scale=sc)
        buf, C = sentinel_out(M, N, F32)
        if ld == last:
            G.gemm(A, W, C, tile=tile, **kw)
            torch.cuda.synchronize()
            assert torch.equal(C, ref)
        else:
            assert far_span(M, K // 32, ld) + FAR_GUARD <= backing.numel()
            with pytest.raises(ValueError, match="spans 2 GiB"):
                G.gemm(A, W, C, tile=tile, **kw)
            with pytest.raises(RuntimeError):
                G._launch(G.load(), A, W, C, M, N, K, tile, "mx",
                          torch.cuda.current_stream().cuda_stream, **kw)
            torch.cuda.synchronize()
        untouched(buf, M, N)


@pytest.mark.parametrize("tile", ["128x128", "256x128"])
@pytest.mark.parametrize("fp4", [False, True], ids=["mxfp8", "mxfp4"])
@pytest.mark.parametrize("fmt", ["mx", "mxfp4"])
def test_gate4_output_scales(far, tile, fp4, fmt):
    """The ``c_scale_ld`` check of the quantising epilogue: ``out_scale`` on the largest aligned
    pitch with ``M * pitch < 2^31`` is written byte for byte as the torch quantiser of the exact
    product writes it, and nothing else in the backing is; the next pitch is refused."""
    from ddlb_amd.ops import gemm as G
    from ddlb_amd.ops import mx

    M, N = X.GATE_SCALED
    K = 512 if fp4 else 256
    q4 = fmt == "mxfp4"
    al = 8 if q4 else 4
    a, w, s_a, s_w, ref = _scaled_case(fp4, M, N, K)
    q_ref, s_ref = (mx.quantize_mxfp4_reference if q4 else mx.quantize_mx_reference)(ref)
    ncol = N // 2 if q4 else N
    last, nxt = gate_ld(lambda ld: X.scale_rows_ok(M, ld), al)
    backing = far.get()
    qdt = G.out_quant_dtype(fmt)
    for ld in (last, nxt):
        out_scale = far_out(backing, M, N // 32, torch.uint8, ld)
        qbuf, q = _near_bytes(M, ncol, 32)
        kw = dict(a_scale=s_a, w_scale=s_w, out_scale=out_scale)
        if ld == last:
            G.gemm(a, w, q.view(qdt), tile=tile, out_quant=fmt, **kw)
            torch.cuda.synchronize()
            assert torch.equal(out_scale, s_ref)
            assert torch.equal(q, q_ref.view(torch.uint8))
        else:
            assert far_span(M, N // 32, ld) + FAR_GUARD <= backing.numel()
            with pytest.raises(ValueError, match="spans 2 GiB"):
                G.gemm(a, w, q.view(qdt), tile=tile, out_quant=fmt, **kw)
            with pytest.raises(RuntimeError):
                G._launch(G.load(), a, w, q.view(qdt), M, N, K, tile, "mx",
                          torch.cuda.current_stream().cuda_stream, **kw)
            torch.cuda.synchronize()
            out_scale = out_scale[:0]                                # nothing may be written
        untouched_far(backing, out_scale)
        _near_untouched(qbuf, M if ld == last else 0, ncol)


# ---------------------------------------------------------------------------- c. quantisers
def _wide(rows, k, seed, dtype):
    """randn * 2^U{-20..20}, one exponent per 32-element block (rows pairwise distinct)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(rows, k // 32, 32, generator=g)
    ex = torch.randint(-20, 21, (rows, k // 32, 1), generator=g)
    return torch.ldexp(x, ex).reshape(rows, k).to(dtype).to(DEV)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
@pytest.mark.parametrize("fp4", [False, True], ids=["mx", "mxfp4"])
@pytest.mark.parametrize("which", ["x", "q", "s"])
def test_row_quantiser_far(far, fp4, dtype, which):
    """``mx_quant_kernel`` through the native binding (it takes ``ldx``, ``ldq``, ``lds``):
    300 rows 16 MiB + 16 apart, so ``row * ldx * ESZ`` / ``row * ldq`` / ``row * lds`` pass 2^31
    and 2^32."""
    from ddlb_amd.ops import load, mx
    from ddlb_amd.ops.gemm import dtype_code

    R, K = 300, 256
    qcols = K // 2 if fp4 else K
    x = _wide(R, K, 50 + fp4, dtype)
    q_ref, s_ref = (mx.quantize_mxfp4_reference if fp4 else mx.quantize_mx_reference)(x)
    backing = far.get()
    X_ = far_view(backing, x, FAR_PITCH) if which == "x" else padded(x)
    qbuf, q = (None, far_out(backing, R, qcols, torch.uint8, FAR_PITCH)) if which == "q" \
        else _near_bytes(R, qcols, 24)
    sbuf, s = (None, far_out(backing, R, K // 32, torch.uint8, FAR_PITCH)) if which == "s" \
        else _near_bytes(R, K // 32, 9)
    (load().mxfp4_quantize if fp4 else load().mx_quantize)(
        X_.data_ptr(), q.data_ptr(), s.data_ptr(), X_.stride(0), q.stride(0), s.stride(0), R, K,
        dtype_code(dtype), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(s, s_ref), f"{int((s != s_ref).sum())} scale bytes differ"
    assert torch.equal(q, q_ref.view(torch.uint8))
    for buf, view, cols in ((qbuf, q, qcols), (sbuf, s, K // 32)):
        if buf is None:
            untouched_far(backing, view)
        else:
            _near_untouched(buf, R, cols)


def _wide_t(R, C, seed, dtype):
    """``[R, C]`` input whose exponent changes from one COLUMN block to the next."""
    return _wide(C, R, seed, dtype).t().contiguous()


def _t_ref(x, fmt):
    from ddlb_amd.ops.mx import quantize_mx_t_reference

    qt, st = quantize_mx_t_reference(x, fmt)
    return qt.view(torch.uint8), st


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
@pytest.mark.parametrize("fmt", ["mx", "mxfp4"])
@pytest.mark.parametrize("which", ["x", "qt", "st"])
def test_quantize_mx_t_under_the_2gib_refusal(far, fmt, dtype, which):
    """``quantize_mx_t`` through the Python API with ``x`` on the largest row stride
    ``_check_quant_t`` accepts (just under its 2 GiB refusal), then with each preallocated output
    on its largest accepted pitch; one stride further Python refuses."""
    from ddlb_amd.ops.mx import quantize_mx_t

    R, C = 256, 200
    fp4 = fmt == "mxfp4"
    esz = _esz(dtype)
    ncol, sal = (R // 2 if fp4 else R), (8 if fp4 else 4)
    qdt = torch.float4_e2m1fn_x2 if fp4 else FP8
    x = _wide_t(R, C, 60 + fp4, dtype)
    qt_ref, st_ref = _t_ref(x, fmt)
    backing = far.get()
    x_last, x_next = gate_ld(lambda ld: R * max(ld, C) * esz < 2 ** 31, X.align_of(16, esz))
    q_last, q_next = gate_ld(lambda ld: C * ld < 2 ** 31, 16)
    s_last, s_next = gate_ld(lambda ld: C * ld < 2 ** 31, sal)
    if which == "x":
        qt, st = quantize_mx_t(far_view(backing, x, x_last * esz), fmt=fmt)
        torch.cuda.synchronize()
        assert torch.equal(qt.view(torch.uint8), qt_ref) and torch.equal(st, st_ref)
        with pytest.raises(ValueError, match="spans 2 GiB"):
            quantize_mx_t(far_view(backing, x, x_next * esz), fmt=fmt)
        return
    for ld in ((q_last, q_next) if which == "qt" else (s_last, s_next)):
        if which == "qt":
            qt = far_out(backing, C, ncol, torch.uint8, ld)
            sbuf, st = _near_bytes(C, R // 32, 8)
        else:
            st = far_out(backing, C, R // 32, torch.uint8, ld)
            qbuf, qt = _near_bytes(C, ncol, 32)
        if ld == (q_next if which == "qt" else s_next):
            with pytest.raises(ValueError, match="spans 2 GiB"):
                quantize_mx_t(padded(x), fmt=fmt, out=(qt.view(qdt), st))
            continue
        quantize_mx_t(padded(x), fmt=fmt, out=(qt.view(qdt), st))
        torch.cuda.synchronize()
        assert torch.equal(qt, qt_ref) and torch.equal(st, st_ref)
        if which == "qt":
            untouched_far(backing, qt)
            _near_untouched(sbuf, C, R // 32)
        else:
            untouched_far(backing, st)
            _near_untouched(qbuf, C, ncol)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
@pytest.mark.parametrize("fmt", ["mx", "mxfp4"])
def test_quantize_mx_2way_under_the_2gib_refusal(far, fmt, dtype):
    """``quantize_mx_2way`` (it allocates its outputs; C = 256: both dimensions are a K) with
    ``x`` on the largest accepted row stride."""
    from ddlb_amd.ops import mx

    R, C = 256, 256
    esz = _esz(dtype)
    x = _wide(R, C, 70, dtype)
    last, nxt = gate_ld(lambda ld: R * max(ld, C) * esz < 2 ** 31, X.align_of(16, esz))
    backing = far.get()
    q, s, qt, st = mx.quantize_mx_2way(far_view(backing, x, last * esz), fmt=fmt)
    torch.cuda.synchronize()
    q_ref, s_ref = (mx.quantize_mxfp4_reference if fmt == "mxfp4" else mx.quantize_mx_reference)(x)
    qt_ref, st_ref = _t_ref(x, fmt)
    assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8)) and torch.equal(s, s_ref)
    assert torch.equal(qt.view(torch.uint8), qt_ref) and torch.equal(st, st_ref)
    with pytest.raises(ValueError, match="spans 2 GiB"):
        mx.quantize_mx_2way(far_view(backing, x, nxt * esz), fmt=fmt)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=_name)
@pytest.mark.parametrize("fmt", ["mx", "mxfp4"])
@pytest.mark.parametrize("which", ["x", "qt", "st"])
def test_transposing_quantiser_native_past_4gib(far, fmt, dtype, which):
    """``mx_quant_t_kernel`` through the native binding, which (unlike Python) does not refuse
    large spans: ``(r0 + r) * ldx``, ``col * ldqt`` and ``col * ldst`` pass 2^32 for the last
    rows of ``x`` and the last columns' rows of ``qt`` / ``st``. The kernel's arithmetic is
    64-bit; Python's stricter 2 GiB rule stays as it is (docs/ARCHITECTURE.md)."""
    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import dtype_code

    R, C = 256, 200
    fp4 = fmt == "mxfp4"
    esz = _esz(dtype)
    ncol = R // 2 if fp4 else R
    x = _wide_t(R, C, 80 + fp4, dtype)
    qt_ref, st_ref = _t_ref(x, fmt)
    assert (R - 1) * T_PITCH_X > 2 ** 32 and (C - 1) * T_PITCH_OUT > 2 ** 32
    backing = far.get()
    X_ = far_view(backing, x, T_PITCH_X) if which == "x" else padded(x)
    qbuf, qt = (None, far_out(backing, C, ncol, torch.uint8, T_PITCH_OUT)) if which == "qt" \
        else _near_bytes(C, ncol, 32)
    sbuf, st = (None, far_out(backing, C, R // 32, torch.uint8, T_PITCH_OUT)) if which == "st" \
        else _near_bytes(C, R // 32, 8)
    load().mx_quantize_t(X_.data_ptr(), qt.data_ptr(), st.data_ptr(), X_.stride(0), qt.stride(0),
                         st.stride(0), R, C, dtype_code(dtype), fp4,
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(st, st_ref), f"{int((st != st_ref).sum())} scale bytes differ"
    assert torch.equal(qt, qt_ref)
    for buf, view, cols in ((qbuf, qt, ncol), (sbuf, st, R // 32)):
        if buf is None:
            untouched_far(backing, view)
        else:
            _near_untouched(buf, C, cols)


# ---------------------------------------------------------------------------- d. copy, reduce
def _periodic(period, repeats, dtype, offset=0):
    """``(i % period) + offset`` for ``i < period * repeats``: a piece that starts at any
    multiple of its length continues the pattern."""
    return (torch.arange(period, device=DEV).repeat(repeats) + offset).to(dtype)


def test_copy_past_4gib(far):
    """``copy_kernel`` (``v * 16``): 2^32 + 16 + 5 bytes, a vector body that passes 2^32 and a
    byte tail, into a destination framed by sentinel bytes. Byte ``i`` holds ``i % 251``:
    2^31 = 187 and 2^32 = 123 (mod 251), so a byte copied from or to 2^31 or 2^32 away differs."""
    from ddlb_amd.ops import load

    far.release()
    n, frame, period = 2 ** 32 + 16 + 5, 4096, 251
    assert 2 ** 31 % period == 187 and 2 ** 32 % period == 123
    _need(2 * n + 2 * frame, "the copy test")
    piece = _periodic(period, 1 << 18, torch.uint8)
    L = piece.numel()
    src = torch.empty(n, dtype=torch.uint8, device=DEV)
    for i in range(0, n, L):
        m = min(L, n - i)
        src[i:i + m] = piece[:m]
    dst = torch.full((n + 2 * frame,), SENT_BYTE, dtype=torch.uint8, device=DEV)
    load().copy(dst.data_ptr() + frame, src.data_ptr(), n, 0,
                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    body = dst[frame:frame + n]
    bad = [torch.count_nonzero(body[i:i + L] != piece[:min(L, n - i)]) for i in range(0, n, L)]
    bad = torch.stack(bad).cpu()
    assert int(bad.sum()) == 0, f"{int(bad.sum())} bytes differ, first piece {int(bad.nonzero()[0])}"
    assert bool((dst[:frame] == SENT_BYTE).all()) and bool((dst[frame + n:] == SENT_BYTE).all())
    del src, dst, body
    _free_gpu_memory()


def test_reduce_sum_past_2g_elements(far):
    """``reduce_sum`` on ``2^31 + 13`` bf16 elements (byte offsets past 2^32, element indices
    past 2^31), the same buffer as both sources: the result is ``2 x``. Element ``i`` holds
    ``i % 7 - 3``: 2^30 = 1 and 2^31 = 2 (mod 7), so the value at ``i`` differs from the values
    at ``i +- 2^30`` and ``i +- 2^31`` (an index that loses bit 30 or 31 reads another number).
    The NaN-filled elements after ``count`` stay NaN."""
    from ddlb_amd.ops import load
    from ddlb_amd.ops.gemm import DT_BF16

    far.release()
    count, period = 2 ** 31 + 13, 7
    assert 2 ** 30 % period == 1 and 2 ** 31 % period == 2
    pad = (count + 7) // 8 * 8 + 8
    _need(4 * pad, "the reduce test")
    piece = _periodic(period, 1 << 21, BF16, offset=-3)
    L = piece.numel()
    src = torch.empty(pad, dtype=BF16, device=DEV)
    for i in range(0, pad, L):
        m = min(L, pad - i)
        src[i:i + m] = piece[:m]
    out = torch.empty(pad, dtype=BF16, device=DEV)
    out.view(torch.int16).fill_(0x7FC0)                               # NaN, in place
    load().reduce_sum(out.data_ptr(), [src.data_ptr(), src.data_ptr()], count, DT_BF16,
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = piece * 2
    bad = [torch.count_nonzero(out[i:i + min(L, count - i)] != want[:min(L, count - i)])
           for i in range(0, count, L)]
    bad = torch.stack(bad).cpu()
    assert int(bad.sum()) == 0, f"{int(bad.sum())} sums differ, first piece {int(bad.nonzero()[0])}"
    assert bool(torch.isnan(out[count:].float()).all()) and out[count:].numel() >= 8
    del src, out
    _free_gpu_memory()


# ---------------------------------------------------------------------------- the budget
def test_peak_memory_stays_under_10_gib(far):
    """The module's peak of ``torch.cuda.max_memory_allocated()``, counted from the module's
    first test (the statistics are reset there) and above what earlier modules still held."""
    peak = torch.cuda.max_memory_allocated()
    print(f"far-offset module: peak {peak} bytes, {far.base} held before it, backing "
          f"{FAR_GUARD + BACKING_BYTES}")
    assert FAR_GUARD + BACKING_BYTES < PEAK_LIMIT
    assert peak - far.base < PEAK_LIMIT, (peak, far.base)
