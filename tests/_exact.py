"""Shared helpers of the exact-arithmetic tests (a plain module: no fixtures, no test).

The operands are integers in -3..3, exact in bf16, f16, f32, f64 and e4m3. With K <= 1024 every
product and every partial sum of ``a @ w.T`` is an integer below 2^24, so an f32 accumulator holds
it exactly whatever the order of the additions: the specification of a GEMM on such operands is
"the exact product, rounded once to the output dtype", and it is compared with ``torch.equal``.

Operands come as views of larger buffers whose padding holds ``POISON`` (a read outside the view
changes the result) and outputs as views of buffers filled with ``SENTINEL`` (a write outside the
view is seen by :func:`untouched`).

The far-offset tests (``tests/test_far_offsets_gpu.py``) place one matrix of a case in a *far*
view: rows megabytes apart behind a 2 GiB front guard (:func:`far_backing`, :func:`far_view`,
:func:`far_out`, :func:`untouched_far`), on leading dimensions that :func:`gate_ld` takes from the
Python copies of the host-side gates below, never from literals."""

import math

import torch

POISON = 5.0
SENTINEL = -7.0
FP8 = torch.float8_e4m3fn
BLOCK = 32


def _filled(shape, value, dtype, device):
    # (torch.full has no e4m3 fill; every value used here is exact in every dtype)
    return torch.full(shape, float(value), dtype=torch.float32, device=device).to(dtype)


def ints(shape, dtype, gen):
    """Integers in -3..3 as ``dtype``, drawn from ``gen`` on its device."""
    x = torch.randint(-3, 4, shape, generator=gen, device=gen.device)
    return x.to(torch.float32).to(dtype)


def padded(x, pad_elems=None, extra_rows=3, poison=POISON, align=16):
    """``x [R, C]`` as the view ``[:R, :C]`` of a ``[R + extra_rows, C + pad_elems]`` buffer
    whose other elements hold ``poison``. The rows stay ``align``-byte aligned: ``pad_elems``
    must keep them so (default: the smallest padding of at least 4 elements that does)."""
    R, C = x.shape
    esz = x.element_size()
    if pad_elems is None:
        pad_elems = next(p for p in range(4, 4 + align + 1) if ((C + p) * esz) % align == 0)
    assert pad_elems > 0 and ((C + pad_elems) * esz) % align == 0, "rows must stay aligned"
    buf = _filled((R + extra_rows, C + pad_elems), poison, x.dtype, x.device)
    buf[:R, :C] = x
    view = buf[:R, :C]
    assert view.data_ptr() % align == 0 and (view.stride(0) * esz) % align == 0
    return view


def sentinel_out(M, N, dtype, pad_cols=4, extra_rows=3, device="cuda"):
    """``(buf, view)``: ``buf [M + extra_rows, N + pad_cols]`` filled with ``SENTINEL`` and
    ``view = buf[:M, :N]``."""
    buf = _filled((M + extra_rows, N + pad_cols), SENTINEL, dtype, device)
    return buf, buf[:M, :N]


def untouched(buf, M, N, rows=None):
    """Assert that every element of ``buf`` outside ``[:M, :N]`` (outside rows ``rows`` and
    columns ``:N`` when the physical rows written are given) still holds ``SENTINEL``."""
    written = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    if rows is None:
        written[:M, :N] = True
    else:
        written[rows, :N] = True
    outside = buf.to(torch.float32)[~written]
    bad = int((outside != SENTINEL).sum())
    assert bad == 0, f"{bad} elements outside the [{M}, {N}] view were written"


def pow2_f64(e):
    """``2^e`` as float64 for an integer tensor ``e`` in [-1022, 1023], built from its bit
    pattern (the fp64 twin of ``ddlb_amd.ops.mx.ldexp_exact``)."""
    return ((e.to(torch.int64) + 1023) << 52).view(torch.float64)


def exact64(a, w):
    """``a @ w.T`` in fp64 (exact for the operands above)."""
    return a.to(torch.float32).double() @ w.to(torch.float32).double().t()


def exact(a, w, out_dtype):
    """The exact product rounded once to f32 (no rounding at all for the operands above with
    K <= 1024) and then to ``out_dtype``."""
    return exact64(a, w).to(torch.float32).to(out_dtype)


def dequant64(q, s):
    """e4m3 ``q [R, K]`` with E8M0 bytes ``s [R, K / 32]`` as float64, never through fp32
    (``3 * 2^127`` is no fp32 number; every such value is an exact fp64 one)."""
    R, K = q.shape
    assert tuple(s.shape) == (R, K // BLOCK)
    v = q.to(torch.float32).double().reshape(R, K // BLOCK, BLOCK)
    return (v * pow2_f64(s.to(torch.int64) - 127).unsqueeze(2)).reshape(R, K)


def exact_scaled(a8, w8, s_a, s_w):
    """The product of the dequantised MX operands, in fp64."""
    return dequant64(a8, s_a) @ dequant64(w8, s_w).t()


def extreme_scales(M, N, K, gen):
    """Scale bytes over the whole E8M0 range the quantiser can emit (0..254) whose products stay
    small: ``s_a = 127 + D[b] + u[r, b]`` and ``s_w = 127 - D[b] + v[n, b]`` with ``D`` spread over
    -125..125 along the K blocks (both ends present) and ``u``, ``v`` in -2..2, so every block's
    net exponent ``u + v`` lies in -4..4 while the bytes themselves reach 0 and 254. Returns
    ``(s_a, s_w, e_a, e_w)``: the uint8 bytes and the int64 exponents ``s - 127``."""
    nb = K // BLOCK
    dev = gen.device
    D = torch.round(torch.linspace(-125, 125, nb, device=dev, dtype=torch.float64)).to(torch.int64)
    u = torch.randint(-2, 3, (M, nb), generator=gen, device=dev)
    v = torch.randint(-2, 3, (N, nb), generator=gen, device=dev)
    e_a = (D.unsqueeze(0) + u).clamp(-127, 127)
    e_w = (-D.unsqueeze(0) + v).clamp(-127, 127)
    return (e_a + 127).to(torch.uint8), (e_w + 127).to(torch.uint8), e_a, e_w


# ---------------------------------------------------------------------------- non-finite values
# The padding of an operand as a caching allocator can leave it: a value that a kernel which loads
# it and multiplies it by a masked zero turns into NaN (POISON x 0 is 0). NaN for the float
# dtypes; the e4m3 NaN byte; 6.0 pairs for packed fp4 data (E2M1 has no NaN); the NaN scale byte.
NONFINITE_POISON = {torch.bfloat16: float("nan"), torch.float16: float("nan"),
                    torch.float32: float("nan"), torch.float64: float("nan"),
                    FP8: 0x7F, "fp4": 0x77, "scale": 255}


def nan_padded(x, kind=None, **kw):
    """:func:`padded` with ``NONFINITE_POISON`` around the view. ``kind`` names the entry for byte
    arrays (``"fp4"``, ``"scale"``); e4m3 and the byte arrays are filled as bytes."""
    key = kind if kind is not None else x.dtype
    fill = NONFINITE_POISON[key]
    if isinstance(fill, float):
        return padded(x, poison=fill, **kw)
    raw = x.view(torch.uint8)
    return padded(raw, poison=fill, **kw).view(x.dtype)


def planted(a, w):
    """Copies of the integer operands ``a [M, K]``, ``w [N, K]`` (M >= 8, N >= 6, K >= 8) with
    non-finite values planted, each plant in a row or column of its own, and the places as a dict:
    NaN in ``A[r0, 0]`` (first row tile, first K-tile), +Inf in ``A[r1 = M - 1, K - 1]`` (ragged
    last row tile, last K-tile), +Inf and -Inf in two columns of ``A[r2]``, NaN in
    ``W[n0, K // 2]``, -Inf in ``W[n1 = N - 1, 0]`` (the scalar column tail). The partner column
    of every Inf is made to hold a negative, a zero and a positive value, so the output row (or
    column) of that Inf holds -Inf, NaN and +Inf. fp8 operands (no Inf in e4m3fn) take only the
    NaN bytes: 0x7F in A, 0xFF in W."""
    M, K = a.shape
    N = w.shape[0]
    assert M >= 8 and N >= 6 and K >= 8
    a, w = a.clone(), w.clone()
    p = dict(r0=1, r1=M - 1, r2=M // 2, n0=2, n1=N - 1, k2p=3, k2m=K - 2)
    if a.dtype == FP8:
        a.view(torch.uint8)[p["r0"], 0] = 0x7F
        w.view(torch.uint8)[p["n0"], K // 2] = 0xFF
        return a, w, p
    inf, nan = float("inf"), float("nan")
    # the partner columns: W[:, K-1], W[:, k2p], W[:, k2m] (rows n0, n1 keep their own plants'
    # columns K // 2 and 0 untouched) and A[:, 0]
    for col in (K - 1, p["k2p"], p["k2m"]):
        w[0, col], w[1, col], w[3, col] = -1.0, 0.0, 2.0
    a[0, 0], a[2, 0], a[3, 0] = -2.0, 0.0, 1.0
    a[p["r0"], 0] = nan
    a[p["r1"], K - 1] = inf
    a[p["r2"], p["k2p"]] = inf
    a[p["r2"], p["k2m"]] = -inf
    w[p["n0"], K // 2] = nan
    w[p["n1"], 0] = -inf
    for col in (K - 1, p["k2p"], p["k2m"]):
        c = w[:, col].float()
        assert bool((c < 0).any()) and bool((c == 0).any()) and bool((c > 0).any())
    c = a[:, 0].float()
    assert bool((c < 0).any()) and bool((c == 0).any()) and bool((c > 0).any())
    return a, w, p


def classes64(a, w):
    """The class rule of ``a @ w.T`` as a plain function, fp64 ``[M, N]``: an element is NaN when
    any product of its dot is NaN (a NaN operand, Inf x 0, or +Inf and -Inf products both
    present), otherwise +-Inf when an infinite product is present, otherwise the exact sum of the
    finite products. Nothing here multiplies or adds a non-finite number: the classes come from
    masks and counts, the sum from the operands' finite parts."""
    A, W = a.to(torch.float32).double(), w.to(torch.float32).double()
    fin_a, fin_w = torch.isfinite(A), torch.isfinite(W)
    Af, Wf = torch.where(fin_a, A, 0.0), torch.where(fin_w, W, 0.0)
    total = Af @ Wf.t()                                   # every non-finite element counted as 0

    def cnt(x, y):                                        # pairs k with x[m, k] and y[n, k]
        return x.double() @ y.double().t()

    nan_a, nan_w = torch.isnan(A), torch.isnan(W)
    inf_a, inf_w = torch.isinf(A), torch.isinf(W)
    ones_a, ones_w = torch.ones_like(fin_a), torch.ones_like(fin_w)
    is_nan = cnt(nan_a, ones_w) + cnt(ones_a, nan_w) > 0                  # a NaN operand
    is_nan |= cnt(inf_a, fin_w & (W == 0)) + cnt(fin_a & (A == 0), inf_w) > 0   # Inf x 0
    # the sign of an infinite product: sign(inf operand) x sign(partner), partner non-zero
    pos_a, neg_a, pos_w, neg_w = A > 0, A < 0, W > 0, W < 0           # (NaN is neither)
    infp_a, infm_a = inf_a & pos_a, inf_a & neg_a
    infp_w, infm_w = inf_w & pos_w, inf_w & neg_w
    # an infinite product needs an infinite operand on at least one side
    n_pos = (cnt(infp_a, pos_w) + cnt(infm_a, neg_w)
             + cnt(pos_a & fin_a, infp_w) + cnt(neg_a & fin_a, infm_w))
    n_neg = (cnt(infp_a, neg_w) + cnt(infm_a, pos_w)
             + cnt(pos_a & fin_a, infm_w) + cnt(neg_a & fin_a, infp_w))
    is_nan |= (n_pos > 0) & (n_neg > 0)
    out = total.clone()
    out[n_pos > 0] = float("inf")
    out[n_neg > 0] = float("-inf")
    out[is_nan] = float("nan")
    return out


def same(got, want):
    """Equal by class, then by value: the NaN masks are equal, and with every NaN set to 0 the
    tensors are ``torch.equal`` (infinities compare by value and sign)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape)
    gn, wn = torch.isnan(got), torch.isnan(want)
    bad = (gn != wn).nonzero()
    assert bad.numel() == 0, f"NaN masks differ at {bad[:8].tolist()} ({bad.shape[0]} places)"
    g0 = torch.nan_to_num(got.double(), nan=0.0, posinf=float("inf"), neginf=float("-inf"))
    w0 = torch.nan_to_num(want.double(), nan=0.0, posinf=float("inf"), neginf=float("-inf"))
    bad = (g0 != w0).nonzero()
    assert bad.numel() == 0, f"values differ at {bad[:8].tolist()} ({bad.shape[0]} places)"


# ---------------------------------------------------------------------------- far views
FAR_GUARD = 2 ** 31
SCAN_CHUNK = 256 << 20    # bytes per scanned piece
_WORD = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _is_raw(dtype):
    return dtype == torch.uint8 or dtype == getattr(torch, "float4_e2m1fn_x2", None)


def fill_word(value, dtype):
    """The 8-byte word (as a signed int64 value) that a buffer full of ``value`` in ``dtype``
    consists of. Byte dtypes (uint8, packed fp4) take ``value & 0xFF``: POISON is byte 5,
    SENTINEL byte 249."""
    if _is_raw(dtype):
        raw = bytes([int(value) & 0xFF])
    else:
        one = torch.tensor([float(value)], dtype=torch.float32).to(dtype)
        raw = bytes(one.view(torch.uint8).tolist())
    return int.from_bytes(raw * (8 // len(raw)), "little", signed=True)


def far_backing(nbytes, guard=FAR_GUARD, device="cuda"):
    """One ``uint8`` allocation of ``guard + nbytes`` (rounded up to 16): far views start at byte
    ``guard``, 16-byte aligned; ``backing.guard`` remembers it.

    Why the guard lies in FRONT of the views: a byte offset truncated to 32 bits lands LOWER in
    the view, and an offset sign-extended from 32 bits lands up to 2 GiB BEFORE the view's base.
    With the default guard of 2^31 bytes both stay inside this one allocation, so a wrong offset
    shows as a wrong value or a written sentinel, never as a GPU fault."""
    assert guard % 16 == 0 and nbytes > 0
    backing = torch.empty(guard + (nbytes + 15) // 16 * 16, dtype=torch.uint8, device=device)
    assert backing.data_ptr() % 16 == 0
    backing.guard = guard
    return backing


def far_span(R, row_bytes, ld_bytes, row0=0):
    """Bytes from the backing's byte ``guard`` to the end of the last row of such a view."""
    return (row0 + R - 1) * ld_bytes + row_bytes


def far_fill(backing, value, dtype):
    """The whole backing holds ``value`` in ``dtype`` (in place: no temporary)."""
    backing.view(torch.int64).fill_(fill_word(value, dtype))


def _far_strided(backing, R, C, dtype, ld_bytes, row0):
    esz = 1 if _is_raw(dtype) else torch.empty((), dtype=dtype).element_size()
    assert ld_bytes % esz == 0 and ld_bytes >= C * esz, "rows must not overlap"
    start = backing.guard + row0 * ld_bytes
    assert start % 16 == 0, "far views are 16-byte aligned"
    assert backing.guard + far_span(R, C * esz, ld_bytes, row0) <= backing.numel(), \
        f"the backing of {backing.numel()} bytes is too small for {R} rows {ld_bytes} apart"
    typed = backing if _is_raw(dtype) else backing.view(dtype)
    view = torch.as_strided(typed, (R, C), (ld_bytes // esz, 1), start // esz)
    assert view.data_ptr() == backing.data_ptr() + start
    return view


def far_view(backing, x, ld_bytes, row0=0, fill=POISON):
    """``x [R, C]`` as an ``as_strided`` view of ``backing`` whose rows lie ``ld_bytes`` apart,
    row 0 at byte ``guard + row0 * ld_bytes``. Before ``x`` is written the WHOLE backing is set to
    ``fill`` in ``x``'s dtype (``POISON``: an operand; ``None``: the backing is left as it is,
    for a second view of one case)."""
    R, C = x.shape
    view = _far_strided(backing, R, C, x.dtype, ld_bytes, row0)
    if fill is not None:
        far_fill(backing, fill, x.dtype)
    view.copy_(x)
    return view


def far_out(backing, R, C, dtype, ld_bytes, row0=0, fill=SENTINEL):
    """An output view like :func:`far_view`'s, the whole backing (the view included) holding
    ``SENTINEL`` in ``dtype``."""
    view = _far_strided(backing, R, C, dtype, ld_bytes, row0)
    if fill is not None:
        far_fill(backing, fill, dtype)
    return view


def untouched_far(backing, *views, rows=None):
    """Assert that every byte of ``backing`` outside the ``[R, C]`` elements of ``views`` (all of
    one dtype; of their rows ``rows`` when given) still holds ``SENTINEL``. The views' contents
    are set aside, the views are set to the sentinel, the backing is scanned as raw 64-bit words
    in pieces of ``SCAN_CHUNK`` bytes (no float or bool copy of any of it), and the
    contents are put back."""
    dtype = views[0].dtype
    assert all(v.dtype == dtype for v in views)
    word = fill_word(SENTINEL, dtype)
    words = backing.view(torch.int64)
    step = SCAN_CHUNK // 8
    assert SCAN_CHUNK <= 256 << 20
    sel = slice(None) if rows is None else rows
    raw = [v if _is_raw(dtype) else v.view(_WORD[v.element_size()]) for v in views]
    kept = [r[sel].clone() for r in raw]
    unit = torch.tensor([word], dtype=torch.int64).view(raw[0].dtype)[0].item()
    for r in raw:
        r[sel] = unit
    # min and max of a piece are reductions with no temporary: every word equals the sentinel
    # word exactly when both do
    ends = torch.stack([torch.stack(torch.aminmax(words[i:i + step]))
                        for i in range(0, words.numel(), step)]).cpu()
    hit = ((ends != word).any(dim=1)).nonzero().flatten().tolist()
    report = None
    if hit:
        i = hit[0] * step
        j = i + int((words[i:i + step] != word).nonzero()[0])
        report = (f"8-byte words outside the view were written in {len(hit)} of {ends.shape[0]} "
                  f"pieces, the first at byte {8 * j - backing.guard:+d} from the view's base")
    for r, k in zip(raw, kept):
        r[sel] = k
    assert report is None, report


def rows_distinct(x, ld_bytes, row0=0):
    """Assert what makes an aliased operand read change the product: the rows of ``x`` are
    pairwise distinct, and the bytes 2^31 and 2^32 before and behind a row's start are either
    the start of another row or padding (which holds POISON), never the inside of a row."""
    R, C = x.shape
    row_bytes = C * x.element_size()
    assert int(torch.unique(x.to(torch.float32), dim=0).shape[0]) == R, "two rows are equal"
    for r in range(R):
        for d in (-2 ** 32, -2 ** 31, 2 ** 31, 2 ** 32):
            o = (row0 + r) * ld_bytes + d
            if o >= 0 and o // ld_bytes - row0 < R:
                assert o % ld_bytes == 0 or o % ld_bytes >= row_bytes, (r, d)


FAR_PITCH = (16 << 20) + 16   # rows from 128 on lie past 2^31, rows from 256 on past 2^32
FAR_SEED = 20
# the shapes of tests/test_far_offsets_gpu.py (M, N; W far swaps them): ragged tiled / generic,
# whole-tile ping-pong, pt4 with a fifth row panel, the gates, the K-split, the scaled GEMMs
FAR_TILED, FAR_PING, FAR_PT4, FAR_GROUPED = (300, 202), (512, 256), (1280, 256), (768, 256)
GATE_C, GATE_KSPLIT, GATE_SCALED = (512, 256), (256, 256), (256, 256)


def far_operands(M, N, K, dtype, seed=FAR_SEED):
    """``a [M, K]``, ``w [N, K]`` of the far-offset tests, drawn on the CPU with a fixed seed (the
    CPU test of their rows and the GPU tests see the same numbers)."""
    g = torch.Generator(device="cpu").manual_seed(seed + 1000003 * M + 1009 * N + K)
    return ints((M, K), dtype, g), ints((N, K), dtype, g)


# ---------------------------------------------------------------------------- the gates
WT_LIMIT = 0x7FFFFFF0     # the record count of the kernels' 32-bit buffer descriptors
PT4_LD_BYTES = 1 << 22    # pt4_ok(): the largest operand row pitch pt4 takes


def c_fits_wt(M, N, ldc, osz, c_grp=0, c_gstride=0):
    """Gate 1, ``c_fits_wt()`` of csrc/gemm/gemm_kernels.h without a C row table: pt4 / t4 store
    C through 32-bit buffer offsets when every C byte lies below ``WT_LIMIT``."""
    if M <= 0:
        return False
    cg = c_grp if c_grp > 0 else M
    cgs = c_gstride if c_gstride > 0 else cg
    last_row = (M - 1) // cg * cgs + (M - 1) % cg
    return (last_row * ldc + N) * osz < WT_LIMIT


def pt4_ld_ok(ld, esz):
    """Gate 2, the pitch clause of ``pt4_ok()``."""
    return ld * esz <= PT4_LD_BYTES


def ksplit_one_launch(S, M, ldc, osz):
    """Gate 3, ``launch_pt4()``: pt4 runs the (slice, tile) pairs of a K-split in one launch when
    the ``S`` partials together stay below ``WT_LIMIT``; at and above, ``gemm_launch`` runs the
    slices one after another."""
    return S * M * ldc * osz < WT_LIMIT


def scale_rows_ok(rows, scale_ld):
    """Gate 4, ``scale_operands_ok()`` / the ``c_scale_ld`` check of csrc/gemm/gemm_mfma.hip and
    their Python twins: the scale rows are addressed by 32-bit byte offsets."""
    return rows * scale_ld < 2 ** 31


def gate_ld(pred, align, hi=2 ** 40):
    """``(last, next)``: the largest multiple of ``align`` for which the monotone predicate
    ``pred(ld)`` holds, and the next multiple, for which it does not."""
    assert pred(align) and not pred(hi // align * align)
    lo, up = 1, hi // align                 # pred(lo * align), not pred(up * align)
    while up - lo > 1:
        mid = (lo + up) // 2
        lo, up = (mid, up) if pred(mid * align) else (lo, mid)
    assert pred(lo * align) and not pred(up * align) and up == lo + 1
    return lo * align, up * align


def align_of(nbytes, esz):
    """Elements per ``nbytes`` bytes (the leading-dimension step that keeps rows so aligned)."""
    return nbytes // math.gcd(nbytes, esz)
