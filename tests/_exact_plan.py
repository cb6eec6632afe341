"""Helpers of the exact-arithmetic tests of the GEMM's plan-level arguments (a plain module: no
fixtures, no test), on top of ``tests/_exact.py``.

A ``Plan`` addresses byte buffers, so every matrix here is *placed*: :func:`place` declares a plan
buffer of ``guard + rows + extra`` rows that lie ``ld > cols`` elements apart and returns a
:class:`Mat` whose ``ref`` is the matrix's first element. Operands are written with ``POISON`` in
every other element of their buffer (:func:`put_operand`), outputs are filled with ``SENTINEL``
(:func:`put_sentinel`) and checked with :func:`check_untouched`, which takes the regions that were
supposed to be written and asserts that nothing else was. :func:`block_layout` scatters the row
blocks of a matrix over two buffers in a permuted order with poison rows between them (the
address table of ``a_shards``); :func:`gather` is its inverse and the CPU-side specification.

All operands are ``ints()`` in -3..3: with ``9 * K_total < 2^24`` (:func:`assert_exact`) every
partial sum is an exact f32 whatever the order of the additions."""

import contextlib
from dataclasses import dataclass
from typing import Tuple

import torch

from _exact import POISON, SENTINEL, _filled, exact, ints

EXTRA_ROWS = 3
KSPLIT_SEED = 7


def assert_exact(k_total):
    """The exactness condition of integer operands in -3..3: every partial sum below 2^24."""
    assert 9 * k_total < 2 ** 24, f"K = {k_total}: a partial sum can leave f32's integers"


def esize(dtype):
    return torch.empty((), dtype=dtype).element_size()


def plan_dt(dtype):
    """The plan's dtype code of a torch dtype."""
    from ddlb_amd.parallel import plan as P

    return {torch.float32: P.DT_F32, torch.float16: P.DT_F16, torch.bfloat16: P.DT_BF16,
            torch.float8_e4m3fn: P.DT_FP8}[dtype]


def padded_ld(cols, dtype, align=16):
    """The smallest leading dimension of at least ``cols + 4`` elements whose rows stay
    ``align``-byte aligned (operands: 16, outputs: 8)."""
    esz = esize(dtype)
    return next(ld for ld in range(cols + 4, cols + 5 + align) if (ld * esz) % align == 0)


@dataclass(frozen=True)
class Mat:
    """A ``[rows, cols]`` matrix inside the plan buffer ``name``: ``guard`` rows in front,
    ``extra`` rows behind, rows ``ld`` elements apart; ``ref`` addresses element (0, 0)."""
    name: str
    ref: object
    rows: int
    cols: int
    ld: int
    dtype: torch.dtype
    guard: int
    extra: int

    @property
    def total_rows(self):
        return self.guard + self.rows + self.extra

    @property
    def row_bytes(self):
        return self.ld * esize(self.dtype)

    def row_ref(self, row):
        """Reference to the first element of row ``row`` of the matrix."""
        return self.ref + row * self.row_bytes


def place(plan, name, rows, cols, dtype, *, align=16, ld=None, guard=0, extra=EXTRA_ROWS):
    """Declare the plan buffer of a padded matrix (operands ``align=16``, outputs ``align=8``)."""
    ld = padded_ld(cols, dtype, align) if ld is None else ld
    esz = esize(dtype)
    assert ld > cols and (ld * esz) % align == 0, "rows must be padded and stay aligned"
    base = plan.buffer(name, (guard + rows + extra) * ld * esz)
    return Mat(name, base + guard * ld * esz, rows, cols, ld, dtype, guard, extra)


def whole(bound, mat):
    """The whole buffer of ``mat`` as a ``[guard + rows + extra, ld]`` tensor."""
    n = mat.total_rows * mat.row_bytes
    return bound.buffer(mat.name)[:n].view(mat.dtype).view(mat.total_rows, mat.ld)


def view(bound, mat):
    """The matrix itself: ``[rows, cols]``."""
    return whole(bound, mat)[mat.guard:mat.guard + mat.rows, :mat.cols]


def put_operand(bound, mat, x=None):
    """``POISON`` in every element of the buffer, then ``x`` in the matrix (``None``: poison
    everywhere, for a buffer filled block by block)."""
    w = whole(bound, mat)
    w.copy_(_filled(tuple(w.shape), POISON, mat.dtype, w.device))
    if x is not None:
        assert tuple(x.shape) == (mat.rows, mat.cols)
        view(bound, mat).copy_(x)


def put_sentinel(bound, mat):
    w = whole(bound, mat)
    w.copy_(_filled(tuple(w.shape), SENTINEL, mat.dtype, w.device))


def only_written(wholes, regions):
    """``wholes``: name -> 2-D output buffer; ``regions``: ``(name, rows, cols)`` with ``rows`` a
    slice or an index tensor of buffer rows: the elements ``[rows, :cols]`` were supposed to be
    written. Asserts that every other element of every buffer still holds ``SENTINEL``."""
    written = {n: torch.zeros(b.shape, dtype=torch.bool, device=b.device)
               for n, b in wholes.items()}
    for name, rows, cols in regions:
        written[name][rows, :cols] = True
    report = []
    for name, buf in wholes.items():
        bad = int((buf.to(torch.float32)[~written[name]] != SENTINEL).sum())
        if bad:
            report.append(f"{name}: {bad}")
    assert not report, "elements written outside the expected regions: " + ", ".join(report)


def check_untouched(bound, mats, regions=()):
    """:func:`only_written` on placed outputs. ``regions``: ``(mat, rows, cols)`` with ``rows``
    relative to the matrix (a slice, an index tensor, or ``None`` for all of them)."""
    conv = []
    for mat, rows, cols in regions:
        if rows is None:
            rows = slice(0, mat.rows)
        if isinstance(rows, slice):
            rows = slice(rows.start + mat.guard, rows.stop + mat.guard)
        else:
            rows = rows + mat.guard
        conv.append((mat.name, rows, cols))
    only_written({m.name: whole(bound, m) for m in mats}, conv)


# ---------------------------------------------------------------------------- block tables
@dataclass(frozen=True)
class Blocks:
    """Row blocks of ``shard_rows`` rows: logical block b starts at row ``where[b][1]`` of
    buffer ``where[b][0]`` (0 or 1); the buffers have ``buf_rows`` rows."""
    shard_rows: int
    where: Tuple[Tuple[int, int], ...]
    buf_rows: Tuple[int, int]
    gap: int


def block_layout(nblocks, shard_rows, seed=0, gap=3):
    """``nblocks`` blocks dealt over two buffers in a permuted order (never the identity for
    more than one block), ``gap`` poison rows in front of, between and behind the blocks."""
    perm = torch.randperm(nblocks, generator=torch.Generator().manual_seed(seed)).tolist()
    if perm == sorted(perm):
        perm = perm[::-1]
    where, count = [None] * nblocks, [0, 0]
    for pos, b in enumerate(perm):
        buf = pos % 2
        where[b] = (buf, gap + count[buf] * (shard_rows + gap))
        count[buf] += 1
    return Blocks(shard_rows, tuple(where),
                  (gap + count[0] * (shard_rows + gap), gap + count[1] * (shard_rows + gap)), gap)


def scatter(a, layout, ld):
    """The two buffers (``[buf_rows, ld]``, ``POISON`` everywhere else) that hold the row blocks
    of ``a``; a block past the last row of ``a`` stays poison."""
    M, K = a.shape
    bufs = [_filled((r, ld), POISON, a.dtype, a.device) for r in layout.buf_rows]
    for b, (buf, row0) in enumerate(layout.where):
        r0 = b * layout.shard_rows
        n = max(0, min(M, r0 + layout.shard_rows) - r0)
        bufs[buf][row0:row0 + n, :K] = a[r0:r0 + n]
    return bufs


def gather(bufs, layout, M, K):
    """The inverse of :func:`scatter`: logical row i is row ``i % shard_rows`` of block
    ``i // shard_rows``. This is what a kernel that reads A through the table must see."""
    parts = []
    for b, (buf, row0) in enumerate(layout.where):
        n = max(0, min(M, (b + 1) * layout.shard_rows) - b * layout.shard_rows)
        parts.append(bufs[buf][row0:row0 + n, :K])
    return torch.cat(parts)


def place_blocks(plan, name, layout, K, dtype):
    """The two plan buffers of a block layout and the address table (one ref per block)."""
    ld = padded_ld(K, dtype)
    mats = [place(plan, f"{name}{i}", layout.buf_rows[i], K, dtype, ld=ld, extra=0)
            for i in (0, 1)]
    table = [mats[buf].row_ref(row0) for buf, row0 in layout.where]
    return mats, table


def put_blocks(bound, mats, layout, a):
    for mat, buf in zip(mats, scatter(a, layout, mats[0].ld)):
        whole(bound, mat).copy_(buf)


# ---------------------------------------------------------------------------- K-split
def ksplit_operands(M, N, K, dtype, seed=KSPLIT_SEED):
    """The operands of the public K-split tests, drawn on the CPU (the CPU test of the two
    specifications and the GPU test see the same numbers)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return ints((M, K), dtype, g), ints((N, K), dtype, g)


def ksplit_specs(a, w, S, dout):
    """``(once, twice)``: the exact product rounded once to ``dout`` (f32 partials summed and
    rounded by the reduce kernel), and the f32 sum of the ``S`` slice products each rounded to
    ``dout``, rounded once more (output-dtype partials). The sum of at most 64 rounded partials
    of integers below 2^24 / 64 is itself exact in f32."""
    K = a.shape[1]
    assert K % S == 0
    assert_exact(K)
    ks = K // S
    once = exact(a, w, dout)
    parts = [exact(a[:, j * ks:(j + 1) * ks], w[:, j * ks:(j + 1) * ks], dout).to(torch.float32)
             for j in range(S)]
    return once, sum(parts).to(dout)


# ---------------------------------------------------------------------------- run wrapper
@contextlib.contextmanager
def bound_plan(comm, plan):
    """``bind`` ... ``close``: the bound plan of a world-1 communicator."""
    from ddlb_amd.parallel.context import NativeContext

    ctx = NativeContext(comm)
    bound = None
    try:
        bound = ctx.bind(plan)
        yield bound
    finally:
        if bound is not None:
            bound.close()
        ctx.close()


def run(bound):
    """One run of the plan, finished, and no bounded spin gave up."""
    bound.run()
    torch.cuda.synchronize()
    bound.check_health()
