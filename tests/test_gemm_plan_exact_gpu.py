"""Exact-arithmetic sweep of the GEMM's plan-level arguments, the half of ``GemmArgs`` that only
``Plan.gemm`` reaches: ``ksplit``, ``a_shards`` / ``shard_rows``, ``c_shards`` / ``c_shard_rows``,
the arrival gate (``flags`` / ``flag_rows`` / ``nshards`` / ``nsub`` / ``first_shard`` /
``tile_order`` / ``reserve_cus``) and the in-kernel all-gather, in one process on one GPU.

As in ``test_gemm_exact_gpu.py`` the operands are integers in -3..3, so the specification is "the
exact product, rounded once to the output dtype" and every comparison is ``torch.equal`` or a
count of differing elements: there is no tolerance in this module. Operands are padded and
surrounded by poison, outputs are padded buffers filled with a sentinel, and after every run
every element outside the rows and columns that were to be written must still hold it
(``tests/_exact_plan.py``).

Measured on an MI355X: the module's 236 tests take 7.8 s of pytest wall time (8.8 s for the
process); a bind costs about 0.3 ms there, so most test functions stay below 50 ms and the
slowest (the first one, which loads the code objects) takes 0.4 s.

A product equal to the sentinel (-7: just under 1 % of the elements) cannot be told from an
element that was never stored by the sentinel check alone; the equality comparison covers it."""

import functools
import inspect

import pytest
import torch

from _exact import FP8, POISON, exact, ints
from _exact_plan import (assert_exact, block_layout, bound_plan, check_untouched, esize,
                         gather, ksplit_operands, ksplit_specs, place, place_blocks, plan_dt,
                         put_blocks, put_operand, put_sentinel, run, scatter, view, whole)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
AUTO, GENERIC, MX = 0, 1, 2

# (input, output, mode): the forms of the issue
FORMS = [(BF16, BF16, AUTO), (BF16, F32, AUTO), (F16, F32, AUTO), (F32, F32, AUTO),
         (FP8, BF16, AUTO), (FP8, F32, MX)]
BF, MXF = (BF16, BF16, AUTO), (FP8, F32, MX)


@pytest.fixture(scope="module")
def comm():
    import os

    from conftest import free_port
    from ddlb_amd.communicator import Communicator

    os.environ["DDLB_CHILD_INIT_METHOD"] = f"tcp://127.0.0.1:{free_port()}"
    c = Communicator()
    c.ensure_process_group()
    yield c
    Communicator.reset()
    os.environ.pop("DDLB_CHILD_INIT_METHOD", None)


def _name(dt):
    return str(dt).replace("torch.", "").replace("float8_e4m3fn", "fp8").replace("float", "f")


def _form_id(form):
    return f"{_name(form[0])}-{_name(form[1])}-{('auto', 'generic', 'mx')[form[2]]}"


def _tiles():
    from ddlb_amd.ops.gemm import TILES

    return dict(TILES)


def _t(name):
    return _tiles()[name]


def _k(din, ktiles):
    """K of ``ktiles`` 128-byte K-tiles."""
    return ktiles * 128 // esize(din)


def _make_case(din, M, N, K):
    assert_exact(K)
    g = torch.Generator(device=DEV).manual_seed(1000003 * M + 1009 * N + K + 17)
    return ints((M, K), din, g), ints((N, K), din, g)


_case = functools.lru_cache(maxsize=None)(_make_case)  # (the large case calls _make_case)


@functools.lru_cache(maxsize=None)
def _ref(din, M, N, K, S=1):
    """The exact f32 products of the S K-slices of the case (K = the whole K), never changed."""
    a, w = _case(din, M, N, K)
    ks = K // S
    return tuple(exact(a[:, j * ks:(j + 1) * ks], w[:, j * ks:(j + 1) * ks], F32)
                 for j in range(S))


def _differing(got, want):
    return int((got != want).sum())


# ---------------------------------------------------------------------------- one GEMM, checked
def _gemm_case(comm, form, M, N, K, tile=0, *, S=1, a_blocks=None, c_rows=0, c_grp=None,
               gate=None, act=None, runs=1, refused=False, case=None, force=None, **kw):
    """One ``Plan.gemm`` on placed operands and sentinel outputs; ``runs`` runs, after each the
    exact result in the rows that were to be written and the sentinel everywhere else.

    ``S``: K-split, ``K`` is the slice length. ``a_blocks = (shard_rows, nblocks)``: A through a
    block table. ``c_rows``: direct-store C in slots of that many rows (the buffer passed as
    ``c`` must stay untouched). ``c_grp = (grp, gstride)``: grouped C rows. ``gate``: the
    arrival-gate arguments; a ``signal`` op on the same stream raises exactly the ``nshards``
    flag words first. ``refused``: the launcher must refuse the run and write nothing.
    ``force``: op arguments set after ``Plan.gemm``'s own checks (to reach the launcher's)."""
    from ddlb_amd.parallel.plan import ACT_CODE, Plan, SIG_STREAM

    din, dout, mode = form
    Kt = S * K
    assert_exact(Kt)
    a, w = case if case is not None else _case(din, M, N, Kt)
    refs = [exact(a[:, j * K:(j + 1) * K], w[:, j * K:(j + 1) * K], F32) for j in range(S)] \
        if case is not None else _ref(din, M, N, Kt, S)
    plan = Plan(0, 1, nstreams=1, stream_priority=[0])
    wm = place(plan, "w", N, Kt, din)
    args = dict(M=M, N=N, K=K, ldb=wm.ld, din=plan_dt(din), dout=plan_dt(dout), tile=tile,
                mode=mode, ksplit=S, act=ACT_CODE[act or "none"])
    if a_blocks is not None:
        lay = block_layout(a_blocks[1], a_blocks[0], seed=M + a_blocks[0])
        amats, table = place_blocks(plan, "a", lay, Kt, din)
        args.update(a_shards=table, shard_rows=a_blocks[0], lda=amats[0].ld)
        a_ref = amats[0].ref
    else:
        am = place(plan, "a", M, Kt, din)
        args.update(lda=am.ld)
        a_ref = am.ref
    outs, regions, wants = [], [], []
    # (a forced K-split must be refused; were it launched, its partials would still land here)
    slack = 3 + ((force or {}).get("ksplit", 1) - 1) * M
    if c_rows:
        cm = place(plan, "c", 4, N, dout, align=8, guard=2)  # passed as c: never written
        nslot = -(-M // c_rows)
        slots = [place(plan, f"slot{q}", c_rows, N, dout, align=8, ld=cm.ld, guard=2)
                 for q in range(nslot)]
        args.update(c_shards=[s.ref for s in slots], c_shard_rows=c_rows)
        outs = [cm] + slots
        for q, s in enumerate(slots):
            n = min(M, (q + 1) * c_rows) - q * c_rows
            regions.append((s, slice(0, n), N))
            wants.append((s, slice(0, n), slice(q * c_rows, q * c_rows + n), 0))
    elif c_grp is not None:
        grp, gs = c_grp
        rows = torch.arange(M, device=DEV)
        rows = rows // grp * gs + rows % grp
        cm = place(plan, "c", int(rows.max()) + 1, N, dout, align=8, guard=2, extra=slack)
        args.update(c_grp=grp, c_gstride=gs)
        outs = [cm]
        regions.append((cm, rows, N))
        wants.append((cm, rows, slice(0, M), 0))
    else:
        # partial j: rows [j M, (j + 1) M)
        cm = place(plan, "c", S * M, N, dout, align=8, guard=2, extra=slack)
        outs = [cm]
        for j in range(S):
            regions.append((cm, slice(j * M, (j + 1) * M), N))
            wants.append((cm, slice(j * M, (j + 1) * M), slice(0, M), j))
    args.update(ldc=cm.ld)
    fl = None
    if gate is not None:
        fl = plan.buffer("flags", 256, zero=True)
        ns = gate["nshards"]
        plan.signal(0, [fl + 4 * i for i in range(ns)], method=gate.get("sig", SIG_STREAM))
        args.update(flags=fl, flag_rows=gate.get("flag_rows", M // ns), nshards=ns,
                    nsub=gate.get("nsub", 1), first_shard=gate.get("first_shard", 0),
                    tile_order=gate.get("tile_order", 0),
                    reserve_cus=gate.get("reserve_cus", 0))
    args.update(kw)
    op = plan.gemm(0, a_ref, wm.ref, cm.ref, **args)
    if force:
        op.args.update(force)
    what = f"{_form_id(form)} tile {tile} {(M, N, K)} S={S} {kw or ''}"
    with bound_plan(comm, plan) as bound:
        put_operand(bound, wm, w)
        if a_blocks is not None:
            put_blocks(bound, amats, lay, a)
        else:
            put_operand(bound, am, a)
        if gate is not None and gate.get("graph"):
            # a gated GEMM whose flags another op raises is replayed only where the executor
            # says a capture is allowed; anywhere else the refusal is the answer and it runs eagerly
            if bound.ex.graph_capturable():
                bound.enable_graph(True)
            else:
                with pytest.raises(RuntimeError):
                    bound.enable_graph(True)
        for it in range(runs):
            for m in outs:
                put_sentinel(bound, m)
            if refused:
                with pytest.raises(RuntimeError):
                    bound.run()
                torch.cuda.synchronize()
                bound.check_health()
                check_untouched(bound, outs)
                continue
            run(bound)
            for m, rows, src, j in wants:
                want = refs[j][src]
                if act == "relu":
                    want = want.clamp(min=0)
                bad = _differing(view(bound, m)[rows, :N], want.to(dout))
                assert bad == 0, f"{what} run {it}: {bad} wrong elements in {m.name} rows {rows}"
            check_untouched(bound, outs, regions)
            if fl is not None:  # the run's epoch in exactly the nshards words, zero elsewhere
                words = bound.buffer("flags")[:256].view(torch.int32)
                assert words[:ns].tolist() == [it + 1] * ns and int(words[ns:].abs().sum()) == 0


# ---------------------------------------------------------------------------- a. K-split partials
@pytest.mark.parametrize("form", FORMS, ids=_form_id)
@pytest.mark.parametrize("tile", ["auto", "pt4"])
def test_ksplit_pt4_one_launch(comm, form, tile):
    """pt4's one-launch form: every (slice, tile) pair a virtual tile. One 256 x 256 tile with
    2 K-tiles per slice (virtual tiles outnumber tiles) and a 2 x 3 grid with 4 K-tiles per
    slice, S in {2, 3, 4}; lda / ldb padded beyond S K, ldc padded, partial s at c + s M ldc."""
    for S in (2, 3, 4):
        _gemm_case(comm, form, 256, 256, _k(form[0], 2), _t(tile), S=S)
        _gemm_case(comm, form, 512, 768, _k(form[0], 4), _t(tile), S=S)


@pytest.mark.parametrize("form", [BF, MXF], ids=_form_id)
def test_ksplit_pt4_second_virtual_tile_in_another_slice(comm, form):
    """2304 x 2560, S = 3: 270 (slice, tile) pairs, more than the persistent grid, so a
    workgroup's second virtual tile lies in another slice (another K offset, another partial)."""
    M, N, S = 2304, 2560, 3
    K = _k(form[0], 2)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert (M // 256) * (N // 256) * S == 270 and 270 > cus // 8 * 8
    _gemm_case(comm, form, M, N, K, _t("pt4"), S=S, case=_make_case(form[0], M, N, S * K))


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
@pytest.mark.parametrize("tile", ["t4", "t8", "pt8", "i256", "128x128", "256x128"])
def test_ksplit_slice_by_slice(comm, form, tile):
    """Every kernel but pt4 runs the slices one launch after another: whole tiles, and the ragged
    300 x 202 and 130 x 203 (through the tiled kernels; only ``ops.gemm`` forbids those)."""
    K = _k(form[0], 2)
    _gemm_case(comm, form, 512, 512, K, _t(tile), S=2)
    _gemm_case(comm, form, 300, 202, K, _t(tile), S=3)
    _gemm_case(comm, form, 130, 203, K, _t(tile), S=2)


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_ksplit_pt4_declines(comm, form):
    """3 K-tiles per slice: pt4 (auto and explicit) declines an odd K-tile count and the launcher
    runs the slices one by one; a slice of 100 elements is off the fast path and every slice
    goes to the generic kernel. Either way every partial is exact and in its place."""
    for tile in ("auto", "pt4"):
        _gemm_case(comm, form, 256, 256, _k(form[0], 3), _t(tile), S=2)
        _gemm_case(comm, form, 512, 768, _k(form[0], 3), _t(tile), S=3)
    _gemm_case(comm, form, 130, 70, 100, _t("auto"), S=2)
    _gemm_case(comm, form, 256, 256, 100, _t("pt4"), S=3)


def test_ksplit_refusals(comm):
    """``Plan.gemm`` raises for ksplit > 1 with flags, an A table, a C table, an activation,
    grouped A rows or grouped C rows; the same combinations pushed past it (the op's ``ksplit``
    set afterwards) are refused by the launcher, which writes nothing. ksplit = 65 is refused at
    load time by the plan executor and by the launcher behind the ``gemm`` binding."""
    from ddlb_amd.ops import load
    from ddlb_amd.parallel.plan import Plan

    M, N, K = 512, 512, _k(BF16, 2)
    plan = Plan(0, 1)
    a, b, c = (plan.buffer(n, 1 << 20) for n in "abc")
    base = dict(M=M, N=N, K=K, lda=2 * K, ldb=2 * K, ldc=N, din=plan_dt(BF16),
                dout=plan_dt(BF16), ksplit=2)
    for bad in (dict(flags=plan.buffer("f", 256, zero=True), flag_rows=256, nshards=2),
                dict(a_shards=[a, a + 256 * 4 * K], shard_rows=256),
                dict(c_shards=[c, c + 256 * 2 * N], c_shard_rows=256), dict(act=2),
                dict(a_grp=256, a_gstride=256), dict(c_grp=256, c_gstride=256)):
        with pytest.raises(ValueError, match="ksplit"):
            plan.gemm(0, a, b, c, **base, **bad)
    with pytest.raises(ValueError, match="ksplit"):
        plan.gemm(0, a, b, c, **dict(base, ksplit=0))
    # past Plan.gemm: the launcher's own refusal, C untouched
    K2 = 2 * K  # (the case's whole K: these plans are built unsplit, then split by force)
    for kw in (dict(gate=dict(nshards=2)), dict(a_blocks=(256, 2)), dict(c_rows=256),
               dict(act="relu"), dict(c_grp=(256, 256)), dict(a_grp=256, a_gstride=256)):
        _gemm_case(comm, BF, M, N, K2, _t("auto"), refused=True, force=dict(ksplit=2, K=K), **kw)
        _gemm_case(comm, BF, M, N, K2, _t("t4"), refused=True, force=dict(ksplit=2, K=K), **kw)
    # ksplit = 65: the executor refuses the plan when it is loaded ...
    with pytest.raises(RuntimeError, match="K-split"):
        _gemm_case(comm, BF, 256, 256, K, _t("auto"), force=dict(ksplit=65))
    # ... and the launcher refuses the direct call
    C = load()
    aw, ww = _case(BF16, 256, 256, 65 * 64)
    out = torch.full((65 * 256 + 3, 256), -7.0, dtype=BF16, device=DEV)
    for tile in ("auto", "t4"):
        with pytest.raises(RuntimeError):
            C.gemm(aw.data_ptr(), ww.data_ptr(), out.data_ptr(), aw.stride(0), ww.stride(0), 256,
                   256, 256, 64, plan_dt(BF16), plan_dt(BF16), _t(tile), AUTO, 0, 0, 0, 0,
                   torch.cuda.current_stream().cuda_stream, 0, 65)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all())
    C.gemm(aw.data_ptr(), ww.data_ptr(), out.data_ptr(), aw.stride(0), ww.stride(0), 256, 256, 256,
           64, plan_dt(BF16), plan_dt(BF16), _t("t4"), AUTO, 0, 0, 0, 0,
           torch.cuda.current_stream().cuda_stream, 0, 64)  # 64 slices are the most it takes
    torch.cuda.synchronize()
    refs = _ref(BF16, 256, 256, 65 * 64, 65)
    for j in range(64):
        assert torch.equal(out[j * 256:(j + 1) * 256], refs[j].to(BF16)), j
    assert bool((out[64 * 256:] == -7.0).all())


# ---------------------------------------------------------------------------- b. the public K-split
def _public_ksplit(M, N, K, dtype, S, tile, mode="auto", out_dtype=None):
    """``ops.gemm.gemm(a, w, out, ksplit=S)`` into a dense output between two sentinel guards."""
    from ddlb_amd.ops.gemm import gemm

    a, w = ksplit_operands(M, N, K, dtype)
    dout = out_dtype or dtype
    once, twice = ksplit_specs(a, w, S, dout)
    buf = torch.full((M + 6, N), -7.0, device=DEV).to(dout)
    out = buf[3:3 + M]
    gemm(a.to(DEV), w.to(DEV), out, tile=tile, mode=mode, ksplit=S)
    torch.cuda.synchronize()
    assert bool((buf[:3].float() == -7.0).all()) and bool((buf[3 + M:].float() == -7.0).all())
    return out, once.to(DEV), twice.to(DEV)


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_name)
@pytest.mark.parametrize("M", [256, 512])
def test_public_ksplit_rounds_as_documented(M, dtype, S):
    """``ksplit=S`` through the public op at K = 1024, where bf16 really rounds (4.6 % of the
    products are beyond 256). tile auto / pt4: f32 partials summed in slice order and rounded
    ONCE by the reduce kernel, equal to the exact product rounded once. tile t4: partials in
    the output dtype, their f32 sum rounded once more. In bf16 the two specifications differ
    (S = 2: 226 elements at M = 256, 422 at M = 512; tests/test_exact_refs_cpu.py), so a path
    that took the other one fails; in f16 they coincide."""
    N, K = 256, 1024
    for tile in ("auto", "pt4"):
        out, once, twice = _public_ksplit(M, N, K, dtype, S, tile)
        bad = _differing(out, once)
        assert bad == 0, f"{tile}: {bad} elements differ from the product rounded once " \
                         f"({_differing(out, twice)} from the twice-rounded one)"
    if dtype == BF16 and S == 2:
        assert _differing(once, twice) > 100
    out, once, twice = _public_ksplit(M, N, K, dtype, S, "t4")
    bad = _differing(out, twice)
    assert bad == 0, f"t4: {bad} elements differ from the sum of rounded partials " \
                     f"({_differing(out, once)} from the once-rounded product)"


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("M", [256, 512])
def test_public_ksplit_mx_and_f32(M, S):
    """fp8 ``mode="mx"`` -> bf16 and f32 -> f32 through the same two paths, each against its
    own specification (for f32 they are the same numbers)."""
    N, K = 256, 1024
    for dtype, mode, dout in ((FP8, "mx", BF16), (F32, "auto", F32)):
        for tile in ("auto", "pt4", "t4"):
            out, once, twice = _public_ksplit(M, N, K, dtype, S, tile, mode=mode, out_dtype=dout)
            want = twice if tile == "t4" else once
            bad = _differing(out, want)
            assert bad == 0, f"{_name(dtype)} {tile}: {bad} elements differ"
            if dout == F32:
                assert torch.equal(once, twice)


# ---------------------------------------------------------------------------- c. A through a table
C_FORMS = [(BF16, BF16, AUTO), (F16, F32, AUTO), (F32, F32, AUTO), (FP8, BF16, AUTO), MXF]


@pytest.mark.parametrize("form", C_FORMS, ids=_form_id)
@pytest.mark.parametrize("tile", ["auto", "pt4", "t4", "t8", "pt8"])
def test_a_table_whole_tiles(comm, form, tile):
    """A's row blocks scattered over two buffers in a permuted order, poison rows between them:
    blocks of 256 and 512 rows (pt4: one panel base per tile), and a table with more blocks
    than M uses (M = 768, 4 blocks of 256: the last block is poison)."""
    K = _k(form[0], 2)
    _gemm_case(comm, form, 1024, 512, K, _t(tile), a_blocks=(256, 4))
    _gemm_case(comm, form, 1024, 512, K, _t(tile), a_blocks=(512, 2))
    _gemm_case(comm, form, 768, 512, K, _t(tile), a_blocks=(256, 4))


@pytest.mark.parametrize("form", [BF, (FP8, F32, AUTO), MXF], ids=_form_id)
@pytest.mark.parametrize("tile", sorted(_tiles()))
def test_a_table_off_whole_tiles(comm, form, tile):
    """Every tile code off whole tiles (the ping-pong codes hand over to the 128x128 tiled
    kernel): blocks of 192 rows, so every 128- and 256-row tile straddles a block boundary and
    ``a_row()`` divides per row; blocks of 250 rows with a ragged last tile. For fp8 ``mode``
    mx is silently demoted to the unit-scale fp8 kernel: only the product shows it went right."""
    K = _k(form[0], 2)
    _gemm_case(comm, form, 960, 202, K, _t(tile), a_blocks=(192, 5))
    _gemm_case(comm, form, 1000, 203, K, _t(tile), a_blocks=(250, 4))


def test_a_table_refusals(comm):
    """Refused with C untouched: ``mode`` generic with a table (whole tiles and ragged), and a
    table whose K is off the fast path (the generic kernel cannot read through a table).
    Block scales with a table are refused by the launcher too (``gemm_launch``: ``a_scale`` with
    ``a_table``), but no Python entry point can ask for both: ``Plan.gemm`` has no scales and
    ``ops.gemm.gemm`` no table, which is asserted here instead."""
    from ddlb_amd.ops.gemm import gemm
    from ddlb_amd.parallel.plan import Plan

    K = _k(BF16, 2)
    for form in ((BF16, BF16, GENERIC), (FP8, F32, GENERIC)):
        K = _k(form[0], 2)
        _gemm_case(comm, form, 1024, 512, K, _t("auto"), a_blocks=(256, 4), refused=True)
        _gemm_case(comm, form, 960, 202, K, _t("128x128"), a_blocks=(192, 5), refused=True)
    _gemm_case(comm, BF, 256, 256, 104, _t("auto"), a_blocks=(128, 2), refused=True)
    assert not [p for p in inspect.signature(Plan.gemm).parameters if "scale" in p]
    assert not [p for p in inspect.signature(gemm).parameters if "shard" in p or "table" in p]


# ---------------------------------------------------------------------------- d. direct-store C
D_FORMS = [(BF16, BF16, AUTO), (F16, F16, AUTO), (BF16, F32, AUTO), MXF]


@pytest.mark.parametrize("form", D_FORMS, ids=_form_id)
@pytest.mark.parametrize("tile", ["auto", "pt4", "t4", "t8", "pt8"])
def test_c_table_whole(comm, form, tile):
    """Every slot its own sentinel buffer (padded ldc, guard and extra rows): 4 slots of 256
    rows and 2 of 512, dispatched in order and shard-interleaved (``tile_order`` 2); explicit
    pt4 stores through its table form (CMODE 1). The buffer passed as ``c`` stays untouched."""
    K = _k(form[0], 2)
    for rows in (256, 512):
        for order in (0, 2):
            _gemm_case(comm, form, 1024, 512, K, _t(tile), c_rows=rows, nshards=1024 // rows,
                       tile_order=order)


def test_c_table_relu(comm):
    for tile in ("auto", "pt4", "t4", "t8"):
        _gemm_case(comm, (BF16, F32, AUTO), 1024, 512, _k(BF16, 2), _t(tile), c_rows=256,
                   nshards=4, tile_order=2, act="relu")
    assert int((_ref(BF16, 1024, 512, _k(BF16, 2))[0] < 0).sum()) > 1000


@pytest.mark.parametrize("form", [BF, MXF], ids=_form_id)
@pytest.mark.parametrize("tile", sorted(_tiles()))
def test_c_table_tiled(comm, form, tile):
    """Every tile code off whole tiles: slots of 192 rows (tiles straddle two slots; the
    requested ``tile_order`` 2 must be dropped, since a shard is no whole number of tiles) and
    slots of 256 rows at M = 1000 (the last slot is written in its first 232 rows only)."""
    K = _k(form[0], 2)
    _gemm_case(comm, form, 960, 202, K, _t(tile), c_rows=192, nshards=5, tile_order=2)
    _gemm_case(comm, form, 1000, 203, K, _t(tile), c_rows=256)


@pytest.mark.parametrize("form", [BF, MXF], ids=_form_id)
@pytest.mark.parametrize("tile", ["auto", "pt4", "t4", "t8", "128x128"])
def test_a_table_and_c_table(comm, form, tile):
    """Both tables at once: pt4 declines (its table-A forms have no C table) and t4, or off
    whole tiles the 128x128 tiled kernel, takes the launch."""
    K = _k(form[0], 2)
    _gemm_case(comm, form, 1024, 512, K, _t(tile), a_blocks=(256, 4), c_rows=512)
    _gemm_case(comm, form, 960, 202, K, _t(tile), a_blocks=(192, 5), c_rows=320)


@pytest.mark.parametrize("form", [BF, (BF16, F32, AUTO), MXF], ids=_form_id)
def test_pt4_grouped_c_rows_off_256(comm, form):
    """pt4 with C groups of 384 rows 512 apart and plain A: no write-through panel (c_grp is no
    multiple of 256), so the per-row store form (CMODE 0); the 128 skipped rows after each group
    keep the sentinel. A tile (rows 256..511) straddles two groups."""
    for tile in ("pt4", "t4"):
        _gemm_case(comm, form, 768, 512, _k(form[0], 2), _t(tile), c_grp=(384, 512))


# ---------------------------------------------------------------------------- e. the arrival gate
GATES = [(2, 1, 1), (4, 2, 1), (8, 4, 0), (8, 2, 3)]  # (nshards, nsub, first_shard)


@pytest.mark.parametrize("gate", GATES, ids=lambda g: "-".join(map(str, g)))
@pytest.mark.parametrize("tile", ["pt4", "t4"])
@pytest.mark.parametrize("form", [BF, MXF], ids=_form_id)
def test_gated_dispatch_flags_raised(comm, form, tile, gate):
    """The tile <-> shard <-> flag arithmetic with the flags already raised (a ``signal`` op on
    the same stream sets exactly the ``nshards`` words; the flag buffer is larger and stays zero
    elsewhere): plain A with ``tile_order`` 0 and 1, table A with 1 and 3, ``reserve_cus`` 0 and
    32, three runs each (the epoch advances). A tile computed twice, never or from the wrong
    block fails the exact comparison; a wait on a word outside [0, nshards) never ends and shows
    up through ``check_health()``."""
    ns, nsub, first = gate
    K = _k(form[0], 2)
    for reserve in (0, 32):
        g = dict(nshards=ns, nsub=nsub, first_shard=first, reserve_cus=reserve)
        for order in (0, 1):
            _gemm_case(comm, form, 2048, 512, K, _t(tile), gate=dict(g, tile_order=order), runs=3)
        for order in (1, 3):
            _gemm_case(comm, form, 2048, 512, K, _t(tile), gate=dict(g, tile_order=order),
                       a_blocks=(2048 // ns, ns), runs=3)


def test_gated_own_rows_need_table_a(comm):
    """``tile_order`` 3 on plain A rows stays refused by pt4 (no instantiation skips the own
    rows' flags there), with C untouched."""
    _gemm_case(comm, BF, 2048, 512, _k(BF16, 2), _t("pt4"), refused=True,
               gate=dict(nshards=4, nsub=2, first_shard=1, tile_order=3, reserve_cus=32))


@pytest.mark.parametrize("form", [BF, MXF], ids=_form_id)
def test_gated_tile_spans_two_shards(comm, form):
    """Shards of 320 rows under 128- and 256-row tiles (M = 1280): a tile waits for every shard
    its rows touch (the ``wait_flag_t0`` loop), also off whole tiles."""
    K = _k(form[0], 2)
    g = dict(nshards=4, flag_rows=320)
    _gemm_case(comm, form, 1280, 256, K, _t("t8"), gate=g, runs=2)
    _gemm_case(comm, form, 1280, 256, K, _t("128x128"), gate=g, runs=2)
    _gemm_case(comm, form, 1280, 202, K, _t("128x128"), gate=g, runs=2)


def test_gated_graph_replay(comm):
    """One plain-A and one table-A gated GEMM whose flags a ``SIG_KERNEL`` signal raises, under
    hipGraph replay where ``graph_capturable()`` allows it (a gated GEMM fed by another op is
    not captured by this executor: then the refusal is asserted and the plan runs eagerly)."""
    from ddlb_amd.parallel.context import graph_replay_supported
    from ddlb_amd.parallel.plan import SIG_KERNEL

    assert graph_replay_supported()
    K = _k(BF16, 2)
    g = dict(nshards=8, nsub=4, first_shard=1, reserve_cus=32, sig=SIG_KERNEL, graph=True)
    _gemm_case(comm, BF, 2048, 512, K, _t("pt4"), gate=dict(g, tile_order=1), runs=3)
    _gemm_case(comm, BF, 2048, 512, K, _t("pt4"), gate=dict(g, tile_order=3), a_blocks=(256, 8),
               runs=3)


@pytest.mark.parametrize("mode", [0, 1, 6, 30])
@pytest.mark.parametrize("parts", [1, 8])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_in_kernel_allgather_exact(comm, graph, parts, mode):
    """The in-kernel all-gather as ``test_in_kernel_allgather_world1`` sets it up, at 1024 x 256
    with 2 K-tiles: 2 producers x 2 blocks, 8 copy workgroups, ``parts`` pieces per segment. A
    local buffer stands in for the peer's copy of A (its own half poison); the peer half of the
    gather buffer holds poison before every run, so a tile that did not wait, or a segment
    copied from or to the wrong place, changes the exact product. The gathered rows, their
    padding and C's surroundings are checked too."""
    from ddlb_amd.parallel.plan import Plan, SIG_IN_LAUNCH, SIG_KERNEL, SIG_STREAM

    M, N, K, nsub = 1024, 256, _k(BF16, 2), 2
    half, rows = M // 2, M // (2 * nsub)
    a, w = _case(BF16, M, N, K)
    want = _ref(BF16, M, N, K)[0].to(BF16)
    plan = Plan(0, 1, nstreams=1, stream_priority=[0])
    am = place(plan, "a", M, K, BF16)
    pm = place(plan, "peer", M, K, BF16, ld=am.ld)
    wm = place(plan, "w", N, K, BF16)
    cm = place(plan, "c", M, N, BF16, align=8, guard=2)
    fl = plan.buffer("flags", 256, zero=True)
    READY, ACK, ARRIVE, CNT = fl, fl + 8, fl + 16, fl + 48
    sig = SIG_KERNEL if graph else SIG_STREAM
    plan.signal(0, [READY + 4], method=sig)
    plan.signal(0, [ARRIVE + 4 * j for j in range(nsub)], method=sig)
    ag = dict(ctas=8, parts=parts, rank=0, src=[am.ref, pm.ref], ack=[ACK, ACK + 4], ready=READY,
              count=CNT, mode=mode, wait_acks=[ACK, ACK + 4] if mode & 16 else None)
    plan.gemm(0, am.ref, wm.ref, cm.ref, M=M, N=N, K=K, lda=am.ld, ldb=wm.ld, ldc=cm.ld,
              din=plan_dt(BF16), dout=plan_dt(BF16), tile=_t("pt4"), flags=ARRIVE, flag_rows=rows,
              nshards=2 * nsub, nsub=nsub, first_shard=0, tile_order=1, ag=ag)
    plan.wait_signal(0, [ACK + 4], method=SIG_IN_LAUNCH if mode & 16 else sig)
    with bound_plan(comm, plan) as bound:
        if graph:  # the in-kernel all-gather sets its own gate flags: captured
            assert bound.ex.graph_capturable()
            bound.enable_graph(True)
        put_operand(bound, wm, w)
        put_operand(bound, pm)
        view(bound, pm)[half:].copy_(a[half:])
        for it in range(3):
            put_operand(bound, am)
            view(bound, am)[:half].copy_(a[:half])
            put_sentinel(bound, cm)
            run(bound)
            bad = _differing(view(bound, cm), want)
            assert bad == 0, f"run {it}: {bad} wrong elements"
            check_untouched(bound, [cm], [(cm, None, N)])
            assert torch.equal(view(bound, am), a), f"run {it}: the gathered rows"
            wa = whole(bound, am).float()
            assert bool((wa[:M, K:] == POISON).all()) and bool((wa[M:] == POISON).all())


def test_scatter_is_what_the_gpu_reads():
    """The block layout on the device equals the CPU-side specification (``gather`` inverts
    ``scatter`` there too)."""
    a, _ = _case(BF16, 960, 202, _k(BF16, 2))
    lay = block_layout(5, 192, seed=3)
    bufs = scatter(a, lay, a.shape[1] + 8)
    assert torch.equal(gather(bufs, lay, 960, a.shape[1]), a)
