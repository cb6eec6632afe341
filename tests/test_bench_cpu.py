"""bench.py orchestration on the CPU: parent/child process model, gloo coordination, MAX over
ranks, the one-line JSON contract (GPU-free path: the pytorch candidate on gloo)."""

import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--steps", "3", "--warmup", "1", "-m", "256", "-n", "64", "-k", "64",
        "--algorithm", "pytorch(rccl+hipblaslt)", "--dtype", "float32"]
FULL = ARGS + ["--full"]  # the reference check, harness timing and diagnostics live behind it


def _json_line(out: str):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def _env():
    env = dict(os.environ, DDLB_DEVICE="cpu")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
              "DDLB_CHILD_INIT_METHOD"):
        env.pop(k, None)
    return env


def test_bench_world1_cpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *FULL],
                       capture_output=True, text=True, timeout=300, env=_env())
    assert r.returncode == 0, r.stderr[-3000:]
    d = _json_line(r.stdout)
    # stdout holds the JSON line only (children's and libraries' stdout goes to stderr)
    assert [ln for ln in r.stdout.splitlines() if ln.strip()] == [r.stdout.strip()]
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert key in d
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["valid"] is True
    assert d["value"] > 0 and d["scaling"] == "weak"


def test_bench_world2_cpu():
    from conftest import free_port

    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", *FULL]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=400, env=_env())
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and d["valid"] is True
    assert abs(d["value"] - 2 * d["per_gpu_tflops"]) < 1e-2


def test_bench_gpus2_without_launcher_cpu():
    """``--gpus 2`` started as a plain ``python bench.py`` (no WORLD_SIZE): bench.py runs
    torch.distributed.run itself as a child and relays exactly one JSON line (the driver's N>1
    record must not depend on how it launches the script)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", *FULL],
                       capture_output=True, text=True, timeout=400, env=_env())
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and d["valid"] is True
    assert "without a launcher" in r.stderr
    assert len([ln for ln in r.stdout.splitlines() if ln.strip()]) == 1


def _prewarm_worker(rank, world, port, q):
    import time

    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      LOCAL_WORLD_SIZE=str(world), DDLB_DEVICE="cpu",
                      DDLB_CHILD_INIT_METHOD=f"tcp://127.0.0.1:{port}")
    sys.path.insert(0, ROOT)
    import bench
    from ddlb_amd.communicator import Communicator

    class SlowOnRank1:  # rank 1's run() is 4x slower: a wall-clock prewarm would diverge
        def run(self):
            time.sleep(0.004 if rank == 1 else 0.001)

    comm = Communicator()
    comm.ensure_process_group()
    q.put((rank, bench.prewarm_runs(SlowOnRank1(), comm, prewarm_ms=40.0)))
    comm.destroy()


def test_prewarm_runs_agree_across_ranks():
    """Every rank must issue the same number of run() calls (each holds collectives / epoch-
    matched signals): the pre-warm count is MAX-reduced, not taken from each rank's clock."""
    import multiprocessing as mp

    from conftest import free_port

    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), free_port()
    procs = [ctx.Process(target=_prewarm_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    # equal counts is the property; the count itself depends on the host's sleep granularity
    # under load (rank 0 alone would ask for ~40 / 1.x ms, rank 1 for ~10)
    assert got[0] == got[1] and got[0] >= 8, got


def test_bench_rowwise_world2_cpu():
    """--primitive tp_rowwise: GEMM + reduce-scatter; strong scaling, so the whole-job value is
    the reference harness number itself (ranks share one [m,k]x[k,n])."""
    from conftest import free_port

    args = ["--steps", "3", "--warmup", "1", "-m", "256", "-n", "64", "-k", "64", "--dtype",
            "float32", "--primitive", "tp_rowwise", "--algorithm", "row/pytorch(rccl+hipblaslt)",
            "--full"]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", *args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=400, env=_env())
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and d["valid"] is True and d["scaling"] == "strong"
    assert d["metric"].startswith("tp_rowwise")
    assert abs(d["value"] - d["harness_tflops"]) < 1e-6
    assert abs(d["per_gpu_tflops"] - d["harness_tflops"] / 2) < 1e-6


def test_candidate_pools():
    sys.path.insert(0, ROOT)
    import bench

    col8 = bench.candidate_pool("tp_columnwise", "bfloat16", 8)
    assert any(c[0] == "direct/ipc" for c in col8) and all(c[0][:4] != "row/" for c in col8)
    # the forms that cannot hang by construction lead (direct/ipc, the in-kernel all-gather),
    # then the CTA-capped RCCL-fed fused GEMM; the vendor slot last; no vendor-library GEMM
    # behind native; dominated / host-bound forms only on request (extra)
    natives = [c for c in col8 if c[1] == "native"]
    assert [c[0] for c in natives[:3]] == ["direct/ipc", "coll_pipeline/ipc/agk32/s4/graph",
                                           "coll_pipeline/rccl/s4/fused"]
    assert not any(c[2].get("multicast_protocol") == "batch_memcpy" for c in col8)
    extra = bench.candidate_pool("tp_columnwise", "bfloat16", 8, extra=True)
    assert len(extra) > len(col8) and {c[0] for c in col8} <= {c[0] for c in extra}
    assert col8[-1][1] == "pytorch"
    assert {c[2]["backend"] for c in natives[:5]} == {"rccl", "ipc"}
    for pool in (col8, bench.candidate_pool("tp_rowwise", "bfloat16", 8),
                 bench.candidate_pool("tp_columnwise", "bfloat16", 1)):
        assert not any("blas" in str(c[2]) for c in pool)
    row1 = bench.candidate_pool("tp_rowwise", "bfloat16", 1)
    assert [c[0] for c in row1 if c[1] == "native"] == ["row/gemm (world=1)/auto",
                                                       "row/gemm (world=1)/t4"]
    fp8 = bench.candidate_pool("tp_columnwise", "float8_e4m3fn", 1)
    labels = [c[0] for c in fp8]
    assert "gemm (world=1)/auto/mx" in labels
    assert "compute_only(hipblaslt)" not in labels  # torch.matmul has no fp8


class _FakeJob:
    """Scripted Job: ``script[label]`` = list of results returned by successive measure()
    calls of that candidate (tuning first, then the final run)."""

    rank = 0

    def left(self):
        return 1e9

    def __init__(self, pool, script):
        self.by_opts = {json.dumps(o, sort_keys=True): lbl for lbl, _, o in pool}
        self.script = {k: list(v) for k, v in script.items()}
        self.calls = []

    def bcast(self, obj):
        return obj

    def log(self, msg):
        pass

    def measure(self, impl, opts, steps, warmup, validate, timeout, prewarm_ms=0.0,
                harness_iters=0):
        label = self.by_opts[json.dumps(opts, sort_keys=True)]
        self.calls.append((label, validate))
        return self.script[label].pop(0)


def _args(**kw):
    import argparse

    d = dict(tune_rounds=1, tune_steps=5, validate=True, candidate_timeout=10.0,
             tune_budget_s=1e9, tune_cap_s=1e9, prewarm_ms=0.0, steps=5, warmup=1,
             final_reserve_s=0.0, harness_iters=0)
    d.update(kw)
    return argparse.Namespace(**d)


def _ok(ms, valid=True, why=""):
    return {"ok": True, "ms": ms, "valid": valid, "validation": why}


def test_autotune_rejects_fast_invalid_candidate():
    """A candidate that is fastest but computes the wrong numbers never wins: the
    tuning runs validate, and an invalid result counts as a failure."""
    sys.path.insert(0, ROOT)
    import bench

    pool = [("fast-wrong", "native", {"x": 1}), ("slow-right", "native", {"x": 2}),
            ("vendor", "pytorch", {"x": 3})]
    job = _FakeJob(pool, {"fast-wrong": [_ok(0.5, False, "mismatch")],
                          "slow-right": [_ok(1.0), _ok(1.1)], "vendor": [_ok(2.0)]})
    tune = {}
    chosen, fallbacks = bench.autotune(job, pool, _args(), 2, tune)
    assert chosen[0] == "slow-right"
    assert all(v for _, v in job.calls), "tuning must validate"
    assert "invalid" in tune["fast-wrong"]
    assert [c[0] for c in fallbacks] == ["vendor"]
    cand, final = bench.final_measure(job, chosen, fallbacks, _args(), tune)
    assert cand[0] == "slow-right" and final["valid"] is True


def test_final_falls_back_when_winner_does_not_validate():
    sys.path.insert(0, ROOT)
    import bench

    pool = [("a", "native", {"x": 1}), ("b", "native", {"x": 2}), ("v", "pytorch", {"x": 3})]
    job = _FakeJob(pool, {"a": [_ok(0.5), _ok(0.5, False, "bad last step")],
                          "b": [_ok(0.7), {"ok": False, "error": "timeout after 10s"}],
                          "v": [_ok(0.9), _ok(0.95)]})
    tune = {}
    chosen, fallbacks = bench.autotune(job, pool, _args(), 2, tune)
    assert chosen[0] == "a" and [c[0] for c in fallbacks] == ["b", "v"]
    cand, final = bench.final_measure(job, chosen, fallbacks, _args(), tune)
    assert cand[0] == "v" and final["valid"] is True
    assert tune["final_fallback_from"] == "a" and len(tune["final_rejected"]) == 2


def test_final_reports_invalid_when_nothing_validates():
    sys.path.insert(0, ROOT)
    import bench

    pool = [("a", "native", {"x": 1})]
    job = _FakeJob(pool, {"a": [_ok(0.5, False, "bad")]})
    cand, final = bench.final_measure(job, pool[0], [], _args(), {})
    assert cand[0] == "a" and final["valid"] is False


def test_autotune_skips_families_failing_preflight():
    """A candidate family whose preflight check failed is never run; the vendor slot never
    becomes the headline while a native candidate succeeded."""
    sys.path.insert(0, ROOT)
    import bench

    pool = [("r", "native", {"backend": "rccl"}),
            ("i", "native", {"backend": "ipc", "multicast_protocol": "kernel"}),
            ("v", "pytorch", {"backend": "nccl"})]
    job = _FakeJob(pool, {"r": [_ok(0.9)], "v": [_ok(0.5)]})
    tune = {}
    pre = {"rccl": "ok (3 ms)", "ipc": "ok", "ipc_kernel": "failed: timeout",
           "torch_nccl": "ok"}
    chosen, fallbacks = bench.autotune(job, pool, _args(), 8, tune, pre)
    assert chosen[0] == "r" and [c[0] for c in fallbacks] == ["v"]
    assert tune["i"].startswith("skipped (ipc_kernel")
    assert [c for c, _ in job.calls] == ["r", "v"]


def test_autotune_drops_family_after_two_timeouts():
    sys.path.insert(0, ROOT)
    import bench

    pool = [(f"i{j}", "native", {"backend": "ipc", "multicast_protocol": "memcpy", "j": j})
            for j in range(4)] + [("r", "native", {"backend": "rccl"})]
    to = {"ok": False, "error": "timeout after 45s"}
    job = _FakeJob(pool, {"i0": [to], "i1": [to], "r": [_ok(1.0)]})
    tune = {}
    chosen, _ = bench.autotune(job, pool, _args(), 8, tune, {})
    assert chosen[0] == "r"
    assert "timed out twice" in tune["i2"] and "timed out twice" in tune["i3"]


def test_deadline_stops_tuning_and_final():
    """No time left before the deadline: tuning skips, the final run is not started."""
    sys.path.insert(0, ROOT)
    import bench

    pool = [("a", "native", {"x": 1}), ("b", "native", {"x": 2})]
    job = _FakeJob(pool, {"a": [_ok(1.0)]})
    job.left = lambda: 35.0 if job.calls else 1e9  # 35 - 30 reserved < 10 s
    tune = {}
    chosen, _ = bench.autotune(job, pool, _args(final_reserve_s=30.0), 2, tune)
    assert chosen[0] == "a" and tune["b"].startswith("skipped (deadline")
    job.left = lambda: 12.0
    cand, final = bench.final_measure(job, chosen, [], _args(), tune)
    assert final is None and "deadline" in tune["final_rejected"][0]


def test_bench_world2_cpu_preflight_fields():
    """The JSON line names the timing mode, the preflight outcome and the vendor time; a
    scripted preflight failure of a family is reported (DDLB_PREFLIGHT_FAKE)."""
    from conftest import free_port

    env = _env()
    env["DDLB_PREFLIGHT_FAKE"] = json.dumps({"torch_nccl": "ok", "rccl": "ok",
                                             "ipc": "failed: scripted"})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", *FULL]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=400, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    d = _json_line(r.stdout)
    assert d["preflight"]["ipc"] == "failed: scripted"
    assert d["timing"].startswith("cpu_clock window")
    assert d["harness_mean_ms"] > 0 and d["max_err"] <= d["err_bound"]
    # first-contact diagnostics at world > 1: every part reported -- here
    # with the native layer absent, as its own error -- inside the budget
    diag = d["diag"]
    assert set(diag) >= {"xgmi", "rccl", "trace", "budget_s", "wall_s", "job_s"}
    assert set(diag["xgmi"]) == {"0", "1"}  # every rank's probe
    for part in ("rccl", "trace"):
        assert "error" in diag[part] or "skipped" in diag[part], diag[part]
    assert diag["wall_s"] <= diag["budget_s"] + 5 and diag["job_s"] <= diag["budget_s"] + 45


def test_autotune_drops_candidates_of_failed_primitive_phases():
    """Mocked failures of the primitive-level preflight phases drop exactly their families: the
    RCCL-fed fused GEMM (rccl_fused), the in-kernel all-gather (ipc_agk) and, for tp_rowwise, the
    direct-store epilogue (ipc_dstore)."""
    sys.path.insert(0, ROOT)
    import bench

    pool = [("rf", "native", {"backend": "rccl", "algorithm": "coll_pipeline", "fused": True}),
            ("r", "native", {"backend": "rccl", "algorithm": "coll_pipeline"}),
            ("agk", "native", {"backend": "ipc", "algorithm": "coll_pipeline", "fused": True,
                               "multicast_protocol": "kernel", "graph": True}),
            ("k", "native", {"backend": "ipc", "multicast_protocol": "kernel", "graph": True})]
    job = _FakeJob(pool, {"r": [_ok(1.0)], "k": [_ok(0.9)]})
    pre = {"rccl": "ok", "rccl_fused": "failed: AssertionError", "ipc": "ok", "ipc_ksig": "ok",
           "ipc_kernel": "ok", "ipc_agk": "failed: timeout", "torch_nccl": "ok"}
    tune = {}
    chosen, _ = bench.autotune(job, pool, _args(), 8, tune, pre)
    assert chosen[0] == "k"
    assert tune["rf"].startswith("skipped (rccl_fused") and tune["agk"].startswith("skipped (ipc_agk")
    row_pool = [("d", "native", {"backend": "ipc", "algorithm": "p2p_pipeline", "fused": True,
                                 "graph": False}),
                ("m", "native", {"backend": "ipc", "algorithm": "p2p_pipeline", "graph": False})]
    job = _FakeJob(row_pool, {"m": [_ok(2.0)]})
    tune = {}
    pre = {"ipc": "ok", "ipc_ksig": "ok", "ipc_sdma": "ok", "ipc_dstore": "failed: timeout"}
    chosen, _ = bench.autotune(job, row_pool, _args(primitive="tp_rowwise"), 8, tune, pre)
    assert chosen[0] == "m" and tune["d"].startswith("skipped (ipc_dstore")


def test_fused_rccl_hangs_do_not_drop_plain_rccl():
    """Timeouts are charged to a candidate's most specific mechanism: two hangs of the RCCL-fed
    fused GEMM skip the other fused candidates, never the plain RCCL pipelines."""
    sys.path.insert(0, ROOT)
    import bench

    fused = {"backend": "rccl", "algorithm": "coll_pipeline", "fused": True}
    pool = [("f1", "native", dict(fused, s=8)), ("f2", "native", dict(fused, s=4)),
            ("f3", "native", dict(fused, s=2)), ("r", "native", {"backend": "rccl", "s": 4})]
    to = {"ok": False, "error": "timeout after 45s"}
    job = _FakeJob(pool, {"f1": [to], "f2": [to], "r": [_ok(1.0)]})
    tune = {}
    chosen, _ = bench.autotune(job, pool, _args(), 8, tune, {})
    assert chosen[0] == "r"
    assert "rccl_fused candidates timed out twice" in tune["f3"]


def _budget_run(pool, hang, t_ok=10.0, t_hang=45.0, budget=300.0, world=8, primitive=None):
    """autotune over ``pool`` on a scripted clock: every candidate takes t_ok s, the ``hang``
    labels time out after t_hang s."""
    import bench

    clock = [0.0]
    job = _FakeJob(pool, {})

    def measure(impl, opts, steps, warmup, validate, timeout, prewarm_ms=0.0, harness_iters=0):
        label = job.by_opts[json.dumps(opts, sort_keys=True)]
        job.calls.append((label, validate))
        if label in hang:
            clock[0] += t_hang
            return {"ok": False, "error": f"timeout after {t_hang:.0f}s"}
        clock[0] += t_ok
        return _ok(1.0 + 0.01 * len(job.calls))

    job.measure = measure
    kw = dict(tune_budget_s=budget, tune_cap_s=360.0, final_reserve_s=100.0)
    if primitive:
        kw["primitive"] = primitive
    orig = bench.time.time
    bench.time.time = lambda: clock[0]
    try:
        tune = {}
        bench.autotune(job, pool, _args(**kw), world, tune, {})
    finally:
        bench.time.time = orig
    return tune, clock[0]


def test_pool_fits_tuning_budget():
    """at N = 8 every default pool (columnwise bf16 / fp8, rowwise) is tried in full
    inside --tune-budget-s (300 s) even when two candidates hang for the whole candidate timeout
    (45 s) and every other one takes 10 s (2-rank rehearsals: ~3 s per candidate)."""
    sys.path.insert(0, ROOT)
    import bench

    for prim, dt in [("tp_columnwise", "bfloat16"), ("tp_columnwise", "float8_e4m3fn"),
                     ("tp_rowwise", "bfloat16")]:
        pool = bench.candidate_pool(prim, dt, 8)
        natives = [c[0] for c in pool if c[1] == "native"]
        # worst case: the two hangs are the last natives (nothing is skipped after them)
        tune, spent = _budget_run(pool, set(natives[-2:]), primitive=prim)
        skipped = [k for k, v in tune.items() if isinstance(v, str) and "deadline" in v]
        assert not skipped, (prim, dt, len(pool), spent, skipped)
        assert spent <= 300.0 + 45.0, (prim, dt, spent)


def test_diagnose_parts_budget_and_errors():
    """ddlb_amd.parallel.diagnose.run: parts in order, a raising part reported with its error
    (the others still run), parts past the budget skipped, wall times recorded."""
    from ddlb_amd.parallel import diagnose

    t = [0.0]

    def clock():
        return t[0]

    def slow():
        t[0] += 20.0
        return {"ok": 1}

    def bad():
        raise RuntimeError("no native layer\nsecond line")

    res = diagnose.run({"xgmi": slow, "rccl": bad, "trace": slow, "late": slow}, 30.0,
                       clock=clock)
    assert res["xgmi"] == {"ok": 1, "wall_s": 20.0}
    assert res["rccl"]["error"] == "RuntimeError: no native layer"
    assert res["trace"]["wall_s"] == 20.0
    assert res["late"]["skipped"].startswith("budget")
    assert res["wall_s"] == 40.0


def test_diagnose_message_sizes():
    from ddlb_amd.parallel import diagnose

    sz = diagnose.message_sizes("tp_columnwise", 65536, 1024, 1024, 8, 2)
    assert sz == {"ag_shard": 16 << 20, "ag_stage_s4": 4 << 20, "ag_stage_s8": 2 << 20}
    sz = diagnose.message_sizes("tp_rowwise", 16384, 8192, 8192, 8, 2)
    assert sz["rs_block"] == 2048 * 8192 * 2
    per = diagnose.merge_ranks([{"rccl": {"x": 1}, "xgmi": {"a": 1}}, {"xgmi": {"a": 2}}])
    assert per["rccl"] == {"x": 1} and per["xgmi"] == {"0": {"a": 1}, "1": {"a": 2}}


def _bench(args, env=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args],
                       capture_output=True, text=True, timeout=300, env=env or _env())
    assert r.returncode == 0, r.stderr[-3000:]
    return _json_line(r.stdout)


def test_plain_run_is_lean_and_dumps_the_same_outputs(tmp_path):
    """A plain run reports the headline only (no reference check, no harness timing, no vendor
    slots, no search) and --dump-outputs writes the last timed step's result: float32, the full
    [m, n] at this size, the product of the seeded inputs, identical from a plain and a --full
    run (same arguments, same inputs)."""
    import numpy as np
    import torch

    from ddlb_amd.primitives.base import uniform_pm1

    plain = _bench([*ARGS, "--dump-outputs", str(tmp_path / "plain")])
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0 and plain["full"] is False
    assert plain["valid"] is None and plain["harness_mean_ms"] is None
    assert plain["max_err"] is None and plain["vendor_ms"] == {} and plain["autotune_ms"] == {}
    assert "diag" not in plain
    assert plain["outputs"] == {"out": [[256, 64], [256, 64]]}
    full = _bench([*FULL, "--dump-outputs", str(tmp_path / "full")])
    assert full["valid"] is True and full["harness_mean_ms"] > 0 and full["full"] is True
    for key in ("metric", "unit", "higher_is_better", "dtype"):
        assert plain[key] == full[key]
    a, b = np.load(tmp_path / "plain" / "out.npy"), np.load(tmp_path / "full" / "out.npy")
    assert a.dtype == np.float32 and a.shape == (256, 64)
    assert np.array_equal(a, b)
    g = torch.Generator().manual_seed(42)  # the primitive's inputs: A [m, k], then B [k, n]
    A = uniform_pm1((256, 64), "float32", g, "cpu")
    B = uniform_pm1((64, 64), "float32", g, "cpu")
    assert np.abs(a - (A.double() @ B.double()).numpy()).max() <= 64 * 2.0 ** -20


def test_dump_outputs_samples_large_results(tmp_path, monkeypatch):
    """Over the size budget the dump keeps whole rows, drawn once from a seeded generator, in
    row order: the same rows in every call, inside the budget; one over-long row falls back to
    elements of the flattened result. float64 / integer results are written as float64."""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import bench

    monkeypatch.setattr(bench, "DUMP_BYTES", 4096)
    t = torch.arange(1000 * 16, dtype=torch.float32).reshape(1000, 16).to(torch.bfloat16)
    done = bench.dump_outputs(str(tmp_path / "a"), {"out": t})
    bench.dump_outputs(str(tmp_path / "b"), {"out": t})
    a, b = np.load(tmp_path / "a" / "out.npy"), np.load(tmp_path / "b" / "out.npy")
    assert done == {"out": [[64, 16], [1000, 16]]}
    assert a.dtype == np.float32 and a.shape == (64, 16) and a.nbytes <= 4096
    assert np.array_equal(a, b)
    rows = np.random.default_rng(bench.DUMP_SEED).choice(1000, 64, replace=False)
    assert np.array_equal(a, t.float().numpy()[np.sort(rows)])
    wide = torch.arange(2 * 4096, dtype=torch.int64).reshape(2, 4096)
    bench.dump_outputs(str(tmp_path / "c"), {"out": wide})
    c = np.load(tmp_path / "c" / "out.npy")
    assert c.dtype == np.float64 and c.shape == (512,) and np.all(np.diff(c) > 0)
    small = torch.ones(3, 5, dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "d"), {"out": small})
    assert np.load(tmp_path / "d" / "out.npy").dtype == np.float64
